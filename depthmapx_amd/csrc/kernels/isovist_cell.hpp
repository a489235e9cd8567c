// isovist_cell.hpp -- the isovist of one cell centre, one source for the host and the HIP kernel
// (all functions are __host__ __device__; plain g++ compiles it too).  Compile with -ffp-contract=off.
//
// isovist_cell restates, for the full circle (startangle == endangle) at a cell centre, and isovist_point for any
// point and any (startangle, endangle):
//   Isovist::makeit                      salalib/isovist.cpp:31-120
//   Isovist::make / drawnode / addBlock  salalib/isovist.cpp:146-268
//   Isovist::setData                     salalib/isovist.cpp:270-335
//   the occlusion loop of VGAIsovist::run  salalib/vgamodules/vgaisovist.cpp:53-75
//   BSPNode::classify                    genlib/bsptree.h:43-53
//   intersection_point, dist(point, line)  genlib/p2dpoly.h:483-486, p2dpoly.cpp:433-470, :525-563
//
// m_gaps and m_blocks are std::set<IsoSeg> keyed on (startangle, endangle) with exact comparison.  Here both
// are arrays kept sorted by that key: an insert with an equal key is dropped, erase + insert re-sorts, and
// the blocks are read in key order.  addBlock's walk is followed literally, the `gap++` after the middle
// split included; gaps flagged tagdelete stay in the list (and can be met again by the second addBlock of a
// wall that spans angle 0) until the end of drawnode.
//
// The BSP tree is walked front to back without a stack (parent links): the tree of a 500-piece arc is 500
// deep.  The walk ends as soon as no gap is left; every drawnode after that would change nothing.
//
// All arithmetic is FP64; values are rounded to float only where the reference calls setValue /
// setOccDistance.  acos, sin and cos are the platform's.
#pragma once
#include <cmath>
#include <cstdint>

#include "../host/geometry.hpp"
#include "span.hpp"

namespace dmx {

constexpr double ISO_PI = 3.14159265358979323846;   // M_PI

// error flags of isovist_cell
enum IsoError : int { ISO_OK = 0, ISO_GAP_CAPACITY = 1, ISO_BLOCK_CAPACITY = 2 };

// The flattened tree (host/bsptree.hpp): node k holds the line seg[4k..4k+3] = start.x, start.y, end.x, end.y
// (Line::start() / end(): start has the smaller x), its children and its parent (-1: none).
struct IsoTree {
    const double* seg;
    const int32_t* left;
    const int32_t* right;
    const int32_t* parent;
    int32_t nnodes;
};

// PointMap geometry for depixelate / pixelate (pointdata.h:353-357, pointdata.cpp:263-283)
struct IsoGrid {
    double blx, bly, spacing;
    int cols, rows;
};

// Per-cell list storage.  Element i, field f of the gap list is g[(i * 2 + f) * stride] (start, end) with its
// tagdelete flag gf[i * stride]; of the block list b[(i * 6 + f) * stride] (startangle, endangle, startpoint,
// endpoint), in insertion order, with bo[i * stride] the i-th block in key order.  stride 1 on the host; on the
// GPU the lists of a workgroup's lanes are interleaved.
struct IsoStore {
    double* g;
    int32_t* gf;
    double* b;
    int32_t* bo;
    int64_t stride;
    int gcap, bcap;
    int ng, nb;
    int maxg;   // the most gaps the list held (diagnostics)
    DMX_HD double& gs(int i) { return g[(int64_t)(i * 2) * stride]; }
    DMX_HD double& ge(int i) { return g[(int64_t)(i * 2 + 1) * stride]; }
    DMX_HD int32_t& gflag(int i) { return gf[(int64_t)i * stride]; }
    DMX_HD double& bf(int i, int f) { return b[(int64_t)(i * 6 + f) * stride]; }
    DMX_HD int32_t& border(int i) { return bo[(int64_t)i * stride]; }   // i-th block in key order
};

DMX_HD bool iso_key_less(double s1, double e1, double s2, double e2) {   // IsoSeg operator<
    return s1 == s2 ? e1 < e2 : s1 < s2;
}

DMX_HD void iso_gap_erase(IsoStore& S, int i) {
    for (int k = i; k + 1 < S.ng; k++) {
        S.gs(k) = S.gs(k + 1);
        S.ge(k) = S.ge(k + 1);
        S.gflag(k) = S.gflag(k + 1);
    }
    S.ng--;
}

// std::set::insert: the index of the new element, or of the element with an equal key (nothing inserted,
// *added = false); -1 when the list is full
DMX_HD int iso_gap_insert(IsoStore& S, double s, double e, int32_t flag, bool* added) {
    int i = 0;
    while (i < S.ng && iso_key_less(S.gs(i), S.ge(i), s, e)) i++;
    *added = false;
    if (i < S.ng && !iso_key_less(s, e, S.gs(i), S.ge(i))) return i;
    if (S.ng >= S.gcap) return -1;
    for (int k = S.ng; k > i; k--) {
        S.gs(k) = S.gs(k - 1);
        S.ge(k) = S.ge(k - 1);
        S.gflag(k) = S.gflag(k - 1);
    }
    S.gs(i) = s;
    S.ge(i) = e;
    S.gflag(i) = flag;
    S.ng++;
    if (S.ng > S.maxg) S.maxg = S.ng;
    *added = true;
    return i;
}

// m_blocks.insert: the blocks stay where they are appended, bo keeps their order by key
DMX_HD bool iso_block_insert(IsoStore& S, double a, double b, Vec2 pa, Vec2 pb) {
    int i = 0;
    while (i < S.nb && iso_key_less(S.bf(S.border(i), 0), S.bf(S.border(i), 1), a, b)) i++;
    if (i < S.nb && !iso_key_less(a, b, S.bf(S.border(i), 0), S.bf(S.border(i), 1))) return true;   // equal key: dropped
    if (S.nb >= S.bcap) return false;
    for (int k = S.nb; k > i; k--) S.border(k) = S.border(k - 1);
    const int at = S.nb;
    S.border(i) = at;
    S.bf(at, 0) = a; S.bf(at, 1) = b;
    S.bf(at, 2) = pa.x; S.bf(at, 3) = pa.y;
    S.bf(at, 4) = pb.x; S.bf(at, 5) = pb.y;
    S.nb++;
    return true;
}

// ---- genlib/p2dpoly.h pieces
DMX_HD Vec2 iso_normalise(Vec2 v) {   // Point2f::normalise: scale(1.0 / length())
    const double s = 1.0 / sqrt(v.x * v.x + v.y * v.y);
    return Vec2{v.x * s, v.y * s};
}
DMX_HD double iso_det(Vec2 a, Vec2 b) { return a.x * b.y - a.y * b.x; }
DMX_HD double iso_dot(Vec2 a, Vec2 b) { return a.x * b.x + a.y * b.y; }
DMX_HD double iso_len(Vec2 a) { return sqrt(a.x * a.x + a.y * a.y); }
DMX_HD double iso_dist(Vec2 a, Vec2 b) {   // sqrt(sqr(dx) + sqr(dy))
    return sqrt((a.x - b.x) * (a.x - b.x) + (a.y - b.y) * (a.y - b.y));
}
DMX_HD double iso_angle(Vec2 v) {   // Point2f::angle (p2dpoly.h:136)
    return (v.y < 0) ? (2.0 * ISO_PI - acos(v.x)) : acos(v.x);
}
DMX_HD bool iso_approxeq(Vec2 a, Vec2 b, double tol) { return fabs(a.x - b.x) <= tol && fabs(a.y - b.y) <= tol; }

DMX_HD double seg_grad_y(const Seg& s) { return s.sign() * s.r.height() / s.r.width(); }   // grad(YAXIS)
DMX_HD double seg_grad_x(const Seg& s) { return s.sign() * s.r.width() / s.r.height(); }   // grad(XAXIS)
DMX_HD Vec2 seg_midpoint(const Seg& s) {
    const Vec2 a = s.start(), b = s.end();
    return Vec2{(a.x + b.x) / 2, (a.y + b.y) / 2};
}

// intersection_point(a, b, tolerance) (p2dpoly.h:483-486): where the line through b meets a
DMX_HD Vec2 seg_intersection_point(const Seg& a, const Seg& l, double tolerance) {
    double loc;
    if (a.r.width() >= a.r.height()) {   // XAXIS
        if (l.r.width() == 0.0) {
            loc = l.r.blx;
        } else {
            const double lg = seg_grad_y(l), g = seg_grad_y(a);
            if (fabs(lg - g) <= tolerance) {
                const Vec2 p = seg_midpoint(l);
                loc = (p.x > a.r.trx) ? a.r.trx : ((p.x < a.r.blx) ? a.r.blx : p.x);
            } else {
                loc = ((a.ay() - g * a.ax()) - (l.ay() - lg * l.ax())) / (lg - g);
            }
        }
        const double g = seg_grad_y(a);
        return Vec2{loc, g * loc + (a.ay() - g * a.ax())};
    }
    if (l.r.height() == 0.0) {
        loc = l.r.bly;
    } else {
        const double lg = seg_grad_x(l), g = seg_grad_x(a);
        if (fabs(lg - g) <= tolerance) {
            const Vec2 p = seg_midpoint(l);
            loc = (p.y > a.r.tr_y) ? a.r.tr_y : ((p.y < a.r.bly) ? a.r.bly : p.y);
        } else {
            loc = ((a.ax() - g * a.ay()) - (l.ax() - lg * l.ay())) / (lg - g);
        }
    }
    const double g = seg_grad_x(a);
    return Vec2{g * loc + (a.ax() - g * a.ay()), loc};
}

// dist(point, Line(p1, p2)) (p2dpoly.cpp:539-563)
DMX_HD double iso_dist_seg(Vec2 point, const Seg& line) {
    const Vec2 s = line.start(), e = line.end();
    const Vec2 alpha{e.x - s.x, e.y - s.y}, beta{point.x - e.x, point.y - e.y};
    const Vec2 gamma{s.x - e.x, s.y - e.y}, delta{point.x - s.x, point.y - s.y};
    if (iso_dot(alpha, beta) > 0) return iso_len(beta);
    if (iso_dot(gamma, delta) > 0) return iso_len(delta);
    if (iso_len(alpha) < 1e-9 * iso_len(beta)) return iso_len(beta);
    return fabs(iso_det(alpha, beta)) / iso_len(alpha);
}

DMX_HD Seg iso_tree_seg(const IsoTree& T, int k) {
    const double* p = T.seg + 4 * (int64_t)k;
    return make_seg(Vec2{p[0], p[1]}, Vec2{p[2], p[3]});
}

// BSPNode::classify: true = BSPLEFT
DMX_HD bool iso_classify_left(const Seg& li, Vec2 p) {
    const Vec2 s = li.start(), e = li.end();
    const Vec2 v0 = iso_normalise(Vec2{e.x - s.x, e.y - s.y});
    const Vec2 v1 = iso_normalise(Vec2{p.x - s.x, p.y - s.y});
    return iso_det(v0, v1) >= 0;
}

// Isovist::addBlock (isovist.cpp:208-268); false when a list is full (err says which)
DMX_HD bool iso_add_block(IsoStore& S, const Seg& li, Vec2 centre, double startangle, double endangle, int* err) {
    int gap = 0;
    bool finished = false;
    while (!finished) {
        while (gap < S.ng && S.ge(gap) < startangle) gap++;
        if (gap < S.ng && S.gs(gap) < endangle + 1e-9) {
            double a, b;
            const double gs = S.gs(gap), ge = S.ge(gap);
            const int32_t gflag = S.gflag(gap);
            bool added;
            if (gs > startangle - 1e-9) {
                a = gs;
                if (ge < endangle + 1e-9) {
                    b = ge;
                    S.gflag(gap) = 1;
                } else {
                    b = endangle;
                    iso_gap_erase(S, gap);
                    gap = iso_gap_insert(S, endangle, ge, gflag, &added);
                }
            } else {
                a = startangle;
                if (ge < endangle + 1e-9) {
                    b = ge;
                    iso_gap_erase(S, gap);
                    gap = iso_gap_insert(S, gs, startangle, gflag, &added);
                } else {
                    b = endangle;
                    const int at = iso_gap_insert(S, endangle, ge, 0, &added);
                    if (at < 0) { *err |= ISO_GAP_CAPACITY; return false; }
                    if (added && at <= gap) gap++;
                    iso_gap_erase(S, gap);
                    gap = iso_gap_insert(S, gs, startangle, gflag, &added);
                    if (gap >= 0) gap++;   // "advance past gap just added"
                }
            }
            if (gap < 0) { *err |= ISO_GAP_CAPACITY; return false; }
            const Vec2 pa = seg_intersection_point(li, make_seg(centre, Vec2{centre.x + cos(a), centre.y + sin(a)}), 0.0);
            const Vec2 pb = seg_intersection_point(li, make_seg(centre, Vec2{centre.x + cos(b), centre.y + sin(b)}), 0.0);
            if (!iso_block_insert(S, a, b, pa, pb)) { *err |= ISO_BLOCK_CAPACITY; return false; }
        } else {
            finished = true;
        }
        if (gap >= S.ng) break;
        gap++;
    }
    return true;
}

// Isovist::drawnode (isovist.cpp:167-206)
DMX_HD bool iso_drawnode(IsoStore& S, const Seg& li, Vec2 centre, int* err) {
    const Vec2 s = li.start(), e = li.end();
    const double angle1 = iso_angle(iso_normalise(Vec2{s.x - centre.x, s.y - centre.y}));
    const double angle2 = iso_angle(iso_normalise(Vec2{e.x - centre.x, e.y - centre.y}));
    bool ok;
    if (angle2 > angle1) {
        if (angle2 - angle1 >= ISO_PI) {
            ok = iso_add_block(S, li, centre, 0.0, angle1, err) && iso_add_block(S, li, centre, angle2, 2.0 * ISO_PI, err);
        } else {
            ok = iso_add_block(S, li, centre, angle1, angle2, err);
        }
    } else {
        if (angle1 - angle2 >= ISO_PI) {
            ok = iso_add_block(S, li, centre, 0.0, angle2, err) && iso_add_block(S, li, centre, angle1, 2.0 * ISO_PI, err);
        } else {
            ok = iso_add_block(S, li, centre, angle2, angle1, err);
        }
    }
    if (!ok) return false;
    int w = 0;
    for (int i = 0; i < S.ng; i++) {
        if (S.gflag(i)) continue;
        if (w != i) {
            S.gs(w) = S.gs(i);
            S.ge(w) = S.ge(i);
            S.gflag(w) = 0;
        }
        w++;
    }
    S.ng = w;
    return true;
}

// Isovist::make: front to back by classify(centre), stackless
DMX_HD bool iso_walk(const IsoTree& T, IsoStore& S, Vec2 centre, int* err) {
    if (T.nnodes <= 0) return true;
    int node = 0;
    int from = 0;   // 0 entering from the parent, 1 back from the first child, 2 back from the second
    for (;;) {
        const Seg li = iso_tree_seg(T, node);
        const bool lft = iso_classify_left(li, centre);
        const int first = lft ? T.left[node] : T.right[node];
        const int second = lft ? T.right[node] : T.left[node];
        if (from == 0) {
            if (S.ng == 0) return true;   // nothing left to see: every further drawnode is a no-op
            if (first >= 0) { node = first; continue; }
            from = 1;
        }
        if (from == 1) {
            if (!iso_drawnode(S, li, centre, err)) return false;
            if (second >= 0 && S.ng > 0) { node = second; from = 0; continue; }
            from = 2;
        }
        // leaving this node
        const int par = T.parent[node];
        if (par < 0) return true;
        const bool plft = iso_classify_left(iso_tree_seg(T, par), centre);
        const int pfirst = plft ? T.left[par] : T.right[par];
        from = (node == pfirst) ? 1 : 2;
        node = par;
    }
}

// setData's loop body for the polygon edge (p1, p2), streamed
struct IsoAccum {
    double area, cx, cy, max_radial, min_radial;
    int n;
    Vec2 first, prev;
    DMX_HD void edge(Vec2 centre, Vec2 p1, Vec2 p2, int i) {
        double a_i = (p1.x * p2.y - p2.x * p1.y) / 2.0;
        area += a_i;
        a_i /= 6.0;
        cx += (p1.x + p2.x) * a_i;
        cy += (p1.y + p2.y) * a_i;
        const double dpoint = iso_dist(centre, p1);
        const double dline = iso_dist_seg(centre, make_seg(p1, p2));
        if (i != 0) {
            if (dline < min_radial) min_radial = dline;
            if (dpoint > max_radial) max_radial = dpoint;
        } else {
            max_radial = dpoint;
            min_radial = dline;
        }
    }
    DMX_HD void point(Vec2 centre, Vec2 p) {   // m_poly.push_back(p)
        if (n == 0) first = p;
        else edge(centre, prev, p, n - 1);
        prev = p;
        n++;
    }
    DMX_HD void close(Vec2 centre) {
        if (n > 0) edge(centre, prev, first, n - 1);
    }
};

// One cell.  out8 (table order: Area, Compactness, Drift Angle, Drift Magnitude, Max Radial, Min Radial,
// Occlusivity, Perimeter) gets column 0, and the rest unless simple.  occ_dist: the cell's 32 occ distances
// (set to 0, then the last point of a bin wins) or null.  sink.begin(n) is called once with an upper bound of
// the pushes that follow, then sink.push(bin, packed PixelRef) in the reference's push order.
// Returns ISO_OK or the capacity flags; on a capacity error nothing has been written.
template <class Sink>
DMX_HD int isovist_cell(const IsoTree& T, IsoStore& S, const IsoGrid& G, double tolerance, int px, int py, bool simple,
                        float* out8, float* occ_dist, Sink& sink) {
    const Vec2 centre{G.blx + G.spacing * 1.0 * double(px), G.bly + G.spacing * 1.0 * double(py)};
    int err = 0;
    S.ng = 0;
    S.nb = 0;
    S.gs(0) = 0.0;
    S.ge(0) = 2.0 * ISO_PI;
    S.gflag(0) = 0;
    S.ng = 1;
    S.maxg = 1;
    if (!iso_walk(T, S, centre, &err)) return err;

    // makeit's polygon pass (complete isovist), setData's sums and the occlusion points, streamed
    IsoAccum A;
    A.area = 0.0; A.cx = 0.0; A.cy = 0.0; A.max_radial = 0.0; A.min_radial = 0.0; A.n = 0;
    A.first = Vec2{0, 0}; A.prev = Vec2{0, 0};
    double perimeter = 0.0, occluded_perimeter = 0.0;
    if (occ_dist)
        for (int k = 0; k < 32; k++) occ_dist[k] = 0.0f;
    sink.begin(S.nb);
    auto occlusion = [&](Vec2 pt, double d) {   // vgaisovist.cpp:64-75
        const int bin = whichbin(pt.x - centre.x, pt.y - centre.y);
        if (d > 1.5) {
            // PointMap::pixelate, constrained
            int rx = (short)cvt_i32_x86(floor((pt.x - G.blx + (G.spacing / 2.0)) / G.spacing));
            int ry = (short)cvt_i32_x86(floor((pt.y - G.bly + (G.spacing / 2.0)) / G.spacing));
            if (rx < 0) rx = 0;
            else if (rx >= (short)G.cols) rx = G.cols - 1;
            if (ry < 0) ry = 0;
            else if (ry >= (short)G.rows) ry = G.rows - 1;
            if (rx != px || ry != py) sink.push(bin, (int32_t)(((uint32_t)rx << 16) + ((uint32_t)ry & 0xffffu)));
        }
        if (occ_dist) occ_dist[bin] = (float)d;
    };
    Vec2 prev_end{0, 0};
    for (int i = 0; i < S.nb; i++) {
        const int bi = S.border(i);
        const Vec2 sp{S.bf(bi, 2), S.bf(bi, 3)}, ep{S.bf(bi, 4), S.bf(bi, 5)};
        if (i != 0 && !iso_approxeq(prev_end, sp, tolerance)) {
            A.point(centre, sp);
            const double occluded = iso_dist(prev_end, sp);
            perimeter += occluded;
            occluded_perimeter += occluded;
            if (iso_dist(prev_end, centre) < iso_dist(sp, centre)) occlusion(prev_end, occluded);
            else occlusion(sp, occluded);
        }
        A.point(centre, ep);
        perimeter += iso_dist(sp, ep);
        prev_end = ep;
    }
    if (S.nb) {
        const Vec2 fs{S.bf(S.border(0), 2), S.bf(S.border(0), 3)};
        if (!iso_approxeq(prev_end, fs, tolerance)) {
            A.point(centre, fs);
            const double occluded = iso_dist(prev_end, fs);
            perimeter += occluded;
            occluded_perimeter += occluded;
            if (occluded > 1.5) {
                if (iso_dist(prev_end, centre) < iso_dist(fs, centre)) occlusion(prev_end, occluded);
                else occlusion(fs, occluded);
            }
        }
    }
    A.close(centre);
    const double sc = 2.0 / fabs(A.area);
    const Vec2 centroid{A.cx * sc, A.cy * sc};
    Vec2 drift{centroid.x - centre.x, centroid.y - centre.y};
    const double driftmag = iso_len(drift);
    drift = iso_normalise(drift);
    const double driftang = iso_angle(drift);
    out8[0] = (float)A.area;
    if (!simple) {
        out8[1] = (float)(4.0 * ISO_PI * A.area / (perimeter * perimeter));
        out8[2] = (float)(180.0 * driftang / ISO_PI);
        out8[3] = (float)driftmag;
        out8[4] = (float)A.max_radial;
        out8[5] = (float)A.min_radial;
        out8[6] = (float)occluded_perimeter;
        out8[7] = (float)perimeter;
    }
    return ISO_OK;
}

// One isovist at any point of the drawing, full circle or view cone: Isovist::makeit(root, centre, region,
// startangle, endangle) (isovist.cpp:31-120) and setData over its m_poly, which MetaGraph::makeIsovist
// (mgraph.cpp:491-521) runs per point.  tolerance = max(region.width(), region.height()) * 1e-9.
//   complete    startangle == endangle, or (0, 2 pi): one gap (0, 2 pi), no centre vertex
//   start > end the cone spans angle 0: gaps (0, end) and (start, 2 pi); the centre is pushed once, before the first
//               block whose startangle compares equal to the cone's
//   otherwise   one gap (start, end) ("parity"); the centre is pushed after the last block, before the closing test
// The occlusion bins of VGAIsovist::run are not made here.  vsink.begin(n) is called once with an upper bound of
// the pushes that follow (2 nb + 2: at most two a block, the centre, the closing vertex), then vsink.push(p) for
// every m_poly.push_back in order.  out8 as for isovist_cell.  Returns ISO_OK or the capacity flags; on a capacity
// error nothing has been written and the sink has not been begun.
template <class VSink>
DMX_HD int isovist_point(const IsoTree& T, IsoStore& S, double tolerance, Vec2 centre, double startangle,
                         double endangle, bool simple, float* out8, VSink& vsink) {
    bool complete = false;
    if (startangle == endangle || (startangle == 0.0 && endangle == 2.0 * ISO_PI)) {
        startangle = 0.0;
        endangle = 2.0 * ISO_PI;
        complete = true;
    }
    bool parity = false;
    int err = 0;
    S.ng = 0;
    S.nb = 0;
    S.maxg = 0;
    bool added;
    if (startangle > endangle) {
        if (iso_gap_insert(S, 0.0, endangle, 0, &added) < 0 || iso_gap_insert(S, startangle, 2.0 * ISO_PI, 0, &added) < 0)
            return ISO_GAP_CAPACITY;
    } else {
        parity = true;
        if (iso_gap_insert(S, startangle, endangle, 0, &added) < 0) return ISO_GAP_CAPACITY;
    }
    if (!iso_walk(T, S, centre, &err)) return err;

    IsoAccum A;
    A.area = 0.0; A.cx = 0.0; A.cy = 0.0; A.max_radial = 0.0; A.min_radial = 0.0; A.n = 0;
    A.first = Vec2{0, 0}; A.prev = Vec2{0, 0};
    double perimeter = 0.0, occluded_perimeter = 0.0;
    vsink.begin(2 * S.nb + 2);
    auto poly = [&](Vec2 p) {   // m_poly.push_back(p)
        A.point(centre, p);
        vsink.push(p);
    };
    bool markedcentre = false;
    Vec2 prev_end{0, 0};
    for (int i = 0; i < S.nb; i++) {
        const int bi = S.border(i);
        const Vec2 sp{S.bf(bi, 2), S.bf(bi, 3)}, ep{S.bf(bi, 4), S.bf(bi, 5)};
        if (!complete && !markedcentre && !parity && S.bf(bi, 0) == startangle) {
            poly(centre);
            markedcentre = true;
        }
        if (i != 0 && !iso_approxeq(prev_end, sp, tolerance)) {
            poly(sp);
            const double occluded = iso_dist(prev_end, sp);
            perimeter += occluded;
            occluded_perimeter += occluded;
        }
        poly(ep);
        perimeter += iso_dist(sp, ep);
        prev_end = ep;
    }
    if (!complete && parity) poly(centre);   // "if parity is true, the centre point must be last not first"
    if (S.nb) {
        const Vec2 fs{S.bf(S.border(0), 2), S.bf(S.border(0), 3)};
        if (!iso_approxeq(prev_end, fs, tolerance)) {
            poly(fs);
            const double occluded = iso_dist(prev_end, fs);
            perimeter += occluded;
            occluded_perimeter += occluded;
        }
    }
    A.close(centre);
    const double sc = 2.0 / fabs(A.area);
    const Vec2 centroid{A.cx * sc, A.cy * sc};
    Vec2 drift{centroid.x - centre.x, centroid.y - centre.y};
    const double driftmag = iso_len(drift);
    drift = iso_normalise(drift);
    const double driftang = iso_angle(drift);
    out8[0] = (float)A.area;
    if (!simple) {
        out8[1] = (float)(4.0 * ISO_PI * A.area / (perimeter * perimeter));
        out8[2] = (float)(180.0 * driftang / ISO_PI);
        out8[3] = (float)driftmag;
        out8[4] = (float)A.max_radial;
        out8[5] = (float)A.min_radial;
        out8[6] = (float)occluded_perimeter;
        out8[7] = (float)perimeter;
    }
    return ISO_OK;
}

}  // namespace dmx
