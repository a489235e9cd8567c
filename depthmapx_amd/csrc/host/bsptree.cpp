// bsptree.cpp -- see bsptree.hpp.  Compile with -ffp-contract=off.
#include "bsptree.hpp"

#include <cmath>
#include <utility>

#include "../kernels/isovist_cell.hpp"

namespace dmx {
namespace {

struct Tagged {
    Seg line;
    int tag;
};

double mid_dist(const Seg& l, Vec2 m) { return iso_dist(seg_midpoint(l), m); }

// BSPTree::pickMidpointLine (bsptree.cpp:78-114); par < 0: no parent
int pick_midpoint_line(const std::vector<Tagged>& lines, const Seg* par) {
    int chosen = -1;
    Vec2 midpoint{0, 0};
    for (const Tagged& t : lines) {
        const Vec2 s = t.line.start(), e = t.line.end();
        midpoint.x += s.x + e.x;
        midpoint.y += s.y + e.y;
    }
    const double div = 2.0 * lines.size();
    midpoint.x /= div;
    midpoint.y /= div;
    bool ver = true;
    if (par && par->r.height() > par->r.width()) ver = false;
    double chosendist = -1.0;
    for (size_t i = 0; i < lines.size(); i++) {
        const Seg& line = lines[i].line;
        const bool want = ver ? line.r.height() > line.r.width() : line.r.width() > line.r.height();
        if (want && (chosen == -1 || mid_dist(line, midpoint) < chosendist)) {
            chosen = (int)i;
            chosendist = mid_dist(line, midpoint);
        }
    }
    if (chosen == -1) {
        for (size_t i = 0; i < lines.size(); i++) {
            if (chosen == -1 || mid_dist(lines[i].line, midpoint) < chosendist) {
                chosen = (int)i;
                chosendist = mid_dist(lines[i].line, midpoint);
            }
        }
    }
    return chosen;
}

// BSPTree::makeLines (bsptree.cpp:123-182): sets node's line, returns the lines left and right of it
void make_lines(const std::vector<Tagged>& lines, const Seg* par, Tagged& node, std::vector<Tagged>& leftlines,
                std::vector<Tagged>& rightlines) {
    const int chosen = lines.size() > 3 ? pick_midpoint_line(lines, par) : 0;
    node = lines[chosen];
    const Seg& chosenLine = node.line;
    const Vec2 cs = chosenLine.start(), ce = chosenLine.end();
    const Vec2 v0 = iso_normalise(Vec2{ce.x - cs.x, ce.y - cs.y});
    for (size_t i = 0; i < lines.size(); i++) {
        if ((int)i == chosen) continue;
        const Seg& testline = lines[i].line;
        const int tag = lines[i].tag;
        const Vec2 ts = testline.start(), te = testline.end();
        const Vec2 v1 = iso_normalise(Vec2{ts.x - cs.x, ts.y - cs.y});
        const Vec2 v2 = iso_normalise(Vec2{te.x - cs.x, te.y - cs.y});
        const double a = (ts.x == cs.x && ts.y == cs.y) ? 0 : iso_det(v0, v1);
        const double b = (te.x == cs.x && te.y == cs.y) ? 0 : iso_det(v0, v2);
        if (a >= 0 && b >= 0) {
            leftlines.push_back(lines[i]);
        } else if (a <= 0 && b <= 0) {
            rightlines.push_back(lines[i]);
        } else {
            const Vec2 p = seg_intersection_point(chosenLine, testline, 0.0);
            const Seg x = make_seg(ts, p), y = make_seg(p, te);
            if (a >= 0) {
                if (x.length() > 0.0) leftlines.push_back(Tagged{x, tag});
                if (y.length() > 0.0) rightlines.push_back(Tagged{y, tag});
            } else {
                if (x.length() > 0.0) rightlines.push_back(Tagged{x, tag});
                if (y.length() > 0.0) leftlines.push_back(Tagged{y, tag});
            }
        }
    }
}

}  // namespace

void bsp_build(const double* lines, int64_t nlines, BspTree& T) {
    T = BspTree();
    std::vector<Tagged> all;
    for (int64_t k = 0; k < nlines; k++) {
        const Seg s = make_seg(Vec2{lines[4 * k], lines[4 * k + 1]}, Vec2{lines[4 * k + 2], lines[4 * k + 3]});
        if (s.length() > 0.0) all.push_back(Tagged{s, (int)k});
    }
    if (all.empty()) return;
    struct Item {
        int node, depth;
        std::vector<Tagged> lines;
    };
    std::vector<Item> stack;
    auto new_node = [&](int parent) {
        T.seg.insert(T.seg.end(), 4, 0.0);
        T.tag.push_back(-1);
        T.left.push_back(-1);
        T.right.push_back(-1);
        T.parent.push_back(parent);
        return (int)T.tag.size() - 1;
    };
    stack.push_back(Item{new_node(-1), 1, std::move(all)});
    while (!stack.empty()) {
        Item it = std::move(stack.back());
        stack.pop_back();
        if (it.depth > T.depth) T.depth = it.depth;
        Seg parseg;
        const int par = T.parent[it.node];
        if (par >= 0) parseg = make_seg(Vec2{T.seg[4 * par], T.seg[4 * par + 1]}, Vec2{T.seg[4 * par + 2], T.seg[4 * par + 3]});
        Tagged node;
        std::vector<Tagged> l, r;
        make_lines(it.lines, par >= 0 ? &parseg : nullptr, node, l, r);
        const Vec2 s = node.line.start(), e = node.line.end();
        T.seg[4 * it.node] = s.x; T.seg[4 * it.node + 1] = s.y;
        T.seg[4 * it.node + 2] = e.x; T.seg[4 * it.node + 3] = e.y;
        T.tag[it.node] = node.tag;
        if (!l.empty()) {
            const int c = new_node(it.node);
            T.left[it.node] = c;
            stack.push_back(Item{c, it.depth + 1, std::move(l)});
        }
        if (!r.empty()) {
            const int c = new_node(it.node);
            T.right[it.node] = c;
            stack.push_back(Item{c, it.depth + 1, std::move(r)});
        }
    }
}

}  // namespace dmx
