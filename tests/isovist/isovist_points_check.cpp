// isovist_points_check.cpp -- host run of isovists at arbitrary points for tests/test_isovist_points_host.py: the
// BSP builder (csrc/host/bsptree.cpp) and the per-point routine the kernel uses (isovist_point of
// csrc/kernels/isovist_cell.hpp).  Plain g++, -ffp-contract=off; also built with -fsanitize=address,undefined.
//
//   isovist_points_check points LINES.bin NLINES POINTS.bin N blx bly trx try OUTDIR [GCAP BCAP]
//       LINES.bin float64 [NLINES][4], POINTS.bin float64 [N][4] = x, y, startangle, endangle; the region gives the
//       tolerance (max(width, height) * 1e-9).  Dumps into OUTDIR cols.bin float32 [N][8], cnt.bin int32 [N] (the
//       vertices of each polygon), xy.bin float64 [sum][2] and info.txt (max_blocks, max_gaps, max_upper: the
//       largest bound a sink was begun with, over: the pushes beyond a bound, which must be 0).
//   isovist_points_check cells LINES.bin NLINES blx bly trx try SPACING FILLX FILLY
//       isovist_point at every filled cell's centre, full circle, with the point map's region, against
//       isovist_cell: prints "cells N mismatches M" (bitwise, all eight columns).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../depthmapx_amd/csrc/host/bsptree.hpp"
#include "../../depthmapx_amd/csrc/host/pointmap.hpp"
#include "../../depthmapx_amd/csrc/kernels/isovist_cell.hpp"

using namespace dmx;

template <typename T> static void dump(const std::string& path, const std::vector<T>& v) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); exit(2); }
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
    fclose(f);
}

static std::vector<double> read_f64(const char* path, size_t n) {
    std::vector<double> v(n);
    FILE* f = fopen(path, "rb");
    if (!f || fread(v.data(), 8, n, f) != n) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fclose(f);
    return v;
}

struct VertexSink {
    std::vector<double> xy;
    int upper = 0, over = 0;
    void begin(int n) { xy.clear(); upper = n; over = 0; }
    void push(Vec2 p) {
        if ((int)xy.size() / 2 >= upper) over++;
        xy.push_back(p.x);
        xy.push_back(p.y);
    }
};
struct NoOccSink {
    void begin(int) {}
    void push(int, int32_t) {}
};

int main(int argc, char** argv) {
    if (argc < 9) { fprintf(stderr, "usage: see the source\n"); return 2; }
    const bool cells = strcmp(argv[1], "cells") == 0;
    const int64_t nlines = atoll(argv[3]);
    const std::vector<double> lines = read_f64(argv[2], (size_t)nlines * 4);
    const int a0 = cells ? 4 : 6;
    if (argc < a0 + (cells ? 7 : 5)) { fprintf(stderr, "usage: see the source\n"); return 2; }
    const Rect region{atof(argv[a0]), atof(argv[a0 + 1]), atof(argv[a0 + 2]), atof(argv[a0 + 3])};
    const int gcap = (!cells && argc > 11) ? atoi(argv[11]) : 256, bcap = (!cells && argc > 12) ? atoi(argv[12]) : 1024;
    std::vector<double> gbuf((size_t)gcap * 2), bbuf((size_t)bcap * 6);
    std::vector<int32_t> gflag((size_t)gcap), border((size_t)bcap);
    VertexSink sink;
    if (cells) {
        const double spacing = atof(argv[8]);
        PointMapHost h(region, spacing, lines.data(), nlines);
        if (h.fill(atof(argv[9]), atof(argv[10]), 0) != 0) { fprintf(stderr, "fill failed\n"); return 1; }
        BspTree bt;
        bsp_build(h.drawing().data(), (int64_t)h.drawing().size() / 4, bt);
        const IsoTree T{bt.seg.data(), bt.left.data(), bt.right.data(), bt.parent.data(), (int32_t)bt.nodes()};
        const IsoGrid G{h.bottom_left().x, h.bottom_left().y, h.spacing(), h.cols(), h.rows()};
        const Rect& gr = h.grid_region();
        const double tolerance = (gr.width() > gr.height() ? gr.width() : gr.height()) * 1e-9;
        long long n = 0, bad = 0;
        for (int x = 0; x < h.cols(); x++)
            for (int y = 0; y < h.rows(); y++) {
                if (!(h.state()[h.index(x, y)] & CELL_FILLED)) continue;
                n++;
                float a[8], b[8];
                IsoStore S{gbuf.data(), gflag.data(), bbuf.data(), border.data(), 1, gcap, bcap, 0, 0, 0};
                NoOccSink none;
                if (isovist_cell(T, S, G, tolerance, x, y, false, a, nullptr, none)) return 3;
                const Vec2 centre{G.blx + G.spacing * 1.0 * double(x), G.bly + G.spacing * 1.0 * double(y)};
                if (isovist_point(T, S, tolerance, centre, 0.0, 0.0, false, b, sink)) return 3;
                if (memcmp(a, b, sizeof(a)) != 0) bad++;
            }
        printf("cells %lld mismatches %lld\n", n, bad);
        return bad ? 1 : 0;
    }
    const int64_t n = atoll(argv[5]);
    const std::vector<double> pts = read_f64(argv[4], (size_t)n * 4);
    const std::string out = argv[10];
    BspTree bt;
    bsp_build(lines.data(), nlines, bt);
    if (bt.nodes() == 0) { fprintf(stderr, "no lines\n"); return 1; }
    const IsoTree T{bt.seg.data(), bt.left.data(), bt.right.data(), bt.parent.data(), (int32_t)bt.nodes()};
    const double tolerance = (region.width() > region.height() ? region.width() : region.height()) * 1e-9;
    std::vector<float> cols;
    std::vector<int32_t> cnt;
    std::vector<double> xy;
    int max_blocks = 0, max_gaps = 0, max_upper = 0, over = 0;
    for (int64_t k = 0; k < n; k++) {
        float row[8];
        IsoStore S{gbuf.data(), gflag.data(), bbuf.data(), border.data(), 1, gcap, bcap, 0, 0, 0};
        const int err = isovist_point(T, S, tolerance, Vec2{pts[4 * k], pts[4 * k + 1]}, pts[4 * k + 2], pts[4 * k + 3], false,
                                      row, sink);
        if (err) { fprintf(stderr, "capacity error %d at point %lld\n", err, (long long)k); return 3; }
        if (S.nb > max_blocks) max_blocks = S.nb;
        if (S.maxg > max_gaps) max_gaps = S.maxg;
        if (sink.upper > max_upper) max_upper = sink.upper;
        over += sink.over;
        cols.insert(cols.end(), row, row + 8);
        cnt.push_back((int32_t)sink.xy.size() / 2);
        xy.insert(xy.end(), sink.xy.begin(), sink.xy.end());
    }
    dump(out + "/cols.bin", cols);
    dump(out + "/cnt.bin", cnt);
    dump(out + "/xy.bin", xy);
    FILE* f = fopen((out + "/info.txt").c_str(), "w");
    fprintf(f, "max_blocks %d\nmax_gaps %d\nmax_upper %d\nover %d\n", max_blocks, max_gaps, max_upper, over);
    fclose(f);
    return 0;
}
