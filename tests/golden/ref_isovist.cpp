// ref_isovist.cpp -- fixture generator only: run by hand through make_golden_isovist.py, never by build(),
// by a test or on a GPU machine.
//
// Our own driver, linked against the reference library oracle/_ref/libsalaref.a (compiled by oracle/Makefile).
// It runs the reference's VGA isovist analysis (MetaGraph::analyseGraph(OUTPUT_ISOVIST) -> VGAIsovist::run)
//
//   --lines L.csv --spacing s --fill x,y [--filltype 0|1] [--variants K] [--write OUT.graph] --out DIR
//
// import -> grid -> fill -> makeGraph -> analyseGraph, all in memory, K times over.  Variant 0 is the plain
// run and the one that is stored (and written to OUT.graph).  The other variants sample what the reference's
// result depends on besides its input:
//   variants 1 .. K/2-1   another pafsrand seed (BSPTree::makeLines picks pafrand() % size for sets of at most
//                         3 lines, so the tree depends on the state of the global LCG);
//   variants K/2 .. K-1   another seed, and acos / sin / cos nudged: this executable defines the three
//                         functions itself, forwards to libm through dlsym(RTLD_NEXT, ...) and moves the result by
//                         0 or +-1 ulp, chosen by a hash of the argument and the variant (link with -fno-builtin).
// Dumps
//   DIR/isovist.bin     float32 [N][8]  the columns in table order: Isovist Area, Compactness, Drift Angle, Drift
//                                       Magnitude, Max Radial, Min Radial, Occlusivity, Perimeter; row (node) order
//   DIR/occ_dist.bin    float32 [N][32] Bin::m_occ_distance
//   DIR/occ_counts.bin  int32 [N][32]   sizes of Node::m_occlusion_bins
//   DIR/occ_pixels.bin  int32 [total]   their PixelRefs (int(PixelRef)), by node, bin, push order
//   DIR/hashes.bin      uint64 [K][N]   per variant and node, a hash over all of the above
//   DIR/state.bin       int32 [cols*rows]  Point::m_state, x-major
//   DIR/grid.txt        cols, rows, nodes, region, bottom_left, t_isovist (variant 0, single thread)
#include <dlfcn.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <cmath>
#include <deque>
#include <fstream>
#include <functional>
#include <iostream>
#include <list>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#define protected public
#define private public
#include "salalib/mgraph.h"
#include "salalib/ngraph.h"
#include "salalib/importutils.h"
#include "genlib/pafmath.h"
#undef protected
#undef private

static unsigned long long g_salt = 0;   // 0: libm's own results

static double nudged(const char* name, double x, int which) {
    typedef double (*fn_t)(double);
    static fn_t fns[3] = {nullptr, nullptr, nullptr};
    if (!fns[which]) fns[which] = (fn_t)dlsym(RTLD_NEXT, name);
    const double r = fns[which](x);
    if (!g_salt || r == 0.0 || !(r == r)) return r;
    unsigned long long b;
    memcpy(&b, &x, 8);
    unsigned long long z = (b ^ (g_salt * 0x9E3779B97F4A7C15ull)) + (unsigned long long)which;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    switch (z % 3) {
    case 0: return r;
    case 1: return nextafter(r, INFINITY);
    default: return nextafter(r, -INFINITY);
    }
}
extern "C" double acos(double x) noexcept { return nudged("acos", x, 0); }
extern "C" double sin(double x) noexcept { return nudged("sin", x, 1); }
extern "C" double cos(double x) noexcept { return nudged("cos", x, 2); }

template <typename T> static void dump(const std::string& path, const std::vector<T>& v) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); exit(2); }
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
    fclose(f);
}

static void fnv(unsigned long long& h, const void* p, size_t n) {
    const unsigned char* c = (const unsigned char*)p;
    for (size_t i = 0; i < n; i++) { h ^= c[i]; h *= 0x100000001B3ull; }
}

int main(int argc, char** argv) {
    std::string linesCsv, writeOut, outDir = ".";
    double spacing = -1;
    int filltype = 0, K = 1;
    std::vector<Point2f> fills;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() { if (i + 1 >= argc) { fprintf(stderr, "missing arg for %s\n", a.c_str()); exit(2); } return std::string(argv[++i]); };
        if (a == "--lines") linesCsv = next();
        else if (a == "--write") writeOut = next();
        else if (a == "--spacing") spacing = atof(next().c_str());
        else if (a == "--filltype") filltype = atoi(next().c_str());
        else if (a == "--variants") K = atoi(next().c_str());
        else if (a == "--fill") { std::string p = next(); double x, y; sscanf(p.c_str(), "%lf,%lf", &x, &y); fills.push_back(Point2f(x, y)); }
        else if (a == "--out") outDir = next();
        else { fprintf(stderr, "unknown arg %s\n", a.c_str()); return 2; }
    }
    MetaGraph mg;
    {
        std::ifstream f(linesCsv);
        if (!depthmapX::importFile(mg, f, nullptr, linesCsv, depthmapX::ImportType::DRAWINGMAP,
                                   depthmapX::ImportFileType::CSV)) {
            fprintf(stderr, "import failed\n");
            return 1;
        }
    }
    QtRegion reg = mg.getRegion();
    mg.addNewPointMap();
    mg.setGrid(spacing, Point2f(0.0, 0.0));
    for (auto& p : fills) {
        if (!reg.contains(p)) { fprintf(stderr, "Point outside of target region\n"); return 1; }
        mg.makePoints(p, filltype, nullptr);
    }
    if (!mg.makeGraph(nullptr, 0, -1)) { fprintf(stderr, "makeGraph failed\n"); return 1; }
    PointMap& pm = mg.getDisplayedPointMap();
    const size_t cols = pm.getCols(), rows = pm.getRows();
    static const char* NAMES[8] = {"Isovist Area", "Isovist Compactness", "Isovist Drift Angle", "Isovist Drift Magnitude",
                                   "Isovist Max Radial", "Isovist Min Radial", "Isovist Occlusivity", "Isovist Perimeter"};
    std::vector<unsigned long long> hashes;
    double t_first = 0;
    size_t N = 0;
    // the stored variant runs last, so that OUT.graph and the dumps hold it
    for (int kk = 0; kk < K; kk++) {
        const int v = (kk + 1) % K;
        if (v != 0) pafsrand(1000u + 7919u * (unsigned)v);
        g_salt = (v >= K / 2 && v != 0) ? (unsigned long long)v : 0ull;
        Options opt;
        opt.output_type = Options::OUTPUT_ISOVIST;
        auto t0 = std::chrono::steady_clock::now();
        const bool ok = mg.analyseGraph(nullptr, opt, false);
        auto t1 = std::chrono::steady_clock::now();
        g_salt = 0;
        if (!ok) { fprintf(stderr, "analyseGraph failed\n"); return 1; }
        AttributeTable& at = pm.getAttributeTable();
        int col[8];
        for (int c = 0; c < 8; c++) col[c] = (int)at.getColumnIndex(NAMES[c]);
        std::vector<float> iso, od;
        std::vector<int> oc, op;
        std::vector<unsigned long long> hv;
        for (auto it = at.begin(); it != at.end(); ++it) {
            unsigned long long h = 0xCBF29CE484222325ull;
            for (int c = 0; c < 8; c++) {
                const float f = it->getRow().getValue(col[c]);
                iso.push_back(f);
                fnv(h, &f, 4);
            }
            Point& pt = pm.getPoint(it->getKey().value);
            for (int b = 0; b < 32; b++) {
                const float d = pt.m_node->bin(b).m_occ_distance;
                od.push_back(d);
                fnv(h, &d, 4);
                const std::vector<PixelRef>& occ = pt.m_node->m_occlusion_bins[b];
                const int n = (int)occ.size();
                oc.push_back(n);
                fnv(h, &n, 4);
                for (const PixelRef& p : occ) {
                    const int pi = int(p);
                    op.push_back(pi);
                    fnv(h, &pi, 4);
                }
            }
            hv.push_back(h);
        }
        N = hv.size();
        if (hashes.empty()) hashes.resize((size_t)K * N);
        std::copy(hv.begin(), hv.end(), hashes.begin() + (size_t)v * N);
        if (v == 0) {
            t_first = std::chrono::duration<double>(t1 - t0).count();
            dump(outDir + "/isovist.bin", iso);
            dump(outDir + "/occ_dist.bin", od);
            dump(outDir + "/occ_counts.bin", oc);
            dump(outDir + "/occ_pixels.bin", op);
        }
    }
    dump(outDir + "/hashes.bin", hashes);
    std::vector<int> state(cols * rows);
    for (size_t i = 0; i < cols; i++)
        for (size_t j = 0; j < rows; j++) state[i * rows + j] = pm.getPoint(PixelRef(i, j)).m_state;
    dump(outDir + "/state.bin", state);
    if (!writeOut.empty()) mg.write(writeOut, METAGRAPH_VERSION, false);
    FILE* f = fopen((outDir + "/grid.txt").c_str(), "w");
    fprintf(f, "cols %zu\nrows %zu\nnodes %zu\nvariants %d\n", cols, rows, N, K);
    fprintf(f, "region %.17g %.17g %.17g %.17g\n", reg.bottom_left.x, reg.bottom_left.y, reg.top_right.x, reg.top_right.y);
    fprintf(f, "bottom_left %.17g %.17g\n", pm.m_bottom_left.x, pm.m_bottom_left.y);
    fprintf(f, "t_isovist %.6f\n", t_first);
    fclose(f);
    return 0;
}
