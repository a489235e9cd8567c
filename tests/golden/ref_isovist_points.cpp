// ref_isovist_points.cpp -- fixture generator only: run by hand through make_golden_isovist_points.py, never by
// build(), by a test or on a GPU machine.
//
// Our own driver, linked against the reference library oracle/_ref/libsalaref.a (compiled by oracle/Makefile).
// It makes isovists at given points the way depthmapXcli -m ISOVIST does (runmethods.cpp:635-647):
//
//   --lines L.csv --points P.bin --n N [--variants K] --out DIR
//
// P.bin: float64 [N][4] = x, y, startangle, endangle, as passed to MetaGraph::makeIsovist(comm, p, start, end,
// false) -> Isovist::makeit.  Per variant v a fresh MetaGraph imports the drawing, makes the N isovists and the
// "Isovists" data map is read back: the shapes' m_points and the attribute rows.  Variant 0 is the plain run; the
// others sample what the reference's result depends on besides its input, as ref_isovist.cpp does:
//   variants 1 .. K/2-1   another pafsrand seed (the BSP tree depends on the state of the global LCG);
//   variants K/2 .. K-1   another seed, and acos / sin / cos nudged by 0 or +-1 ulp (link with -fno-builtin).
// Dumps, per variant v,
//   DIR/v<v>_cols.bin   float32 [N][8]  Isovist Area, Compactness, Drift Angle, Drift Magnitude, Max Radial, Min
//                                       Radial, Occlusivity, Perimeter
//   DIR/v<v>_cnt.bin    int32 [N]       vertices of each shape (0: no polygon shape was made)
//   DIR/v<v>_xy.bin     float64 [sum][2] SalaShape::m_points, shape after shape
// and DIR/info.txt: region (MetaGraph::m_region), t_isovists (variant 0: seconds of the N makeIsovist calls after
// the first, which builds the tree, plus that first call's seconds as t_first).
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

int main(int argc, char** argv) {
    std::string linesCsv, pointsBin, outDir = ".";
    long long N = 0;
    int K = 1;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() { if (i + 1 >= argc) { fprintf(stderr, "missing arg for %s\n", a.c_str()); exit(2); } return std::string(argv[++i]); };
        if (a == "--lines") linesCsv = next();
        else if (a == "--points") pointsBin = next();
        else if (a == "--n") N = atoll(next().c_str());
        else if (a == "--variants") K = atoi(next().c_str());
        else if (a == "--out") outDir = next();
        else { fprintf(stderr, "unknown arg %s\n", a.c_str()); return 2; }
    }
    std::vector<double> pts((size_t)N * 4);
    {
        FILE* f = fopen(pointsBin.c_str(), "rb");
        if (!f || fread(pts.data(), 8, pts.size(), f) != pts.size()) { fprintf(stderr, "cannot read points\n"); return 2; }
        fclose(f);
    }
    static const char* NAMES[8] = {"Isovist Area", "Isovist Compactness", "Isovist Drift Angle", "Isovist Drift Magnitude",
                                   "Isovist Max Radial", "Isovist Min Radial", "Isovist Occlusivity", "Isovist Perimeter"};
    double t_first = 0, t_rest = 0;
    QtRegion reg;
    for (int v = 0; v < K; v++) {
        MetaGraph mg;
        {
            std::ifstream f(linesCsv);
            if (!depthmapX::importFile(mg, f, nullptr, linesCsv, depthmapX::ImportType::DRAWINGMAP,
                                       depthmapX::ImportFileType::CSV)) {
                fprintf(stderr, "import failed\n");
                return 1;
            }
        }
        reg = mg.getRegion();
        if (v != 0) pafsrand(1000u + 7919u * (unsigned)v);
        g_salt = (v >= K / 2 && v != 0) ? (unsigned long long)v : 0ull;
        std::vector<int> refs;
        for (long long k = 0; k < N; k++) {
            auto t0 = std::chrono::steady_clock::now();
            const size_t before = mg.m_dataMaps.empty() ? 0 : mg.m_dataMaps[0].getAllShapes().size();
            if (!mg.makeIsovist(nullptr, Point2f(pts[4 * k], pts[4 * k + 1]), pts[4 * k + 2], pts[4 * k + 3], false)) {
                fprintf(stderr, "makeIsovist failed\n");
                return 1;
            }
            auto t1 = std::chrono::steady_clock::now();
            if (v == 0) (k == 0 ? t_first : t_rest) += std::chrono::duration<double>(t1 - t0).count();
            ShapeMap& map = mg.m_dataMaps[0];
            // the shape this call made (none for an empty polygon: makePolyShape returns -1)
            refs.push_back(map.getAllShapes().size() > before ? map.getAllShapes().rbegin()->first : -1);
        }
        g_salt = 0;
        ShapeMap& map = mg.m_dataMaps[0];
        if (map.getName() != "Isovists") { fprintf(stderr, "no Isovists data map\n"); return 1; }
        AttributeTable& at = map.getAttributeTable();
        int col[8];
        for (int c = 0; c < 8; c++) col[c] = (int)at.getColumnIndex(NAMES[c]);
        std::vector<float> cols;
        std::vector<int> cnt;
        std::vector<double> xy;
        for (long long k = 0; k < N; k++) {
            if (refs[k] < 0) {
                for (int c = 0; c < 8; c++) cols.push_back(-1.0f);
                cnt.push_back(0);
                continue;
            }
            const SalaShape& sh = map.getAllShapes().at(refs[k]);
            AttributeRow& row = at.getRow(AttributeKey(refs[k]));
            for (int c = 0; c < 8; c++) cols.push_back(row.getValue(col[c]));
            // a polygon of one or two vertices becomes a point or a line shape: not a polygon fixture
            const bool isPoly = sh.isPolygon();
            cnt.push_back(isPoly ? (int)sh.m_points.size() : 0);
            if (isPoly)
                for (const Point2f& p : sh.m_points) { xy.push_back(p.x); xy.push_back(p.y); }
        }
        char name[64];
        snprintf(name, sizeof(name), "/v%d_", v);
        dump(outDir + name + "cols.bin", cols);
        dump(outDir + name + "cnt.bin", cnt);
        dump(outDir + name + "xy.bin", xy);
    }
    FILE* f = fopen((outDir + "/info.txt").c_str(), "w");
    fprintf(f, "region %.17g %.17g %.17g %.17g\n", reg.bottom_left.x, reg.bottom_left.y, reg.top_right.x, reg.top_right.y);
    fprintf(f, "t_first %.6f\nt_isovists %.6f\n", t_first, t_rest);
    fclose(f);
    return 0;
}
