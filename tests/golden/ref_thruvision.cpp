// ref_thruvision.cpp -- fixture generator only: run by hand through make_golden_thruvision.py, never by
// build(), by a test or on a GPU machine.
//
// Our own driver, linked against the reference library oracle/_ref/libsalaref.a (compiled by oracle/Makefile).
// It runs the reference's VGA through vision (MetaGraph::analyseGraph(OUTPUT_THRU_VISION) ->
// VGAThroughVision::run) in two ways:
//
//   (a) --lines L.csv | --drawing D.graph  --spacing s --fill x,y [--fill ...] --out DIR
//       import -> grid -> fill -> makeGraph -> analyseGraph, all in memory; dumps
//         DIR/thruvision.bin  float32 [N]   the "Through vision" column in row (node) order
//         DIR/state.bin       int32 [cols*rows]  Point::m_state, x-major
//         DIR/nruns.bin       int32 [N]     runs per node
//         DIR/runs.bin        int16 [R][4]  x0,y0,x1,y1 in Node::first()..next() order
//         DIR/lines.bin       float64 [L][4]  the drawing lines
//         DIR/grid.txt        cols, rows, region, bottom_left, nodes, t_thruvision
//   (b) --analyse IN.graph --write OUT.graph --out DIR
//       readFromFile -> analyseGraph -> write (what depthmapXcli -m VGA -vm thruvision does); dumps
//       thruvision.bin and grid.txt as above.
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
#undef protected
#undef private

template <typename T> static void dump(const std::string& path, const std::vector<T>& v) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); exit(2); }
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
    fclose(f);
}

int main(int argc, char** argv) {
    std::string linesCsv, drawing, analyse, writeOut, outDir = ".";
    double spacing = -1;
    std::vector<Point2f> fills;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() { if (i + 1 >= argc) { fprintf(stderr, "missing arg for %s\n", a.c_str()); exit(2); } return std::string(argv[++i]); };
        if (a == "--lines") linesCsv = next();
        else if (a == "--drawing") drawing = next();
        else if (a == "--analyse") analyse = next();
        else if (a == "--write") writeOut = next();
        else if (a == "--spacing") spacing = atof(next().c_str());
        else if (a == "--fill") { std::string p = next(); double x, y; sscanf(p.c_str(), "%lf,%lf", &x, &y); fills.push_back(Point2f(x, y)); }
        else if (a == "--out") outDir = next();
        else { fprintf(stderr, "unknown arg %s\n", a.c_str()); return 2; }
    }
    MetaGraph mg;
    if (!analyse.empty()) {
        if (mg.readFromFile(analyse) != MetaGraph::OK) { fprintf(stderr, "readFromFile failed\n"); return 1; }
    } else {
        if (!drawing.empty()) {
            if (mg.readFromFile(drawing) != MetaGraph::OK) { fprintf(stderr, "readFromFile failed\n"); return 1; }
        } else {
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
            mg.makePoints(p, 0, nullptr);
        }
        if (!mg.makeGraph(nullptr, 0, -1)) { fprintf(stderr, "makeGraph failed\n"); return 1; }
    }
    PointMap& pm = mg.getDisplayedPointMap();
    const size_t cols = pm.getCols(), rows = pm.getRows();
    Options opt;
    opt.output_type = Options::OUTPUT_THRU_VISION;
    auto t0 = std::chrono::steady_clock::now();
    if (!mg.analyseGraph(nullptr, opt, false)) { fprintf(stderr, "analyseGraph failed\n"); return 1; }
    auto t1 = std::chrono::steady_clock::now();
    AttributeTable& at = pm.getAttributeTable();
    const int col = (int)at.getColumnIndex("Through vision");
    std::vector<float> tv;
    std::vector<int> nruns;
    std::vector<short> runs;
    for (auto it = at.begin(); it != at.end(); ++it) {
        tv.push_back(it->getRow().getValue(col));
        Point& pt = pm.getPoint(it->getKey().value);
        int n = 0;
        for (int b = 0; b < 32; b++)
            for (auto& pv : pt.m_node->bin(b).m_pixel_vecs) {
                runs.push_back(pv.m_start.x); runs.push_back(pv.m_start.y);
                runs.push_back(pv.m_end.x); runs.push_back(pv.m_end.y);
                n++;
            }
        nruns.push_back(n);
    }
    dump(outDir + "/thruvision.bin", tv);
    if (analyse.empty()) {
        std::vector<int> state(cols * rows);
        for (size_t i = 0; i < cols; i++)
            for (size_t j = 0; j < rows; j++) state[i * rows + j] = pm.getPoint(PixelRef(i, j)).m_state;
        dump(outDir + "/state.bin", state);
        dump(outDir + "/nruns.bin", nruns);
        dump(outDir + "/runs.bin", runs);
        std::vector<double> lines;
        for (const auto& pixelGroup : *pm.m_drawingFiles)
            for (const auto& pixel : pixelGroup.m_spacePixels)
                if (pixel.isShown())
                    for (const auto& l : pixel.getAllShapesAsLines()) {
                        lines.push_back(l.start().x); lines.push_back(l.start().y);
                        lines.push_back(l.end().x); lines.push_back(l.end().y);
                    }
        dump(outDir + "/lines.bin", lines);
    }
    if (!writeOut.empty()) mg.write(writeOut, METAGRAPH_VERSION, false);
    QtRegion reg = mg.getRegion();
    FILE* f = fopen((outDir + "/grid.txt").c_str(), "w");
    fprintf(f, "cols %zu\nrows %zu\nnodes %zu\n", cols, rows, tv.size());
    fprintf(f, "region %.17g %.17g %.17g %.17g\n", reg.bottom_left.x, reg.bottom_left.y, reg.top_right.x, reg.top_right.y);
    fprintf(f, "bottom_left %.17g %.17g\n", pm.m_bottom_left.x, pm.m_bottom_left.y);
    fprintf(f, "t_thruvision %.6f\n", std::chrono::duration<double>(t1 - t0).count());
    fclose(f);
    return 0;
}
