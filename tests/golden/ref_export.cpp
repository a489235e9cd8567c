// ref_export.cpp -- fixture generator only: run by hand through make_golden_export.py, never by build(), by a
// test or on a GPU machine.
//
// Our own driver, linked against the reference library oracle/_ref/libsalaref.a (compiled by oracle/Makefile).
// It writes what depthmapXcli -m EXPORT writes for the displayed point map (dm_runmethods::exportData,
// depthmapXcli/runmethods.cpp:649-677):
//
//   DIR/data.csv         PointMap::outputSummary(stream, ',')             -em pointmap-data-csv
//   DIR/links.csv        PointMap::outputLinksAsCSV(stream, ",")          -em pointmap-links-csv
//   DIR/connections.csv  PointMap::outputConnectionsAsCSV(stream, ",")    -em pointmap-connections-csv
//   DIR/contents.bin     with --contents: int32, per node (x-major) its count, then Node::contents as PixelRef ints
//   DIR/info.txt         cols, rows, nodes, enumerated (cells Node::first()..next() visit), dropped (those that
//                        addIfNotExists left out), outside (those outside the grid: the export is not run then, it
//                        would index out of bounds), t_connections (wall seconds of outputConnectionsAsCSV)
//
// for the map of   (a) --graph IN.graph                                   MetaGraph::readFromFile
//                  (b) --lines L.csv --spacing s --fill x,y [--merge a,b ...] [--write OUT.graph]
//                      import -> grid -> fill -> makeGraph -> PointMap::mergePixels(a, b) (PixelRef ints), in memory;
//                      OUT.graph is that MetaGraph as the CLI writes it.
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

int main(int argc, char** argv) {
    std::string linesCsv, graph, writeOut, outDir = ".";
    double spacing = -1;
    bool contents = false;
    std::vector<Point2f> fills;
    std::vector<std::pair<int, int>> merges;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() { if (i + 1 >= argc) { fprintf(stderr, "missing arg for %s\n", a.c_str()); exit(2); } return std::string(argv[++i]); };
        if (a == "--lines") linesCsv = next();
        else if (a == "--graph") graph = next();
        else if (a == "--write") writeOut = next();
        else if (a == "--spacing") spacing = atof(next().c_str());
        else if (a == "--fill") { std::string p = next(); double x, y; sscanf(p.c_str(), "%lf,%lf", &x, &y); fills.push_back(Point2f(x, y)); }
        else if (a == "--merge") { std::string p = next(); int x, y; sscanf(p.c_str(), "%d,%d", &x, &y); merges.push_back({x, y}); }
        else if (a == "--contents") contents = true;
        else if (a == "--out") outDir = next();
        else { fprintf(stderr, "unknown arg %s\n", a.c_str()); return 2; }
    }
    MetaGraph mg;
    if (!graph.empty()) {
        if (mg.readFromFile(graph) != MetaGraph::OK) { fprintf(stderr, "readFromFile failed\n"); return 1; }
    } else {
        std::ifstream f(linesCsv);
        if (!depthmapX::importFile(mg, f, nullptr, linesCsv, depthmapX::ImportType::DRAWINGMAP,
                                   depthmapX::ImportFileType::CSV)) {
            fprintf(stderr, "import failed\n");
            return 1;
        }
        QtRegion reg = mg.getRegion();
        mg.addNewPointMap();
        mg.setGrid(spacing, Point2f(0.0, 0.0));
        for (auto& p : fills) {
            if (!reg.contains(p)) { fprintf(stderr, "Point outside of target region\n"); return 1; }
            mg.makePoints(p, 0, nullptr);
        }
        if (!mg.makeGraph(nullptr, 0, -1)) { fprintf(stderr, "makeGraph failed\n"); return 1; }
        for (auto& m : merges) mg.getDisplayedPointMap().mergePixels(PixelRef(m.first), PixelRef(m.second));
        if (!writeOut.empty()) mg.write(writeOut, METAGRAPH_VERSION, false);
    }
    PointMap& pm = mg.getDisplayedPointMap();
    const size_t cols = pm.getCols(), rows = pm.getRows();
    long long nodes = 0, enumerated = 0, dropped = 0, outside = 0;
    std::vector<int> cont;
    for (size_t i = 0; i < cols; i++)
        for (size_t j = 0; j < rows; j++) {
            Point& pnt = pm.m_points(j, i);
            if (!(pnt.filled() && pnt.m_node)) continue;
            nodes++;
            long long n = 0;
            for (pnt.m_node->first(); !pnt.m_node->is_tail(); pnt.m_node->next()) {
                const PixelRef p = pnt.m_node->cursor();
                if (p.x < 0 || p.y < 0 || (size_t)p.x >= cols || (size_t)p.y >= rows) outside++;
                n++;
            }
            PixelRefVector hood;
            pnt.m_node->contents(hood);
            enumerated += n;
            dropped += n - (long long)hood.size();
            if (contents) {
                cont.push_back((int)hood.size());
                for (auto& p : hood) cont.push_back((int)p);
            }
        }
    double t_conn = -1;
    {
        std::ofstream s(outDir + "/data.csv");
        pm.outputSummary(s, ',');
    }
    {
        std::ofstream s(outDir + "/links.csv");
        pm.outputLinksAsCSV(s, ",");
    }
    if (!outside) {
        std::ofstream s(outDir + "/connections.csv");
        auto t0 = std::chrono::steady_clock::now();
        pm.outputConnectionsAsCSV(s, ",");
        s.flush();
        t_conn = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    if (contents) {
        FILE* f = fopen((outDir + "/contents.bin").c_str(), "wb");
        if (!cont.empty()) fwrite(cont.data(), sizeof(int), cont.size(), f);
        fclose(f);
    }
    FILE* f = fopen((outDir + "/info.txt").c_str(), "w");
    fprintf(f, "cols %zu\nrows %zu\nnodes %lld\nenumerated %lld\ndropped %lld\noutside %lld\nt_connections %.6f\n", cols, rows,
            nodes, enumerated, dropped, outside, t_conn);
    fclose(f);
    return 0;
}
