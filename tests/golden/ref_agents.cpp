// ref_agents.cpp -- fixture generator only: run by hand through make_golden_agents.py, never by build(), by a
// test or on a GPU machine.
//
// Our own driver, linked against the reference library oracle/_ref/libsalaref.a (compiled by oracle/Makefile).
//   --lines L.csv | --drawing D.graph  --spacing s --fill x,y [--fill ...]
//   --fov f --steps k --seed n --locseed n --timesteps T --rate r --lifetime l --nagents N [--release cx,cy ...]
//   --out DIR
// import -> grid -> fill -> makeGraph, then
//   (1) the agent table, with the reference's own pafrand / prandom / prandomr / invcumpoisson / pickPixel under
//       the engine's two-stream rule: stream 0 seeded --seed gives, per timestep, the count
//       invcumpoisson(prandomr(), rate) and, per agent, its seed (the next pafrand) and with release cells
//       pafrand() % nrelease; stream 1 seeded --locseed repeats pickPixel(prandom(1)) until the cell is filled (a
//       draw of 0 is drawn again).  moves = min(lifetime, timesteps - release timestep).  The first N are kept.
//   (2) per agent of the table: pafsrand(seed), a reference Agent on a SEL_STANDARD AgentSet with OUTPUT_COUNTS,
//       onInit(start, -1), onMove() x moves.  An agent stuck after onInit is not moved (its next look reads bins
//       at a NaN direction).
// Dumps DIR/table.bin int32 [N][3] (start cell x-major, seed, moves), counts.bin uint32 [cols*rows] (the "Gate
// Counts" column), final_cell.bin int32 [N], final_loc.bin float64 [N][2], stuck.bin uint8 [N], trails.bin int32
// [8][lifetime] (the cell after each move of the first 8 agents, -1 beyond their moves), stats.txt (what the
// driver can observe from outside: moves made, looks, moves that stopped).
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
#include "salalib/agents/agent.h"
#include "salalib/agents/agentset.h"
#include "salalib/agents/agenthelpers.h"
#include "genlib/pafmath.h"
#undef protected
#undef private

template <typename T> static void dump(const std::string& path, const std::vector<T>& v) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); exit(2); }
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
    fclose(f);
}

int main(int argc, char** argv) {
    std::string linesCsv, drawing, outDir = ".";
    double spacing = -1, rate = 1.0;
    int fov = 15, steps = 3, timesteps = 400, lifetime = 200, nagents = 256;
    unsigned seed = 0, locseed = 0;
    std::vector<Point2f> fills;
    std::vector<std::pair<int, int>> release;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() { if (i + 1 >= argc) { fprintf(stderr, "missing arg for %s\n", a.c_str()); exit(2); } return std::string(argv[++i]); };
        if (a == "--lines") linesCsv = next();
        else if (a == "--drawing") drawing = next();
        else if (a == "--spacing") spacing = atof(next().c_str());
        else if (a == "--fill") { std::string p = next(); double x, y; sscanf(p.c_str(), "%lf,%lf", &x, &y); fills.push_back(Point2f(x, y)); }
        else if (a == "--release") { std::string p = next(); int x, y; sscanf(p.c_str(), "%d,%d", &x, &y); release.push_back({x, y}); }
        else if (a == "--fov") fov = atoi(next().c_str());
        else if (a == "--steps") steps = atoi(next().c_str());
        else if (a == "--seed") seed = (unsigned)strtoul(next().c_str(), nullptr, 10);
        else if (a == "--locseed") locseed = (unsigned)strtoul(next().c_str(), nullptr, 10);
        else if (a == "--timesteps") timesteps = atoi(next().c_str());
        else if (a == "--rate") rate = atof(next().c_str());
        else if (a == "--lifetime") lifetime = atoi(next().c_str());
        else if (a == "--nagents") nagents = atoi(next().c_str());
        else if (a == "--out") outDir = next();
        else { fprintf(stderr, "unknown arg %s\n", a.c_str()); return 2; }
    }
    MetaGraph mg;
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
    PointMap& pm = mg.getDisplayedPointMap();
    const int cols = (int)pm.getCols(), rows = (int)pm.getRows();

    // (1) the table
    std::vector<int> table;
    pafsrand(seed, 0);
    pafsrand(locseed, 1);
    int n = 0;
    for (int t = 0; t < timesteps && n < nagents; t++) {
        const int q = invcumpoisson(prandomr(0), rate);
        for (int k = 0; k < q; k++) {
            const unsigned as = pafrand(0);
            PixelRef pix;
            if (!release.empty()) {
                const auto& r = release[pafrand(0) % release.size()];
                pix = PixelRef(r.first, r.second);
            } else {
                for (;;) {
                    const double v = prandom(1);
                    if (v == 0.0) continue;
                    pix = pm.pickPixel(v);
                    if (pm.getPoint(pix).filled()) break;
                }
            }
            if (n < nagents) {
                table.push_back(pix.x * rows + pix.y);
                table.push_back((int)as);
                table.push_back(std::min(lifetime, timesteps - t));
            }
            n++;
        }
    }
    n = std::min(n, nagents);
    if (n < nagents) { fprintf(stderr, "only %d agents released\n", n); return 1; }

    // (2) the agents
    AgentSet set;
    set.m_sel_type = AgentProgram::SEL_STANDARD;
    set.m_steps = steps;
    set.m_vbin = (fov == 32) ? -1 : (fov - 1) / 2;   // runmethods.cpp:499-504
    set.m_lifetime = lifetime;
    AttributeTable& at = pm.getAttributeTable();
    const int col = (int)at.getOrInsertColumn(g_col_total_counts);
    std::vector<int> final_cell(n), trails(8 * (size_t)lifetime, -1);
    std::vector<double> final_loc(2 * (size_t)n);
    std::vector<unsigned char> stuck(n);
    long long moves_made = 0, looks = 0, stopped = 0;
    for (int a = 0; a < n; a++) {
        const int cell = table[3 * a], moves = table[3 * a + 2];
        pafsrand((unsigned)table[3 * a + 1], 0);
        Agent ag(&set, &pm, Agent::OUTPUT_COUNTS);
        ag.onInit(PixelRef(cell / rows, cell % rows), -1);
        looks++;
        const bool init_stuck = ag.m_stuck;
        for (int m = 0; m < moves; m++) {
            if (!init_stuck && !ag.m_stuck) {
                ag.m_step = 5;   // (only counted by the reference: a look sets it to 0, the step adds 1)
                ag.onMove();
                if (!ag.m_stuck) {
                    moves_made++;
                    if (ag.m_step == 1) looks++;
                    if (ag.m_stopped) stopped++;
                } else {
                    looks++;
                }
            }
            if (a < 8) trails[(size_t)a * lifetime + m] = ag.m_node.x * rows + ag.m_node.y;
        }
        final_cell[a] = ag.m_node.x * rows + ag.m_node.y;
        final_loc[2 * a] = ag.m_loc.x;
        final_loc[2 * a + 1] = ag.m_loc.y;
        stuck[a] = ag.m_stuck ? 1 : 0;
    }
    std::vector<unsigned> counts((size_t)cols * rows, 0u);
    for (auto it = at.begin(); it != at.end(); ++it) {
        const PixelRef p(it->getKey().value);
        const float v = it->getRow().getValue(col);
        counts[(size_t)p.x * rows + p.y] = v > 0 ? (unsigned)v : 0u;   // a fresh column holds -1
    }
    dump(outDir + "/table.bin", table);
    dump(outDir + "/counts.bin", counts);
    dump(outDir + "/final_cell.bin", final_cell);
    dump(outDir + "/final_loc.bin", final_loc);
    dump(outDir + "/stuck.bin", stuck);
    dump(outDir + "/trails.bin", trails);
    FILE* f = fopen((outDir + "/stats.txt").c_str(), "w");
    fprintf(f, "cols %d\nrows %d\nmoves %lld\nlooks %lld\nstopped %lld\n", cols, rows, moves_made, looks, stopped);
    fclose(f);
    return 0;
}
