// agents_check.cpp -- the agent routine and the release schedule of kernels/agent_step.hpp on the host, one
// thread, over graph arrays read from raw files.  Built and run by tests/test_agents_host.py (and by
// tests/golden/make_golden_agents.py for the per-case counters); plain g++ with -ffp-contract=off.
//
//   agents_check DIR
// reads DIR/meta.txt ("key value" lines: cols rows spacing blx bly nodes nruns fov steps seed locseed timesteps
// rate lifetime nagents ntrail nrelease), state.bin int32 [cols*rows], bins.bin int32 [N][32][4], runs.bin int16
// [R][4], gridconn.bin uint8 [N], release.bin int32 [nrelease]; writes DIR/out_table.bin int32 [n][3],
// out_counts.bin uint32 [cols*rows], out_final_cell.bin int32 [n], out_final_loc.bin float64 [n][2], out_stuck.bin
// uint8 [n], out_trails.bin int32 [ntrail][lifetime], out_counts_split.bin (the counts again, every agent as a first
// part of moves / 3 moves plus a re-run from the start that counts from there), out_stats.txt.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../depthmapx_amd/csrc/kernels/agent_step.hpp"

using namespace dmx;

template <typename T> static std::vector<T> slurp(const std::string& path, size_t n) {
    std::vector<T> v(n);
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { perror(path.c_str()); exit(2); }
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "%s: short read\n", path.c_str()); exit(2); }
    fclose(f);
    return v;
}
template <typename T> static void dump(const std::string& path, const std::vector<T>& v) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); exit(2); }
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: agents_check DIR\n"); return 2; }
    const std::string d = argv[1];
    std::map<std::string, double> m;
    {
        FILE* f = fopen((d + "/meta.txt").c_str(), "r");
        if (!f) { perror("meta.txt"); return 2; }
        char key[64];
        double v;
        while (fscanf(f, "%63s %lf", key, &v) == 2) m[key] = v;
        fclose(f);
    }
    const int cols = (int)m["cols"], rows = (int)m["rows"];
    const size_t C = (size_t)cols * rows, N = (size_t)m["nodes"], R = (size_t)m["nruns"];
    const int fov = (int)m["fov"], steps = (int)m["steps"], lifetime = (int)m["lifetime"];
    const int nagents = (int)m["nagents"], ntrail = (int)m["ntrail"], nrelease = (int)m["nrelease"];
    auto state = slurp<int32_t>(d + "/state.bin", C);
    auto bins = slurp<int32_t>(d + "/bins.bin", N * 128);
    auto runs = slurp<AgentRun>(d + "/runs.bin", R);
    auto gridconn = slurp<uint8_t>(d + "/gridconn.bin", N);
    auto release = slurp<int32_t>(d + "/release.bin", (size_t)nrelease);

    std::vector<int32_t> cell_node(C, -1), filled(C, 0), bin_nruns(N * 32);
    std::vector<uint16_t> bin_count(N * 32);
    std::vector<int64_t> start(N);
    {
        int32_t k = 0;
        for (size_t c = 0; c < C; c++)
            if (state[c] & 2) { cell_node[c] = k++; filled[c] = 1; }   // Point::FILLED
        if ((size_t)k != N) { fprintf(stderr, "filled cells %d != nodes %zu\n", k, N); return 2; }
        int64_t acc = 0;
        for (size_t n = 0; n < N; n++) {
            start[n] = acc;
            for (int b = 0; b < 32; b++) {
                bin_count[n * 32 + b] = (uint16_t)bins[(n * 32 + b) * 4 + 1];
                bin_nruns[n * 32 + b] = bins[(n * 32 + b) * 4 + 3];
                acc += bin_nruns[n * 32 + b];
            }
        }
        if ((size_t)acc != R) { fprintf(stderr, "bins do not account for the runs\n"); return 2; }
    }

    std::vector<int32_t> start_cell(nagents), moves(nagents);
    std::vector<uint32_t> seed(nagents);
    const int64_t total = ag_schedule(cols, rows, filled.data(), (uint32_t)m["seed"], (int)m["timesteps"], m["rate"],
                                      lifetime, release.data(), nrelease, (uint32_t)m["locseed"], start_cell.data(),
                                      seed.data(), moves.data(), nagents);
    if (total < nagents) { fprintf(stderr, "schedule: %lld agents\n", (long long)total); return 1; }

    AgentMap M{};
    M.cols = cols; M.rows = rows;
    M.spacing = m["spacing"]; M.blx = m["blx"]; M.bly = m["bly"];
    M.cell_node = cell_node.data(); M.gridconn = gridconn.data();
    M.bin_count = bin_count.data(); M.bin_nruns = bin_nruns.data();
    M.node_run_start = start.data(); M.pool = runs.data();
    M.vbin = fov == 32 ? -1 : (fov - 1) / 2;
    M.inv_steps = 1.0 / steps;
    M.rc[0] = cos(AG_PI / 4.0); M.rs[0] = sin(AG_PI / 4.0);
    M.rc[1] = cos(-AG_PI / 4.0); M.rs[1] = sin(-AG_PI / 4.0);

    std::vector<uint32_t> counts(C, 0u);
    std::vector<int32_t> table((size_t)nagents * 3), final_cell(nagents), trails((size_t)ntrail * lifetime, -1);
    std::vector<double> final_loc((size_t)nagents * 2);
    std::vector<uint8_t> stuck(nagents);
    AgentStats T{};
    long long flagged = 0;
    for (int a = 0; a < nagents; a++) {
        table[3 * a] = start_cell[a]; table[3 * a + 1] = (int32_t)seed[a]; table[3 * a + 2] = moves[a];
        AgentState S;
        int done = 0;
        // first as the device runs it (stopping at an ambiguous look), to count the agents it would flag ...
        {
            std::vector<uint32_t> scratch(C, 0u);
            AgentStats T2{};
            ag_run_host(M, start_cell[a], seed[a], moves[a], 0, scratch.data(), nullptr, true, S, T2, done);
            if (S.flag) flagged++;
        }
        // ... then to the end
        ag_run_host(M, start_cell[a], seed[a], moves[a], 0, counts.data(),
                    a < ntrail ? trails.data() + (size_t)a * lifetime : nullptr, false, S, T, done);
        final_cell[a] = S.x * rows + S.y;
        final_loc[2 * a] = S.lx; final_loc[2 * a + 1] = S.ly;
        stuck[a] = (uint8_t)S.stuck;
    }
    // the API's re-run of an agent the device stopped after k moves: the device holds the counts of the first k moves,
    // the host run from the start adds those of the later moves only (count_from = k)
    std::vector<uint32_t> split(C, 0u);
    for (int a = 0; a < nagents; a++) {
        const int k = moves[a] / 3;
        AgentState S;
        AgentStats Ts{};
        int done = 0;
        ag_run_host(M, start_cell[a], seed[a], k, 0, split.data(), nullptr, false, S, Ts, done);
        ag_run_host(M, start_cell[a], seed[a], moves[a], k, split.data(), nullptr, false, S, Ts, done);
    }
    dump(d + "/out_counts_split.bin", split);
    dump(d + "/out_table.bin", table);
    dump(d + "/out_counts.bin", counts);
    dump(d + "/out_final_cell.bin", final_cell);
    dump(d + "/out_final_loc.bin", final_loc);
    dump(d + "/out_stuck.bin", stuck);
    dump(d + "/out_trails.bin", trails);
    FILE* f = fopen((d + "/out_stats.txt").c_str(), "w");
    fprintf(f, "moves %lld\nlooks %lld\nfallbacks %lld\ndiag_taken %lld\nstopped %lld\nclamps %lld\nflagged %lld\n",
            T.moves, T.looks, T.fallbacks, T.diag_taken, T.stopped, T.clamps, flagged);
    fclose(f);
    return 0;
}
