// agent_step.hpp -- one standard agent of the agent analysis (salalib/agents/agent.cpp: Agent::onInit :29-58,
// onMove :60-112, onStep / diagonalStep / goodStep :121-197, onStandardLook :238-282, for an AgentSet of
// SEL_STANDARD) over the run-length graph, shared by the kernel (agents.hip), the host re-run of flagged agents
// (api/agents.hip) and a stand-alone host check (tests/agents/agents_check.cpp).
//
// The agent is the reference's, operation by operation (-ffp-contract=off: no a*b+c contraction on either side):
//   * pafrand / prandom / prandomr (genlib/pafmath.cpp:24-54, pafmath.h:52-56) over one 64-bit LCG state PER AGENT,
//     started as pafsrand(seed) starts the reference's global one.  Agents never interact, so an agent with its own
//     stream walks exactly the path the reference's Agent walks after pafsrand(seed).
//   * Point2f::normalise is scale(1.0 / length()) (p2dpoly.h:119-129): a multiply by the reciprocal.
//   * PointMap::pixelate(p, false) (pointdata.cpp:263-283) and depixelate (pointdata.h:353-357) in their order.
//   * rotate(+-pi/4) (p2dpoly.h:130-135) with cos / sin of the constant taken once on the host (AgentMap::rc, rs).
//   * binfromvec (agent.h:105) over Point2f::angle (p2dpoly.h:136) needs acos, whose last bit may differ between
//     the device's and the host's libm.  That matters only within rounding of a bin boundary, so a look whose
//     scaled angle lies within AG_AMB_EPS of an integer raises AG_FLAG_AMBIGUOUS (the device stops the agent there,
//     the API runs it again on the host); an acos argument that is not finite or outside [-1, 1] raises
//     AG_FLAG_NAN and ends the agent on both sides (the reference converts a NaN to int there: undefined).
//
// Defined here where the reference is not:
//   * an agent whose look finds no cell even in the whole isovist is stuck for good: it makes no further step and
//     counts nothing (the reference's stuck agent returns from onMove before stepping, so its counts agree; its
//     next look reads bins at a NaN direction);
//   * a `chosen` beyond the cells a bin's runs enumerate (a re-read map whose runs the 4-bit shift or the 16-bit
//     count dropped) takes the bin's last cell and is counted in AgentStats::clamps; a bin with a count and no run
//     at all leaves the agent stuck;
//   * a step whose destination is not a finite coordinate is a step out of the grid.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define DMX_AG_HD __host__ __device__ inline
#else
#define DMX_AG_HD inline
#endif

namespace dmx {

constexpr double AG_PI = 3.14159265358979323846;   // M_PI
constexpr double AG_AMB_EPS = 1e-9;
constexpr uint64_t AG_MULT = 0x71A7FA85ull, AG_CONST = 0xF5E958B9ull;   // g_mult, g_const
constexpr uint32_t AG_RAND_MAX = 0x0FFFFFFFu;                            // PAF_RAND_MAX
enum { AG_FLAG_AMBIGUOUS = 1, AG_FLAG_NAN = 2 };

// layout of kernels/common.hpp's Run
struct AgentRun {
    int16_t x0, y0, x1, y1;
};

struct AgentMap {
    int cols, rows;
    double spacing, blx, bly;
    const int32_t* cell_node;        // [cols * rows] x-major cell -> node, -1: not FILLED
    const uint8_t* gridconn;         // [N]
    const uint16_t* bin_count;       // [N][32] Bin::m_node_count as stored
    const int32_t* bin_nruns;        // [N][32]
    const int64_t* node_run_start;   // [N]
    const AgentRun* pool;
    int vbin;                        // AgentProgram::m_vbin (-1: the whole isovist)
    double inv_steps;                // 1.0 / m_steps
    double rc[2], rs[2];             // cos, sin of +pi/4 and of -pi/4
    // host only (null on the device and where pool is a host array): the runs [r0, r0 + nr) of one bin, fetched on
    // demand instead of read from pool -- the API's re-run of a flagged agent reads the device's run pool this way
    const AgentRun* (*fetch_runs)(void* user, int64_t r0, int nr);
    void* fetch_user;
};

struct AgentState {
    uint64_t rng;
    int x, y;             // m_node
    double lx, ly;        // m_loc
    double tx, ty;        // m_target
    double vx, vy;        // m_vector
    int stuck, flag;
};

struct AgentStats {
    long long moves, looks, fallbacks, diag_taken, stopped, clamps;
};

DMX_AG_HD uint32_t ag_pafrand(uint64_t& s) {
    s = AG_MULT * s + AG_CONST;
    return (uint32_t)((s >> 32) & AG_RAND_MAX);
}
DMX_AG_HD double ag_prandom(uint64_t& s) { return double(ag_pafrand(s)) / double(AG_RAND_MAX); }
DMX_AG_HD double ag_prandomr(uint64_t& s) { return double(ag_pafrand(s)) / double(AG_RAND_MAX + 1u); }

// direction of bin b (Node::make, ngraph.cpp:43-54): 0 horizontal, 1 vertical, 2 along (+1,+1), 3 along (+1,-1)
DMX_AG_HD int ag_bin_dir(int b) {
    if (b == 4 || b == 20) return 2;
    if (b == 12 || b == 28) return 3;
    if ((b > 4 && b < 12) || (b > 20 && b < 28)) return 1;
    return 0;
}
// cells Bin::first() .. next() yield for one run of bin b (ngraph.cpp:392-406): the start, then steps until the
// moved cursor's col(dir) passes the end's -- never fewer than one
DMX_AG_HD int ag_run_cells(AgentRun ru, int b) {
    const int span = (ag_bin_dir(b) == 1) ? ((int)ru.y1 - (int)ru.y0) : ((int)ru.x1 - (int)ru.x0);
    return span > 0 ? span + 1 : 1;
}
// cell i of the run
DMX_AG_HD void ag_run_cell(AgentRun ru, int b, int i, int& cx, int& cy) {
    const int dir = ag_bin_dir(b);
    cx = ru.x0 + ((dir == 1) ? 0 : i);
    cy = ru.y0 + ((dir == 0) ? 0 : ((dir == 3) ? -i : i));
}

// binfromvec(m_vector); flag: see the header
DMX_AG_HD int ag_binfromvec(double vx, double vy, int& flag) {
    if (!(vx >= -1.0 && vx <= 1.0)) {
        flag |= AG_FLAG_NAN;
        return 0;
    }
    const double a = (vy < 0) ? (2.0 * AG_PI - acos(vx)) : acos(vx);
    const double v = 32.0 * (0.5 * a / AG_PI) + 0.5;
    if (fabs(v - rint(v)) < AG_AMB_EPS) flag |= AG_FLAG_AMBIGUOUS;
    return int(v);
}

// first bin and number of bins of a look (onStandardLook :239-250)
DMX_AG_HD void ag_look_range(int vbin_prog, bool whole, int bfv, int& directionbin, int& nb) {
    int vbin = vbin_prog;
    if (whole || vbin == -1) vbin = 16;
    directionbin = 32 + bfv - vbin;
    nb = vbin * 2 + 1;
    if (nb > 32) nb = 32;
}

// the look found cell (cx, cy): m_target and the new m_vector (:278-281)
DMX_AG_HD void ag_look_target(const AgentMap& M, AgentState& S, int cx, int cy) {
    S.tx = M.blx + M.spacing * double(cx);
    S.ty = M.bly + M.spacing * double(cy);
    double dx = S.tx - S.lx, dy = S.ty - S.ly;
    const double s = 1.0 / sqrt(dx * dx + dy * dy);
    S.vx = dx * s;
    S.vy = dy * s;
}
// the look found nothing (:257-261)
DMX_AG_HD void ag_look_stuck(AgentState& S) {
    S.stuck = 1;
    S.tx = S.lx;
    S.ty = S.ly;
    S.vx = 0.0;
    S.vy = 0.0;
}

// onStandardLook, one thread.  bfv = binfromvec(m_vector), taken by the caller (who stops on its flag).
DMX_AG_HD void ag_look(const AgentMap& M, AgentState& S, int bfv, AgentStats& T) {
    T.looks++;
    const int c = S.x * M.rows + S.y;
    const int64_t k = M.cell_node[c];
    if (k < 0) {
        ag_look_stuck(S);
        return;
    }
    const uint16_t* cnt = M.bin_count + k * 32;
    int directionbin = 0, nb = 0, choices = 0;
    for (int pass = 0; pass < 2; pass++) {
        ag_look_range(M.vbin, pass == 1, bfv, directionbin, nb);
        choices = 0;
        for (int i = 0; i < nb; i++) choices += cnt[(directionbin + i) % 32];
        if (choices) break;
        if (pass == 0) T.fallbacks++;
    }
    if (!choices) {
        ag_look_stuck(S);
        return;
    }
    int chosen = (int)(ag_pafrand(S.rng) % (uint32_t)choices);
    for (; chosen >= cnt[directionbin % 32]; directionbin++) chosen -= cnt[directionbin % 32];
    const int b = directionbin % 32;
    const int32_t* bnr = M.bin_nruns + k * 32;
    int64_t r0 = M.node_run_start[k];
    for (int i = 0; i < b; i++) r0 += bnr[i];
    const int nr = bnr[b];
    if (nr <= 0) {
        T.clamps++;
        ag_look_stuck(S);
        return;
    }
#if !defined(__HIP_DEVICE_COMPILE__)
    const AgentRun* runs = M.fetch_runs ? M.fetch_runs(M.fetch_user, r0, nr) : M.pool + r0;
#else
    const AgentRun* runs = M.pool + r0;
#endif
    int cx = 0, cy = 0;
    bool found = false;
    for (int r = 0; r < nr && !found; r++) {
        const AgentRun ru = runs[r];
        const int n = ag_run_cells(ru, b);
        if (chosen < n) {
            ag_run_cell(ru, b, chosen, cx, cy);
            found = true;
        } else {
            chosen -= n;
        }
    }
    if (!found) {
        const AgentRun ru = runs[nr - 1];
        ag_run_cell(ru, b, ag_run_cells(ru, b) - 1, cx, cy);
        T.clamps++;
    }
    ag_look_target(M, S, cx, cy);
}

// PointMap::pixelate(p, false), one coordinate; a coordinate that is not finite or far outside lands outside
DMX_AG_HD int ag_pixelate(double p, double bl, double spacing, int n) {
    const double f = floor((p - bl + (spacing / 2.0)) / spacing);
    if (!(f >= -1.0 && f <= double(n))) return -1;
    return int(f);
}

// goodStep: the destination lies in the grid and the current cell's grid connection towards it is set
// (connectValue, agent.h:129-139; a destination equal to the current cell tests CONNECT_W, as the reference does)
DMX_AG_HD bool ag_good_step(const AgentMap& M, const AgentState& S, int nx, int ny) {
    if (nx < 0 || nx >= M.cols || ny < 0 || ny >= M.rows) return false;
    const int dx = nx - S.x, dy = ny - S.y;
    int bit;
    if (dy > 0) bit = 0x02 << (1 - dx);
    else if (dy < 0) bit = 0x20 << (dx + 1);
    else if (dx == 1) bit = 0x01;
    else bit = 0x10;
    const int32_t k = M.cell_node[S.x * M.rows + S.y];
    const int gc = k >= 0 ? M.gridconn[k] : 0;
    return (gc & bit & 0xFF) != 0;
}

// the start of onMove (:60-84) up to the look: true when the agent looks in this move
DMX_AG_HD bool ag_move_wants_look(const AgentMap& M, AgentState& S) {
    const double ddx = S.lx - S.tx, ddy = S.ly - S.ty;
    if (sqrt(ddx * ddx + ddy * ddy) < M.spacing) return true;
    return ag_prandomr(S.rng) < M.inv_steps;
}

// onStep and what onMove does after it: true when the agent entered a new cell that is FILLED (to be counted)
DMX_AG_HD bool ag_step(const AgentMap& M, AgentState& S, AgentStats& T) {
    T.moves++;
    const int ox = S.x, oy = S.y;
    const double nlx = S.lx + (M.spacing * S.vx), nly = S.ly + (M.spacing * S.vy);
    const int nx = ag_pixelate(nlx, M.blx, M.spacing, M.cols), ny = ag_pixelate(nly, M.bly, M.spacing, M.rows);
    if (nx != S.x || ny != S.y) {
        if (ag_good_step(M, S, nx, ny)) {
            S.x = nx; S.y = ny;
            S.lx = nlx; S.ly = nly;
        } else {
            // diagonalStep
            double l1x, l1y, l2x, l2y;
            int n1x, n1y, n2x, n2y;
            {
                const double x = S.vx * M.rc[0] - S.vy * M.rs[0], y = S.vy * M.rc[0] + S.vx * M.rs[0];
                l1x = S.lx + (M.spacing * x); l1y = S.ly + (M.spacing * y);
                n1x = ag_pixelate(l1x, M.blx, M.spacing, M.cols); n1y = ag_pixelate(l1y, M.bly, M.spacing, M.rows);
            }
            {
                const double x = S.vx * M.rc[1] - S.vy * M.rs[1], y = S.vy * M.rc[1] + S.vx * M.rs[1];
                l2x = S.lx + (M.spacing * x); l2y = S.ly + (M.spacing * y);
                n2x = ag_pixelate(l2x, M.blx, M.spacing, M.cols); n2y = ag_pixelate(l2y, M.bly, M.spacing, M.rows);
            }
            const bool first1 = ag_pafrand(S.rng) % 2 == 0;
            int take = 0;
            if (first1) {
                if (ag_good_step(M, S, n1x, n1y)) take = 1;
                else if (ag_good_step(M, S, n2x, n2y)) take = 2;
            } else {
                if (ag_good_step(M, S, n2x, n2y)) take = 2;
                else if (ag_good_step(M, S, n1x, n1y)) take = 1;
            }
            if (take == 1) { S.x = n1x; S.y = n1y; S.lx = l1x; S.ly = l1y; }
            else if (take == 2) { S.x = n2x; S.y = n2y; S.lx = l2x; S.ly = l2y; }
            if (take) T.diag_taken++;
            else T.stopped++;
        }
    } else {
        S.lx = nlx; S.ly = nly;
    }
    return (S.x != ox || S.y != oy) && M.cell_node[S.x * M.rows + S.y] >= 0;
}

// onInit up to its look (the caller looks at the whole isovist, then calls ag_init_end)
DMX_AG_HD void ag_init_begin(const AgentMap& M, AgentState& S, int cell, uint32_t seed) {
    S.rng = seed;
    S.x = cell / M.rows; S.y = cell % M.rows;
    S.lx = M.blx + M.spacing * double(S.x);
    S.ly = M.bly + M.spacing * double(S.y);
    S.tx = 0.0; S.ty = 0.0;
    S.vx = 1.0; S.vy = 0.0;
    S.stuck = 0; S.flag = 0;
}
// m_vector.normalise() after the look
DMX_AG_HD void ag_init_end(AgentState& S) {
    const double s = 1.0 / sqrt(S.vx * S.vx + S.vy * S.vy);
    S.vx *= s;
    S.vy *= s;
}

// Host only from here.
// One agent from its release to its last move on one thread: the host routine.  counts [cols * rows] is added to
// from move `count_from` on (the API's re-run of an agent the device stopped after that many moves); trail
// [moves] or null receives the cell after each move.  ambiguous_stops: stop at an ambiguous look as the device does.
inline void ag_run_host(const AgentMap& M, int cell, uint32_t seed, int moves, int count_from, uint32_t* counts,
                        int32_t* trail, bool ambiguous_stops, AgentState& S, AgentStats& T, int& done_moves) {
    ag_init_begin(M, S, cell, seed);
    done_moves = 0;
    auto look = [&](bool whole_first) {
        int fl = 0;
        const int bfv = ag_binfromvec(S.vx, S.vy, fl);
        if ((fl & AG_FLAG_NAN) || (ambiguous_stops && fl)) {
            S.flag |= fl;
            return false;
        }
        if (whole_first) {
            AgentMap W = M;
            W.vbin = -1;
            ag_look(W, S, bfv, T);
        } else {
            ag_look(M, S, bfv, T);
        }
        return true;
    };
    if (look(true)) ag_init_end(S);
    for (int m = 0; m < moves; m++) {
        if (!S.stuck && !S.flag) {
            bool ok = true;
            if (ag_move_wants_look(M, S)) ok = look(false);
            if (ok && !S.stuck && ag_step(M, S, T) && m >= count_from) counts[S.x * M.rows + S.y]++;
            if (ok) done_moves = m + 1;
        }
        if (trail) trail[m] = S.x * M.rows + S.y;
    }
    if (S.stuck) done_moves = moves;
}

// invcumpoisson (genlib/pafmath.cpp:76-91)
inline int ag_invcumpoisson(double p, double lambda) {
    if (p <= 0) return 0;
    if (p >= 1) p = 1 - 1e-9;
    double f = exp(-lambda);
    int i = 0;
    for (double c = f; c < p; c += f) {
        i++;
        f *= lambda / double(i);
    }
    return i;
}

// The release ensemble (AgentEngine::run :66-84, AgentSet::init :28-40) with streams of its own: `seed` drives
// the per-timestep count invcumpoisson(prandomr(), rate), then per agent its seed (the next pafrand) and, with
// release cells, pafrand() % nrelease; without, a stream seeded `locseed` repeats pickPixel(prandom())
// (pointdata.cpp:1771-1775) until the cell is FILLED (a draw of exactly 0, where the reference indexes cell -1,
// is drawn again).  moves = min(lifetime, timesteps - release timestep).  Returns the number of agents; writes
// the first cap.  -1: a release cell outside the grid or not FILLED; -2: no FILLED cell to pick.
inline int64_t ag_schedule(int cols, int rows, const int32_t* state_filled /* [cols*rows] != 0: FILLED */,
                           uint32_t seed, int timesteps, double rate, int lifetime, const int32_t* release,
                           int64_t nrelease, uint32_t locseed, int32_t* start_cell, uint32_t* agent_seed,
                           int32_t* moves, int64_t cap) {
    const int64_t C = (int64_t)cols * rows;
    for (int64_t i = 0; i < nrelease; i++)
        if (release[i] < 0 || release[i] >= C || !state_filled[release[i]]) return -1;
    if (nrelease == 0) {
        bool any = false;
        for (int64_t c = 0; c < C && !any; c++) any = state_filled[c] != 0;
        if (!any) return -2;
    }
    uint64_t S = seed, L = locseed;
    int64_t n = 0;
    for (int t = 0; t < timesteps; t++) {
        const int q = ag_invcumpoisson(ag_prandomr(S), rate);
        for (int k = 0; k < q; k++) {
            const uint32_t as = ag_pafrand(S);
            int32_t cell;
            if (nrelease) {
                cell = release[ag_pafrand(S) % (uint64_t)nrelease];
            } else {
                for (;;) {
                    const double v = ag_prandom(L);
                    if (v == 0.0) continue;
                    const int which = (int)ceil(v * double(rows) * double(cols)) - 1;
                    const int px = which % cols, py = which / cols;
                    if (py >= rows) continue;
                    cell = px * rows + py;
                    if (state_filled[cell]) break;
                }
            }
            if (n < cap) {
                start_cell[n] = cell;
                agent_seed[n] = as;
                moves[n] = lifetime < timesteps - t ? lifetime : timesteps - t;
            }
            n++;
        }
    }
    return n;
}

} // namespace dmx
