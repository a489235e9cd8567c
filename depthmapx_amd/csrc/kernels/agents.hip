// agents.hip -- the agent analysis (standard agents, Gate Counts): every agent of a release table walked from
// its release to its last move (agent_step.hpp: the reference's Agent::onInit / onMove / onStep / onStandardLook
// operation by operation, one LCG stream per agent).
//
// Work model: independent waves; a wave takes 64 agents of the table at a time from one grid counter (progress
// and cancel ride on it, ctl_poll; the cancel word is read again every AG_CANCEL_EVERY moves).  One lane owns one
// agent for the scalar part of a move: the distance test, the turn draw, the step with its pixelate, grid-
// connection test and diagonal tries.  The look is wave-cooperative: lanes with a pending look are served one at
// a time (ballot, broadcast of the owner's node, heading bin and generator state); the 64 lanes load the node's 32
// bin counts and run counts, sum the counts of the look's bins, find the bin of `chosen` by a prefix scan in walk
// order, then load that bin's runs 64 at a time and prefix-scan their cell counts (ag_run_cells, the rule of
// conn_run in connections.hip) to the run and offset of `chosen`.  The owner lane finishes the look (target and
// new heading).  All shuffles sit in wave-uniform control flow.
//
// Counts leave as vector atomicAdd on a uint32 array, one entry per cell, so the result does not depend on the
// order agents are processed in.  An agent whose look is ambiguous (ag_binfromvec) stops there with its flag
// and the number of moves it completed: the API runs it again on the host and adds the counts of the later moves
// (its counters do not enter the kernel's totals: the host run's do).
// Vector stores only; no kernel traps, printf or assert.
#pragma once
#include "agent_step.hpp"
#include "common.hpp"

namespace dmx {

constexpr int AG_THREADS = 256;
constexpr int AG_CANCEL_EVERY = 32;
static_assert(sizeof(AgentRun) == sizeof(Run), "AgentRun is Run");

struct AgentsParams {
    AgentMap M;
    int64_t nagents;
    const int32_t* start_cell;
    const uint32_t* agent_seed;
    const int32_t* moves;
    unsigned int* counts;          // [cols * rows], zeroed by the host
    int32_t* final_cell;           // [n]
    double* final_loc;             // [n][2]
    unsigned char* stuck;          // [n]
    unsigned char* flag;           // [n] AG_FLAG_*
    int32_t* done_moves;           // [n] moves completed (all of them unless flagged)
    int32_t* trail;                // [ntrail][trail_stride] preset to -1, or null
    int64_t ntrail;
    int trail_stride;
    int* work_counter;
    DmxCtl* ctl;
    unsigned long long* stats;     // [0..5] moves, looks, fallbacks, diagonal steps taken, moves stopped, bins clamped
};

__device__ __forceinline__ uint64_t ag_shfl64(uint64_t v, int src) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)(v & 0xFFFFFFFFull), src);
    const unsigned hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ int ag_wave_sum(int v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ int ag_wave_incl(int v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const int a = __shfl_up(v, d);
        if (lane >= d) v += a;
    }
    return v;
}

// onStandardLook for the agent of lane src, by the whole wave (called in wave-uniform control flow).  bfv: each
// lane's binfromvec(m_vector), read from src; whole: the first pass already takes the whole isovist (onInit).
__device__ __forceinline__ void ag_look_wave(const AgentMap& M, AgentState& S, AgentStats& T, int lane, int src,
                                             int bfv_mine, bool whole) {
    const bool owner = lane == src;
    const int ax = __shfl(S.x, src), ay = __shfl(S.y, src);
    const int bfv = __shfl(bfv_mine, src);
    if (owner) T.looks++;
    const int64_t k = M.cell_node[ax * M.rows + ay];
    if (k < 0) {
        if (owner) ag_look_stuck(S);
        return;
    }
    const int cnt = lane < 32 ? (int)M.bin_count[k * 32 + lane] : 0;
    const int nrn = lane < 32 ? M.bin_nruns[k * 32 + lane] : 0;
    int directionbin = 0, nb = 0, choices = 0;
    for (int pass = 0; pass < 2; pass++) {
        ag_look_range(whole ? -1 : M.vbin, pass == 1, bfv, directionbin, nb);
        const int pos = (lane - directionbin) & 31;   // this lane's bin in walk order
        choices = ag_wave_sum((lane < 32 && pos < nb) ? cnt : 0);
        if (choices) break;
        if (pass == 0 && owner) T.fallbacks++;
    }
    if (!choices) {
        if (owner) ag_look_stuck(S);
        return;
    }
    uint64_t rng = ag_shfl64(S.rng, src);
    int chosen = (int)(ag_pafrand(rng) % (uint32_t)choices);
    if (owner) S.rng = rng;
    // the bin of chosen: lane i holds the i-th bin of the walk
    const int bi = (directionbin + lane) & 31;
    int ci = __shfl(cnt, bi);
    if (lane >= nb) ci = 0;
    const int incl = ag_wave_incl(ci, lane);
    const int wl = __ffsll((long long)__ballot(incl > chosen)) - 1;   // exists: chosen < choices
    const int b = __shfl(bi, wl);
    chosen -= __shfl(incl - ci, wl);
    // the bin's runs
    const int64_t r0 = M.node_run_start[k] + ag_wave_sum(lane < b ? nrn : 0);
    const int nr = __shfl(nrn, b);
    if (nr <= 0) {
        if (owner) { T.clamps++; ag_look_stuck(S); }
        return;
    }
    int cx = 0, cy = 0;
    bool found = false;
    for (int rr = 0; rr < nr; rr += 64) {
        const int r = rr + lane;
        AgentRun ru{0, 0, 0, 0};
        int n = 0;
        if (r < nr) {
            ru = M.pool[r0 + r];
            n = ag_run_cells(ru, b);
        }
        const int ri = ag_wave_incl(n, lane);
        const int total = __shfl(ri, 63);
        if (chosen < total) {
            const int w = __ffsll((long long)__ballot(ri > chosen)) - 1;
            int tx = 0, ty = 0;
            ag_run_cell(ru, b, chosen - (ri - n), tx, ty);   // meaningful in lane w
            cx = __shfl(tx, w);
            cy = __shfl(ty, w);
            found = true;
            break;
        }
        chosen -= total;
    }
    if (!found) {
        const AgentRun ru = M.pool[r0 + nr - 1];
        ag_run_cell(ru, b, ag_run_cells(ru, b) - 1, cx, cy);
        if (owner) T.clamps++;
    }
    if (owner) ag_look_target(M, S, cx, cy);
}

__device__ __forceinline__ void ag_serve_looks(const AgentMap& M, AgentState& S, AgentStats& T, int lane, bool need,
                                               int bfv, bool whole) {
    unsigned long long pending = __ballot(need);
    while (pending) {
        const int src = __ffsll((long long)pending) - 1;
        ag_look_wave(M, S, T, lane, src, bfv, whole);
        pending &= pending - 1;
    }
}

__global__ void __launch_bounds__(AG_THREADS) agents_kernel(AgentsParams P) {
    const AgentMap& M = P.M;
    const int lane = threadIdx.x & 63;
    AgentStats T{0, 0, 0, 0, 0, 0};
    for (;;) {
        int w = 0;
        if (lane == 0) w = ctl_poll(P.ctl, atomicAdd(P.work_counter, 1));
        w = __shfl(w, 0);
        const int64_t a = (int64_t)w * 64 + lane;
        if ((int64_t)w * 64 >= P.nagents) break;
        const bool active = a < P.nagents;
        AgentState S;
        AgentStats Ta{0, 0, 0, 0, 0, 0};   // this agent's; they enter the totals unless the host runs the agent again
        int mymoves = 0, done = 0;
        {
            bool need = false;
            int bfv = 0;
            if (active) {
                mymoves = P.moves[a];
                ag_init_begin(M, S, P.start_cell[a], P.agent_seed[a]);
                int fl = 0;
                bfv = ag_binfromvec(S.vx, S.vy, fl);
                if (fl) S.flag |= fl;
                else need = true;
            } else {
                ag_init_begin(M, S, 0, 0u);
            }
            ag_serve_looks(M, S, Ta, lane, need, bfv, true);
            if (active && !S.flag) ag_init_end(S);
        }
        int maxm = mymoves;
        for (int off = 32; off >= 1; off >>= 1) maxm = max(maxm, __shfl_xor(maxm, off));
        bool cancelled = false;
        for (int m = 0; m < maxm; m++) {
            if (P.ctl && (m % AG_CANCEL_EVERY) == AG_CANCEL_EVERY - 1) {
                int c = 0;
                if (lane == 0) c = __hip_atomic_load(&P.ctl->cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if (__shfl(c, 0)) { cancelled = true; break; }
            }
            const bool mine = active && m < mymoves;
            bool live = mine && !S.stuck && !S.flag;
            bool need = false;
            int bfv = 0;
            if (live && ag_move_wants_look(M, S)) {
                int fl = 0;
                bfv = ag_binfromvec(S.vx, S.vy, fl);
                if (fl) { S.flag |= fl; live = false; }
                else need = true;
            }
            ag_serve_looks(M, S, Ta, lane, need, bfv, false);
            if (live) {
                if (!S.stuck && ag_step(M, S, Ta)) atomicAdd(&P.counts[S.x * M.rows + S.y], 1u);
                done = m + 1;
            }
            if (mine && P.trail && a < P.ntrail && m < P.trail_stride)
                P.trail[a * P.trail_stride + m] = S.x * M.rows + S.y;
        }
        if (cancelled) break;
        if (active && !(S.flag & AG_FLAG_AMBIGUOUS)) {
            T.moves += Ta.moves; T.looks += Ta.looks; T.fallbacks += Ta.fallbacks;
            T.diag_taken += Ta.diag_taken; T.stopped += Ta.stopped; T.clamps += Ta.clamps;
        }
        if (active) {
            if (S.stuck) done = mymoves;
            P.final_cell[a] = S.x * M.rows + S.y;
            P.final_loc[2 * a] = S.lx;
            P.final_loc[2 * a + 1] = S.ly;
            P.stuck[a] = (unsigned char)S.stuck;
            P.flag[a] = (unsigned char)S.flag;
            P.done_moves[a] = done;
        }
    }
    long long v[6] = {T.moves, T.looks, T.fallbacks, T.diag_taken, T.stopped, T.clamps};
    for (int i = 0; i < 6; i++) {
        for (int off = 32; off >= 1; off >>= 1) v[i] += __shfl_xor(v[i], off);
        if (lane == 0 && v[i]) atomicAdd(&P.stats[i], (unsigned long long)v[i]);
    }
}

} // namespace dmx
