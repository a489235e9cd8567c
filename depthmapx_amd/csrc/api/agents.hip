// api/agents.hip -- the agent analysis (dmx_agent_schedule, dmx_agents, dmx_ctx_last_agents; kernels/agents.hip,
// kernels/agent_step.hpp).
// Part of the dmx_api.hip unity build: included inside its extern "C" block, after the context and the
// internal types (dmx_ctx, dmx_pointmap, dmx_graph); not compiled on its own.

int dmx_agent_schedule(const dmx_pointmap* pm, uint32_t seed, int32_t timesteps, double release_rate, int32_t lifetime,
                       const int32_t* release_cells, int64_t nrelease, int32_t locseed, int32_t* start_cell,
                       uint32_t* agent_seed, int32_t* moves, int64_t cap, int64_t* nagents) {
    if (!pm || !nagents || timesteps < 0 || lifetime < 0 || nrelease < 0 || cap < 0 || (nrelease && !release_cells) ||
        (cap && (!start_cell || !agent_seed || !moves)))
        return fail(DMX_ERR_ARG, "bad arguments");
    if (!(release_rate >= 0.0) || release_rate > 700.0)   // exp(-rate) must stay a normal number
        return fail(DMX_ERR_ARG, "release rate out of range");
    const PointMapHost& h = *pm->host;
    const auto& st = h.state();
    std::vector<int32_t> filled(st.size());
    for (size_t c = 0; c < st.size(); c++) filled[c] = (st[c] & CELL_FILLED) ? 1 : 0;
    const int64_t n = ag_schedule(h.cols(), h.rows(), filled.data(), seed, timesteps, release_rate, lifetime,
                                  release_cells, nrelease, (uint32_t)locseed, start_cell, agent_seed, moves, cap);
    if (n == -1) return fail(DMX_ERR_ARG, "a release cell is outside the grid or not filled");
    if (n == -2) return fail(DMX_ERR_STATE, "the map has no filled cell to release agents on");
    *nagents = n;
    return DMX_OK;
}

// the runs of one bin for the host re-run of a flagged agent, copied from the device's pool when the look needs them
struct AgentRunFetch {
    hipStream_t s;
    const Run* pool;
    std::vector<AgentRun> buf;
    hipError_t err = hipSuccess;
};
static const AgentRun* agent_fetch_runs(void* user, int64_t r0, int nr) {
    AgentRunFetch& F = *(AgentRunFetch*)user;
    F.buf.assign((size_t)std::max(nr, 1), AgentRun{0, 0, 0, 0});
    if (nr > 0 && F.err == hipSuccess) F.err = copy_sync(F.s, F.buf.data(), F.pool + r0, (size_t)nr * 8, hipMemcpyDeviceToHost);
    return F.buf.data();
}

int dmx_agents(dmx_ctx* ctx, dmx_graph* g, int32_t vbin, int32_t steps, int64_t nagents, const int32_t* start_cell,
               const uint32_t* agent_seed, const int32_t* moves, uint32_t* counts, int32_t* final_cell,
               double* final_loc, uint8_t* stuck, int32_t* trail, int64_t ntrail) {
    SAME_DEVICE(ctx, g);
    release_sym_scatter(g);
    if (!ctx || !g || !counts || nagents < 0 || ntrail < 0 || (nagents && (!start_cell || !agent_seed || !moves)))
        return fail(DMX_ERR_ARG, "bad arguments");
    if (vbin < -1 || vbin > 16) return fail(DMX_ERR_ARG, "vbin must be -1 (the whole isovist) or 0 .. 16");
    if (steps < 1) return fail(DMX_ERR_ARG, "steps must be at least 1");
    if (g->node_begin != 0 || g->node_end != g->nnodes)
        return fail(DMX_ERR_STATE, "agents need the whole graph (assemble the shards first)");
    if (nagents >= ((int64_t)1 << 31)) return fail(DMX_ERR_UNSUPPORTED, "agents: more than 2^31 agents in one call");
    HIPCHK(hipSetDevice(ctx->device));
    PointMapHost& h = *g->pm->host;
    const int cols = h.cols(), rows = h.rows();
    const int64_t C = (int64_t)cols * rows, N = g->nnodes;
    if (!g->pm->d_cell_node.p || g->pm->nnodes != N) return fail(DMX_ERR_STATE, "the graph's map is not on the device");
    const auto& st = h.state();
    int maxmoves = 0;
    for (int64_t a = 0; a < nagents; a++) {
        if (start_cell[a] < 0 || start_cell[a] >= C || !(st[start_cell[a]] & CELL_FILLED))
            return fail(DMX_ERR_ARG, "an agent starts outside the grid or on a cell that is not filled");
        if (moves[a] < 0) return fail(DMX_ERR_ARG, "negative number of moves");
        maxmoves = std::max(maxmoves, moves[a]);
    }
    ntrail = trail ? std::min(ntrail, nagents) : 0;
    ctx->last_agents_s = ctx->last_agents_host_s = 0;
    for (auto& v : ctx->last_agents) v = 0;
    hipStream_t s = ctx->stream;
    const int64_t na = std::max<int64_t>(nagents, 1);
    DevBuf<int32_t> d_start, d_moves, d_final, d_done, d_trail;
    DevBuf<uint32_t> d_seed, d_counts;
    DevBuf<double> d_loc;
    DevBuf<unsigned char> d_stuck, d_flag;
    HIPCHK(d_start.alloc(na)); HIPCHK(d_moves.alloc(na)); HIPCHK(d_seed.alloc(na));
    HIPCHK(d_final.alloc(na)); HIPCHK(d_done.alloc(na)); HIPCHK(d_loc.alloc(2 * na));
    HIPCHK(d_stuck.alloc(na)); HIPCHK(d_flag.alloc(na));
    HIPCHK(d_counts.alloc(std::max<int64_t>(C, 1)));
    const size_t ntr = (size_t)ntrail * (size_t)maxmoves;
    HIPCHK(d_trail.alloc(std::max<size_t>(ntr, 1)));
    HIPCHK(hipMemsetAsync(d_counts.p, 0, (size_t)std::max<int64_t>(C, 1) * 4, s));
    HIPCHK(hipMemsetAsync(d_trail.p, 0xFF, std::max<size_t>(ntr, 1) * 4, s));
    HIPCHK(hipMemsetAsync(ctx->counters.p, 0, 16 * sizeof(int), s));
    HIPCHK(hipMemsetAsync(ctx->stats.p, 0, 32 * sizeof(unsigned long long), s));
    if (nagents) {
        HIPCHK(hipMemcpyAsync(d_start.p, start_cell, (size_t)nagents * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_moves.p, moves, (size_t)nagents * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_seed.p, agent_seed, (size_t)nagents * 4, hipMemcpyHostToDevice, s));
    }
    AgentsParams P{};
    AgentMap& M = P.M;
    M.cols = cols; M.rows = rows;
    M.spacing = h.spacing(); M.blx = h.bottom_left().x; M.bly = h.bottom_left().y;
    M.cell_node = g->pm->d_cell_node.p;
    M.gridconn = g->gridconn.p; M.bin_count = g->bin_count.p; M.bin_nruns = g->bin_nruns.p;
    M.node_run_start = g->node_run_start.p; M.pool = (const AgentRun*)g->pool.p;
    M.vbin = vbin;
    M.inv_steps = 1.0 / steps;
    // the +-pi/4 rotations of diagonalStep: cos and sin of the constant, the host's
    M.rc[0] = cos(AG_PI / 4.0); M.rs[0] = sin(AG_PI / 4.0);
    M.rc[1] = cos(-AG_PI / 4.0); M.rs[1] = sin(-AG_PI / 4.0);
    P.nagents = nagents;
    P.start_cell = d_start.p; P.agent_seed = d_seed.p; P.moves = d_moves.p;
    P.counts = d_counts.p; P.final_cell = d_final.p; P.final_loc = d_loc.p; P.stuck = d_stuck.p; P.flag = d_flag.p;
    P.done_moves = d_done.p;
    P.trail = ntr ? d_trail.p : nullptr; P.ntrail = ntrail; P.trail_stride = maxmoves;
    P.work_counter = ctx->counters.p; P.ctl = ctx->d_ctl; P.stats = ctx->stats.p;
    const int64_t nchunks = (nagents + 63) / 64;
    // A/B hook (measurements; tests of the re-run path): no kernel, every agent through the host
    // re-run on one thread.  Such a call shows in dmx_ctx_last_agents: every agent is counted as run again on the
    // host, and the kernel seconds are those of an empty span.
    // "lazy": with the run pool read on demand, as for a flagged agent; else with the whole pool downloaded first
    // (the host routine's own speed).
    const char* hook_v = policy::hook("DMX_AGENTS_HOST");
    const bool host_all = hook_v != nullptr;
    const bool lazy_pool = !host_all || !std::strcmp(hook_v, "lazy");
    HIPCHK(hipEventRecord(ctx->ev0, s));
    if (nagents && !host_all) {
        const int wpb = AG_THREADS / 64;
        const int64_t nb = std::max<int64_t>(1, std::min<int64_t>((nchunks + wpb - 1) / wpb, (int64_t)ctx->num_cu * 8));
        hipLaunchKernelGGL(agents_kernel, dim3((unsigned)nb), dim3(AG_THREADS), 0, s, P);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ctx->ev1, s));
    ctx->h_ctl->progress = 0;
    HIPCHK(wait_progress(ctx, DMX_PHASE_VGA, nchunks, 1));   // progress posts, the cancel flag
    CANCEL_POINT(ctx);
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->last_agents_s = ms * 1e-3;
    std::vector<uint32_t> hcounts((size_t)std::max<int64_t>(C, 1));
    std::vector<int32_t> hfinal((size_t)na), hdone((size_t)na), htrail(std::max<size_t>(ntr, 1));
    std::vector<double> hloc((size_t)na * 2);
    std::vector<unsigned char> hstuck((size_t)na), hflag((size_t)na);
    unsigned long long stt[6];
    HIPCHK(hipMemcpyAsync(hcounts.data(), d_counts.p, hcounts.size() * 4, hipMemcpyDeviceToHost, s));
    if (nagents) {
        HIPCHK(hipMemcpyAsync(hfinal.data(), d_final.p, (size_t)nagents * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hdone.data(), d_done.p, (size_t)nagents * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hloc.data(), d_loc.p, (size_t)nagents * 16, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hstuck.data(), d_stuck.p, (size_t)nagents, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hflag.data(), d_flag.p, (size_t)nagents, hipMemcpyDeviceToHost, s));
    }
    if (ntr) HIPCHK(hipMemcpyAsync(htrail.data(), d_trail.p, ntr * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(copy_sync(s, stt, ctx->stats.p, sizeof(stt), hipMemcpyDeviceToHost));
    if (host_all)
        for (int64_t a = 0; a < nagents; a++) { hflag[a] = AG_FLAG_AMBIGUOUS; hdone[a] = 0; }
    double host_t0 = now_s();
    AgentStats T{(long long)stt[0], (long long)stt[1], (long long)stt[2], (long long)stt[3], (long long)stt[4],
                 (long long)stt[5]};
    // agents the device stopped at an ambiguous look: run again from their start with the host routine, which
    // adds the counts of the moves the device did not make (the moves before are the same, bit for bit)
    long long reruns = 0;
    std::vector<int32_t> hcn, hbn;
    std::vector<uint8_t> hgc;
    std::vector<uint16_t> hbc;
    std::vector<int64_t> hrs;
    std::vector<AgentRun> hpool;
    AgentRunFetch fetch;
    fetch.s = s; fetch.pool = g->pool.p;
    for (int64_t a = 0; a < nagents; a++) {
        if (!(hflag[a] & AG_FLAG_AMBIGUOUS)) continue;
        if (!reruns) {
            hcn.resize((size_t)C); hgc.resize((size_t)N); hbc.resize((size_t)N * 32); hbn.resize((size_t)N * 32);
            hrs.resize((size_t)N);
            HIPCHK(copy_sync(s, hcn.data(), g->pm->d_cell_node.p, (size_t)C * 4, hipMemcpyDeviceToHost));
            HIPCHK(copy_sync(s, hgc.data(), g->gridconn.p, (size_t)N, hipMemcpyDeviceToHost));
            HIPCHK(copy_sync(s, hbc.data(), g->bin_count.p, (size_t)N * 64, hipMemcpyDeviceToHost));
            HIPCHK(copy_sync(s, hbn.data(), g->bin_nruns.p, (size_t)N * 128, hipMemcpyDeviceToHost));
            HIPCHK(copy_sync(s, hrs.data(), g->node_run_start.p, (size_t)N * 8, hipMemcpyDeviceToHost));
            // the per-node arrays (213 bytes a node) come whole; the run pool (8 bytes a run, 35.7 GB on the 1000^2
            // bench map) is read a bin at a time as the looks need it
            if (!lazy_pool && g->nruns) {
                hpool.resize((size_t)g->nruns);
                HIPCHK(copy_sync(s, hpool.data(), g->pool.p, (size_t)g->nruns * 8, hipMemcpyDeviceToHost));
            }
            host_t0 = now_s();
        }
        reruns++;
        AgentMap H = M;
        H.cell_node = hcn.data(); H.gridconn = hgc.data(); H.bin_count = hbc.data(); H.bin_nruns = hbn.data();
        H.node_run_start = hrs.data(); H.pool = hpool.data();
        if (lazy_pool) { H.pool = nullptr; H.fetch_runs = agent_fetch_runs; H.fetch_user = &fetch; }
        AgentState S;
        AgentStats T2{0, 0, 0, 0, 0, 0};
        int done = 0;
        // the kernel kept this agent's counters out of its totals: the whole run's enter them here
        ag_run_host(H, start_cell[a], agent_seed[a], moves[a], hdone[a], hcounts.data(),
                    a < ntrail ? htrail.data() + (size_t)a * maxmoves : nullptr, false, S, T2, done);
        T.moves += T2.moves; T.looks += T2.looks; T.fallbacks += T2.fallbacks;
        T.diag_taken += T2.diag_taken; T.stopped += T2.stopped; T.clamps += T2.clamps;
        hfinal[a] = S.x * rows + S.y;
        hloc[2 * a] = S.lx; hloc[2 * a + 1] = S.ly;
        hstuck[a] = (unsigned char)S.stuck;
    }
    HIPCHK(fetch.err);
    ctx->last_agents_host_s = reruns ? now_s() - host_t0 : 0.0;   // the host routine, without the download
    ctx->last_agents[0] = T.moves; ctx->last_agents[1] = T.looks; ctx->last_agents[2] = reruns;
    ctx->last_agents[3] = T.clamps; ctx->last_agents[4] = T.fallbacks; ctx->last_agents[5] = T.diag_taken;
    ctx->last_agents[6] = T.stopped;
    ctx->last_stats[7] = nagents;
    std::memcpy(counts, hcounts.data(), (size_t)C * 4);
    if (nagents) {
        if (final_cell) std::memcpy(final_cell, hfinal.data(), (size_t)nagents * 4);
        if (final_loc) std::memcpy(final_loc, hloc.data(), (size_t)nagents * 16);
        if (stuck) std::memcpy(stuck, hstuck.data(), (size_t)nagents);
    }
    if (ntr) std::memcpy(trail, htrail.data(), ntr * 4);
    return DMX_OK;
}

int dmx_ctx_last_agents(dmx_ctx* ctx, double* seconds, int64_t* out4) {
    if (!ctx) return fail(DMX_ERR_ARG, "ctx is NULL");
    if (seconds) *seconds = ctx->last_agents_s;
    if (out4)
        for (int i = 0; i < 4; i++) out4[i] = ctx->last_agents[i];
    return DMX_OK;
}

int dmx_ctx_last_agents_detail(dmx_ctx* ctx, double* host_seconds, int64_t* out3) {
    if (!ctx) return fail(DMX_ERR_ARG, "ctx is NULL");
    if (host_seconds) *host_seconds = ctx->last_agents_host_s;
    if (out3)
        for (int i = 0; i < 3; i++) out3[i] = ctx->last_agents[4 + i];
    return DMX_OK;
}
