// api/thruvision.hip -- VGA through vision (dmx_vga_thruvision).
// Part of the dmx_api.hip unity build: included inside its extern "C" block, after the context and the
// internal types (dmx_ctx, dmx_pointmap, dmx_graph); not compiled on its own.

// VGAThroughVision::run: the counts the sources [sb, se) add, for every node.  Merge links play no part and
// context-filled sources are not skipped (vgathroughvision.cpp:47-56).
int dmx_vga_thruvision(dmx_ctx* ctx, dmx_graph* g, int64_t sb, int64_t se, float* out, int64_t* counts) {
    SAME_DEVICE(ctx, g);
    release_sym_scatter(g);
    if (!ctx || !g || !out) return fail(DMX_ERR_ARG, "bad arguments");
    if (g->node_begin != 0 || g->node_end != g->nnodes)
        return fail(DMX_ERR_STATE, "VGA needs the whole graph (assemble the shards first)");
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t N = g->nnodes;
    if (se < 0 || se > N) se = N;
    if (sb < 0 || sb > se) return fail(DMX_ERR_ARG, "source range out of bounds");
    if (N >= CTL_STOP) return fail(DMX_ERR_UNSUPPORTED, "through vision: more than 2^29 nodes");
    PointMapHost& h = *g->pm->host;
    const int cols = h.cols(), rows = h.rows();
    const int64_t C = (int64_t)cols * rows;
    // variant (B) with a kTvWindow^2 window unless the hook says otherwise: 0 = variant (A), n = an n x n window
    int win = policy::hook_int("DMX_TV_WINDOW", policy::kTvWindow);
    if (win < 0 || (size_t)win * win * 4 > (size_t)policy::kTvWindowMaxBytes)
        return fail(DMX_ERR_ARG, "DMX_TV_WINDOW out of range");
    const size_t lds = (size_t)win * win * 4;
    hipStream_t s = ctx->stream;
    DevBuf<unsigned long long> d_counts;
    DevBuf<long long> d_out;
    DevBuf<ThruVisionParams> d_par;
    HIPCHK(d_counts.alloc(std::max<int64_t>(C, 1)));
    HIPCHK(d_out.alloc(std::max<int64_t>(N, 1)));
    HIPCHK(d_par.alloc(1));
    HIPCHK(hipMemsetAsync(d_counts.p, 0, (size_t)std::max<int64_t>(C, 1) * 8, s));
    HIPCHK(hipMemsetAsync(ctx->counters.p, 0, 16 * sizeof(int), s));
    HIPCHK(hipMemsetAsync(ctx->stats.p, 0, 32 * sizeof(unsigned long long), s));
    ThruVisionParams P;
    P.cols = cols; P.rows = rows;
    P.node_cell = g->pm->d_node_cell.p;
    P.node_run_start = g->node_run_start.p; P.node_nruns = g->node_nruns.p; P.pool = g->pool.p;
    P.src_begin = sb; P.src_end = se;
    P.counts = d_counts.p;
    P.work_counter = ctx->counters.p;
    P.ctl = ctx->d_ctl;
    P.stats = ctx->stats.p;
    P.win = win;
    HIPCHK(hipMemcpyAsync(d_par.p, &P, sizeof(P), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // P is a local: copied before it goes out of use
    const int64_t nsrc = se - sb;
    auto kern = win > 0 ? thruvision_kernel<true> : thruvision_kernel<false>;
    HIPCHK(hipEventRecord(ctx->ev0, s));
    if (nsrc > 0) {
        int occ = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, TV_THREADS, lds));
        const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(nsrc, (int64_t)ctx->num_cu * std::max(occ, 1)));
        hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(TV_THREADS), lds, s, d_par.p);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(thruvision_gather_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, N,
                           g->pm->d_node_cell.p, d_counts.p, d_out.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ctx->ev1, s));
    ctx->h_ctl->progress = 0;
    HIPCHK(wait_progress(ctx, DMX_PHASE_VGA, nsrc, 1));   // progress posts, the cancel flag
    CANCEL_POINT(ctx);
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->last_vga_s = ms * 1e-3;
    std::vector<long long> hc((size_t)N, 0);
    if (nsrc > 0 && N > 0) HIPCHK(copy_sync(s, hc.data(), d_out.p, (size_t)N * 8, hipMemcpyDeviceToHost));
    unsigned long long st[2];
    HIPCHK(copy_sync(s, st, ctx->stats.p, sizeof(st), hipMemcpyDeviceToHost));
    ctx->last_stats[7] = nsrc;
    ctx->last_stats[44] = (long long)st[0];   // lines walked
    ctx->last_stats[45] = (long long)st[1];   // pixel steps
    ctx->last_stats[46] = win;                // accumulation variant: 0 (A), else the window side of (B)
    // the reference counts in Point::m_misc, an int: a total above INT32_MAX is refused, not wrapped
    for (int64_t k = 0; k < N; k++)
        if (hc[k] > (long long)INT32_MAX)
            return fail(DMX_ERR_UNSUPPORTED, "through vision: a cell's count exceeds the reference's int counter");
    for (int64_t k = 0; k < N; k++) {
        out[k] = static_cast<float>((int)hc[k]);   // float(m_misc), vgathroughvision.cpp:96
        if (counts) counts[k] = hc[k];
    }
    return DMX_OK;
}
