// api/connections.hip -- a graph's neighbourhoods as PixelRef lists and as the connections CSV
// (dmx_graph_connections, dmx_graph_connections_csv; kernels/connections.hip).
// Part of the dmx_api.hip unity build: included inside its extern "C" block, after the context and the
// internal types (dmx_ctx, dmx_pointmap, dmx_graph); not compiled on its own.

// Count, scan and -- when the caller's buffer holds the result -- emit the nodes [nb, ne).  elem: bytes of an item
// of buf (4 for refs, 1 for text).  Outputs are written only after everything succeeded.
static int conn_passes(dmx_ctx* ctx, dmx_graph* g, int64_t nb, int64_t ne, int mode, const char* delim, int64_t* off,
                       void* buf, int64_t cap, int elem, int64_t* total_out) {
    SAME_DEVICE(ctx, g);
    release_sym_scatter(g);
    if (!ctx || !g || cap < 0) return fail(DMX_ERR_ARG, "bad arguments");
    const int64_t N = g->nnodes;
    if (ne < 0) ne = N;
    if (nb < 0 || nb > ne || ne > N) return fail(DMX_ERR_ARG, "node range out of bounds");
    const int64_t n = ne - nb;
    ctx->last_conn_s[0] = ctx->last_conn_s[1] = 0;
    for (auto& v : ctx->last_conn) v = 0;
    if (n == 0) {
        if (off) off[0] = 0;
        if (total_out) *total_out = 0;
        return DMX_OK;
    }
    if (nb < g->node_begin || ne > g->node_end)
        return fail(DMX_ERR_STATE, "the graph does not hold these nodes (a shard: assemble the whole graph first)");
    if (n >= CTL_STOP) return fail(DMX_ERR_UNSUPPORTED, "connections: more than 2^29 nodes in one call");
    HIPCHK(hipSetDevice(ctx->device));
    PointMapHost& h = *g->pm->host;
    hipStream_t s = ctx->stream;
    ConnParams P{};
    P.cols = h.cols(); P.rows = h.rows();
    P.tw = (P.cols + 7) / 8; P.th = (P.rows + 7) / 8;
    const int64_t nt = (int64_t)P.tw * P.th;
    const size_t bm_bytes = (size_t)nt * 8;
    // the bitmap in LDS next to the kernels' static arrays, or in HBM slices; the hook forces the slices (tests)
    const bool gbm = bm_bytes + policy::kConnStaticLds > (size_t)policy::kLdsPassBudget || policy::hook("DMX_CONN_GBM");
    const size_t lds = gbm ? 0 : bm_bytes;
    DevBuf<int64_t> d_items, d_off, d_tiles;
    DevBuf<unsigned char> d_dup, d_out;
    DevBuf<unsigned long long> d_bm;
    const int64_t nst = (n + CC_SCAN_TILE - 1) / CC_SCAN_TILE;
    HIPCHK(d_items.alloc(n));
    HIPCHK(d_off.alloc(n + 1));
    HIPCHK(d_tiles.alloc(nst + 1));
    HIPCHK(d_dup.alloc(n));
    P.node_cell = g->pm->d_node_cell.p;
    P.node_run_start = g->node_run_start.p; P.node_nruns = g->node_nruns.p; P.bin_nruns = g->bin_nruns.p;
    P.pool = g->pool.p;
    P.seed_tiles = g->pm->d_seed_tiles.p;
    P.node_begin = nb; P.node_end = ne; P.local0 = g->node_begin;
    P.mode = mode;
    P.dlen = delim ? (int)std::strlen(delim) : 0;
    for (int i = 0; i < P.dlen; i++) P.delim[i] = (unsigned char)delim[i];
    P.work_counter = ctx->counters.p;
    P.ctl = ctx->d_ctl;
    P.items = d_items.p; P.dup = d_dup.p; P.stats = ctx->stats.p; P.off = d_off.p;
    auto blocks = [&](auto kern, int64_t& nblk) -> int {
        int occ = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, CONN_THREADS, lds));
        nblk = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)ctx->num_cu * std::max(occ, 1)));
        if (gbm) {
            // bitmap slices within a quarter of the free memory
            size_t fr = 0, tot = 0;
            HIPCHK(hipMemGetInfo(&fr, &tot));
            nblk = std::max<int64_t>(1, std::min<int64_t>(nblk, (int64_t)((fr + cached_bytes()) / policy::kMemShareDiv / bm_bytes)));
            HIPCHK(d_bm.alloc((size_t)nblk * nt));
            P.gbm = d_bm.p;
        }
        return DMX_OK;
    };
    // pass 1: items (bytes) of every node, then their exclusive scan
    HIPCHK(hipMemsetAsync(ctx->counters.p, 0, 16 * sizeof(int), s));
    HIPCHK(hipMemsetAsync(ctx->stats.p, 0, 32 * sizeof(unsigned long long), s));
    ctx->h_ctl->progress = 0;
    int64_t nblk = 1;
    {
        auto kern = gbm ? conn_count_kernel<true> : conn_count_kernel<false>;
        if (int rc = blocks(kern, nblk)) return rc;
        HIPCHK(hipEventRecord(ctx->ev0, s));
        hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(CONN_THREADS), lds, s, P);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(cc_scan_reduce_kernel, dim3((unsigned)nst), dim3(CC_THREADS), 0, s, d_items.p, n, d_tiles.p);
    hipLaunchKernelGGL(cc_scan_tiles_kernel, dim3(1), dim3(CC_THREADS), 0, s, d_tiles.p, nst);
    hipLaunchKernelGGL(cc_scan_down_kernel, dim3((unsigned)nst), dim3(CC_THREADS), 0, s, d_items.p, n, d_tiles.p, nst, d_off.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev1, s));
    HIPCHK(hipStreamSynchronize(s));
    CANCEL_POINT(ctx);   // a cancelled counting pass left nodes uncounted
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->last_conn_s[0] = ms * 1e-3;
    std::vector<int64_t> hoff((size_t)n + 1);
    HIPCHK(copy_sync(s, hoff.data(), d_off.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost));
    unsigned long long st[3];
    HIPCHK(copy_sync(s, st, ctx->stats.p, sizeof(st), hipMemcpyDeviceToHost));
    const int64_t total = hoff[(size_t)n];
    const bool emit = buf && cap >= total;
    // pass 2: the kept cells at their scanned offsets
    std::vector<unsigned char> hout;
    if (emit && total > 0) {
        HIPCHK(d_out.alloc((size_t)total * elem));
        P.refs = (int32_t*)d_out.p;
        P.text = d_out.p;
        HIPCHK(hipMemsetAsync(ctx->counters.p, 0, 16 * sizeof(int), s));
        auto kern = gbm ? conn_emit_kernel<true> : conn_emit_kernel<false>;
        if (int rc = blocks(kern, nblk)) return rc;
        HIPCHK(hipEventRecord(ctx->ev0, s));
        hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(CONN_THREADS), lds, s, P);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->ev1, s));
    }
    ctx->h_ctl->progress = 0;
    HIPCHK(wait_progress(ctx, DMX_PHASE_VGA, n, 1));   // progress posts, the cancel flag
    CANCEL_POINT(ctx);
    if (emit && total > 0) {
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        ctx->last_conn_s[1] = ms * 1e-3;
        hout.resize((size_t)total * elem);
        HIPCHK(copy_sync(s, hout.data(), d_out.p, hout.size(), hipMemcpyDeviceToHost));
    }
    ctx->last_conn[0] = gbm ? 1 : 0;
    ctx->last_conn[1] = (long long)st[0];
    ctx->last_conn[2] = (long long)st[1];
    ctx->last_conn[3] = (long long)st[2];
    ctx->last_stats[7] = n;
    if (!hout.empty()) std::memcpy(buf, hout.data(), hout.size());
    if (off) std::memcpy(off, hoff.data(), hoff.size() * 8);
    if (total_out) *total_out = total;
    return DMX_OK;
}

int dmx_graph_connections(dmx_ctx* ctx, dmx_graph* g, int64_t node_begin, int64_t node_end, int flags, int64_t* off,
                          int32_t* refs, int64_t cap, int64_t* total) {
    if (flags & ~DMX_CONN_EXPORT) return fail(DMX_ERR_ARG, "unknown flags");
    return conn_passes(ctx, g, node_begin, node_end, (flags & DMX_CONN_EXPORT) ? CONN_EXPORT : CONN_CONTENTS, nullptr,
                       off, refs, cap, 4, total);
}

int dmx_graph_connections_csv(dmx_ctx* ctx, dmx_graph* g, int64_t node_begin, int64_t node_end, const char* delim,
                              int64_t* off, char* buf, int64_t cap, int64_t* size) {
    if (!delim || !*delim || std::strlen(delim) > 8) return fail(DMX_ERR_ARG, "the delimiter must hold 1 to 8 bytes");
    return conn_passes(ctx, g, node_begin, node_end, CONN_TEXT, delim, off, buf, cap, 1, size);
}

int dmx_ctx_last_connections(dmx_ctx* ctx, double* count_s, double* emit_s, int64_t* out4) {
    if (!ctx) return fail(DMX_ERR_ARG, "ctx is NULL");
    if (count_s) *count_s = ctx->last_conn_s[0];
    if (emit_s) *emit_s = ctx->last_conn_s[1];
    if (out4)
        for (int i = 0; i < 4; i++) out4[i] = ctx->last_conn[i];
    return DMX_OK;
}
