// api/isovist.hip -- VGA isovist analysis (dmx_vga_isovist, dmx_ctx_last_isovist).
// Part of the dmx_api.hip unity build: included inside its extern "C" block, after the context and the
// internal types (dmx_ctx, dmx_pointmap, dmx_graph); not compiled on its own.

// One launch of isovist_kernel over `items` work items with per-lane lists of (gcap, bcap) entries.
static int isovist_launch(dmx_ctx* ctx, IsovistParams& P, int64_t items, int gcap, int bcap, DevBuf<double>& d_gaps,
                          DevBuf<int32_t>& d_gflags, DevBuf<double>& d_blocks, DevBuf<int32_t>& d_border,
                          DevBuf<IsovistParams>& d_par) {
    hipStream_t s = ctx->stream;
    int occ = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, isovist_kernel, ISO_THREADS, 0));
    // (DMX_ISO_WAVES: the A/B record of profiles/isovist_ab.jsonl)
    const int per_cu = std::max(1, std::min(occ, std::min(policy::hook_int("DMX_ISO_WAVES", policy::kIsoWavesPerCu), 32)));
    const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(items, (int64_t)ctx->num_cu * per_cu));
    // the lists of every workgroup's 64 lanes (every extent the kernel indexes is sized here)
    HIPCHK(d_gaps.alloc((size_t)nb * gcap * 2 * 64));
    HIPCHK(d_gflags.alloc((size_t)nb * gcap * 64));
    HIPCHK(d_blocks.alloc((size_t)nb * bcap * 6 * 64));
    HIPCHK(d_border.alloc((size_t)nb * bcap * 64));
    P.gcap = gcap; P.bcap = bcap;
    P.gaps = d_gaps.p; P.gap_flags = d_gflags.p; P.blocks = d_blocks.p; P.block_order = d_border.p;
    HIPCHK(hipMemsetAsync(ctx->counters.p, 0, 16 * sizeof(int), s));
    HIPCHK(hipMemcpyAsync(d_par.p, &P, sizeof(P), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // P is the caller's: copied before it changes
    HIPCHK(hipEventRecord(ctx->ev0, s));
    hipLaunchKernelGGL(isovist_kernel, dim3((unsigned)nb), dim3(ISO_THREADS), 0, s, d_par.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev1, s));
    return DMX_OK;
}

int dmx_vga_isovist(dmx_ctx* ctx, dmx_graph* g, int simple_version, int64_t sb, int64_t se, float* out, float* occ_dist,
                    int32_t* occ_counts, int32_t* occ_pixels, int64_t occ_cap, int64_t* occ_total) {
    SAME_DEVICE(ctx, g);
    if (!ctx || !g || !out) return fail(DMX_ERR_ARG, "bad arguments");
    release_sym_scatter(g);
    if (g->node_begin != 0 || g->node_end != g->nnodes)
        return fail(DMX_ERR_STATE, "VGA needs the whole graph (assemble the shards first)");
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t N = g->nnodes;
    if (se < 0 || se > N) se = N;
    if (sb < 0 || sb > se) return fail(DMX_ERR_ARG, "source range out of bounds");
    PointMapHost& h = *g->pm->host;
    const std::vector<double>& lines = g->has_drawing ? g->drawing : h.drawing();
    const double t0 = now_s();
    BspTree bt;
    bsp_build(lines.data(), (int64_t)lines.size() / 4, bt);
    ctx->last_iso_bsp_s = now_s() - t0;
    if (bt.nodes() == 0) return fail(DMX_ERR_STATE, "isovist: no drawing lines known (dmx_graph_set_drawing)");
    if (bt.nodes() > (int64_t)INT32_MAX) return fail(DMX_ERR_UNSUPPORTED, "isovist: more than 2^31 tree nodes");
    int rc = upload_pointmap(ctx, g->pm);
    if (rc != DMX_OK) return rc;
    if (g->pm->nnodes != N) return fail(DMX_ERR_STATE, "isovist: the graph's nodes are not the map's filled cells");
    const int cols = h.cols(), rows = h.rows();
    const int tw = (cols + 7) / 8, th = (rows + 7) / 8;
    if ((int64_t)tw * th >= CTL_STOP) return fail(DMX_ERR_UNSUPPORTED, "isovist: more than 2^29 tiles");
    const int gcap = policy::hook_int("DMX_ISO_GCAP", policy::kIsoGapCap);
    const int bcap = policy::hook_int("DMX_ISO_BCAP", policy::kIsoBlockCap);
    // the first gap (0, 2 pi) is stored before any capacity test
    if (gcap < 1 || gcap > policy::kIsoCapMax || bcap < 1 || bcap > policy::kIsoCapMax)
        return fail(DMX_ERR_ARG, "DMX_ISO_GCAP / DMX_ISO_BCAP out of range");
    const bool want_occ = occ_dist || occ_counts || occ_pixels || occ_total;
    hipStream_t s = ctx->stream;
    const int64_t T = bt.nodes();
    DevBuf<double> d_seg, d_gaps, d_blocks;
    DevBuf<int32_t> d_left, d_right, d_parent, d_gflags, d_border, d_occ_n, d_list;
    DevBuf<float> d_out, d_od;
    DevBuf<uint8_t> d_status;
    DevBuf<int2> d_pool;
    DevBuf<long long> d_occ_start;
    DevBuf<unsigned long long> d_cursor;
    DevBuf<IsovistParams> d_par;
    const int64_t N1 = std::max<int64_t>(N, 1);
    HIPCHK(d_seg.alloc((size_t)T * 4));
    HIPCHK(d_left.alloc(T)); HIPCHK(d_right.alloc(T)); HIPCHK(d_parent.alloc(T));
    HIPCHK(d_out.alloc((size_t)N1 * 8));
    HIPCHK(d_status.alloc(N1));
    HIPCHK(d_cursor.alloc(1));
    HIPCHK(d_par.alloc(1));
    if (want_occ) {
        HIPCHK(d_od.alloc((size_t)N1 * 32));
        HIPCHK(d_occ_start.alloc(N1));
        HIPCHK(d_occ_n.alloc(N1));
    }
    HIPCHK(hipMemcpyAsync(d_seg.p, bt.seg.data(), (size_t)T * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_left.p, bt.left.data(), (size_t)T * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_right.p, bt.right.data(), (size_t)T * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_parent.p, bt.parent.data(), (size_t)T * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    IsovistParams P;
    std::memset(&P, 0, sizeof(P));
    P.tree = IsoTree{d_seg.p, d_left.p, d_right.p, d_parent.p, (int32_t)T};
    P.grid = IsoGrid{h.bottom_left().x, h.bottom_left().y, h.spacing(), cols, rows};
    const Rect& gr = h.grid_region();   // PointMap::getRegion()
    P.tolerance = std::max(gr.width(), gr.height()) * 1e-9;
    P.tw = tw; P.th = th;
    P.simple = simple_version ? 1 : 0;
    P.want_occ = want_occ ? 1 : 0;
    P.cell_node = g->pm->d_cell_node.p; P.node_cell = g->pm->d_node_cell.p; P.node_flags = g->pm->d_node_flags.p;
    P.src_begin = sb; P.src_end = se;
    P.out = d_out.p; P.occ_dist = d_od.p; P.status = d_status.p;
    P.pool_cursor = d_cursor.p; P.occ_start = d_occ_start.p; P.occ_n = d_occ_n.p;
    P.work_counter = ctx->counters.p;
    P.ctl = ctx->d_ctl;
    P.stats = ctx->stats.p;
    std::vector<uint8_t> status((size_t)N, 0);
    std::vector<int32_t> flagged;
    unsigned long long pool_cap = want_occ ? (unsigned long long)N1 * policy::kIsoPoolPerNode : 0ull;
    double kernel_s = 0;
    for (int attempt = 0;; attempt++) {
        if (want_occ) HIPCHK(d_pool.alloc((size_t)pool_cap));
        P.pool = d_pool.p; P.pool_cap = pool_cap;
        P.list = nullptr; P.nlist = 0;
        HIPCHK(hipMemsetAsync(d_status.p, 0, (size_t)N1, s));
        HIPCHK(hipMemsetAsync(d_cursor.p, 0, 8, s));
        HIPCHK(hipMemsetAsync(ctx->stats.p, 0, 32 * sizeof(unsigned long long), s));
        if (se > sb) {
            rc = isovist_launch(ctx, P, (int64_t)tw * th, gcap, bcap, d_gaps, d_gflags, d_blocks, d_border, d_par);
            if (rc != DMX_OK) return rc;
        }
        ctx->h_ctl->progress = 0;
        HIPCHK(wait_progress(ctx, DMX_PHASE_VGA, (int64_t)tw * th, 1));   // progress posts, the cancel flag
        CANCEL_POINT(ctx);
        float ms = 0;
        if (se > sb) HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        kernel_s += ms * 1e-3;
        // cells whose lists were too small: once more, with larger lists (list mode, 64 nodes a work item)
        if (N > 0) HIPCHK(copy_sync(s, status.data(), d_status.p, (size_t)N, hipMemcpyDeviceToHost));
        flagged.clear();
        for (int64_t k = 0; k < N; k++)
            if (status[k] == 2) flagged.push_back((int32_t)k);
        if (!flagged.empty()) {
            const int gcap2 = (int)std::min<int64_t>((int64_t)gcap * policy::kIsoRetryFactor, policy::kIsoCapMax);
            const int bcap2 = (int)std::min<int64_t>((int64_t)bcap * policy::kIsoRetryFactor, policy::kIsoCapMax);
            HIPCHK(d_list.alloc(flagged.size()));
            HIPCHK(copy_sync(s, d_list.p, flagged.data(), flagged.size() * 4, hipMemcpyHostToDevice));
            P.list = d_list.p; P.nlist = (int)flagged.size();
            P.ctl = nullptr;   // the second launch is short: it posts no progress (cancel is taken after it)
            rc = isovist_launch(ctx, P, ((int64_t)flagged.size() + 63) / 64, gcap2, bcap2, d_gaps, d_gflags, d_blocks,
                                d_border, d_par);
            P.ctl = ctx->d_ctl;
            if (rc != DMX_OK) return rc;
            HIPCHK(hipStreamSynchronize(s));
            CANCEL_POINT(ctx);
            HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
            kernel_s += ms * 1e-3;
            HIPCHK(copy_sync(s, status.data(), d_status.p, (size_t)N, hipMemcpyDeviceToHost));
            for (int32_t k : flagged)
                if (status[k] != 1)
                    return fail(DMX_ERR_CAPACITY, "isovist: a cell needs more gaps or blocks than the retry capacity");
        }
        unsigned long long used = 0;
        HIPCHK(copy_sync(s, &used, d_cursor.p, 8, hipMemcpyDeviceToHost));
        if (!want_occ || used <= pool_cap) break;
        if (attempt >= 2) return fail(DMX_ERR_CAPACITY, "isovist: the occlusion pool stayed too small");
        pool_cap = used + used / 8 + 1024;   // (the retry's reservations differ: its cells come last)
        d_pool.reset();
    }
    unsigned long long st[2];
    HIPCHK(copy_sync(s, st, ctx->stats.p, sizeof(st), hipMemcpyDeviceToHost));
    ctx->last_vga_s = kernel_s;
    ctx->last_iso_kernel_s = kernel_s;
    ctx->last_iso[0] = T;
    ctx->last_iso[1] = bt.depth;
    ctx->last_iso[2] = (long long)flagged.size();
    ctx->last_iso[3] = (long long)st[0];
    // results of the rows written
    std::vector<float> hout((size_t)N * 8);
    if (N > 0) HIPCHK(copy_sync(s, hout.data(), d_out.p, (size_t)N * 32, hipMemcpyDeviceToHost));
    std::vector<float> hod;
    std::vector<long long> hstart;
    std::vector<int32_t> hn;
    std::vector<int2> hpool;
    if (want_occ && N > 0) {
        hod.resize((size_t)N * 32);
        hstart.resize((size_t)N);
        hn.resize((size_t)N);
        unsigned long long used = 0;
        HIPCHK(copy_sync(s, &used, d_cursor.p, 8, hipMemcpyDeviceToHost));
        hpool.resize((size_t)used);
        HIPCHK(copy_sync(s, hod.data(), d_od.p, (size_t)N * 128, hipMemcpyDeviceToHost));
        HIPCHK(copy_sync(s, hstart.data(), d_occ_start.p, (size_t)N * 8, hipMemcpyDeviceToHost));
        HIPCHK(copy_sync(s, hn.data(), d_occ_n.p, (size_t)N * 4, hipMemcpyDeviceToHost));
        if (used) HIPCHK(copy_sync(s, hpool.data(), d_pool.p, (size_t)used * 8, hipMemcpyDeviceToHost));
    }
    int64_t total = 0;
    for (int64_t k = sb; k < se; k++)
        if (status[k] == 1 && want_occ) total += hn[k];
    const bool pixels = occ_pixels && occ_cap >= total;
    int64_t at = 0;
    for (int64_t k = sb; k < se; k++) {
        if (status[k] != 1) continue;   // a cell the reference skips
        out[k * 8] = hout[k * 8];
        if (!simple_version)
            for (int c = 1; c < 8; c++) out[k * 8 + c] = hout[k * 8 + c];
        if (!want_occ) continue;
        if (occ_dist) std::memcpy(occ_dist + k * 32, hod.data() + k * 32, 128);
        int32_t cnt[32] = {};
        const int2* e = hpool.data() + hstart[k];
        if (hstart[k] < 0 || (size_t)(hstart[k] + hn[k]) > hpool.size()) return fail(DMX_ERR_STATE, "internal: occlusion pool");
        for (int i = 0; i < hn[k]; i++) {
            if ((unsigned)e[i].x >= 32u) return fail(DMX_ERR_STATE, "internal: occlusion bin out of range");
            cnt[e[i].x]++;
        }
        if (occ_counts) std::memcpy(occ_counts + k * 32, cnt, 128);
        if (pixels) {
            int64_t off[32];
            for (int b = 0; b < 32; b++) { off[b] = at; at += cnt[b]; }
            for (int i = 0; i < hn[k]; i++) occ_pixels[off[e[i].x]++] = e[i].y;   // stable: push order inside a bin
        }
    }
    if (occ_total) *occ_total = total;
    return DMX_OK;
}

int dmx_ctx_last_isovist(dmx_ctx* ctx, double* bsp_s, double* kernel_s, int64_t* out4) {
    if (!ctx) return fail(DMX_ERR_ARG, "ctx is NULL");
    if (bsp_s) *bsp_s = ctx->last_iso_bsp_s;
    if (kernel_s) *kernel_s = ctx->last_iso_kernel_s;
    if (out4)
        for (int i = 0; i < 4; i++) out4[i] = ctx->last_iso[i];
    return DMX_OK;
}
