// api/isovist_points.hip -- a batch of isovists at caller-given points (dmx_isovists).
// Part of the dmx_api.hip unity build: included inside its extern "C" block, after api/isovist.hip; not compiled
// on its own.

// One launch of isovist_points_kernel over `items` work items with per-lane lists of (gcap, bcap) entries.
static int isovist_points_launch(dmx_ctx* ctx, IsoPointsParams& P, int64_t items, int gcap, int bcap,
                                 DevBuf<double>& d_gaps, DevBuf<int32_t>& d_gflags, DevBuf<double>& d_blocks,
                                 DevBuf<int32_t>& d_border, DevBuf<IsoPointsParams>& d_par) {
    hipStream_t s = ctx->stream;
    int occ = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, isovist_points_kernel, ISOP_THREADS, 0));
    // (DMX_ISO_PWAVES: the A/B record of profiles/isovist_points.jsonl)
    const int per_cu =
        std::max(1, std::min(occ, std::min(policy::hook_int("DMX_ISO_PWAVES", policy::kIsoPointsWavesPerCu), 32)));
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
    hipLaunchKernelGGL(isovist_points_kernel, dim3((unsigned)nb), dim3(ISOP_THREADS), 0, s, d_par.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev1, s));
    return DMX_OK;
}

// The launch order: launch position i runs caller point order[i].  Morton: by the interleaved 16-bit cell of the
// point over the region (points outside take the nearest cell), ties in the caller's order.
static void isovist_points_order(const double* points, int64_t n, const double* reg, bool morton, std::vector<int64_t>& order) {
    order.resize((size_t)n);
    for (int64_t k = 0; k < n; k++) order[k] = k;
    if (!morton || n < 2) return;
    auto spread = [](uint32_t v) {
        uint64_t x = v;
        x = (x | (x << 8)) & 0x00FF00FFull;
        x = (x | (x << 4)) & 0x0F0F0F0Full;
        x = (x | (x << 2)) & 0x33333333ull;
        x = (x | (x << 1)) & 0x55555555ull;
        return (uint32_t)x;
    };
    const double w = reg[2] - reg[0], h = reg[3] - reg[1];
    auto cell = [](double v, double lo, double ext) {
        const double t = ext > 0 ? (v - lo) / ext * 65536.0 : 0.0;
        return (uint32_t)(t < 0 ? 0.0 : (t > 65535.0 ? 65535.0 : t));
    };
    std::vector<std::pair<uint32_t, int64_t>> key((size_t)n);
    for (int64_t k = 0; k < n; k++)
        key[k] = {spread(cell(points[2 * k], reg[0], w)) | (spread(cell(points[2 * k + 1], reg[1], h)) << 1), k};
    std::sort(key.begin(), key.end());
    for (int64_t k = 0; k < n; k++) order[k] = key[k].second;
}

int dmx_isovists(dmx_ctx* ctx, const double* lines, int64_t nlines, const double* region, const double* points,
                 const double* angles, int64_t n, int simple_version, float* out, int64_t* poly_off, double* poly_xy,
                 int64_t poly_cap, int64_t* poly_total) {
    if (!ctx || n < 0 || nlines < 0 || (nlines > 0 && !lines) || (n > 0 && (!points || !out)) || poly_cap < 0)
        return fail(DMX_ERR_ARG, "bad arguments");
    for (int64_t k = 0; k < nlines * 4; k++)
        if (!std::isfinite(lines[k])) return fail(DMX_ERR_ARG, "isovists: a line coordinate is not finite");
    for (int64_t k = 0; k < n * 2; k++)
        if (!std::isfinite(points[k]) || (angles && !std::isfinite(angles[k])))
            return fail(DMX_ERR_ARG, "isovists: a point coordinate or an angle is not finite");
    if (region)
        for (int k = 0; k < 4; k++)
            if (!std::isfinite(region[k])) return fail(DMX_ERR_ARG, "isovists: the region is not finite");
    const bool want_poly = poly_off || poly_xy || poly_total;
    if (n == 0) {
        if (poly_off) poly_off[0] = 0;
        if (poly_total) *poly_total = 0;
        return DMX_OK;
    }
    HIPCHK(hipSetDevice(ctx->device));
    const double t0 = now_s();
    BspTree bt;
    bsp_build(lines, nlines, bt);
    const double bsp_s = now_s() - t0;
    if (bt.nodes() == 0) return fail(DMX_ERR_STATE, "isovists: no drawing lines");
    if (bt.nodes() > (int64_t)INT32_MAX) return fail(DMX_ERR_UNSUPPORTED, "isovists: more than 2^31 tree nodes");
    const int64_t T = bt.nodes();
    // the links the kernel follows stay inside the tree
    for (int64_t k = 0; k < T; k++)
        if (bt.left[k] < -1 || bt.left[k] >= T || bt.right[k] < -1 || bt.right[k] >= T || bt.parent[k] < -1 || bt.parent[k] >= T)
            return fail(DMX_ERR_STATE, "internal: BSP tree link out of range");
    const int64_t items = (n + 63) / 64;
    if (items >= CTL_STOP) return fail(DMX_ERR_UNSUPPORTED, "isovists: more than 2^35 points in one call");
    const int gcap = policy::hook_int("DMX_ISO_GCAP", policy::kIsoGapCap);
    const int bcap = policy::hook_int("DMX_ISO_BCAP", policy::kIsoBlockCap);
    const int vpool = policy::hook_int("DMX_ISO_VPOOL", policy::kIsoVertexPoolPerPoint);
    if (gcap < 1 || gcap > policy::kIsoCapMax || bcap < 1 || bcap > policy::kIsoCapMax || vpool < 1 || vpool > policy::kIsoCapMax)
        return fail(DMX_ERR_ARG, "DMX_ISO_GCAP / DMX_ISO_BCAP / DMX_ISO_VPOOL out of range");
    // MetaGraph::m_region: given, or the bounding box of the drawing
    double reg[4];
    if (region) {
        for (int k = 0; k < 4; k++) reg[k] = region[k];
    } else {
        reg[0] = reg[2] = lines[0];
        reg[1] = reg[3] = lines[1];
        for (int64_t k = 0; k < nlines * 2; k++) {
            const double x = lines[2 * k], y = lines[2 * k + 1];
            reg[0] = std::min(reg[0], x); reg[2] = std::max(reg[2], x);
            reg[1] = std::min(reg[1], y); reg[3] = std::max(reg[3], y);
        }
    }
    const double tolerance = std::max(reg[2] - reg[0], reg[3] - reg[1]) * 1e-9;
    const char* oh = policy::hook("DMX_ISO_ORDER");
    const bool morton = oh ? strcmp(oh, "caller") != 0 : policy::kIsoPointsMorton != 0;
    std::vector<int64_t> order;
    isovist_points_order(points, n, reg, morton, order);
    std::vector<double> pts((size_t)n * 4);
    for (int64_t i = 0; i < n; i++) {
        const int64_t k = order[i];
        pts[4 * i] = points[2 * k];
        pts[4 * i + 1] = points[2 * k + 1];
        pts[4 * i + 2] = angles ? angles[2 * k] : 0.0;
        pts[4 * i + 3] = angles ? angles[2 * k + 1] : 0.0;
    }
    hipStream_t s = ctx->stream;
    DevBuf<double> d_seg, d_gaps, d_blocks, d_pts;
    DevBuf<int32_t> d_left, d_right, d_parent, d_gflags, d_border, d_poly_n;
    DevBuf<int64_t> d_list;
    DevBuf<float> d_out;
    DevBuf<uint8_t> d_status;
    DevBuf<double2> d_pool;
    DevBuf<long long> d_poly_start;
    DevBuf<unsigned long long> d_cursor;
    DevBuf<IsoPointsParams> d_par;
    HIPCHK(d_seg.alloc((size_t)T * 4));
    HIPCHK(d_left.alloc(T)); HIPCHK(d_right.alloc(T)); HIPCHK(d_parent.alloc(T));
    HIPCHK(d_pts.alloc((size_t)n * 4));
    HIPCHK(d_out.alloc((size_t)n * 8));
    HIPCHK(d_status.alloc(n));
    HIPCHK(d_cursor.alloc(1));
    HIPCHK(d_par.alloc(1));
    if (want_poly) {
        HIPCHK(d_poly_start.alloc(n));
        HIPCHK(d_poly_n.alloc(n));
    }
    HIPCHK(hipMemcpyAsync(d_seg.p, bt.seg.data(), (size_t)T * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_left.p, bt.left.data(), (size_t)T * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_right.p, bt.right.data(), (size_t)T * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_parent.p, bt.parent.data(), (size_t)T * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_pts.p, pts.data(), (size_t)n * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    IsoPointsParams P;
    std::memset(&P, 0, sizeof(P));
    P.tree = IsoTree{d_seg.p, d_left.p, d_right.p, d_parent.p, (int32_t)T};
    P.tolerance = tolerance;
    P.simple = simple_version ? 1 : 0;
    P.want_poly = want_poly ? 1 : 0;
    P.pts = d_pts.p;
    P.n = n;
    P.out = d_out.p; P.status = d_status.p;
    P.pool_cursor = d_cursor.p; P.poly_start = d_poly_start.p; P.poly_n = d_poly_n.p;
    P.work_counter = ctx->counters.p;
    P.ctl = ctx->d_ctl;
    P.stats = ctx->stats.p;
    std::vector<uint8_t> status((size_t)n, 0);
    std::vector<int64_t> flagged;
    unsigned long long pool_cap = want_poly ? (unsigned long long)n * (unsigned long long)vpool : 0ull;
    unsigned long long used = 0;
    double kernel_s = 0;
    for (int attempt = 0;; attempt++) {
        if (want_poly) HIPCHK(d_pool.alloc((size_t)pool_cap));
        P.pool = d_pool.p; P.pool_cap = pool_cap;
        P.list = nullptr; P.nlist = 0;
        HIPCHK(hipMemsetAsync(d_status.p, 0, (size_t)n, s));
        HIPCHK(hipMemsetAsync(d_cursor.p, 0, 8, s));
        HIPCHK(hipMemsetAsync(ctx->stats.p, 0, 32 * sizeof(unsigned long long), s));
        int rc = isovist_points_launch(ctx, P, items, gcap, bcap, d_gaps, d_gflags, d_blocks, d_border, d_par);
        if (rc != DMX_OK) return rc;
        ctx->h_ctl->progress = 0;
        HIPCHK(wait_progress(ctx, DMX_PHASE_VGA, items, 1));   // progress posts, the cancel flag
        CANCEL_POINT(ctx);
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        kernel_s += ms * 1e-3;
        // points whose lists were too small: once more, with larger lists (list mode, 64 points a work item)
        HIPCHK(copy_sync(s, status.data(), d_status.p, (size_t)n, hipMemcpyDeviceToHost));
        flagged.clear();
        for (int64_t k = 0; k < n; k++)
            if (status[k] == 2) flagged.push_back(k);
        if (!flagged.empty()) {
            const int gcap2 = (int)std::min<int64_t>((int64_t)gcap * policy::kIsoRetryFactor, policy::kIsoCapMax);
            const int bcap2 = (int)std::min<int64_t>((int64_t)bcap * policy::kIsoRetryFactor, policy::kIsoCapMax);
            HIPCHK(d_list.alloc(flagged.size()));
            HIPCHK(copy_sync(s, d_list.p, flagged.data(), flagged.size() * 8, hipMemcpyHostToDevice));
            P.list = d_list.p; P.nlist = (int64_t)flagged.size();
            P.ctl = nullptr;   // the second launch is short: it posts no progress (cancel is taken after it)
            rc = isovist_points_launch(ctx, P, ((int64_t)flagged.size() + 63) / 64, gcap2, bcap2, d_gaps, d_gflags, d_blocks,
                                       d_border, d_par);
            P.ctl = ctx->d_ctl;
            if (rc != DMX_OK) return rc;
            HIPCHK(hipStreamSynchronize(s));
            CANCEL_POINT(ctx);
            HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
            kernel_s += ms * 1e-3;
            HIPCHK(copy_sync(s, status.data(), d_status.p, (size_t)n, hipMemcpyDeviceToHost));
            for (int64_t k : flagged)
                if (status[k] != 1)
                    return fail(DMX_ERR_CAPACITY, "isovists: a point needs more gaps or blocks than the retry capacity");
        }
        for (int64_t k = 0; k < n; k++)
            if (status[k] != 1) return fail(DMX_ERR_STATE, "internal: isovists: a point was not run");
        HIPCHK(copy_sync(s, &used, d_cursor.p, 8, hipMemcpyDeviceToHost));
        if (!want_poly || used <= pool_cap) break;
        if (attempt >= 2) return fail(DMX_ERR_CAPACITY, "isovists: the vertex pool stayed too small");
        pool_cap = used;   // every point reserves 2 nb + 2 whatever the order: the count is the need
        d_pool.reset();
    }
    unsigned long long st[2];
    HIPCHK(copy_sync(s, st, ctx->stats.p, sizeof(st), hipMemcpyDeviceToHost));
    std::vector<float> hout((size_t)n * 8);
    HIPCHK(copy_sync(s, hout.data(), d_out.p, (size_t)n * 32, hipMemcpyDeviceToHost));
    std::vector<long long> hstart;
    std::vector<int32_t> hn;
    std::vector<int64_t> where;   // launch position of each caller point
    int64_t total = 0;
    if (want_poly) {
        hstart.resize((size_t)n);
        hn.resize((size_t)n);
        HIPCHK(copy_sync(s, hstart.data(), d_poly_start.p, (size_t)n * 8, hipMemcpyDeviceToHost));
        HIPCHK(copy_sync(s, hn.data(), d_poly_n.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; i++) {
            if (hn[i] < 0 || hstart[i] < 0 || (unsigned long long)hstart[i] + (unsigned long long)hn[i] > used)
                return fail(DMX_ERR_STATE, "internal: isovists: vertex pool");
            total += hn[i];
        }
    }
    const bool vertices = poly_xy && poly_cap >= total && want_poly;
    std::vector<double2> hpool;
    if (vertices && used) {
        hpool.resize((size_t)used);
        HIPCHK(copy_sync(s, hpool.data(), d_pool.p, (size_t)used * 16, hipMemcpyDeviceToHost));
    }
    // every failure is behind: the outputs, in the caller's order
    ctx->last_iso_bsp_s = bsp_s;
    ctx->last_iso_kernel_s = kernel_s;
    ctx->last_iso[0] = T;
    ctx->last_iso[1] = bt.depth;
    ctx->last_iso[2] = (long long)flagged.size();
    ctx->last_iso[3] = (long long)st[0];
    for (int64_t i = 0; i < n; i++) {
        const int64_t k = order[i];
        out[k * 8] = hout[i * 8];
        if (!simple_version)
            for (int c = 1; c < 8; c++) out[k * 8 + c] = hout[i * 8 + c];
    }
    if (want_poly) {
        where.resize((size_t)n);
        for (int64_t i = 0; i < n; i++) where[order[i]] = i;
        int64_t at = 0;
        for (int64_t k = 0; k < n; k++) {
            const int64_t i = where[k];
            if (poly_off) poly_off[k] = at;
            if (vertices && hn[i]) std::memcpy(poly_xy + 2 * at, hpool.data() + hstart[i], (size_t)hn[i] * 16);
            at += hn[i];
        }
        if (poly_off) poly_off[n] = at;
        if (poly_total) *poly_total = total;
    }
    return DMX_OK;
}
