// api/chunk.hip -- the .graph PointMap chunk: parse, load, columns, serialise.
// Part of the dmx_api.hip unity build: included inside its extern "C" block, after the context and the
// internal types (dmx_ctx, dmx_pointmap, dmx_graph); not compiled on its own.

// ---------------------------------------------------------------- .graph PointMap chunk
struct dmx_chunk {
    ParsedChunk pc;
};

int dmx_graph_from_runs(dmx_ctx* ctx, dmx_pointmap* pm, int64_t nnodes, const int32_t* bins, const int16_t* runs,
                        int64_t nruns, const uint8_t* gridconn, const float* attrs, dmx_graph** out) {
    if (!ctx || !pm || !out || nnodes < 0 || nruns < 0 || (nnodes && !bins) || (nruns && !runs))
        return fail(DMX_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    int rc = upload_pointmap(ctx, pm);
    if (rc) return rc;
    if (nnodes != pm->nnodes) return fail(DMX_ERR_ARG, "node count does not match the filled cells of the map");
    const int64_t N = nnodes;
    std::vector<int32_t> bn((size_t)std::max<int64_t>(N, 1) * 32), nr((size_t)std::max<int64_t>(N, 1));
    std::vector<uint16_t> bc((size_t)std::max<int64_t>(N, 1) * 32);
    std::vector<float> bd((size_t)std::max<int64_t>(N, 1) * 32);
    std::vector<int64_t> st((size_t)std::max<int64_t>(N, 1));
    int64_t acc = 0;
    for (int64_t k = 0; k < N; k++) {
        int s = 0;
        for (int b = 0; b < 32; b++) {
            const int32_t* r = bins + (k * 32 + b) * 4;
            bn[k * 32 + b] = r[3];
            bc[k * 32 + b] = (uint16_t)r[1];
            std::memcpy(&bd[k * 32 + b], &r[2], 4);
            s += r[3];
        }
        nr[k] = s;
        st[k] = acc;
        acc += s;
    }
    if (acc != nruns) return fail(DMX_ERR_ARG, "bins do not account for the runs");
    std::unique_ptr<dmx_graph> g(new dmx_graph());
    g->ctx = ctx; g->pm = pm; g->nnodes = N; g->node_begin = 0; g->node_end = N; g->nruns = nruns;
    inherit_merges(g.get());
    HIPCHK(g->pool.alloc(std::max<int64_t>(nruns, 1)));
    HIPCHK(g->node_run_start.alloc(std::max<int64_t>(N, 1)));
    HIPCHK(g->node_nruns.alloc(std::max<int64_t>(N, 1)));
    HIPCHK(g->bin_nruns.alloc(std::max<int64_t>(N, 1) * 32));
    HIPCHK(g->bin_count.alloc(std::max<int64_t>(N, 1) * 32));
    HIPCHK(g->bin_dist.alloc(std::max<int64_t>(N, 1) * 32));
    HIPCHK(g->attrs.alloc(std::max<int64_t>(N, 1) * 3));
    HIPCHK(g->gridconn.alloc(std::max<int64_t>(N, 1)));
    hipStream_t s = ctx->stream;
    if (nruns) HIPCHK(hipMemcpyAsync(g->pool.p, runs, nruns * 8, hipMemcpyHostToDevice, s));
    if (N) {
        HIPCHK(hipMemcpyAsync(g->node_run_start.p, st.data(), N * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(g->node_nruns.p, nr.data(), N * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(g->bin_nruns.p, bn.data(), N * 32 * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(g->bin_count.p, bc.data(), N * 32 * 2, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(g->bin_dist.p, bd.data(), N * 32 * 4, hipMemcpyHostToDevice, s));
        if (attrs) HIPCHK(hipMemcpyAsync(g->attrs.p, attrs, N * 12, hipMemcpyHostToDevice, s));
        else HIPCHK(hipMemsetAsync(g->attrs.p, 0, N * 12, s));
        if (gridconn) HIPCHK(hipMemcpyAsync(g->gridconn.p, gridconn, N, hipMemcpyHostToDevice, s));
        else HIPCHK(hipMemsetAsync(g->gridconn.p, 0, N, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    *out = g.release();
    return DMX_OK;
}

// the columns of dmx_chunk_write / dmx_graph_chunk_write: values and setmask [ncols][nnodes], insertion order
static std::vector<ChunkColumn> chunk_columns(int64_t nnodes, int ncols, const char* const* names, const float* values,
                                              const uint8_t* locked, const uint8_t* setmask) {
    std::vector<ChunkColumn> cols((size_t)ncols);
    for (int i = 0; i < ncols; i++) {
        cols[i].name = names[i];
        cols[i].locked = locked ? locked[i] != 0 : false;
        cols[i].values.assign(values + (size_t)i * nnodes, values + (size_t)(i + 1) * nnodes);
        if (setmask) cols[i].set.assign(setmask + (size_t)i * nnodes, setmask + (size_t)(i + 1) * nnodes);
    }
    return cols;
}

int dmx_chunk_write(const dmx_pointmap* pm, int64_t nnodes, const int32_t* bins, const int16_t* runs, int64_t nruns,
                    const uint8_t* gridconn, int ncols, const char* const* names, const float* values,
                    const uint8_t* locked, const uint8_t* setmask, int displayed, int boundary, uint8_t* buf, int64_t cap,
                    int64_t* size) {
    if (!pm || !size || nnodes < 0 || ncols < 0 || (ncols && (!names || !values))) return fail(DMX_ERR_ARG, "bad arguments");
    const std::vector<ChunkColumn> cols = chunk_columns(nnodes, ncols, names, values, locked, setmask);
    std::vector<uint8_t> out;
    std::string err;
    if (write_pointmap_chunk(*pm->host, nnodes, bins, runs, nruns, gridconn, cols, displayed, boundary != 0, out, err))
        return fail(DMX_ERR_ARG, err);
    *size = (int64_t)out.size();
    if (buf) {
        if (cap < (int64_t)out.size()) return fail(DMX_ERR_ARG, "buffer too small");
        std::memcpy(buf, out.data(), out.size());
    }
    return DMX_OK;
}

int dmx_chunk_parse(const uint8_t* buf, int64_t size, dmx_chunk** out) {
    if (!buf || !out || size <= 0) return fail(DMX_ERR_ARG, "bad arguments");
    std::unique_ptr<dmx_chunk> c(new dmx_chunk());
    std::string err;
    if (read_pointmap_chunk(buf, (size_t)size, c->pc, err)) return fail(DMX_ERR_ARG, err);
    *out = c.release();
    return DMX_OK;
}

int dmx_chunk_free(dmx_chunk* c) {
    delete c;
    return DMX_OK;
}

int dmx_chunk_info(const dmx_chunk* c, int32_t* cols, int32_t* rows, double* spacing, double* bl, int64_t* nnodes,
                   int64_t* nruns, int32_t* ncols, int32_t* displayed_sorted, int64_t* bytes_used) {
    if (!c) return fail(DMX_ERR_ARG, "chunk is NULL");
    const ParsedChunk& p = c->pc;
    if (cols) *cols = p.cols;
    if (rows) *rows = p.rows;
    if (spacing) *spacing = p.spacing;
    if (bl) { bl[0] = p.blx; bl[1] = p.bly; }
    if (nnodes) *nnodes = (int64_t)p.gridconn.size();
    if (nruns) *nruns = (int64_t)p.runs.size() / 4;
    if (ncols) *ncols = (int32_t)p.columns.size();
    if (displayed_sorted) *displayed_sorted = p.displayed_sorted;
    if (bytes_used) *bytes_used = (int64_t)p.bytes_used;
    return DMX_OK;
}

int dmx_chunk_column(const dmx_chunk* c, int i, char* name, int name_cap, float* values, int* locked) {
    if (!c || i < 0 || i >= (int)c->pc.columns.size()) return fail(DMX_ERR_ARG, "bad column");
    const ChunkColumn& col = c->pc.columns[i];
    if (name && name_cap > 0) {
        const size_t n = std::min<size_t>(col.name.size(), (size_t)name_cap - 1);
        std::memcpy(name, col.name.data(), n);
        name[n] = 0;
    }
    if (values && !col.values.empty()) std::memcpy(values, col.values.data(), col.values.size() * 4);
    if (locked) *locked = col.locked ? 1 : 0;
    return DMX_OK;
}

int dmx_chunk_arrays(const dmx_chunk* c, int32_t* state, int32_t* bins, int16_t* runs, uint8_t* gridconn) {
    if (!c) return fail(DMX_ERR_ARG, "chunk is NULL");
    const ParsedChunk& p = c->pc;
    if (state) std::memcpy(state, p.state.data(), p.state.size() * 4);
    if (bins && !p.bins.empty()) std::memcpy(bins, p.bins.data(), p.bins.size() * 4);
    if (runs && !p.runs.empty()) std::memcpy(runs, p.runs.data(), p.runs.size() * 2);
    if (gridconn && !p.gridconn.empty()) std::memcpy(gridconn, p.gridconn.data(), p.gridconn.size());
    return DMX_OK;
}

int dmx_pointmap_set_state(dmx_pointmap* pm, const int32_t* state) {
    if (!pm || !state) return fail(DMX_ERR_ARG, "bad arguments");
    PointMapHost& h = *pm->host;
    h.restore_fill(state);
    pm->version++;
    return DMX_OK;
}

int dmx_chunk_load(dmx_ctx* ctx, const dmx_chunk* c, const double* region, dmx_pointmap** pm_out, dmx_graph** g_out) {
    if (!ctx || !c || !region || !pm_out || !g_out) return fail(DMX_ERR_ARG, "bad arguments");
    const ParsedChunk& p = c->pc;
    if (!p.processed) return fail(DMX_ERR_STATE, "the point map has no graph (run VISPREP -pm first)");
    Rect r{region[0], region[1], region[2], region[3]};
    std::unique_ptr<dmx_pointmap> pm(new dmx_pointmap());
    pm->host.reset(new PointMapHost(r, p.spacing, nullptr, 0));
    pm->host->load_state(p.cols, p.rows, p.spacing, Vec2{p.blx, p.bly}, p.state.data());
    const int64_t N = (int64_t)p.gridconn.size();
    std::vector<float> attrs((size_t)std::max<int64_t>(N, 1) * 3, 0.0f);
    const char* mk[3] = {"Connectivity", "Point First Moment", "Point Second Moment"};
    for (int j = 0; j < 3; j++)
        for (const auto& col : p.columns)
            if (col.name == mk[j] && (int64_t)col.values.size() == N)
                for (int64_t k = 0; k < N; k++) attrs[k * 3 + j] = col.values[k];
    dmx_graph* g = nullptr;
    int rc = dmx_graph_from_runs(ctx, pm.get(), N, p.bins.data(), p.runs.data(), (int64_t)p.runs.size() / 4,
                                 p.gridconn.data(), attrs.data(), &g);
    if (rc) return rc;
    std::unique_ptr<dmx_graph> gg(g);
    {
        std::vector<int32_t> per_cell, uniq;
        rc = normalize_merges(pm->host->cells(), p.merge_pairs.data(), (int64_t)p.merge_pairs.size() / 2, per_cell, uniq,
                              true);
        if (rc) return rc;
        pm->host->set_merge(std::move(per_cell));
    }
    inherit_merges(g);
    *pm_out = pm.release();
    *g_out = gg.release();
    return DMX_OK;
}

int dmx_pointmap_set_merges(dmx_pointmap* pm, const int32_t* cell_pairs, int64_t n) {
    if (!pm || n < 0 || (n && !cell_pairs)) return fail(DMX_ERR_ARG, "bad arguments");
    std::vector<int32_t> per_cell, uniq;
    if (int rc = normalize_merges(pm->host->cells(), cell_pairs, n, per_cell, uniq)) return rc;
    pm->host->set_merge(std::move(per_cell));
    return DMX_OK;
}

int dmx_graph_set_merges(dmx_graph* g, const int32_t* cell_pairs, int64_t n) {
    if (!g || n < 0 || (n && !cell_pairs)) return fail(DMX_ERR_ARG, "bad arguments");
    std::vector<int32_t> per_cell, uniq;
    if (int rc = normalize_merges(g->pm->host->cells(), cell_pairs, n, per_cell, uniq)) return rc;
    // the links belong to the points (Point::m_merge): the map gets them too, so a chunk written from it
    // saves them and a graph made from it again follows them
    g->pm->host->set_merge(std::move(per_cell));
    g->merges = std::move(uniq);
    g->merges_ready = false;
    // the asymmetric mode's preparation was made (or refused) for the previous links: its reference graph has none
    asym_invalidate(g);
    if (g->merges.empty()) {   // prepare_merges returns early on no links: drop the previous links' device state
        g->nmamb = 0;
        g->d_mamb.reset();
        g->d_mpairs.reset();
        g->d_merge_cell.reset();
    }
    return DMX_OK;
}

int dmx_chunk_merges(const dmx_chunk* c, int32_t* cell_pairs, int64_t* n) {
    if (!c || !n) return fail(DMX_ERR_ARG, "bad arguments");
    std::vector<int32_t> per_cell, uniq;
    const ParsedChunk& p = c->pc;
    if (int rc = normalize_merges((int64_t)p.cols * p.rows, p.merge_pairs.data(), (int64_t)p.merge_pairs.size() / 2,
                                  per_cell, uniq, true))
        return rc;
    const int64_t m = (int64_t)uniq.size() / 2;
    if (cell_pairs) {
        if (*n < m) return fail(DMX_ERR_ARG, "buffer too small");
        std::memcpy(cell_pairs, uniq.data(), uniq.size() * 4);
    }
    *n = m;
    return DMX_OK;
}

// The attribute rows in key order, and which of them the map's layers show (isObjectVisible, layermanager.h:84-87:
// LayerManagerImpl::m_visibleLayers & the row's layer key; m_visibleLayers is the second int64 the layer block
// stores, layermanagerimpl.cpp:90-105).
int dmx_chunk_rows(const dmx_chunk* c, int32_t* keys, uint8_t* visible) {
    if (!c) return fail(DMX_ERR_ARG, "chunk is NULL");
    const ParsedChunk& p = c->pc;
    int64_t shown = 1;   // a fresh LayerManagerImpl: "Everything" visible
    if (p.layers_raw.size() >= 16) std::memcpy(&shown, p.layers_raw.data() + 8, 8);
    for (size_t i = 0; i < p.row_keys.size(); i++) {
        if (keys) keys[i] = p.row_keys[i];
        if (visible) visible[i] = ((i < p.row_layers.size() ? p.row_layers[i] : 1) & shown) != 0;
    }
    return DMX_OK;
}

// Point::m_merge as stored: (cell, partner cell) of every point with a link, in x-major order of the cell.
int dmx_chunk_merge_records(const dmx_chunk* c, int32_t* cell_pairs, int64_t* n) {
    if (!c || !n) return fail(DMX_ERR_ARG, "bad arguments");
    const ParsedChunk& p = c->pc;
    const int64_t m = (int64_t)p.merge_pairs.size() / 2;
    if (cell_pairs) {
        if (*n < m) return fail(DMX_ERR_ARG, "buffer too small");
        if (m) std::memcpy(cell_pairs, p.merge_pairs.data(), p.merge_pairs.size() * 4);
    }
    *n = m;
    return DMX_OK;
}

// The isovist analysis's per-node data a parsed chunk stores (Bin::m_occ_distance, Node::m_occlusion_bins).
int dmx_chunk_occlusion(const dmx_chunk* c, float* occ_dist, int32_t* occ_counts, int32_t* occ_pixels, int64_t cap,
                        int64_t* total) {
    if (!c) return fail(DMX_ERR_ARG, "chunk is NULL");
    const ParsedChunk& p = c->pc;
    if (occ_dist && !p.occ_dist.empty()) std::memcpy(occ_dist, p.occ_dist.data(), p.occ_dist.size() * 4);
    if (occ_counts && !p.occ_counts.empty()) std::memcpy(occ_counts, p.occ_counts.data(), p.occ_counts.size() * 4);
    if (occ_pixels && cap >= (int64_t)p.occ_pixels.size() && !p.occ_pixels.empty())
        std::memcpy(occ_pixels, p.occ_pixels.data(), p.occ_pixels.size() * 4);
    if (total) *total = (int64_t)p.occ_pixels.size();
    return DMX_OK;
}

int dmx_chunk_set_occlusion(dmx_chunk* c, const float* occ_dist, const int32_t* occ_counts, const int32_t* occ_pixels) {
    if (!c || !occ_dist || !occ_counts) return fail(DMX_ERR_ARG, "bad arguments");
    int64_t total = 0;
    for (size_t i = 0; i < c->pc.gridconn.size() * 32; i++) total += occ_counts[i] > 0 ? occ_counts[i] : 0;
    if (total && !occ_pixels) return fail(DMX_ERR_ARG, "occlusion counts without pixels");
    std::string err;
    if (chunk_set_occlusion(c->pc, occ_dist, occ_counts, occ_pixels, err)) return fail(DMX_ERR_ARG, err);
    return DMX_OK;
}

int dmx_chunk_flags(const dmx_chunk* c, int* processed, int* boundary, int64_t* merges, int64_t* nrows) {
    if (!c) return fail(DMX_ERR_ARG, "chunk is NULL");
    if (processed) *processed = c->pc.processed ? 1 : 0;
    if (boundary) *boundary = c->pc.boundary ? 1 : 0;
    if (merges) *merges = c->pc.merges;
    if (nrows) *nrows = (int64_t)c->pc.row_keys.size();
    return DMX_OK;
}

int dmx_chunk_set_column(dmx_chunk* c, const char* name, const float* values, const uint8_t* setmask, int locked,
                         int make_displayed) {
    if (!c || !name || (!values && !c->pc.row_keys.empty())) return fail(DMX_ERR_ARG, "bad arguments");
    const int idx = chunk_set_column(c->pc, name, values, setmask, locked != 0);
    if (make_displayed) c->pc.displayed_phys = idx;
    return DMX_OK;
}

int dmx_chunk_set_displayed(dmx_chunk* c, int physical_column) {
    if (!c) return fail(DMX_ERR_ARG, "chunk is NULL");
    c->pc.displayed_phys = physical_column;
    return DMX_OK;
}

int dmx_chunk_set_name(dmx_chunk* c, const char* name) {
    if (!c || !name) return fail(DMX_ERR_ARG, "bad arguments");
    c->pc.name = name;
    return DMX_OK;
}

int dmx_chunk_select_cells(dmx_chunk* c, const int32_t* cells, int64_t n) {
    if (!c || (n && !cells)) return fail(DMX_ERR_ARG, "bad arguments");
    ParsedChunk& p = c->pc;
    const int64_t C = (int64_t)p.cols * p.rows;
    if ((int64_t)p.point_off.size() != C + 1) return fail(DMX_ERR_STATE, "chunk has no point records");
    for (int64_t i = 0; i < n; i++) {
        const int64_t cell = cells[i];
        if (cell < 0 || cell >= C) return fail(DMX_ERR_ARG, "cell outside the grid");
        if (!(p.state[cell] & CELL_FILLED)) continue;   // PointMap::setCurSel keeps filled cells only
        int32_t st;
        std::memcpy(&st, &p.points_raw[p.point_off[cell]], 4);
        st |= CELL_SELECTED;
        std::memcpy(&p.points_raw[p.point_off[cell]], &st, 4);
    }
    return DMX_OK;
}

int dmx_chunk_unmake(dmx_chunk* c, int remove_links) {
    if (!c) return fail(DMX_ERR_ARG, "chunk is NULL");
    std::string err;
    if (chunk_unmake(c->pc, remove_links != 0, err)) return fail(DMX_ERR_STATE, err);
    return DMX_OK;
}

// ---------------------------------------------------------------- the chunk's records on the GPU (chunk_codec.hip)
// Two slabs of the record stream in device memory and two in pinned host memory, with the events that order them.
struct CodecStage {
    DevBuf<uint8_t> dev[2];
    uint8_t* pin[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};     // the slab's last operation (its copy)
    hipEvent_t kernel[2] = {nullptr, nullptr};   // encode: the slab's kernels
    ~CodecStage() {
        for (int i = 0; i < 2; i++) {
            if (pin[i]) (void)hipHostFree(pin[i]);
            if (done[i]) (void)hipEventDestroy(done[i]);
            if (kernel[i]) (void)hipEventDestroy(kernel[i]);
        }
    }
    hipError_t init(size_t bytes, int nbuf) {
        for (int i = 0; i < nbuf; i++) {
            hipError_t e = dev[i].alloc(bytes);
            if (e == hipSuccess) e = hipHostMalloc((void**)&pin[i], std::max<size_t>(bytes, 1), hipHostMallocDefault);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&done[i], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&kernel[i], hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
};

static int64_t codec_slab_bytes() {
    const int64_t s = policy::hook_int("DMX_CODEC_SLAB", 0);
    return s > 0 ? s : policy::kCodecSlabBytes;
}

int dmx_graph_chunk_write(dmx_graph* g, const char* map_name, int ncols, const char* const* names, const float* values,
                          const uint8_t* locked, const uint8_t* setmask, int displayed, int boundary, uint8_t* buf,
                          int64_t cap, int64_t* size) {
    if (!g || !size || ncols < 0 || (ncols && (!names || !values))) return fail(DMX_ERR_ARG, "bad arguments");
    if (g->node_begin != 0 || g->node_end != g->nnodes)
        return fail(DMX_ERR_STATE, "a shard of a graph cannot be written as a chunk (assemble the whole graph first)");
    dmx_ctx* ctx = g->ctx;
    const PointMapHost& h = *g->pm->host;
    const int64_t N = g->nnodes, C = h.cells();
    // a name of its own: the bytes PointMap::read + ::write give for the renamed map (dmx_chunk_set_name + serialize)
    const bool named = map_name && std::strcmp(map_name, "VGA Map") != 0;
    if (named && ncols > 4096) return fail(DMX_ERR_ARG, "not a PointMap chunk");
    const std::vector<ChunkColumn> cols = chunk_columns(N, ncols, names, values, locked, setmask);
    std::vector<uint8_t> head, tail;
    std::string err;
    if (write_pointmap_head(h, N, true, cols, displayed, named ? map_name : "VGA Map", named, head, err))
        return fail(DMX_ERR_ARG, err);
    write_pointmap_tail(true, boundary != 0, tail);
    // per cell: the state as written, the merge partner, the node
    std::vector<int32_t> state(h.state()), cell_node((size_t)C, -1);
    {
        int32_t k = 0;
        for (int64_t c = 0; c < C; c++) {
            if (state[c] & CELL_FILLED) cell_node[c] = k++;
            if (named) state[c] &= kChunkStateMask;
        }
    }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DevBuf<int32_t> d_state, d_merge, d_cell_node;
    DevBuf<int64_t> d_sizes, d_offsets, d_tiles;
    DevBuf<int> d_err;
    const bool links = !h.merge().empty();
    const int64_t nt = (C + CC_SCAN_TILE - 1) / CC_SCAN_TILE;
    HIPCHK(d_state.alloc(C));
    HIPCHK(d_cell_node.alloc(C));
    if (links) HIPCHK(d_merge.alloc(C));
    HIPCHK(d_sizes.alloc(C));
    HIPCHK(d_offsets.alloc(C + 1));
    HIPCHK(d_tiles.alloc(nt + 1));
    HIPCHK(d_err.alloc(1));
    HIPCHK(hipMemcpyAsync(d_state.p, state.data(), C * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_cell_node.p, cell_node.data(), C * 4, hipMemcpyHostToDevice, s));
    if (links) HIPCHK(hipMemcpyAsync(d_merge.p, h.merge().data(), C * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_err.p, 0, sizeof(int), s));
    // sizes, then their exclusive scan
    hipLaunchKernelGGL(cc_size_kernel, dim3((unsigned)((C * 32 + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, s, C,
                       d_cell_node.p, g->bin_nruns.p, g->bin_count.p, d_sizes.p, d_err.p);
    hipLaunchKernelGGL(cc_scan_reduce_kernel, dim3((unsigned)nt), dim3(CC_THREADS), 0, s, d_sizes.p, C, d_tiles.p);
    hipLaunchKernelGGL(cc_scan_tiles_kernel, dim3(1), dim3(CC_THREADS), 0, s, d_tiles.p, nt);
    hipLaunchKernelGGL(cc_scan_down_kernel, dim3((unsigned)nt), dim3(CC_THREADS), 0, s, d_sizes.p, C, d_tiles.p, nt,
                       d_offsets.p);
    HIPCHK(hipGetLastError());
    int bad = 0;
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&bad, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(copy_sync(s, &total, d_offsets.p + C, 8, hipMemcpyDeviceToHost));
    if (bad) return fail(DMX_ERR_ARG, "bin with a node count but no runs");
    *size = (int64_t)head.size() + total + (int64_t)tail.size();
    if (!buf || cap < *size) return DMX_OK;
    std::vector<int64_t> off((size_t)C + 1);
    HIPCHK(copy_sync(s, off.data(), d_offsets.p, (C + 1) * 8, hipMemcpyDeviceToHost));
    std::memcpy(buf, head.data(), head.size());
    uint8_t* rec = buf + head.size();
    // the records, slab by slab: the next slab's kernels run beside the copy of this one
    if (!ctx->codec_stream) HIPCHK(hipStreamCreateWithFlags(&ctx->codec_stream, hipStreamNonBlocking));
    const int64_t slab = std::min(codec_slab_bytes(), std::max<int64_t>(total, 1));
    const int64_t ns = (total + slab - 1) / slab;
    CodecStage stg;
    HIPCHK(stg.init((size_t)slab, ns > 1 ? 2 : 1));
    const CodecCells M{d_state.p, links ? d_merge.p : nullptr, d_cell_node.p, d_offsets.p, h.rows(),
                       h.spacing(), h.bottom_left().x, h.bottom_left().y};
    auto drain = [&](int64_t j) -> hipError_t {   // slab j from its pinned buffer into buf
        hipError_t e = hipEventSynchronize(stg.done[j & 1]);
        if (e != hipSuccess) return e;
        const int64_t s0 = j * slab, s1 = std::min(total, s0 + slab);
        std::memcpy(rec + s0, stg.pin[j & 1], (size_t)(s1 - s0));
        return hipSuccess;
    };
    for (int64_t j = 0; j < ns; j++) {
        const int b = (int)(j & 1);
        if (j >= 2) HIPCHK(drain(j - 2));
        const int64_t s0 = j * slab, s1 = std::min(total, s0 + slab);
        // the cells whose records meet [s0, s1)
        const int64_t c0 = (std::upper_bound(off.begin(), off.end(), s0) - off.begin()) - 1;
        const int64_t c1 = std::lower_bound(off.begin(), off.end(), s1) - off.begin();
        hipLaunchKernelGGL(cc_cells_kernel, dim3((unsigned)((c1 - c0 + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, s,
                           M, g->gridconn.p, c0, c1, s0, s1, stg.dev[b].p);
        hipLaunchKernelGGL(cc_nodes_kernel, dim3((unsigned)(c1 - c0)), dim3(CC_THREADS), 0, s, M, g->pool.p,
                           g->node_run_start.p, g->bin_nruns.p, g->bin_count.p, g->bin_dist.p, c0, c1, s0, s1,
                           stg.dev[b].p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(stg.kernel[b], s));
        HIPCHK(hipStreamWaitEvent(ctx->codec_stream, stg.kernel[b], 0));
        HIPCHK(hipMemcpyAsync(stg.pin[b], stg.dev[b].p, (size_t)(s1 - s0), hipMemcpyDeviceToHost, ctx->codec_stream));
        HIPCHK(hipEventRecord(stg.done[b], ctx->codec_stream));
    }
    for (int64_t j = std::max<int64_t>(ns - 2, 0); j < ns; j++) HIPCHK(drain(j));
    HIPCHK(hipStreamSynchronize(s));
    std::memcpy(rec + total, tail.data(), tail.size());
    return DMX_OK;
}

int dmx_chunk_scan(const uint8_t* buf, int64_t size, int32_t* cols, int32_t* rows, int64_t* nnodes, int64_t* nruns,
                   int64_t* bytes_used) {
    if (!buf || size <= 0) return fail(DMX_ERR_ARG, "bad arguments");
    ChunkScan sc;
    std::string err;
    if (scan_pointmap_chunk(buf, (size_t)size, false, sc, err)) return fail(DMX_ERR_ARG, err);
    if (cols) *cols = sc.cols;
    if (rows) *rows = sc.rows;
    if (nnodes) *nnodes = sc.nnodes;
    if (nruns) *nruns = sc.nruns;
    if (bytes_used) *bytes_used = (int64_t)sc.bytes_used;
    return DMX_OK;
}

int dmx_chunk_load_bytes(dmx_ctx* ctx, const uint8_t* buf, int64_t size, const double* region, dmx_pointmap** pm_out,
                         dmx_graph** g_out) {
    if (!ctx || !buf || size <= 0 || !region || !pm_out || !g_out) return fail(DMX_ERR_ARG, "bad arguments");
    ChunkScan sc;
    {
        std::string err;
        if (scan_pointmap_chunk(buf, (size_t)size, true, sc, err)) return fail(DMX_ERR_ARG, err);
    }
    if (!sc.processed) return fail(DMX_ERR_STATE, "the point map has no graph (run VISPREP -pm first)");
    Rect r{region[0], region[1], region[2], region[3]};
    std::unique_ptr<dmx_pointmap> pm(new dmx_pointmap());
    pm->host.reset(new PointMapHost(r, sc.spacing, nullptr, 0));
    pm->host->load_state(sc.cols, sc.rows, sc.spacing, Vec2{sc.blx, sc.bly}, sc.state.data());
    HIPCHK(hipSetDevice(ctx->device));
    if (int rc = upload_pointmap(ctx, pm.get())) return rc;
    const int64_t N = sc.nnodes, N1 = std::max<int64_t>(N, 1);
    if (N != pm->nnodes) return fail(DMX_ERR_ARG, "node count does not match the filled cells of the map");
    // the three makeGraph attributes, where the table has the column and a row for every node
    std::vector<float> attrs((size_t)N1 * 3, 0.0f);
    if (sc.nrows == N)
        for (int64_t k = 0; k < N; k++)
            for (int j = 0; j < 3; j++)
                if (sc.has_attr[j]) attrs[k * 3 + j] = sc.attrs[k * 3 + j];
    std::vector<int64_t> start((size_t)N1, 0);
    int64_t acc = 0, longest = 0;
    for (int64_t k = 0; k < N; k++) {
        start[k] = acc;
        acc += sc.node_nruns[k];
        longest = std::max<int64_t>(longest, sc.node_len[k]);
    }
    std::unique_ptr<dmx_graph> g(new dmx_graph());
    g->ctx = ctx; g->pm = pm.get(); g->nnodes = N; g->node_begin = 0; g->node_end = N; g->nruns = acc;
    HIPCHK(g->pool.alloc(std::max<int64_t>(acc, 1)));
    HIPCHK(g->node_run_start.alloc(N1));
    HIPCHK(g->node_nruns.alloc(N1));
    HIPCHK(g->bin_nruns.alloc(N1 * 32));
    HIPCHK(g->bin_count.alloc(N1 * 32));
    HIPCHK(g->bin_dist.alloc(N1 * 32));
    HIPCHK(g->attrs.alloc(N1 * 3));
    HIPCHK(g->gridconn.alloc(N1));
    hipStream_t s = ctx->stream;
    DevBuf<int64_t> d_off;
    HIPCHK(d_off.alloc(N1));
    if (N) {
        HIPCHK(hipMemcpyAsync(g->node_run_start.p, start.data(), N * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(g->node_nruns.p, sc.node_nruns.data(), N * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(g->attrs.p, attrs.data(), N * 12, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(g->gridconn.p, sc.gridconn.data(), N, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_off.p, sc.node_off.data(), N * 8, hipMemcpyHostToDevice, s));
        // the node records, slab by slab: whole nodes whose bins lie within one slab's bytes of each other (a node
        // longer than the slab goes alone); the bytes between them (occlusion bins, cells without a node) ride along
        const int64_t slab = std::max(std::min(codec_slab_bytes(), sc.node_off[N - 1] + sc.node_len[N - 1] - sc.node_off[0]),
                                      longest);
        CodecStage stg;
        HIPCHK(stg.init((size_t)slab, 2));
        int64_t k0 = 0;
        for (int64_t j = 0; k0 < N; j++) {
            const int b = (int)(j & 1);
            const int64_t f0 = sc.node_off[k0];
            int64_t k1 = k0 + 1;
            while (k1 < N && sc.node_off[k1] + sc.node_len[k1] - f0 <= slab) k1++;
            const int64_t f1 = sc.node_off[k1 - 1] + sc.node_len[k1 - 1];
            if (j >= 2) HIPCHK(hipEventSynchronize(stg.done[b]));   // the buffers' previous slab is decoded
            std::memcpy(stg.pin[b], buf + f0, (size_t)(f1 - f0));
            HIPCHK(hipMemcpyAsync(stg.dev[b].p, stg.pin[b], (size_t)(f1 - f0), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(cc_decode_kernel, dim3((unsigned)(k1 - k0)), dim3(CC_THREADS), 0, s, stg.dev[b].p, f0, d_off.p,
                               g->node_run_start.p, k0, k1, g->pool.p, g->bin_nruns.p, g->bin_count.p, g->bin_dist.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(stg.done[b], s));
            k0 = k1;
        }
        HIPCHK(hipStreamSynchronize(s));
    }
    {
        std::vector<int32_t> per_cell, uniq;
        int rc = normalize_merges(pm->host->cells(), sc.merge_pairs.data(), (int64_t)sc.merge_pairs.size() / 2, per_cell,
                                  uniq, true);
        if (rc) return rc;
        pm->host->set_merge(std::move(per_cell));
    }
    inherit_merges(g.get());
    *pm_out = pm.release();
    *g_out = g.release();
    return DMX_OK;
}

int dmx_chunk_serialize(const dmx_chunk* c, uint8_t* buf, int64_t cap, int64_t* size) {
    if (!c || !size) return fail(DMX_ERR_ARG, "bad arguments");
    std::vector<uint8_t> out;
    std::string err;
    if (write_parsed_chunk(c->pc, out, err)) return fail(DMX_ERR_STATE, err);
    *size = (int64_t)out.size();
    if (buf) {
        if (cap < (int64_t)out.size()) return fail(DMX_ERR_ARG, "buffer too small");
        std::memcpy(buf, out.data(), out.size());
    }
    return DMX_OK;
}
