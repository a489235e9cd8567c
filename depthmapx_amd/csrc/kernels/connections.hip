// kernels/connections.hip -- a node's neighbourhood expanded from its run-length bins: Node::contents
// (salalib/ngraph.cpp:158-191 over Bin::first / next / cursor, :392-416) and the edge list
// PointMap::outputConnectionsAsCSV writes from it (salalib/pointdata.cpp:656-681).
//
// Enumeration of one node: bins 0..31, the runs of a bin in stored order, the cells of a run from its start along the
// bin's direction (Node::make, ngraph.cpp:43-54) until col(dir) passes the end's; the start cell is always visited,
// a diagonal bin is one span walked cell by cell.  Position p of the enumeration is cell i = p - prefix[r] of run r.
// A cell that occurred at an earlier position is dropped (addIfNotExists), cells outside the grid are dropped (the
// reference indexes out of bounds there).  The export flavour keeps, of what is left, the FILLED cells behind the
// source in x-major order.
//
// Two passes, one workgroup a node, nodes dealt through a work counter (progress / cancel as in thruvision.hip):
//   conn_count_kernel   marks the node's cells in a tiled bitmap (8x8-cell words, the layout of vga_tile.hip; in LDS
//                       while the grid fits, else in a per-workgroup slice of HBM, as vga_local.hip).  What survives
//                       deduplication is the SET of marked cells, whatever the order: items = popcount (contents) or
//                       popcount(marked & filled & behind the source) (export), bytes = the sum of the kept cells'
//                       line lengths.  A node whose marked cells are fewer than its enumerated cells inside the grid
//                       holds a duplicate: flagged for the emitting pass.
//   (exclusive scan of the items or bytes: the cc_scan_* kernels of chunk_codec.hip)
//   conn_emit_kernel    walks the enumeration in position order, 256 positions at a time, and writes the kept cells at
//                       the node's scanned offset plus a workgroup prefix sum: the output order is the reference's and
//                       does not depend on scheduling.  A node without duplicates needs no bitmap here (every cell
//                       inside the grid is a first occurrence).  A flagged node takes the exact path: per chunk of
//                       positions, a cell already marked by an EARLIER chunk is a duplicate; the others mark
//                       themselves, and only when two of them met in the same word bit (the atomic OR returned the bit
//                       set) the chunk compares its cells pairwise, the lower position keeping the cell.  A test-and-
//                       set alone would pick a winner, not the first.
// Text lines ("\n" from delim to) are assembled in LDS per chunk and leave as aligned dwords; only the bytes in
// front of the first and behind the last whole dword of a chunk are byte stores, so two workgroups never store to
// the same dword.  Vector stores only; no kernel traps.
#pragma once
#include "common.hpp"

namespace dmx {

constexpr int CONN_THREADS = 256;
constexpr int CONN_LINE_MAX = 32;   // "\n" + 10 digits + 8 bytes of delimiter + 10 digits = 29
enum { CONN_CONTENTS = 0, CONN_EXPORT = 1, CONN_TEXT = 2 };   // refs of Node::contents, refs of the export, its text

struct ConnParams {
    int cols, rows, tw, th;
    const int32_t* node_cell;            // [N] global node -> x-major cell
    const int64_t* node_run_start;       // graph arrays: indexed by the node's index in the graph (node - local0)
    const int32_t* node_nruns;
    const int32_t* bin_nruns;
    const Run* pool;
    const unsigned long long* seed_tiles;   // bit set: the cell is not FILLED (or padding)
    int64_t node_begin, node_end, local0;
    int mode;
    int dlen;
    unsigned char delim[8];
    int* work_counter;
    DmxCtl* ctl;
    unsigned long long* gbm;             // HBM bitmap slices (nt words a workgroup) or null
    int64_t* items;                      // [n] kept cells (refs) or bytes (text) of each node of the range
    unsigned char* dup;                  // [n] the node holds a duplicate
    unsigned long long* stats;           // [0] nodes with duplicates, [1] cells dropped as duplicates, [2] outside the grid
    const int64_t* off;                  // [n + 1] scanned items (emit)
    int32_t* refs;                       // emit, refs form
    unsigned char* text;                 // emit, text form
};

// bitmap word access: LDS, or an HBM slice read and written past the CU's L1 (the workgroup's waves share it)
template <bool GBM> __device__ __forceinline__ unsigned long long conn_bm_load(unsigned long long* p) {
    if (GBM) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}
template <bool GBM> __device__ __forceinline__ void conn_bm_clear(unsigned long long* p) {
    if (GBM) __hip_atomic_store(p, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = 0ull;
}
template <bool GBM> __device__ __forceinline__ unsigned long long conn_bm_or(unsigned long long* p, unsigned long long m) {
    if (GBM) return __hip_atomic_fetch_or(p, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return atomicOr(p, m);
}

__device__ __forceinline__ int conn_digits(uint32_t v) {
    int n = 1;
    while (v >= 10u) { v /= 10u; n++; }
    return n;
}
// decimal of v into dst[0 .. n), n = conn_digits(v)
__device__ __forceinline__ void conn_put_digits(unsigned char* dst, uint32_t v, int n) {
    for (int i = n - 1; i >= 0; i--) { dst[i] = (unsigned char)('0' + v % 10u); v /= 10u; }
}

// A run as the reference walks it: start, step, cells (>= 1: the start is visited before the end is compared).
struct ConnRun {
    int x0, y0, dx, dy, n;
};
__device__ __forceinline__ ConnRun conn_run(Run ru, int bin) {
    ConnRun c;
    const int dir = cc_bin_dir(bin);
    c.x0 = ru.x0; c.y0 = ru.y0;
    c.dx = (dir == CC_DIR_V) ? 0 : 1;
    c.dy = (dir == CC_DIR_V || dir == CC_DIR_PD) ? 1 : ((dir == CC_DIR_ND) ? -1 : 0);
    const int span = (dir == CC_DIR_V) ? ((int)ru.y1 - (int)ru.y0) : ((int)ru.x1 - (int)ru.x0);
    c.n = span > 0 ? span + 1 : 1;
    return c;
}
// the steps [lo, hi] of the run that lie inside the grid (empty: lo > hi)
__device__ __forceinline__ void conn_clip(const ConnRun& c, int cols, int rows, int& lo, int& hi) {
    lo = 0; hi = c.n - 1;
    if (c.dx) { lo = max(lo, -c.x0); hi = min(hi, cols - 1 - c.x0); }
    else if (c.x0 < 0 || c.x0 >= cols) hi = -1;
    if (c.dy > 0) { lo = max(lo, -c.y0); hi = min(hi, rows - 1 - c.y0); }
    else if (c.dy < 0) { lo = max(lo, c.y0 - (rows - 1)); hi = min(hi, c.y0); }
    else if (c.y0 < 0 || c.y0 >= rows) hi = -1;
}

// the bin of run r of a node: binstart[b] = runs in bins 0 .. b - 1 (33 entries)
__device__ __forceinline__ int conn_bin_of(const int* binstart, int r) {
    int b = 0;
    for (int s = 16; s >= 1; s >>= 1)
        if (binstart[b + s] <= r) b += s;
    return b;
}

// exclusive prefix of v over the workgroup, *total its sum.  wsum: CONN_THREADS / 64 + 1 entries of LDS.
__device__ __forceinline__ int conn_exscan(int v, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int a = __shfl_up(incl, d);
        if (lane >= d) incl += a;
    }
    __syncthreads();   // wsum's previous readers are done
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < CONN_THREADS / 64; w++) {
        if (w < wave) base += wsum[w];
        tot += wsum[w];
    }
    *total = tot;
    return base + incl - v;
}

// take the next node of the range (one grab a workgroup; the grab polls the control block)
__device__ __forceinline__ int64_t conn_next(const ConnParams& P, int* s_w) {
    __syncthreads();
    if (threadIdx.x == 0) *s_w = ctl_poll(P.ctl, atomicAdd(P.work_counter, 1));
    __syncthreads();
    return P.node_begin + *s_w;
}

// the 33 bin starts of node k into LDS (first wave)
__device__ __forceinline__ void conn_bin_starts(const int32_t* bin_nruns, int64_t k, int* binstart) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        const int v = lane < 32 ? bin_nruns[k * 32 + lane] : 0;
        int incl = v;
        for (int d = 1; d < 32; d <<= 1) {
            const int a = __shfl_up(incl, d);
            if (lane >= d) incl += a;
        }
        if (lane < 32) binstart[lane + 1] = incl;
        if (lane == 0) binstart[0] = 0;
    }
}

template <bool GBM>
__global__ void __launch_bounds__(CONN_THREADS) conn_count_kernel(ConnParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long conn_lds[];
    __shared__ int s_w, s_binstart[33];
    __shared__ long long s_red[3][CONN_THREADS / 64];
    const int nt = P.tw * P.th;
    unsigned long long* const bm = GBM ? P.gbm + (size_t)blockIdx.x * nt : conn_lds;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long dup_nodes = 0, dup_cells = 0;   // thread 0's
    for (int64_t node = conn_next(P, &s_w); node < P.node_end; node = conn_next(P, &s_w)) {
        const int64_t k = node - P.local0;
        const int src = P.node_cell[node];
        const int sx = src / P.rows, sy = src % P.rows;
        for (int t = threadIdx.x; t < nt; t += CONN_THREADS) conn_bm_clear<GBM>(&bm[t]);
        conn_bin_starts(P.bin_nruns, k, s_binstart);
        __syncthreads();
        const int64_t rs = P.node_run_start[k];
        const int nr = P.node_nruns[k];
        long long e_in = 0, e_all = 0;
        for (int r = threadIdx.x; r < nr; r += CONN_THREADS) {
            const ConnRun c = conn_run(P.pool[rs + r], conn_bin_of(s_binstart, r));
            int lo, hi;
            conn_clip(c, P.cols, P.rows, lo, hi);
            e_all += c.n;
            if (lo > hi) continue;
            e_in += hi - lo + 1;
            Run in;
            in.x0 = (int16_t)(c.x0 + lo * c.dx); in.y0 = (int16_t)(c.y0 + lo * c.dy);
            in.x1 = (int16_t)(c.x0 + hi * c.dx); in.y1 = (int16_t)(c.y0 + hi * c.dy);
            run_tile_words(P.tw, in, [&](int w, unsigned long long m) { conn_bm_or<GBM>(&bm[w], m); });
        }
        __syncthreads();
        // the set of marked cells: how many, how many of them the export keeps, and their lines' bytes
        long long u = 0, items = 0;
        const int flen = 1 + conn_digits(((uint32_t)sx << 16) + (uint32_t)(sy & 0xffff)) + P.dlen;
        for (int t = threadIdx.x; t < nt; t += CONN_THREADS) {
            unsigned long long m = conn_bm_load<GBM>(&bm[t]);
            u += __popcll(m);
            if (P.mode == CONN_CONTENTS) continue;
            const int tx = t % P.tw, ty = t / P.tw;
            m &= ~P.seed_tiles[t];
            // behind the source in x-major order: x > sx, or x == sx and y > sy
            if (tx * 8 + 7 < sx) m = 0ull;
            else if (tx * 8 <= sx) {
                const int lx = sx - tx * 8;
                unsigned long long keep = ~(0x0101010101010101ull * (0xFFull >> (7 - lx)));   // columns right of sx
                const int yl = sy + 1 - ty * 8;                                                   // rows >= yl of column sx
                if (yl < 8) keep |= (0x0101010101010101ull << lx) & (yl <= 0 ? ~0ull : (~0ull << (8 * yl)));
                m &= keep;
            }
            if (P.mode == CONN_EXPORT) items += __popcll(m);
            else
                while (m) {
                    const int b = __builtin_ctzll(m);
                    m &= m - 1;
                    const uint32_t x = (uint32_t)(tx * 8 + (b & 7)), y = (uint32_t)(ty * 8 + (b >> 3));
                    items += flen + conn_digits((x << 16) + (y & 0xffffu));
                }
        }
        if (P.mode == CONN_CONTENTS) items = u;
        for (int off = 32; off >= 1; off >>= 1) {
            u += __shfl_xor(u, off);
            items += __shfl_xor(items, off);
            e_in += __shfl_xor(e_in, off);
            e_all += __shfl_xor(e_all, off);
        }
        if (lane == 0) { s_red[0][wave] = u; s_red[1][wave] = items; s_red[2][wave] = e_in; }
        __syncthreads();
        if (threadIdx.x == 0) {
            long long ut = 0, it = 0, et = 0;
            for (int w = 0; w < CONN_THREADS / 64; w++) { ut += s_red[0][w]; it += s_red[1][w]; et += s_red[2][w]; }
            P.items[node - P.node_begin] = it;
            P.dup[node - P.node_begin] = et != ut;
            if (et != ut) { dup_nodes++; dup_cells += (unsigned long long)(et - ut); }
        }
        if (lane == 0 && e_all != e_in) atomicAdd(&P.stats[2], (unsigned long long)(e_all - e_in));   // each wave its own
    }
    if (threadIdx.x == 0 && dup_nodes) {
        atomicAdd(&P.stats[0], dup_nodes);
        atomicAdd(&P.stats[1], dup_cells);
    }
}

template <bool GBM>
__global__ void __launch_bounds__(CONN_THREADS) conn_emit_kernel(ConnParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long conn_lds[];
    __shared__ int s_w, s_binstart[33], s_wsum[CONN_THREADS / 64 + 1], s_conf;
    __shared__ int s_pref[CONN_THREADS + 1];          // cells before each run of the tile of runs
    __shared__ ConnRun s_run[CONN_THREADS];
    __shared__ int s_cell[CONN_THREADS];              // exact path: the chunk's candidate cells
    __shared__ __attribute__((aligned(16))) unsigned char s_text[CONN_THREADS * CONN_LINE_MAX];
    __shared__ unsigned char s_from[12];
    const int nt = P.tw * P.th;
    unsigned long long* const bm = GBM ? P.gbm + (size_t)blockIdx.x * nt : conn_lds;
    const int tid = threadIdx.x;
    for (int64_t node = conn_next(P, &s_w); node < P.node_end; node = conn_next(P, &s_w)) {
        const int64_t k = node - P.local0, kn = node - P.node_begin;
        const int64_t o0 = P.off[kn], oend = P.off[kn + 1];
        if (oend == o0) continue;   // nothing kept
        const bool exact = P.dup[kn] != 0;
        const int src = P.node_cell[node];
        const int sx = src / P.rows, sy = src % P.rows;
        const uint32_t fromv = ((uint32_t)sx << 16) + (uint32_t)(sy & 0xffff);
        const int fdig = conn_digits(fromv);
        if (exact)
            for (int t = tid; t < nt; t += CONN_THREADS) conn_bm_clear<GBM>(&bm[t]);
        conn_bin_starts(P.bin_nruns, k, s_binstart);
        if (tid == 0 && P.mode == CONN_TEXT) conn_put_digits(s_from, fromv, fdig);
        __syncthreads();
        const int64_t rs = P.node_run_start[k];
        const int nr = P.node_nruns[k];
        int64_t base = o0;   // items (bytes) of the node written so far, the same in every thread
        for (int r0 = 0; r0 < nr; r0 += CONN_THREADS) {
            // a tile of runs: their walks and the prefix of their lengths
            ConnRun mine;
            mine.n = 0;
            if (r0 + tid < nr) mine = conn_run(P.pool[rs + r0 + tid], conn_bin_of(s_binstart, r0 + tid));
            int T;
            const int ex = conn_exscan(mine.n, s_wsum, &T);
            s_pref[tid] = ex;
            s_run[tid] = mine;
            if (tid == 0) s_pref[CONN_THREADS] = T;
            __syncthreads();
            for (int p0 = 0; p0 < T; p0 += CONN_THREADS) {
                const int p = p0 + tid;
                int x = -1, y = -1;
                bool kept = false;
                if (p < T) {
                    int j = 0;   // the last run of the tile that starts at or before p (empty slots start at T)
                    for (int s = CONN_THREADS / 2; s >= 1; s >>= 1)
                        if (s_pref[j + s] <= p) j += s;
                    const ConnRun c = s_run[j];
                    const int i = p - s_pref[j];
                    x = c.x0 + i * c.dx;
                    y = c.y0 + i * c.dy;
                    kept = x >= 0 && x < P.cols && y >= 0 && y < P.rows;
                }
                const int w = kept ? (y >> 3) * P.tw + (x >> 3) : 0;
                const unsigned long long bit = 1ull << ((y & 7) * 8 + (x & 7));
                if (exact) {
                    // first occurrences only: not marked by an earlier chunk, and the lowest position of this chunk
                    if (tid == 0) s_conf = 0;
                    if (kept && (conn_bm_load<GBM>(&bm[w]) & bit)) kept = false;
                    s_cell[tid] = kept ? x * P.rows + y : -1;
                    __syncthreads();
                    if (kept && (conn_bm_or<GBM>(&bm[w], bit) & bit)) s_conf = 1;
                    __syncthreads();
                    if (s_conf && kept) {
                        const int me = s_cell[tid];
                        for (int q = 0; q < tid; q++)
                            if (s_cell[q] == me) { kept = false; break; }
                    }
                }
                if (kept && P.mode != CONN_CONTENTS) {
                    kept = !(P.seed_tiles[w] & bit) && (x > sx || (x == sx && y > sy));
                }
                const uint32_t tov = ((uint32_t)x << 16) + (uint32_t)(y & 0xffff);
                const int tdig = kept ? conn_digits(tov) : 0;
                const int size = !kept ? 0 : (P.mode == CONN_TEXT ? 1 + fdig + P.dlen + tdig : 1);
                int total;
                const int at = conn_exscan(size, s_wsum, &total);
                // (the counting pass sized the node's span [o0, oend); no store may leave it)
                if (P.mode != CONN_TEXT) {
                    if (kept && base + at < oend) P.refs[base + at] = (int32_t)tov;
                } else if (total) {
                    total = (int)min((int64_t)total, max(oend - base, (int64_t)0));
                    if (kept) {
                        unsigned char* l = s_text + at;
                        l[0] = '\n';
                        for (int i = 0; i < fdig; i++) l[1 + i] = s_from[i];
                        for (int i = 0; i < P.dlen; i++) l[1 + fdig + i] = P.delim[i];
                        conn_put_digits(l + 1 + fdig + P.dlen, tov, tdig);
                    }
                    __syncthreads();
                    // [base, base + total) of the text: bytes up to the first aligned dword, dwords, bytes behind
                    unsigned char* const g = P.text + base;
                    const int head = min((int)((4 - ((size_t)g & 3)) & 3), total);
                    const int ndw = (total - head) >> 2;
                    const int tail = head + ndw * 4;
                    if (tid < head) g[tid] = s_text[tid];
                    for (int d = tid; d < ndw; d += CONN_THREADS) {
                        const unsigned char* s = s_text + head + d * 4;
                        *(uint32_t*)(g + head + d * 4) = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) |
                                                          ((uint32_t)s[3] << 24);
                    }
                    if (tid < total - tail) g[tail + tid] = s_text[tail + tid];
                }
                base += total;
                __syncthreads();   // s_text, s_cell and s_conf are free for the next chunk
            }
            __syncthreads();   // s_pref / s_run are free for the next tile of runs
        }
    }
}

} // namespace dmx
