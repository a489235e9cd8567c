// kernels/chunk_codec.hip -- the Point / Node records of a .graph PointMap chunk, encoded from and decoded into
// the device graph (Point::write point.cpp:51-73, Node::write / Bin::write / PixelVec::write ngraph.cpp:209-220,
// :447-472, :517-583; Bin::read / PixelVec::read :420-445, :491-563).  The host twin is host/graphio.cpp; every
// quirk there is kept here bit for bit.
//
// Encode, three steps:
//   cc_size_kernel      bytes of every cell's record: 34, and for a cell with a node 32 x 11 + 128 more plus each
//                       bin's payload (none for a u16 count of 0, 6 for a diagonal bin, 8 + 4 (u16 runs - 1) else)
//   cc_scan_*           64-bit exclusive scan of the sizes in x-major cell order (reduce, scan of the tile sums by
//                       one workgroup, down-sweep)
//   cc_cells_kernel     the 18-byte head and the 16-byte m_location of every cell (34 bytes a cell: byte stores)
//   cc_nodes_kernel     one workgroup a node: the 32 bins and the empty occlusion bins.  Records start at odd
//                       offsets and the run entries are 4 bytes at odd offsets, so the workgroup assembles its
//                       span of the stream in LDS, CC_WINDOW bytes at a time, and writes the window out as aligned
//                       dwords (a wave stores 256 contiguous bytes); only the bytes in front of the first and behind
//                       the last whole dword of the span are byte stores, so two workgroups never store to the same
//                       dword.
// A launch covers a byte range [s0, s1) of the record stream (a slab): every store is clipped to it, so a record
// may begin in one slab and end in a later one.
//
// Decode: cc_decode_kernel, one workgroup a node, reads only [node_off, node_off + node_len) of the chunk, the
// extent scan_pointmap_chunk walked with the same hops; it writes bin_nruns / bin_count / bin_dist and the node's
// runs (the cumulative 4-bit shift is a wave prefix sum with a carry across tiles of 64 entries).
#pragma once
#include "common.hpp"

namespace dmx {

constexpr int CC_THREADS = 256;
constexpr int CC_WINDOW = 16384;          // bytes of the stream a workgroup assembles in LDS at a time
constexpr int CC_SCAN_ITEMS = 8;          // cells a thread scans
constexpr int CC_SCAN_TILE = CC_THREADS * CC_SCAN_ITEMS;
constexpr int CC_DIR_H = 1, CC_DIR_V = 2, CC_DIR_PD = 4, CC_DIR_ND = 8, CC_DIR_DIAG = 12;

// Bin direction of bin b (Node::make, ngraph.cpp:43-54)
__host__ __device__ inline int cc_bin_dir(int b) {
    if (b == 4 || b == 20) return CC_DIR_PD;
    if (b == 12 || b == 28) return CC_DIR_ND;
    if ((b > 4 && b < 12) || (b > 20 && b < 28)) return CC_DIR_V;
    return CC_DIR_H;
}

// Bytes of a bin's run payload as Bin::write emits it; -1: a node count without runs (the writer refuses it).
__device__ __forceinline__ int cc_payload_bytes(int b, unsigned count16, int nr) {
    if (!count16) return 0;
    if (nr <= 0) return -1;
    if (cc_bin_dir(b) & CC_DIR_DIAG) return 6;
    const int len = nr & 0xFFFF;   // the u16 cast of the run count
    return 8 + 4 * (len > 0 ? len - 1 : 0);
}

// ---------------------------------------------------------------- sizes
// 32 lanes a cell, one a bin; sizes[c] = bytes of cell c's record.  *err is set for a bin with a count and no runs.
__global__ void __launch_bounds__(CC_THREADS) cc_size_kernel(int64_t C, const int32_t* __restrict__ cell_node,
                                                               const int32_t* __restrict__ bin_nruns,
                                                               const uint16_t* __restrict__ bin_count,
                                                               int64_t* __restrict__ sizes, int* __restrict__ err) {
    const int64_t t = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const int64_t c = t >> 5;
    const int b = (int)(t & 31);
    const int k = c < C ? cell_node[c] : -1;
    int sz = 0;
    if (k >= 0) {
        const int pay = cc_payload_bytes(b, bin_count[(int64_t)k * 32 + b], bin_nruns[(int64_t)k * 32 + b]);
        if (pay < 0) atomicOr(err, 1);
        sz = 11 + (pay > 0 ? pay : 0);
    }
    for (int d = 16; d >= 1; d >>= 1) sz += __shfl_xor(sz, d, 32);
    if (b == 0 && c < C) sizes[c] = 34 + (k >= 0 ? sz + 128 : 0);
}

// ---------------------------------------------------------------- 64-bit exclusive scan
// exclusive prefix of v over the workgroup; *total = the workgroup's sum.  tmp: CC_THREADS entries of LDS.
__device__ __forceinline__ int64_t cc_block_exscan(int64_t v, int64_t* tmp, int64_t* total) {
    const int t = threadIdx.x;
    tmp[t] = v;
    __syncthreads();
    for (int d = 1; d < CC_THREADS; d <<= 1) {
        const int64_t a = t >= d ? tmp[t - d] : 0;
        __syncthreads();
        tmp[t] += a;
        __syncthreads();
    }
    const int64_t incl = tmp[t];
    *total = tmp[CC_THREADS - 1];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(CC_THREADS) cc_scan_reduce_kernel(const int64_t* __restrict__ sizes, int64_t n,
                                                                      int64_t* __restrict__ tile_sums) {
    __shared__ int64_t tmp[CC_THREADS];
    const int64_t base = (int64_t)blockIdx.x * CC_SCAN_TILE + (int64_t)threadIdx.x * CC_SCAN_ITEMS;
    int64_t s = 0;
    for (int i = 0; i < CC_SCAN_ITEMS; i++)
        if (base + i < n) s += sizes[base + i];
    int64_t total;
    (void)cc_block_exscan(s, tmp, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// one workgroup: tile_sums[0 .. nt) -> their exclusive prefix in place, tile_sums[nt] = the grand total
__global__ void __launch_bounds__(CC_THREADS) cc_scan_tiles_kernel(int64_t* __restrict__ tile_sums, int64_t nt) {
    __shared__ int64_t tmp[CC_THREADS];
    int64_t carry = 0;
    for (int64_t i0 = 0; i0 < nt; i0 += CC_THREADS) {
        const int64_t i = i0 + threadIdx.x;
        const int64_t v = i < nt ? tile_sums[i] : 0;
        int64_t total;
        const int64_t ex = cc_block_exscan(v, tmp, &total);
        if (i < nt) tile_sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tile_sums[nt] = carry;
}

// offsets[0 .. n] = exclusive prefix of sizes (offsets[n] = the total)
__global__ void __launch_bounds__(CC_THREADS) cc_scan_down_kernel(const int64_t* __restrict__ sizes, int64_t n,
                                                                    const int64_t* __restrict__ tile_sums, int64_t nt,
                                                                    int64_t* __restrict__ offsets) {
    __shared__ int64_t tmp[CC_THREADS];
    const int64_t base = (int64_t)blockIdx.x * CC_SCAN_TILE + (int64_t)threadIdx.x * CC_SCAN_ITEMS;
    int64_t v[CC_SCAN_ITEMS];
    int64_t s = 0;
    for (int i = 0; i < CC_SCAN_ITEMS; i++) {
        v[i] = base + i < n ? sizes[base + i] : 0;
        s += v[i];
    }
    int64_t total;
    int64_t acc = tile_sums[blockIdx.x] + cc_block_exscan(s, tmp, &total);
    for (int i = 0; i < CC_SCAN_ITEMS; i++) {
        if (base + i < n) offsets[base + i] = acc;
        acc += v[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[n] = tile_sums[nt];
}

// ---------------------------------------------------------------- encode
struct CodecCells {
    const int32_t* state;      // [C] Point::m_state as written (masked by the caller where the format masks it)
    const int32_t* merge;      // [C] merge partner cell or -1; NULL: no links
    const int32_t* cell_node;  // [C] node of the cell or -1
    const int64_t* offsets;    // [C + 1] start of each cell's record in the record stream
    int rows;
    double spacing, blx, bly;
};

// the slab: bytes [s0, s1) of the record stream land at out[0 .. s1 - s0)
__device__ __forceinline__ void cc_put(uint8_t* out, int64_t s0, int64_t s1, int64_t pos, uint32_t byte) {
    if (pos >= s0 && pos < s1) out[pos - s0] = (uint8_t)byte;
}

// Head (m_state, m_block, dummy, m_grid_connections, m_merge, has-node) and m_location of the cells [c0, c1).
__global__ void __launch_bounds__(CC_THREADS) cc_cells_kernel(CodecCells M, const uint8_t* __restrict__ gridconn,
                                                                int64_t c0, int64_t c1, int64_t s0, int64_t s1,
                                                                uint8_t* __restrict__ out) {
    const int64_t c = c0 + (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (c >= c1) return;
    const int64_t rec = M.offsets[c], end = M.offsets[c + 1];
    const int k = M.cell_node[c];
    const uint32_t st = (uint32_t)M.state[c];
    const int32_t mc = M.merge ? M.merge[c] : -1;
    // the merge partner as PixelRef {short x, short y}; NoPixel = (-1, -1)
    const uint32_t mx = mc >= 0 ? (uint32_t)(uint16_t)(int16_t)(mc / M.rows) : 0xFFFFu;
    const uint32_t my = mc >= 0 ? (uint32_t)(uint16_t)(int16_t)(mc % M.rows) : 0xFFFFu;
    const uint32_t gc = k >= 0 ? gridconn[k] : 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) cc_put(out, s0, s1, rec + j, st >> (8 * j));
#pragma unroll
    for (int j = 4; j < 12; j++) cc_put(out, s0, s1, rec + j, 0u);
    cc_put(out, s0, s1, rec + 12, gc);
    cc_put(out, s0, s1, rec + 13, mx);
    cc_put(out, s0, s1, rec + 14, mx >> 8);
    cc_put(out, s0, s1, rec + 15, my);
    cc_put(out, s0, s1, rec + 16, my >> 8);
    cc_put(out, s0, s1, rec + 17, k >= 0 ? 1u : 0u);
    // PointMap::depixelate (pointdata.h:353-357): bottom left + spacing * x, one multiply and one add in FP64
    const int x = (int)(c / M.rows), y = (int)(c % M.rows);
    const unsigned long long lx = (unsigned long long)__double_as_longlong(__dadd_rn(M.blx, __dmul_rn(M.spacing, (double)x)));
    const unsigned long long ly = (unsigned long long)__double_as_longlong(__dadd_rn(M.bly, __dmul_rn(M.spacing, (double)y)));
#pragma unroll
    for (int j = 0; j < 8; j++) {
        cc_put(out, s0, s1, end - 16 + j, (uint32_t)(lx >> (8 * j)));
        cc_put(out, s0, s1, end - 8 + j, (uint32_t)(ly >> (8 * j)));
    }
}

// ShiftLength {unsigned short shift:4; unsigned short runlength:12;} (ngraph.cpp:536-539)
__device__ __forceinline__ uint32_t cc_shift_length(int shift, int runlength) {
    return ((uint32_t)shift & 0xFu) | (((uint32_t)runlength & 0xFFFu) << 4);
}

// The 32 bins and the 32 empty occlusion bins of the nodes among the cells [c0, c1): one workgroup a cell.
__global__ void __launch_bounds__(CC_THREADS) cc_nodes_kernel(CodecCells M, const Run* __restrict__ pool,
                                                                const int64_t* __restrict__ node_run_start,
                                                                const int32_t* __restrict__ bin_nruns,
                                                                const uint16_t* __restrict__ bin_count,
                                                                const float* __restrict__ bin_dist, int64_t c0, int64_t c1,
                                                                int64_t s0, int64_t s1, uint8_t* __restrict__ out) {
    __shared__ uint32_t win[CC_WINDOW / 4];
    __shared__ uint8_t hdr[32][20];   // each bin's header and first run as written
    __shared__ int hlen[32];          // ... their bytes: 11, 17 (diagonal) or 19
    __shared__ int boff[33];          // start of each bin's bytes behind the cell head; [32]: the occlusion bins
    __shared__ int brun[33];          // the node's runs in front of each bin
    const int64_t c = c0 + blockIdx.x;
    if (c >= c1) return;
    const int k = M.cell_node[c];
    if (k < 0) return;
    const int64_t R0 = M.offsets[c] + 18, R1 = M.offsets[c + 1] - 16;
    const int64_t a = R0 > s0 ? R0 : s0, e = R1 < s1 ? R1 : s1;
    if (a >= e) return;
    const int tid = threadIdx.x;
    const int64_t rs = node_run_start[k];
    if (tid < 64) {   // the first wave: lanes 0..31 take a bin each
        const int b = tid & 31;
        const unsigned count = bin_count[(int64_t)k * 32 + b];
        const int nr = bin_nruns[(int64_t)k * 32 + b];
        int pay = cc_payload_bytes(b, count, nr);
        if (pay < 0) pay = 0;   // (refused by the size pass: never encoded)
        int sz = 11 + pay, rn = nr > 0 ? nr : 0;
        int isz = sz, irn = rn;   // inclusive prefix over the 32 bins
        for (int d = 1; d < 32; d <<= 1) {
            const int ts = __shfl_up(isz, d, 32), tr = __shfl_up(irn, d, 32);
            if (b >= d) { isz += ts; irn += tr; }
        }
        if (tid < 32) {
            boff[b] = isz - sz;
            brun[b] = irn - rn;
            if (b == 31) { boff[32] = isz; brun[32] = irn; }
            const uint32_t dir = nr > 0 ? (uint32_t)cc_bin_dir(b) : 0u;   // empty bins keep NODIR (dmx_graph_copy)
            const uint32_t dist = __float_as_uint(bin_dist[(int64_t)k * 32 + b]);
            uint8_t* h = hdr[b];
            h[0] = (uint8_t)dir;
            h[1] = (uint8_t)count;
            h[2] = (uint8_t)(count >> 8);
            h[3] = (uint8_t)dist; h[4] = (uint8_t)(dist >> 8); h[5] = (uint8_t)(dist >> 16); h[6] = (uint8_t)(dist >> 24);
            h[7] = 0; h[8] = 0; h[9] = 0; h[10] = 0;   // m_occ_distance
            int hl = 11;
            if (pay > 0) {
                const Run r = pool[rs + irn - rn];
                if (dir & CC_DIR_DIAG) {
                    const uint32_t len = (uint32_t)(uint16_t)(r.x1 - r.x0);
                    h[11] = (uint8_t)r.x0; h[12] = (uint8_t)((uint16_t)r.x0 >> 8);
                    h[13] = (uint8_t)r.y0; h[14] = (uint8_t)((uint16_t)r.y0 >> 8);
                    h[15] = (uint8_t)len; h[16] = (uint8_t)(len >> 8);
                    hl = 17;
                } else {
                    const uint32_t n16 = (uint32_t)nr & 0xFFFFu;
                    const uint32_t len = (uint32_t)(uint16_t)((dir & CC_DIR_V) ? r.y1 - r.y0 : r.x1 - r.x0);
                    h[11] = (uint8_t)n16; h[12] = (uint8_t)(n16 >> 8);
                    h[13] = (uint8_t)r.x0; h[14] = (uint8_t)((uint16_t)r.x0 >> 8);
                    h[15] = (uint8_t)r.y0; h[16] = (uint8_t)((uint16_t)r.y0 >> 8);
                    h[17] = (uint8_t)len; h[18] = (uint8_t)(len >> 8);
                    hl = 19;
                }
            }
            hlen[b] = hl;
        }
    }
    __syncthreads();
    uint8_t* wb = reinterpret_cast<uint8_t*>(win);
    // windows start on a dword of the slab buffer
    for (int64_t w = a - ((a - s0) & 3); w < e; w += CC_WINDOW) {
        const int64_t lo = w > a ? w : a, hi = w + CC_WINDOW < e ? w + CC_WINDOW : e;   // [lo, hi): this window's bytes
        // bin headers with the first run
        for (int i = tid; i < 32 * 19; i += CC_THREADS) {
            const int b = i / 19, j = i - b * 19;
            const int64_t pos = R0 + boff[b] + j;
            if (j < hlen[b] && pos >= lo && pos < hi) wb[pos - w] = hdr[b][j];
        }
        // the empty occlusion bins: 32 zero counts
        if (tid < 128) {
            const int64_t pos = R0 + boff[32] + tid;
            if (pos >= lo && pos < hi) wb[pos - w] = 0;
        }
        // the later runs of the H / V bins: primary coordinate, ShiftLength against the run before
        for (int b = 0; b < 32; b++) {
            const int64_t E0 = R0 + boff[b] + 19, E1 = R0 + boff[b + 1];   // the entries' bytes
            if (hlen[b] != 19 || E1 <= lo || E0 >= hi || E1 <= E0) continue;
            const bool vert = (cc_bin_dir(b) & CC_DIR_V) != 0;
            const int64_t first = lo > E0 ? (lo - E0) >> 2 : 0;                     // entries are runs 1, 2, ...
            const int64_t last = ((hi < E1 ? hi : E1) - 1 - E0) >> 2;
            const Run* r = pool + rs + brun[b];
            for (int64_t i = first + tid; i <= last; i += CC_THREADS) {
                const Run cu = r[i + 1], pv = r[i];
                const uint32_t v = vert ? ((uint32_t)(uint16_t)cu.y0 | (cc_shift_length(cu.x0 - pv.x0, cu.y1 - cu.y0) << 16))
                                        : ((uint32_t)(uint16_t)cu.x0 | (cc_shift_length(cu.y0 - pv.y0, cu.x1 - cu.x0) << 16));
                const int64_t pos = E0 + 4 * i;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (pos + j >= lo && pos + j < hi) wb[pos + j - w] = (uint8_t)(v >> (8 * j));
            }
        }
        __syncthreads();
        // the window as aligned dwords; byte stores in front of the first and behind the last whole dword
        const int l = (int)(lo - w), h = (int)(hi - w);
        uint8_t* dst = out + (w - s0);
        for (int o = tid * 4; o < h; o += CC_THREADS * 4) {
            if (o >= l && o + 4 <= h) {
                *reinterpret_cast<uint32_t*>(dst + o) = win[o >> 2];
            } else {
                for (int j = 0; j < 4; j++)
                    if (o + j >= l && o + j < h) dst[o + j] = wb[o + j];
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- decode
__device__ __forceinline__ uint32_t cc_ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t cc_ld32(const uint8_t* p) { return cc_ld16(p) | (cc_ld16(p + 2) << 16); }

// Nodes [k0, k1); `in` holds the chunk's bytes from offset f0 on.  One workgroup a node.
__global__ void __launch_bounds__(CC_THREADS) cc_decode_kernel(const uint8_t* __restrict__ in, int64_t f0,
                                                                 const int64_t* __restrict__ node_off,
                                                                 const int64_t* __restrict__ node_run_start, int64_t k0,
                                                                 int64_t k1, Run* __restrict__ pool,
                                                                 int32_t* __restrict__ bin_nruns,
                                                                 uint16_t* __restrict__ bin_count,
                                                                 float* __restrict__ bin_dist) {
    __shared__ int s_pay[32];   // start of each bin's run payload behind the node's first byte
    __shared__ int s_dir[32];
    __shared__ int s_n[32];     // runs the bin decodes to
    __shared__ int s_rs[32];    // the node's runs in front of the bin
    __shared__ uint32_t s_cnt[32], s_dist[32];
    const int64_t k = k0 + blockIdx.x;
    if (k >= k1) return;
    const uint8_t* base = in + (node_off[k] - f0);
    const int tid = threadIdx.x;
    if (tid == 0) {   // the hops of scan_pointmap_chunk
        int o = 0, rs = 0;
        for (int b = 0; b < 32; b++) {
            const uint32_t dir = base[o], count = cc_ld16(base + o + 1);
            s_dir[b] = (int)dir;
            s_cnt[b] = count;
            s_dist[b] = cc_ld32(base + o + 3);
            o += 11;
            s_pay[b] = o;
            int n = 0;
            if (count) {
                if (dir & CC_DIR_DIAG) {
                    n = 1;
                    o += 6;
                } else {
                    n = (int)cc_ld16(base + o);
                    o += 8 + (n ? (n - 1) * 4 : 0);
                }
            }
            s_n[b] = n;
            s_rs[b] = rs;
            rs += n;
        }
    }
    __syncthreads();
    if (tid < 32) {
        bin_nruns[k * 32 + tid] = s_n[tid];
        bin_count[k * 32 + tid] = (uint16_t)s_cnt[tid];
        bin_dist[k * 32 + tid] = __uint_as_float(s_dist[tid]);
    }
    const int lane = tid & 63;
    Run* dst = pool + node_run_start[k];
    for (int b = tid >> 6; b < 32; b += CC_THREADS / 64) {   // a wave a bin
        const int n = s_n[b], dir = s_dir[b];
        if (n == 0) continue;
        const uint8_t* p = base + s_pay[b];
        Run* q = dst + s_rs[b];
        if (dir & CC_DIR_DIAG) {
            if (lane == 0) {
                const int16_t sx = (int16_t)cc_ld16(p), sy = (int16_t)cc_ld16(p + 2);
                const int len = (int)cc_ld16(p + 4);
                q[0] = Run{sx, sy, (int16_t)(sx + len), dir == CC_DIR_PD ? (int16_t)(sy + len) : (int16_t)(sy - len)};
            }
            continue;
        }
        const bool vert = (dir & CC_DIR_V) != 0;
        const int16_t px0 = (int16_t)cc_ld16(p + 2), py0 = (int16_t)cc_ld16(p + 4);
        const int len0 = (int)cc_ld16(p + 6);
        int carry = 0;   // the shifts of the runs before this tile
        for (int t0 = 0; t0 < n; t0 += 64) {
            const int i = t0 + lane;
            uint32_t ent = 0;
            if (i >= 1 && i < n) ent = cc_ld32(p + 8 + 4 * (i - 1));
            const int primary = (int16_t)(ent & 0xFFFFu), sl = (int)(ent >> 16);
            int cum = sl & 0xF;
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(cum, d, 64);
                if (lane >= d) cum += t;
            }
            cum += carry;
            carry = __shfl(cum, 63, 64);
            if (i < n) {
                Run r;
                if (i == 0) {
                    r = vert ? Run{px0, py0, px0, (int16_t)(py0 + len0)} : Run{px0, py0, (int16_t)(px0 + len0), py0};
                } else if (vert) {
                    const int16_t x = (int16_t)(px0 + cum), y = (int16_t)primary;
                    r = Run{x, y, x, (int16_t)(y + (sl >> 4))};
                } else {
                    const int16_t x = (int16_t)primary, y = (int16_t)(py0 + cum);
                    r = Run{x, y, (int16_t)(x + (sl >> 4)), y};
                }
                q[i] = r;
            }
        }
    }
}

}  // namespace dmx
