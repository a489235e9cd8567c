// isovist.hip -- VGA isovist analysis (-vm isovist): VGAIsovist::run (salalib/vgamodules/vgaisovist.cpp:24-90)
// over Isovist::makeit / setData (salalib/isovist.cpp).  The per-cell routine is isovist_cell.hpp, the same
// source the host test runs; this file is the work model around it.
//
// Work model: one lane per cell, one independent job each.  A workgroup is one wave and takes an 8 x 8 tile of
// grid cells (lane = (y & 7) * 8 + (x & 7)), so its lanes walk nearly the same path through the BSP tree and
// meet nearly the same walls.  Persistent workgroups take tiles from one grid counter; progress and cancel
// ride on it (ctl_poll), as in thruvision_kernel.  Lanes whose cell has no node, lies outside the source range
// or is skipped by the reference (context-filled at an odd PixelRef) idle.
//
// Lists: every lane has a gap list (gcap entries) and a block list (bcap entries) in global memory, the lists
// of a workgroup's 64 lanes interleaved (element i of lane l at [i * 64 + l]) so that lanes at the same list
// position touch one 512-byte line.  A cell that needs more than a capacity writes nothing and is flagged
// (status 2); the host runs the flagged cells again with larger lists through the same kernel in list mode
// (P.list: 64 flagged nodes a work item).  Nothing is truncated.
//
// Occlusion pixels go to one pool: a cell reserves as many entries as it holds blocks (an upper bound of its
// occlusion points) with one atomic add and records where its entries start and how many it wrote.  A pool
// that is too small is seen by the host in the cursor, which keeps counting: it runs again with a pool of
// that size.
#include "common.hpp"
#include "isovist_cell.hpp"

namespace dmx {

constexpr int ISO_THREADS = 64;

struct IsovistParams {
    IsoTree tree;
    IsoGrid grid;
    double tolerance;
    int tw, th;                     // tiles across and down
    int simple, want_occ;
    const int32_t* cell_node;       // [cols * rows] node of a cell or -1
    const int32_t* node_cell;       // [N]
    const uint8_t* node_flags;      // [N] bit 0: context-filled
    int64_t src_begin, src_end;
    const int32_t* list;            // list mode: nodes to run, nlist of them; null: tile mode
    int nlist;
    int gcap, bcap;
    double* gaps;                   // [workgroups][gcap * 2][64]
    int32_t* gap_flags;             // [workgroups][gcap][64]
    double* blocks;                 // [workgroups][bcap * 6][64]
    int32_t* block_order;           // [workgroups][bcap][64]
    float* out;                     // [N][8]
    float* occ_dist;                // [N][32]
    uint8_t* status;                // [N] 0 untouched, 1 written, 2 a list was too small
    int2* pool;                     // (bin, PixelRef) entries
    unsigned long long pool_cap;
    unsigned long long* pool_cursor;
    long long* occ_start;           // [N] first pool entry of the node
    int32_t* occ_n;                 // [N] entries written
    int* work_counter;
    DmxCtl* ctl;
    unsigned long long* stats;      // [0] most blocks a cell held, [1] most gaps
};

struct IsoPoolSink {
    int2* pool;
    unsigned long long cap;
    unsigned long long* cursor;
    long long base;
    int n;
    bool on, ok;
    __device__ void begin(int upper) {
        n = 0;
        ok = false;
        base = 0;
        if (!on) return;
        base = (long long)atomicAdd(cursor, (unsigned long long)upper);
        ok = (unsigned long long)base + (unsigned long long)upper <= cap;
    }
    __device__ void push(int bin, int32_t pix) {
        if (ok) pool[base + n] = make_int2(bin, pix);
        n++;
    }
};

__global__ void __launch_bounds__(ISO_THREADS) isovist_kernel(const IsovistParams* __restrict__ PP) {
    const IsovistParams P = const_params(PP);
    __shared__ int s_item;
    const int lane = threadIdx.x;
    const int nitems = P.list ? (P.nlist + 63) / 64 : P.tw * P.th;
    const int64_t wg = blockIdx.x;
    IsoStore S;
    S.g = P.gaps + wg * P.gcap * 2 * 64 + lane;
    S.gf = P.gap_flags + wg * P.gcap * 64 + lane;
    S.b = P.blocks + wg * P.bcap * 6 * 64 + lane;
    S.bo = P.block_order + wg * P.bcap * 64 + lane;
    S.stride = 64;
    S.gcap = P.gcap;
    S.bcap = P.bcap;
    unsigned long long max_blocks = 0, max_gaps = 0;
    for (;;) {
        __syncthreads();
        if (lane == 0) s_item = ctl_poll(P.ctl, atomicAdd(P.work_counter, 1));
        __syncthreads();
        const int item = s_item;
        if (item >= nitems) break;
        int64_t node = -1;
        int px = 0, py = 0;
        if (P.list) {
            const int k = item * 64 + lane;
            if (k < P.nlist) {
                node = P.list[k];
                const int c = P.node_cell[node];
                px = c / P.grid.rows;
                py = c % P.grid.rows;
            }
        } else {
            px = (item % P.tw) * 8 + (lane & 7);
            py = (item / P.tw) * 8 + (lane >> 3);
            if (px < P.grid.cols && py < P.grid.rows) {
                node = P.cell_node[(int64_t)px * P.grid.rows + py];
                if (node < P.src_begin || node >= P.src_end) node = -1;
            }
        }
        if (node < 0) continue;
        // context-filled cells at odd PixelRefs are skipped (vgaisovist.cpp:50-52)
        if ((P.node_flags[node] & 1) && !((px % 2) == 0 && (py % 2) == 0)) continue;
        float row[8];
        IsoPoolSink sink;
        sink.pool = P.pool; sink.cap = P.pool_cap; sink.cursor = P.pool_cursor;
        sink.on = P.want_occ != 0;
        sink.base = 0; sink.n = 0; sink.ok = false;
        float* od = P.want_occ ? P.occ_dist + node * 32 : nullptr;
        const int err = isovist_cell(P.tree, S, P.grid, P.tolerance, px, py, P.simple != 0, row, od, sink);
        if (err) {
            P.status[node] = 2;
            continue;
        }
        P.out[node * 8] = row[0];
        if (!P.simple)
            for (int k = 1; k < 8; k++) P.out[node * 8 + k] = row[k];
        if (P.want_occ) {
            P.occ_start[node] = sink.base;
            P.occ_n[node] = sink.n;
        }
        P.status[node] = 1;
        if ((unsigned long long)S.nb > max_blocks) max_blocks = (unsigned long long)S.nb;
        if ((unsigned long long)S.maxg > max_gaps) max_gaps = (unsigned long long)S.maxg;
    }
    if (P.stats) {
        if (max_blocks) atomicMax(&P.stats[0], max_blocks);
        if (max_gaps) atomicMax(&P.stats[1], max_gaps);
    }
}

}  // namespace dmx
