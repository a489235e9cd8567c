// isovist_points.hip -- a batch of isovists at caller-given points, full circles or view cones:
// MetaGraph::makeIsovist (salalib/mgraph.cpp:491-521) over Isovist::makeit / setData (salalib/isovist.cpp) per
// point.  The per-point routine is isovist_point of isovist_cell.hpp, the same source the host test runs; this
// file is the work model around it.  It needs no point map and no graph: the tree of the drawing and the points.
//
// Work model: that of isovist_kernel.  One lane per point, one wave per workgroup, persistent workgroups on one
// work counter; a work item is 64 consecutive points of the launch order (the host orders the points so that a
// wave's lanes walk similar paths through the tree, api/isovist_points.hip); progress and cancel ride on the
// counter (ctl_poll).  Gap and block lists per lane in global memory, interleaved per workgroup.  A point that
// needs more than a capacity writes nothing and is flagged (status 2); the host runs the flagged points again with
// larger lists in list mode (P.list: 64 flagged points a work item).  Nothing is truncated.
//
// Polygon vertices go to one pool: a point reserves 2 nb + 2 entries (the bound isovist_point begins its sink
// with) with one atomic add and records where its vertices start and how many it wrote.  The cursor keeps
// counting past the end of a pool that is too small; the host then runs again with a pool of that size.
#include "common.hpp"
#include "isovist_cell.hpp"

namespace dmx {

constexpr int ISOP_THREADS = 64;

struct IsoPointsParams {
    IsoTree tree;
    double tolerance;
    int simple, want_poly;
    const double* pts;              // [n][4] x, y, startangle, endangle, launch order
    int64_t n;
    const int64_t* list;            // list mode: points (launch order) to run, nlist of them; null: all n
    int64_t nlist;
    int gcap, bcap;
    double* gaps;                   // [workgroups][gcap * 2][64]
    int32_t* gap_flags;             // [workgroups][gcap][64]
    double* blocks;                 // [workgroups][bcap * 6][64]
    int32_t* block_order;           // [workgroups][bcap][64]
    float* out;                     // [n][8]
    uint8_t* status;                // [n] 0 untouched, 1 written, 2 a list was too small
    double2* pool;                  // polygon vertices
    unsigned long long pool_cap;
    unsigned long long* pool_cursor;
    long long* poly_start;          // [n] first pool entry of the point
    int32_t* poly_n;                // [n] vertices written
    int* work_counter;
    DmxCtl* ctl;
    unsigned long long* stats;      // [0] most blocks a point held, [1] most gaps
};

struct IsoVertexSink {
    double2* pool;
    unsigned long long cap;
    unsigned long long* cursor;
    long long base;
    int n, upper;
    bool on, ok;
    __device__ void begin(int upper_bound) {
        n = 0;
        ok = false;
        base = 0;
        upper = upper_bound;
        if (!on) return;
        base = (long long)atomicAdd(cursor, (unsigned long long)upper_bound);
        ok = (unsigned long long)base + (unsigned long long)upper_bound <= cap;
    }
    __device__ void push(Vec2 p) {
        if (ok && n < upper) pool[base + n] = make_double2(p.x, p.y);
        n++;
    }
};

__global__ void __launch_bounds__(ISOP_THREADS) isovist_points_kernel(const IsoPointsParams* __restrict__ PP) {
    const IsoPointsParams P = const_params(PP);
    __shared__ int s_item;
    const int lane = threadIdx.x;
    const int64_t total = P.list ? P.nlist : P.n;
    const int nitems = (int)((total + 63) / 64);
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
        int64_t k = (int64_t)item * 64 + lane;
        if (k >= total) continue;
        if (P.list) k = P.list[k];
        const double* p = P.pts + k * 4;
        float row[8];
        IsoVertexSink sink;
        sink.pool = P.pool; sink.cap = P.pool_cap; sink.cursor = P.pool_cursor;
        sink.on = P.want_poly != 0;
        sink.base = 0; sink.n = 0; sink.upper = 0; sink.ok = false;
        const int err = isovist_point(P.tree, S, P.tolerance, Vec2{p[0], p[1]}, p[2], p[3], P.simple != 0, row, sink);
        if (err) {
            P.status[k] = 2;
            continue;
        }
        P.out[k * 8] = row[0];
        if (!P.simple)
            for (int c = 1; c < 8; c++) P.out[k * 8 + c] = row[c];
        if (P.want_poly) {
            P.poly_start[k] = sink.base;
            P.poly_n[k] = sink.n;
        }
        P.status[k] = 1;
        if ((unsigned long long)S.nb > max_blocks) max_blocks = (unsigned long long)S.nb;
        if ((unsigned long long)S.maxg > max_gaps) max_gaps = (unsigned long long)S.maxg;
    }
    if (P.stats) {
        if (max_blocks) atomicMax(&P.stats[0], max_blocks);
        if (max_gaps) atomicMax(&P.stats[1], max_gaps);
    }
}

}  // namespace dmx
