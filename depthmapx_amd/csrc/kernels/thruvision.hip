// thruvision.hip -- VGA through vision (-vm thruvision): VGAThroughVision::run
// (salalib/vgamodules/vgathroughvision.cpp:27-104) over PixelBase::quickPixelateLine (salalib/spacepix.cpp:218-270).
//
// For every source s and every cell x that Node::first()..next() yields for s's node (the cells of its runs, a
// cell once per run that holds it), the reference walks the line p = x -> q = s and adds 1 to every pixel the
// walk emits strictly between its first and last list entries.  The result per cell is an integer count.
//
// The walk is simulated, not solved: at a true half-way point the reference's accumulated FP64 coordinate lands
// on the integer, a hair above it or a hair below it, and only the first two emit two pixels (the smallest case
// is (0,0) -> (6,1): 0.9999999999999999 at i = 3).  So each lane does the same IEEE division dx / t, dy / t and
// the same sequence of FP64 adds from x towards s (the build keeps -ffp-contract=off -fno-fast-math).
//
// Work model: persistent workgroups take sources from one grid counter (progress and cancel ride on it,
// ctl_poll).  A source's runs are read 256 at a time, their lengths prefix-summed in LDS, and the cells of the
// chunk dealt to lanes one line each, so short runs do not idle a wave.
//
// Accumulation, two variants of one kernel (WIN):
//   (A) WIN = false: every increment is a 64-bit atomic add into the global per-cell array;
//   (B) WIN = true: all lines of a source end at the source, so the cells around it take most increments.  A
//       window of win x win 32-bit counters around the source (clamped to the grid) lives in LDS; increments
//       inside it are LDS atomics, those outside go to the global array; the window is added to the global array
//       once per source.
// Counts are kept for every grid cell; the gather kernel keeps the filled ones (those with a node).
#include "common.hpp"

namespace dmx {

constexpr int TV_THREADS = 256;

struct ThruVisionParams {
    int cols, rows;
    const int32_t* node_cell;
    const int64_t* node_run_start;
    const int32_t* node_nruns;
    const Run* pool;
    int64_t src_begin, src_end;
    unsigned long long* counts;   // [cols * rows], x-major, zeroed by the host
    int* work_counter;
    DmxCtl* ctl;
    unsigned long long* stats;    // [0] lines walked, [1] pixel steps
    int win;                      // variant (B): window side in cells (LDS holds win * win counters)
};

// cells Node::first()..next() yields for one run (Bin::next, ngraph.cpp:399-406: the start cell, then steps
// until the moved cursor passes the end, so a run never yields fewer than one cell)
__device__ __forceinline__ int tv_run_cells(Run ru) {
    const int n = (ru.x0 == ru.x1 && ru.y0 != ru.y1) ? (ru.y1 - ru.y0 + 1) : (ru.x1 - ru.x0 + 1);
    return max(n, 1);
}

template <bool WIN>
__device__ __forceinline__ void tv_add(const ThruVisionParams& P, unsigned int* win, int wx0, int wy0, int cx, int cy) {
    if ((unsigned)cx >= (unsigned)P.cols || (unsigned)cy >= (unsigned)P.rows) return;   // (a run outside the grid)
    if (WIN) {
        const unsigned ux = (unsigned)(cx - wx0), uy = (unsigned)(cy - wy0);
        if (ux < (unsigned)P.win && uy < (unsigned)P.win) {
            atomicAdd(&win[ux * P.win + uy], 1u);
            return;
        }
    }
    atomicAdd(&P.counts[(int64_t)cx * P.rows + cy], 1ull);
}

template <bool WIN>
__global__ void __launch_bounds__(TV_THREADS) thruvision_kernel(const ThruVisionParams* __restrict__ PP) {
    const ThruVisionParams P = const_params(PP);
    extern __shared__ __attribute__((aligned(16))) unsigned int tv_win[];   // (B) the window
    __shared__ int s_pref[TV_THREADS + 1];   // exclusive prefix of the chunk's run lengths
    __shared__ Run s_run[TV_THREADS];
    __shared__ int s_wsum[TV_THREADS / 64];
    __shared__ int s_src;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nsrc = (int)(P.src_end - P.src_begin);
    const int nwin = WIN ? P.win * P.win : 0;
    unsigned long long n_lines = 0, n_steps = 0;
    for (;;) {
        if (tid == 0) s_src = ctl_poll(P.ctl, atomicAdd(P.work_counter, 1));
        __syncthreads();
        const int si = s_src;
        if (si >= nsrc) break;
        const int64_t src = P.src_begin + si;
        const int sc = P.node_cell[src];
        const int sx = sc / P.rows, sy = sc % P.rows;
        int wx0 = 0, wy0 = 0;
        if (WIN) {
            // the window around the source, moved inside the grid where it fits
            wx0 = max(0, min(sx - P.win / 2, P.cols - P.win));
            wy0 = max(0, min(sy - P.win / 2, P.rows - P.win));
            for (int i = tid; i < nwin; i += TV_THREADS) tv_win[i] = 0u;
        }
        const int64_t rs = P.node_run_start[src];
        const int nr = P.node_nruns[src];
        for (int r0 = 0; r0 < nr; r0 += TV_THREADS) {
            __syncthreads();   // the previous chunk's readers are done (and the window is zeroed)
            const int r = r0 + tid;
            int len = 0;
            if (r < nr) {
                const Run ru = P.pool[rs + r];
                s_run[tid] = ru;
                len = tv_run_cells(ru);
            }
            int inc = len;   // inclusive scan inside the wave, then over the waves
            for (int off = 1; off < 64; off <<= 1) {
                const int v = __shfl_up(inc, off);
                if (lane >= off) inc += v;
            }
            if (lane == 63) s_wsum[wave] = inc;
            __syncthreads();
            int base = 0;
            for (int w = 0; w < wave; w++) base += s_wsum[w];
            s_pref[tid + 1] = base + inc;
            if (tid == 0) s_pref[0] = 0;
            __syncthreads();
            const int total = s_pref[TV_THREADS];
            const int nrun = min(TV_THREADS, nr - r0);
            for (int j = tid; j < total; j += TV_THREADS) {
                // the run that holds cell j of the chunk: last k with s_pref[k] <= j
                int lo = 0, hi = nrun - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (s_pref[mid] <= j) lo = mid;
                    else hi = mid - 1;
                }
                const Run ru = s_run[lo];
                const int k = j - s_pref[lo];
                const int dir = run_dir(ru);
                int ddx, ddy;
                dir_step(dir, ddx, ddy);
                const int px = ru.x0 + k * ddx, py = ru.y0 + k * ddy;
                if ((unsigned)px >= (unsigned)P.cols || (unsigned)py >= (unsigned)P.rows) continue;
                // quickPixelateLine(p = x, q = s)
                double dx = (double)(sx - px), dy = (double)(sy - py);
                const double adx = fabs(dx), ady = fabs(dy);
                if (adx == ady) continue;   // polarity 0: one list entry, nothing counted
                const bool major_x = adx > ady;
                const double t = major_x ? adx : ady;
                dx /= t;
                dy /= t;
                double ppx = (double)px + 0.5, ppy = (double)py + 0.5;
                const int it = (int)t;
                n_lines++;
                n_steps += (unsigned long long)(it - 1);
                for (int i = 1; i < it; i++) {   // entries of iterations 1 .. t - 1 (0 and t are p and q)
                    ppx += dx;
                    ppy += dy;
                    const double fx = floor(ppx), fy = floor(ppy);
                    if (major_x && fabs(fy - ppy) < 1e-9) {
                        tv_add<WIN>(P, tv_win, wx0, wy0, (int)fx, (int)floor(ppy + 0.5));
                        tv_add<WIN>(P, tv_win, wx0, wy0, (int)fx, (int)floor(ppy - 0.5));
                    } else if (!major_x && fabs(fx - ppx) < 1e-9) {
                        tv_add<WIN>(P, tv_win, wx0, wy0, (int)floor(ppx + 0.5), (int)fy);
                        tv_add<WIN>(P, tv_win, wx0, wy0, (int)floor(ppx - 0.5), (int)fy);
                    } else {
                        tv_add<WIN>(P, tv_win, wx0, wy0, (int)fx, (int)fy);
                    }
                }
            }
        }
        __syncthreads();
        if (WIN) {
            // A window counter cannot wrap before this flush: a line adds to a cell at most once (its major
            // coordinate moves by 1 a step), and one source walks one line per cell of its runs -- fewer than
            // 2^30 for a graph made here (disjoint runs on a grid of int16 coordinates) and at most 32 x 65535
            // for one read from a file (Bin::m_node_count is 16 bits).
            for (int i = tid; i < nwin; i += TV_THREADS) {
                const unsigned int v = tv_win[i];
                const int cx = wx0 + i / P.win, cy = wy0 + i % P.win;
                if (v && cx < P.cols && cy < P.rows) atomicAdd(&P.counts[(int64_t)cx * P.rows + cy], (unsigned long long)v);
            }
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        n_lines += __shfl_xor(n_lines, off);
        n_steps += __shfl_xor(n_steps, off);
    }
    if (lane == 0 && P.stats) {
        atomicAdd(&P.stats[0], n_lines);
        atomicAdd(&P.stats[1], n_steps);
    }
}

// the counts of the filled cells, in node order
__global__ void thruvision_gather_kernel(int64_t n, const int32_t* node_cell, const unsigned long long* counts,
                                         long long* out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = (long long)counts[node_cell[k]];
}

}  // namespace dmx
