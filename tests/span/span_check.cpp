// Host brute-force check of makeGraph's span arithmetic (depthmapx_amd/csrc/kernels/span.hpp) against the
// sieve's per-cell rules (PointMap::sieve2, salalib/pointdata.cpp:1512-1565): for random gap lists,
// sources, octants and depth windows, every row's visible depths (visited by a gap, inside its centre)
// computed cell by cell equal the per-row intervals; and every row's class boundaries equal the per-cell
// bin decisions.  Built and run by tests/test_span_math.py (g++, -ffp-contract=off).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../depthmapx_amd/csrc/kernels/span.hpp"

using namespace dmx;

// ---- `span_check bins`: the per-cell bin decision (span.hpp cell_bin, the makeGraph chunk loop's) on its own.
static SpanOct make_oct(int q, int cx, int cy, double blx, double bly, double sp) {
    SpanOct o;
    o.q = q; o.cx = cx; o.cy = cy; o.blx = blx; o.bly = bly; o.sp = sp;
    o.c0x = blx + sp * 1.0 * (double)cx;
    o.c0y = bly + sp * 1.0 * (double)cy;
    o.obinp = octant_bins(q);
    return o;
}

// Unit coordinates: cell_bin against the class from exact integer predicates (tan 30 = 1 / sqrt 3: ratio >= tan 30
// <=> 3 ind^2 >= depth^2; tan 15 = 2 - sqrt 3: ratio >= tan 15 <=> (2 depth - ind)^2 <= 3 depth^2), every
// (depth <= 4096, ind <= depth), all 8 octants.
static long long check_exact_classes(long long& checked) {
    long long bad = 0;
    for (int q = 0; q < 8; q++) {
        const SpanOct o = make_oct(q, 4100, 4100, 0.0, 0.0, 1.0);
        for (long long d = 1; d <= 4096; d++)
            for (long long i = 0; i <= d; i++) {
                const int k = (i == 0) ? 0 : (i == d) ? 4 : (3 * i * i >= d * d) ? 3 : ((2 * d - i) * (2 * d - i) <= 3 * d * d) ? 2 : 1;
                if (cell_bin(o, (int)d, (int)i) != obin(o.obinp, k)) {
                    if (bad < 10) fprintf(stderr, "exact class: q %d depth %lld row %lld: cell_bin %d, class %d\n", q, d, i, cell_bin(o, (int)d, (int)i), k);
                    bad++;
                }
                checked++;
            }
    }
    return bad;
}

struct Coords { const char* name; double ox, oy, sp; };
// region bottom-left corners and spacings; the grid's bottom-left cell centre comes from PointMap::setGrid
// (pointdata.cpp:122-171): the first two are the rooms of tests/golden/gen_synthetic.py NOISY_ROOMS
static const Coords kCoords[] = {
    {"os07", 530635.42, 183499.82, 0.7},
    {"neg01", -1000.04, 999.96, 0.1},
    {"os004", 5.3e5, 1.8e5, 0.04},
    {"unit", 0.0, 0.0, 1.0},
    {"os2", 530635.696268, 183499.852969, 2.0},
};
static double grid_origin(double b, double sp) {
    double off = fmod(b, sp);
    if (off < sp / 2.0) off += sp;
    if (off > sp / 2.0) off -= sp;
    return b - off;
}

// Every in-grid cell of a G x G grid around each of a set of sources, in its octant(s): cell_bin against plain
// FP64 whichbin(depixelate(cell) - centre).  Diagonal cells (ind == depth) are counted apart.
static void check_noisy(const Coords& c, int G, long long& cells, long long& bad_off, long long& bad_diag) {
    const double blx = grid_origin(c.ox, c.sp), bly = grid_origin(c.oy, c.sp);
    std::mt19937_64 rng(77);
    std::vector<std::pair<int, int>> src = {{0, 0}, {G - 1, 0}, {0, G - 1}, {G - 1, G - 1}, {G / 2, G / 2}, {1, G - 9}};
    for (int i = 0; i < 6; i++) src.push_back({(int)(rng() % G), (int)(rng() % G)});
    for (auto s : src)
        for (int q = 0; q < 8; q++) {
            const SpanOct o = make_oct(q, s.first, s.second, blx, bly, c.sp);
            for (int d = 1; d < G; d++)
                for (int i = 0; i <= d; i++) {
                    int hx, hy;
                    octant_xy(q, s.first, s.second, d, i, hx, hy);
                    if (hx < 0 || hx >= G || hy < 0 || hy >= G) continue;
                    const double px = blx + c.sp * 1.0 * (double)hx, py = bly + c.sp * 1.0 * (double)hy;
                    const int want = whichbin(px - o.c0x, py - o.c0y), got = cell_bin(o, d, i);
                    cells++;
                    if (got != want) {
                        if (i == d) bad_diag++;
                        else {
                            if (bad_off < 10) fprintf(stderr, "%s: source (%d, %d) q %d depth %d row %d: cell_bin %d, whichbin %d\n", c.name, s.first, s.second, q, d, i, got, want);
                            bad_off++;
                        }
                    }
                }
        }
}

// diag_offbin_depths against a count over every source and diagonal cell of a small grid
static int brute_offbin_depths(int G, double blx, double bly, double sp) {
    std::vector<char> hit(G, 0);
    for (int x = 0; x < G; x++)
        for (int y = 0; y < G; y++)
            for (int q = 0; q < 4; q++) {
                const SpanOct o = make_oct(q, x, y, blx, bly, sp);
                for (int d = 1; d < G; d++) {
                    int hx, hy;
                    octant_xy(q, x, y, d, d, hx, hy);
                    if (hx < 0 || hx >= G || hy < 0 || hy >= G) break;
                    const double px = blx + sp * 1.0 * (double)hx, py = bly + sp * 1.0 * (double)hy;
                    if (whichbin(px - o.c0x, py - o.c0y) != cell_bin(o, d, d)) hit[d] = 1;
                }
            }
    int n = 0;
    for (int d = 1; d < G; d++) n += hit[d];
    return n;
}

static int main_bins() {
    long long checked = 0;
    const long long bad_exact = check_exact_classes(checked);
    printf("exact classes: cells %lld, mismatches %lld\n", checked, bad_exact);
    long long bad_off = 0, bad_diag = 0, bad_pre = 0;
    for (const Coords& c : kCoords) {
        const int G = 1400;
        const double blx = grid_origin(c.ox, c.sp), bly = grid_origin(c.oy, c.sp);
        long long cells = 0, off = 0, diag = 0;
        check_noisy(c, G, cells, off, diag);
        const int pre = diag_offbin_depths(G, G, blx, bly, c.sp);
        const int pre_small = diag_offbin_depths(48, 48, blx, bly, c.sp), brute_small = brute_offbin_depths(48, blx, bly, c.sp);
        printf("%s (bottom-left %.17g %.17g, spacing %g): cells %lld, off-diagonal mismatches %lld, diagonal mismatches %lld; "
               "depths with a diagonal cell off its bin: %d of %d (48^2: %d, counted %d)\n", c.name, blx, bly, c.sp, cells, off,
               diag, pre, G - 1, pre_small, brute_small);
        bad_off += off;
        bad_diag += diag;
        // the precheck covers every source: none found by it means none in the sample, and it equals the count
        bad_pre += (pre == 0 && diag != 0) + (pre_small != brute_small);
    }
    printf("noisy off-diagonal mismatches %lld\nnoisy diagonal mismatches %lld\nprecheck mismatches %lld\n", bad_off, bad_diag, bad_pre);
    return (bad_exact || bad_off || bad_pre) ? 1 : (bad_diag ? 2 : 0);
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "bins") return main_bins();
    const int trials = argc > 1 ? atoi(argv[1]) : 2000;
    std::mt19937_64 rng(argc > 2 ? atoll(argv[2]) : 2026);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    long long rows_checked = 0, cells = 0, bad = 0, class_checked = 0;
    for (int t = 0; t < trials; t++) {
        // a gap list inside [0, 1]: sorted cut points, alternate gap / block, gaps longer than 1e-10
        const int ng = 1 + (int)(rng() % 6);
        std::vector<double> cut;
        for (int i = 0; i < 2 * ng; i++) {
            double v = U(rng);
            if (rng() % 8 == 0) v = (double)(rng() % 5) / 4.0;   // exact quarters (0, 1/4, ..., 1)
            if (rng() % 16 == 0) v = 1.0 / (1 + rng() % 7);       // 1/k
            cut.push_back(v);
        }
        std::sort(cut.begin(), cut.end());
        if (rng() % 3 == 0) cut.front() = 0.0;
        if (rng() % 3 == 0) cut.back() = 1.0;
        std::vector<double> gs, ge;
        for (int i = 0; i < ng; i++)
            if (cut[2 * i + 1] > cut[2 * i] + 1e-10 && (gs.empty() || cut[2 * i] > ge.back())) {
                gs.push_back(cut[2 * i]);
                ge.push_back(cut[2 * i + 1]);
            }
        if (gs.empty()) continue;
        const int n = (int)gs.size();
        const int d0 = 1 + (int)(rng() % 1500), d1 = d0 + (int)(rng() % 300);
        // sieve2 per cell: visits[ind][d] = gap index that adds it (centre) or -1
        const int R = d1 + 2;
        std::vector<std::vector<int>> vis(R, std::vector<int>(d1 - d0 + 1, -1));
        for (int d = d0; d <= d1; d++) {
            int firstind = 0;
            for (int g = 0; g < n; g++)
                for (int ind = gap_lo(gs[g], d); ind <= gap_hi(ge[g], d); ind++) {
                    if (ind < firstind) continue;
                    if (ind > d) break;
                    firstind = ind;
                    const bool centre = (double)ind >= gs[g] * d && (double)ind <= ge[g] * d;
                    if (centre) {
                        if (vis[ind][d - d0] != -1) { bad++; fprintf(stderr, "row %d depth %d added twice\n", ind, d); }
                        vis[ind][d - d0] = g;
                    }
                }
        }
        for (int ind = 0; ind < R; ind++) {
            std::vector<int> got(d1 - d0 + 1, -1);
            int last_r = d0 - 1;
            for (int g = n - 1; g >= 0; g--) {
                int p, r;
                span_row_gap(ind, gs[g], ge[g], g > 0, g > 0 ? ge[g - 1] : 0.0, d0, d1, p, r);
                if (p <= r && p <= last_r) { bad++; fprintf(stderr, "gap intervals out of depth order\n"); }
                for (int d = p; d <= r; d++) got[d - d0] = g;
                if (p <= r) last_r = r;
            }
            for (int d = d0; d <= d1; d++) {
                cells += got[d - d0] >= 0;
                if (got[d - d0] != vis[ind][d - d0]) {
                    if (bad < 20)
                        fprintf(stderr, "trial %d row %d depth %d: span %d, sieve %d (gaps %d, d %d..%d)\n", t, ind, d,
                                got[d - d0], vis[ind][d - d0], n, d0, d1);
                    bad++;
                }
            }
            rows_checked++;
        }
        // class boundaries of random rows against the per-cell bins
        SpanOct o;
        o.q = (int)(rng() % 8);
        o.cx = (int)(rng() % 2000);
        o.cy = (int)(rng() % 2000);
        o.sp = (rng() % 2) ? 1.0 : 0.1 + U(rng);
        o.blx = (rng() % 2) ? 0.0 : -1000.0 * U(rng);
        o.bly = (rng() % 2) ? 0.0 : 1000.0 * U(rng);
        o.c0x = o.blx + o.sp * 1.0 * (double)o.cx;
        o.c0y = o.bly + o.sp * 1.0 * (double)o.cy;
        o.obinp = octant_bins(o.q);
        for (int k = 0; k < 40; k++) {
            const int ind = 1 + (int)(rng() % 1200);
            const int t3 = class_last(o, ind, 3, 0.5773502691896257), t2 = class_last(o, ind, 2, 0.2679491924311227);
            for (int d = ind + 1; d <= 5000; d++) {
                const int c = cell_class(o, d, ind);
                const int want = d <= t3 ? 3 : (d <= t2 ? 2 : 1);
                if (c != want) {
                    if (bad < 20) fprintf(stderr, "class: q %d row %d depth %d: cell %d, span %d (t3 %d t2 %d)\n", o.q, ind, d, c, want, t3, t2);
                    bad++;
                }
                class_checked++;
            }
        }
    }
    printf("rows %lld, visible cells %lld, class cells %lld, mismatches %lld\n", rows_checked, cells, class_checked, bad);
    return bad ? 1 : 0;
}
