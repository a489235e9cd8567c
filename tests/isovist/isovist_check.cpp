// isovist_check.cpp -- host run of the isovist analysis for tests/test_isovist_host.py: the BSP builder
// (csrc/host/bsptree.cpp) and the per-cell routine the kernel uses (csrc/kernels/isovist_cell.hpp) over a map
// made by the host point map (csrc/host/pointmap.cpp).  Plain g++, -ffp-contract=off; also built with
// -fsanitize=address,undefined.
//
//   isovist_check LINES.bin NLINES blx bly trx try SPACING FILLX FILLY FILLTYPE OUTDIR [GCAP BCAP]
//
// LINES.bin: float64 [NLINES][4].  Dumps into OUTDIR
//   isovist.bin float32 [N][8] (rows of skipped cells: -1), occ_dist.bin float32 [N][32], occ_counts.bin int32
//   [N][32], occ_pixels.bin int32 [total] (by node, bin, push order), tree_seg.bin float64 [T][4],
//   tree_links.bin int32 [T][4] (tag, left, right, parent), and info.txt (nodes, tree nodes, depth, max gaps, max blocks)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../depthmapx_amd/csrc/host/bsptree.hpp"
#include "../../depthmapx_amd/csrc/host/pointmap.hpp"
#include "../../depthmapx_amd/csrc/kernels/isovist_cell.hpp"

using namespace dmx;

template <typename T> static void dump(const std::string& path, const std::vector<T>& v) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); exit(2); }
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
    fclose(f);
}

struct VecSink {
    std::vector<int32_t> bins, pix;
    void begin(int) { bins.clear(); pix.clear(); }
    void push(int bin, int32_t p) { bins.push_back(bin); pix.push_back(p); }
};

int main(int argc, char** argv) {
    if (argc < 12) { fprintf(stderr, "usage: see the source\n"); return 2; }
    const int64_t nlines = atoll(argv[2]);
    std::vector<double> lines((size_t)nlines * 4);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(lines.data(), 8, lines.size(), f) != lines.size()) { fprintf(stderr, "cannot read lines\n"); return 2; }
    fclose(f);
    const Rect region{atof(argv[3]), atof(argv[4]), atof(argv[5]), atof(argv[6])};
    const double spacing = atof(argv[7]);
    const std::string out = argv[11];
    const int gcap = argc > 12 ? atoi(argv[12]) : 256, bcap = argc > 13 ? atoi(argv[13]) : 1024;
    PointMapHost h(region, spacing, lines.data(), nlines);
    if (h.fill(atof(argv[8]), atof(argv[9]), atoi(argv[10])) != 0) { fprintf(stderr, "fill failed\n"); return 1; }
    BspTree bt;
    bsp_build(h.drawing().data(), (int64_t)h.drawing().size() / 4, bt);
    if (bt.nodes() == 0) { fprintf(stderr, "no lines\n"); return 1; }
    const IsoTree T{bt.seg.data(), bt.left.data(), bt.right.data(), bt.parent.data(), (int32_t)bt.nodes()};
    const IsoGrid G{h.bottom_left().x, h.bottom_left().y, h.spacing(), h.cols(), h.rows()};
    const Rect& gr = h.grid_region();
    const double tolerance = (gr.width() > gr.height() ? gr.width() : gr.height()) * 1e-9;
    std::vector<double> gbuf((size_t)gcap * 2), bbuf((size_t)bcap * 6);
    std::vector<int32_t> gflag((size_t)gcap), border((size_t)bcap);
    std::vector<float> iso, od;
    std::vector<int32_t> oc, op;
    int max_blocks = 0, max_gaps = 0;
    int64_t n = 0;
    for (int x = 0; x < h.cols(); x++)
        for (int y = 0; y < h.rows(); y++) {
            const int32_t st = h.state()[h.index(x, y)];
            if (!(st & CELL_FILLED)) continue;
            n++;
            float row[8], dist[32];
            for (float& v : row) v = -1.0f;
            for (float& v : dist) v = 0.0f;
            std::vector<int32_t> pix[32];
            if (!((st & CELL_CONTEXTFILLED) && !(x % 2 == 0 && y % 2 == 0))) {   // vgaisovist.cpp:50-52
                IsoStore S{gbuf.data(), gflag.data(), bbuf.data(), border.data(), 1, gcap, bcap, 0, 0, 0};
                VecSink sink;
                const int err = isovist_cell(T, S, G, tolerance, x, y, false, row, dist, sink);
                if (err) { fprintf(stderr, "capacity error %d at (%d, %d)\n", err, x, y); return 3; }
                if (S.nb > max_blocks) max_blocks = S.nb;
                if (S.maxg > max_gaps) max_gaps = S.maxg;
                for (size_t k = 0; k < sink.bins.size(); k++) pix[sink.bins[k]].push_back(sink.pix[k]);
            }
            iso.insert(iso.end(), row, row + 8);
            od.insert(od.end(), dist, dist + 32);
            for (int b = 0; b < 32; b++) {
                oc.push_back((int32_t)pix[b].size());
                op.insert(op.end(), pix[b].begin(), pix[b].end());
            }
        }
    dump(out + "/isovist.bin", iso);
    dump(out + "/occ_dist.bin", od);
    dump(out + "/occ_counts.bin", oc);
    dump(out + "/occ_pixels.bin", op);
    dump(out + "/tree_seg.bin", bt.seg);
    std::vector<int32_t> links;
    for (int64_t k = 0; k < bt.nodes(); k++) {
        links.push_back(bt.tag[k]); links.push_back(bt.left[k]);
        links.push_back(bt.right[k]); links.push_back(bt.parent[k]);
    }
    dump(out + "/tree_links.bin", links);
    f = fopen((out + "/info.txt").c_str(), "w");
    fprintf(f, "nodes %lld\ntree_nodes %lld\ndepth %d\nmax_blocks %d\nmax_gaps %d\n", (long long)n, (long long)bt.nodes(), bt.depth,
            max_blocks, max_gaps);
    fclose(f);
    return 0;
}
