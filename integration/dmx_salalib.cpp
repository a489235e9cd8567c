// dmx_salalib.cpp -- salalib-side binding of libdmx.so (see dmx_salalib.h).
//
// Compiled against the reference headers (integration/Makefile: -I/root/reference), it uses only the
// reference's public interface plus one pointer-to-member read of PointMap::m_parentRegion (protected,
// reached through a derived accessor, legal C++).  The engine and the reference exchange a map as the
// PointMap::write image (pointdata.cpp:1158-1188): the engine's writer is byte-identical to the
// reference's (tests/test_graphfile.py), and the reference's own PointMap::read (:1073-1156) turns it
// back into Points, Nodes, the attribute table and its statistics.
#include "dmx_salalib.h"

#include <cstdint>
#include <cstring>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "dmx.h"
#include "genlib/comm.h"
#include "genlib/exceptions.h"
#include "salalib/mgraph.h"
#include "salalib/pointdata.h"

namespace dmxsala {
namespace {

// PointMap keeps the MetaGraph region it was made for by pointer (protected); a derived class may
// name the member, and the pointer-to-member then reads it from any PointMap.
struct RegionAccess : PointMap {
    static const QtRegion* parent(const PointMap& m) { return m.*(&RegionAccess::m_parentRegion); }
};
// the same for MetaGraph::m_view_class, which makeIsovist clears VIEWDATA in
struct ViewAccess : MetaGraph {
    static int& view_class(MetaGraph& m) { return m.*(&ViewAccess::m_view_class); }
};

void check(int status) {
    if (status == DMX_ERR_CANCELLED) throw Communicator::CancelledException();
    if (status != DMX_OK) throw depthmapX::RuntimeException(std::string("libdmx: ") + dmx_last_error());
}

// One engine context per process (one process per GPU).  nullptr when no device is usable: the
// caller falls back to the reference's CPU code.
dmx_ctx* context() {
    static dmx_ctx* ctx = nullptr;
    static bool tried = false;
    if (!tried) {
        tried = true;
        if (dmx_ctx_create(0, &ctx) != DMX_OK) ctx = nullptr;
    }
    return ctx;
}

// Communicator bridge: NUM_RECORDS / CURRENT_RECORD posts and IsCancelled polls, every 0.5 s as the
// reference's qtimer(atime, 500) loops do (pointdata.cpp:1301-1316, vgavisualglobal.cpp:195-202).
struct Progress {
    Communicator* comm;
    bool posted_total = false;
    static int32_t fn(void* user, int32_t, int64_t done, int64_t total) {
        Progress* p = static_cast<Progress*>(user);
        if (!p->posted_total) {
            p->comm->CommPostMessage(Communicator::NUM_RECORDS, (int)total);
            p->posted_total = true;
        }
        p->comm->CommPostMessage(Communicator::CURRENT_RECORD, (int)done);
        return p->comm->IsCancelled() ? 1 : 0;
    }
};

struct ScopedProgress {
    dmx_ctx* ctx;
    Progress p;
    ScopedProgress(dmx_ctx* c, Communicator* comm) : ctx(c), p{comm} {
        if (comm) check(dmx_ctx_set_progress(ctx, &Progress::fn, &p, 0.5));
    }
    ~ScopedProgress() { dmx_ctx_set_progress(ctx, nullptr, nullptr, 0.0); }
};

template <class T, int (*F)(T*)>
struct Owned {
    T* p = nullptr;
    ~Owned() {
        if (p) F(p);
    }
};

std::string serialize(const dmx_chunk* c) {
    int64_t size = 0;
    check(dmx_chunk_serialize(c, nullptr, 0, &size));
    std::string out((size_t)size, '\0');
    check(dmx_chunk_serialize(c, reinterpret_cast<uint8_t*>(&out[0]), size, &size));
    return out;
}

std::string save(PointMap& map) {
    std::ostringstream os(std::ios::out | std::ios::binary);
    map.write(os);
    return os.str();
}

// PointMap::read fills a map object from scratch (MetaGraph::readPointMaps reads into a new map):
// read into a fresh map on the same region and drawing, then move it over `map`.
bool load(PointMap& map, const std::string& bytes) {
    const QtRegion* region = RegionAccess::parent(map);
    PointMap fresh(*region, map.getDrawingFiles(), map.getName());
    std::istringstream is(bytes, std::ios::in | std::ios::binary);
    if (!fresh.read(is)) return false;
    map = std::move(fresh);
    return true;
}

// The drawing lines PointMap::blockLines rasterises (pointdata.cpp:311-321): every shown layer.
std::vector<double> drawing_lines(PointMap& map) {
    std::vector<double> lines;
    for (const auto& file : map.getDrawingFiles())
        for (const auto& layer : file.m_spacePixels)
            if (layer.isShown())
                for (const auto& l : layer.getAllShapesAsLines()) {
                    lines.push_back(l.start().x);
                    lines.push_back(l.start().y);
                    lines.push_back(l.end().x);
                    lines.push_back(l.end().y);
                }
    return lines;
}

}  // namespace

bool saveMap(PointMap& map, void* bytes_out) {
    *static_cast<std::string*>(bytes_out) = save(map);
    return true;
}

bool loadMap(PointMap& map, const void* bytes) { return load(map, *static_cast<const std::string*>(bytes)); }

bool sparkGraph2(PointMap& map, Communicator* comm, bool boundarygraph, double maxdist) {
    dmx_ctx* ctx = context();
    // a processed map keeps the reference path (its sparkGraph2 re-adds attribute rows that exist and
    // throws, attributetable.cpp:278)
    if (!ctx || map.isProcessed()) return false;
    const QtRegion* parent = RegionAccess::parent(map);
    const double region[4] = {parent->bottom_left.x, parent->bottom_left.y, parent->top_right.x, parent->top_right.y};
    const std::vector<double> lines = drawing_lines(map);
    Owned<dmx_pointmap, dmx_pointmap_free> pm;
    check(dmx_pointmap_create(region, map.getSpacing(), lines.data(), (int64_t)lines.size() / 4, &pm.p));
    // the engine's grid is PointMap::setGrid(spacing, (0,0)) on the MetaGraph region (the CLI's grid);
    // a map gridded with another offset stays on the reference path
    int32_t cols = 0, rows = 0;
    double blx = 0, bly = 0;
    check(dmx_pointmap_info(pm.p, &cols, &rows, &blx, &bly, nullptr));
    const Point2f bl = map.depixelate(PixelRef(0, 0));
    if ((size_t)cols != map.getCols() || (size_t)rows != map.getRows() || blx != bl.x || bly != bl.y) return false;
    std::vector<int32_t> state((size_t)cols * rows);
    for (int32_t x = 0; x < cols; x++)
        for (int32_t y = 0; y < rows; y++)
            state[(size_t)x * rows + y] = map.getPoint(PixelRef((short)x, (short)y)).getState();
    check(dmx_pointmap_set_state(pm.p, state.data()));
    // merge links stay on the points and are written back with them (Point::write, point.cpp:51-73)
    std::vector<int32_t> links;
    for (const auto& pr : map.getMergedPixelPairs()) {
        links.push_back((int32_t)pr.first.x * rows + pr.first.y);
        links.push_back((int32_t)pr.second.x * rows + pr.second.y);
    }
    if (!links.empty()) check(dmx_pointmap_set_merges(pm.p, links.data(), (int64_t)links.size() / 2));
    // makeGraph on the GPU
    Owned<dmx_graph, dmx_graph_free> g;
    {
        ScopedProgress sp(ctx, comm);
        check(dmx_makegraph(ctx, pm.p, maxdist, boundarygraph ? 1 : 0, 0, -1, &g.p));
    }
    int64_t n = 0, nb = 0, ne = 0, nruns = 0;
    check(dmx_graph_info(g.p, &n, &nb, &ne, &nruns));
    std::vector<float> attrs((size_t)n * 3);
    std::vector<int32_t> bins((size_t)n * 32 * 4);
    std::vector<int16_t> runs((size_t)std::max<int64_t>(nruns, 1) * 4);
    std::vector<uint8_t> gridconn((size_t)n);
    check(dmx_graph_copy(g.p, attrs.data(), bins.data(), runs.data(), gridconn.data()));
    // the columns sparkGraph2 creates (pointdata.cpp:1266-1270: Connectivity locked), displayed =
    // Connectivity, then the image the reference would write for the made map
    const char* names[3] = {"Connectivity", "Point First Moment", "Point Second Moment"};
    std::vector<float> values((size_t)n * 3);
    for (int j = 0; j < 3; j++)
        for (int64_t k = 0; k < n; k++) values[(size_t)j * n + k] = attrs[(size_t)k * 3 + j];
    const uint8_t locked[3] = {1, 0, 0};
    int64_t size = 0;
    check(dmx_chunk_write(pm.p, n, bins.data(), runs.data(), nruns, gridconn.data(), 3, names, values.data(), locked,
                          nullptr, 0, boundarygraph ? 1 : 0, nullptr, 0, &size));
    std::string img((size_t)size, '\0');
    check(dmx_chunk_write(pm.p, n, bins.data(), runs.data(), nruns, gridconn.data(), 3, names, values.data(), locked,
                          nullptr, 0, boundarygraph ? 1 : 0, reinterpret_cast<uint8_t*>(&img[0]), size, &size));
    Owned<dmx_chunk, dmx_chunk_free> c;
    check(dmx_chunk_parse(reinterpret_cast<const uint8_t*>(img.data()), (int64_t)img.size(), &c.p));
    check(dmx_chunk_set_name(c.p, map.getName().c_str()));
    return load(map, serialize(c.p));
}

bool vgaVisualGlobal(PointMap& map, Communicator* comm, double radius, bool gates_only, bool simple_version) {
    dmx_ctx* ctx = context();
    if (!ctx || !map.isProcessed()) return false;
    const std::string img = save(map);
    Owned<dmx_chunk, dmx_chunk_free> c;
    check(dmx_chunk_parse(reinterpret_cast<const uint8_t*>(img.data()), (int64_t)img.size(), &c.p));
    const QtRegion* parent = RegionAccess::parent(map);
    const double region[4] = {parent->bottom_left.x, parent->bottom_left.y, parent->top_right.x, parent->top_right.y};
    Owned<dmx_pointmap, dmx_pointmap_free> pm;
    Owned<dmx_graph, dmx_graph_free> g;
    check(dmx_chunk_load(ctx, c.p, region, &pm.p, &g.p));
    int64_t n = 0, nb = 0, ne = 0, nruns = 0;
    check(dmx_graph_info(g.p, &n, &nb, &ne, &nruns));
    std::vector<float> out((size_t)n * 7);
    {
        ScopedProgress sp(ctx, comm);
        const int rc = dmx_vga_global(ctx, g.p, radius, gates_only ? 1 : 0, 0, -1, out.data(), nullptr);
        // a configuration the engine does not take (none on this path since round 5: the searches whose result
        // depends on the reference's pop order are re-run in that order, vga_ordered.hip): the reference path
        if (rc == DMX_ERR_UNSUPPORTED) return false;
        check(rc);
    }
    // VGAVisualGlobal::run's columns (vgavisualglobal.cpp:31-63), alphabetical, " R<r>" suffix for a
    // finite radius; a source the reference skips sets nothing, and the HH / P-value / Tekl values need
    // more than one node; displayed = Visual Integration [HH] (:212)
    const std::string suffix = radius != -1 ? " R" + std::to_string((int)radius) : std::string();
    struct Col {
        const char* name;
        int k;
        bool in_simple;
    };
    const Col cols[7] = {{"Visual Entropy", 0, false},         {"Visual Integration [HH]", 1, true},
                         {"Visual Integration [P-value]", 2, false}, {"Visual Integration [Tekl]", 3, false},
                         {"Visual Mean Depth", 4, false},      {"Visual Node Count", 5, false},
                         {"Visual Relativised Entropy", 6, false}};
    std::vector<float> v((size_t)n);
    std::vector<uint8_t> set((size_t)n);
    for (const Col& col : cols) {
        if (simple_version && !col.in_simple) continue;
        for (int64_t i = 0; i < n; i++) {
            const float nodes = out[(size_t)i * 7 + 5];
            const bool ran = nodes >= 1.0f;
            set[i] = (ran && (col.k < 1 || col.k > 3 || nodes > 1.0f)) ? 1 : 0;
            v[i] = out[(size_t)i * 7 + col.k];
        }
        check(dmx_chunk_set_column(c.p, (std::string(col.name) + suffix).c_str(), v.data(), set.data(), 0, col.k == 1));
    }
    return load(map, serialize(c.p));
}

// VGAThroughVision::run (vgathroughvision.cpp:27-104).  The reference path keeps: the gate-counting side branch
// (a column __Internal_Gate, :61-74) and a map that already has the column (getOrInsertColumn keeps its
// statistics, which setValue then adds to, :92).
bool vgaThroughVision(PointMap& map, Communicator* comm) {
    dmx_ctx* ctx = context();
    if (!ctx || !map.isProcessed()) return false;
    if (map.getAttributeTable().hasColumn("__Internal_Gate") || map.getAttributeTable().hasColumn("Through vision"))
        return false;
    const std::string img = save(map);
    Owned<dmx_chunk, dmx_chunk_free> c;
    check(dmx_chunk_parse(reinterpret_cast<const uint8_t*>(img.data()), (int64_t)img.size(), &c.p));
    const QtRegion* parent = RegionAccess::parent(map);
    const double region[4] = {parent->bottom_left.x, parent->bottom_left.y, parent->top_right.x, parent->top_right.y};
    Owned<dmx_pointmap, dmx_pointmap_free> pm;
    Owned<dmx_graph, dmx_graph_free> g;
    check(dmx_chunk_load(ctx, c.p, region, &pm.p, &g.p));
    int64_t n = 0, nb = 0, ne = 0, nruns = 0;
    check(dmx_graph_info(g.p, &n, &nb, &ne, &nruns));
    std::vector<float> out((size_t)n);
    {
        ScopedProgress sp(ctx, comm);
        const int rc = dmx_vga_thruvision(ctx, g.p, 0, -1, out.data(), nullptr);
        if (rc == DMX_ERR_UNSUPPORTED) return false;   // a count above the reference's int: its own (wrapping) code
        check(rc);
    }
    // one column, set for every row, not locked, displayed (:92-101)
    check(dmx_chunk_set_column(c.p, "Through vision", out.data(), nullptr, 0, 1));
    return load(map, serialize(c.p));
}

// VGAIsovist::run (vgaisovist.cpp:24-90): the eight columns, and per node the occlusion bins and occ distances
// (Node::m_occlusion_bins, Bin::m_occ_distance), which travel in the node records of the image.  A map that
// already has "Isovist Area" keeps the reference path (getOrInsertColumn keeps the column's statistics, which
// setValue then adds to).
bool vgaIsovist(PointMap& map, Communicator* comm, bool simple_version) {
    dmx_ctx* ctx = context();
    if (!ctx || !map.isProcessed()) return false;
    if (map.getAttributeTable().hasColumn("Isovist Area")) return false;
    const std::vector<double> lines = drawing_lines(map);
    if (lines.empty()) return false;
    const std::string img = save(map);
    Owned<dmx_chunk, dmx_chunk_free> c;
    check(dmx_chunk_parse(reinterpret_cast<const uint8_t*>(img.data()), (int64_t)img.size(), &c.p));
    const QtRegion* parent = RegionAccess::parent(map);
    const double region[4] = {parent->bottom_left.x, parent->bottom_left.y, parent->top_right.x, parent->top_right.y};
    Owned<dmx_pointmap, dmx_pointmap_free> pm;
    Owned<dmx_graph, dmx_graph_free> g;
    check(dmx_chunk_load(ctx, c.p, region, &pm.p, &g.p));
    check(dmx_graph_set_drawing(g.p, lines.data(), (int64_t)lines.size() / 4));
    int64_t n = 0, nb = 0, ne = 0, nruns = 0;
    check(dmx_graph_info(g.p, &n, &nb, &ne, &nruns));
    // what the skipped cells keep: the occ data the map holds now
    std::vector<float> out((size_t)n * 8, -1.0f), occ_dist((size_t)n * 32);
    std::vector<int32_t> occ_counts((size_t)n * 32), old_pix, new_pix;
    int64_t old_total = 0, total = 0;
    check(dmx_chunk_occlusion(c.p, occ_dist.data(), occ_counts.data(), nullptr, 0, &old_total));
    old_pix.resize((size_t)std::max<int64_t>(old_total, 1));
    check(dmx_chunk_occlusion(c.p, nullptr, nullptr, old_pix.data(), old_total, &old_total));
    const std::vector<int32_t> old_counts = occ_counts;
    // the rows the reference writes: every filled point but the context-filled ones at odd PixelRefs (:48-52)
    std::vector<uint8_t> set;
    for (size_t x = 0; x < map.getCols(); x++)
        for (size_t y = 0; y < map.getRows(); y++) {
            const PixelRef curs((short)x, (short)y);
            if (map.getPoint(curs).filled()) set.push_back(map.getPoint(curs).contextfilled() && !curs.iseven() ? 0 : 1);
        }
    if ((int64_t)set.size() != n) return false;
    {
        ScopedProgress sp(ctx, comm);
        check(dmx_vga_isovist(ctx, g.p, simple_version ? 1 : 0, 0, -1, out.data(), occ_dist.data(), occ_counts.data(),
                              nullptr, 0, &total));
        new_pix.resize((size_t)std::max<int64_t>(total, 1));
        check(dmx_vga_isovist(ctx, g.p, simple_version ? 1 : 0, 0, -1, out.data(), occ_dist.data(), occ_counts.data(),
                              new_pix.data(), total, &total));
    }
    // pixels by node: the new lists of the rows written, the old ones of the skipped rows
    std::vector<int32_t> pix;
    size_t oo = 0, no = 0;
    for (int64_t k = 0; k < n; k++) {
        size_t oc = 0, nc = 0;
        for (int b = 0; b < 32; b++) {
            oc += (size_t)old_counts[(size_t)k * 32 + b];
            if (set[k]) nc += (size_t)occ_counts[(size_t)k * 32 + b];
        }
        if (set[k]) pix.insert(pix.end(), new_pix.begin() + no, new_pix.begin() + no + nc);
        else pix.insert(pix.end(), old_pix.begin() + oo, old_pix.begin() + oo + oc);
        oo += oc;
        no += nc;
    }
    // the columns in the order setData inserts them (isovist.cpp:308-332); none locked, the displayed attribute stays
    static const struct { const char* name; int k; } cols[8] = {
        {"Isovist Area", 0}, {"Isovist Compactness", 1}, {"Isovist Drift Angle", 2}, {"Isovist Drift Magnitude", 3},
        {"Isovist Min Radial", 5}, {"Isovist Max Radial", 4}, {"Isovist Occlusivity", 6}, {"Isovist Perimeter", 7}};
    std::vector<float> v((size_t)n);
    for (const auto& col : cols) {
        if (simple_version && col.k != 0) continue;
        for (int64_t i = 0; i < n; i++) v[i] = out[(size_t)i * 8 + col.k];
        check(dmx_chunk_set_column(c.p, col.name, v.data(), set.data(), 0, 0));
    }
    check(dmx_chunk_set_occlusion(c.p, occ_dist.data(), occ_counts.data(), pix.empty() ? nullptr : pix.data()));
    if (!load(map, serialize(c.p))) return false;
    map.m_hasIsovistAnalysis = true;
    return true;
}

// MetaGraph::makeIsovist (mgraph.cpp:491-521) for a batch of points: one dmx_isovists call makes the polygons and
// the attribute values; each polygon then enters the "Isovists" data map through the reference's own
// makePolyShape / setCentroid, and its row gets the columns in the order Isovist::setData inserts them
// (isovist.cpp:308-332).  The drawing lines are those makeBSPtree partitions (mgraph.cpp:643-664).
int makeIsovists(MetaGraph& mg, const std::vector<Point2f>& points, const std::vector<std::pair<double, double>>& angles,
                 bool simple_version) {
    dmx_ctx* ctx = context();
    if (!ctx || (!angles.empty() && angles.size() != points.size())) return 0;
    std::vector<double> lines;
    for (const auto& file : mg.m_drawingFiles)
        for (const auto& layer : file.m_spacePixels)
            if (layer.isShown())
                for (const auto& shape : layer.getAllShapes())
                    for (const Line& l : shape.second.getAsLines())
                        if (l.length() > 0.0) {
                            lines.push_back(l.start().x);
                            lines.push_back(l.start().y);
                            lines.push_back(l.end().x);
                            lines.push_back(l.end().y);
                        }
    if (lines.empty()) return 0;   // makeBSPtree fails: no isovist is made
    const int64_t n = (int64_t)points.size();
    const QtRegion& r = mg.getRegion();
    const double region[4] = {r.bottom_left.x, r.bottom_left.y, r.top_right.x, r.top_right.y};
    std::vector<double> pts((size_t)n * 2), ang((size_t)n * 2, 0.0);
    for (int64_t k = 0; k < n; k++) {
        pts[2 * k] = points[k].x;
        pts[2 * k + 1] = points[k].y;
        if (!angles.empty()) {
            ang[2 * k] = angles[k].first;
            ang[2 * k + 1] = angles[k].second;
        }
    }
    std::vector<float> out((size_t)n * 8, -1.0f);
    std::vector<int64_t> off((size_t)n + 1, 0);
    std::vector<double> xy;
    int64_t total = 0;
    check(dmx_isovists(ctx, lines.data(), (int64_t)lines.size() / 4, region, pts.data(), ang.data(), n, simple_version ? 1 : 0,
                       out.data(), off.data(), nullptr, 0, &total));
    xy.resize((size_t)std::max<int64_t>(total, 1) * 2);
    check(dmx_isovists(ctx, lines.data(), (int64_t)lines.size() / 4, region, pts.data(), ang.data(), n, simple_version ? 1 : 0,
                       out.data(), off.data(), xy.data(), total, &total));
    if (n == 0) return 1;
    int made = 1;
    ViewAccess::view_class(mg) &= ~MetaGraph::VIEWDATA;
    std::vector<ShapeMap>& maps = mg.getDataMaps();
    int shapelayer = -1;
    for (size_t i = 0; i < maps.size(); i++)
        if (maps[i].getName() == "Isovists") shapelayer = (int)i;
    if (shapelayer == -1) {
        maps.emplace_back("Isovists", ShapeMap::DATAMAP);
        mg.setDisplayedDataMapRef(maps.size() - 1);
        shapelayer = (int)maps.size() - 1;
        mg.setState(mg.getState() | MetaGraph::DATAMAPS);
        made = 2;
    }
    ShapeMap& map = maps[(size_t)shapelayer];
    // the columns in the order setData inserts them; none of them exists before the first isovist
    static const struct { const char* name; int k; } cols[8] = {
        {"Isovist Area", 0}, {"Isovist Compactness", 1}, {"Isovist Drift Angle", 2}, {"Isovist Drift Magnitude", 3},
        {"Isovist Min Radial", 5}, {"Isovist Max Radial", 4}, {"Isovist Occlusivity", 6}, {"Isovist Perimeter", 7}};
    std::vector<Point2f> poly;
    for (int64_t k = 0; k < n; k++) {
        poly.clear();
        for (int64_t v = off[(size_t)k]; v < off[(size_t)k + 1]; v++) poly.push_back(Point2f(xy[2 * v], xy[2 * v + 1]));
        const int polyref = map.makePolyShape(poly, false);   // false: closed polygon
        if (polyref == -1) continue;                          // an empty polygon makes no shape
        map.getAllShapes()[polyref].setCentroid(points[k]);
        AttributeTable& table = map.getAttributeTable();
        AttributeRow& row = table.getRow(AttributeKey(polyref));
        for (const auto& col : cols) {
            if (simple_version && col.k != 0) continue;
            row.setValue(table.getOrInsertColumn(col.name), out[(size_t)k * 8 + col.k]);
        }
    }
    map.overrideDisplayedAttribute(-2);
    map.setDisplayedAttribute(-1);
    mg.setViewClass(MetaGraph::SHOWSHAPETOP);
    return made;
}

}  // namespace dmxsala
