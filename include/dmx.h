/* dmx.h -- C ABI of the MI355X visibility-graph engine (libdmx.so).
 *
 * Drop-in boundary for the depthmapX VISPREP makeGraph + VGA global path.  Every entry point is
 * extern "C", takes plain pointers and sizes, never throws, and returns an int status
 * (DMX_OK = 0, negative on error; dmx_last_error() explains).  The reference interface each one
 * replaces is cited as file:line in orange-vertex/depthmapX.
 *
 * Ownership: the library owns contexts, point maps and graphs (device buffers included); callers
 * release them with the matching *_free.  Host arrays passed in are copied; host arrays passed out
 * are caller-allocated with the sizes the *_info calls report.  Device pointers (dmx_*_device)
 * must be valid on the context's device.  One context per device; one process per GPU.
 */
#ifndef DMX_H
#define DMX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMX_ABI_VERSION 1

enum {
    DMX_OK = 0,
    DMX_ERR_ARG = -1,          /* invalid argument / handle */
    DMX_ERR_HIP = -2,          /* HIP runtime error (no device, launch failure, OOM) */
    DMX_ERR_CAPACITY = -3,     /* a kernel capacity was exceeded even after retries */
    DMX_ERR_STATE = -4,        /* call sequence not allowed (e.g. makegraph on an unfilled map) */
    DMX_ERR_UNSUPPORTED = -5,  /* feature of the reference not (yet) implemented on this path */
    DMX_ERR_OUTSIDE = -6,      /* fill point outside the region ("Point outside of target region") */
    DMX_ERR_CANCELLED = -7     /* dmx_ctx_cancel / the progress callback stopped the operation
                                  (the reference throws Communicator::CancelledException, genlib/comm.h:61-65) */
};

/* Phases reported to the progress callback. */
enum {
    DMX_PHASE_MAKEGRAPH = 1,   /* sources of PointMap::sparkGraph2 (pointdata.cpp:1293-1322) */
    DMX_PHASE_VGA = 2          /* sources of VGAVisualGlobal::run (vgavisualglobal.cpp:195-202) */
};

typedef struct dmx_ctx dmx_ctx;
typedef struct dmx_pointmap dmx_pointmap;
typedef struct dmx_graph dmx_graph;

/* ---- library / device ------------------------------------------------------------------ */
int dmx_abi_version(void);
/* Thread-local message for the last failing call on this thread. */
const char* dmx_last_error(void);
/* Bind a context to HIP device `device` (the process-local ordinal).  No reference counterpart:
 * salalib is single-threaded CPU code. */
int dmx_ctx_create(int device, dmx_ctx** out);
int dmx_ctx_free(dmx_ctx* ctx);
/* Return the device blocks the engine keeps cached for reuse by the next graph of the same size
 * (run pool, scan order, visibility rows) to the HIP runtime.  Optional; allocation failures do it
 * automatically. */
int dmx_release_cached_memory(void);

/* Progress and cancellation, the Communicator contract (genlib/comm.h:59-142): the reference posts the
 * record count and polls IsCancelled every 500 ms inside makeGraph (pointdata.cpp:1301-1316) and VGA
 * (vgavisualglobal.cpp:195-202).  While a makegraph / VGA-global kernel runs, the calling thread
 * calls fn(user, phase, done, total) every interval_s seconds (<= 0: 0.5 s) and once with
 * done == total when the phase completes; a non-zero return requests cancellation.  fn NULL: no
 * polling (the default).  The kernels read the cancel word between sources, so a cancelled call
 * returns DMX_ERR_CANCELLED within one source's time; its outputs are not written (device outputs
 * are undefined).  A context's callback runs on the thread that made the call. */
typedef int32_t (*dmx_progress_fn)(void* user, int32_t phase, int64_t done, int64_t total);
int dmx_ctx_set_progress(dmx_ctx* ctx, dmx_progress_fn fn, void* user, double interval_s);
/* Request cancellation of the operation running on ctx (callable from any thread).  The request is
 * consumed by the operation that observes it; one made while no operation runs cancels the next
 * makegraph, VGA-global, through-vision, isovist, connections or step-depth (metric, angular, visual) call at its first poll -- before that
 * call writes any output.  VGA local / metric / angular do not poll (a pending request waits). */
int dmx_ctx_cancel(dmx_ctx* ctx);
/* Wall time of the kernels of the last makegraph / vga call, measured with HIP events on the
 * context stream (seconds); kernel_ms receives per-kernel averages. */
int dmx_ctx_last_timing(dmx_ctx* ctx, double* makegraph_s, double* vga_s);
/* Work counters of the last calls (for roofline accounting), up to 40 entries (engine.py names them):
 * [0] sieve cells examined, [1] visible (source,target) pairs, [2] runs written,
 * [3] VGA kernel used (0 top-down v1, 1 direction-optimising restricted to top-down,
 *     2 direction-optimising, 3 tile-resolved) | nodes needing exact in-set corrections << 8,
 * [4] runs read by the BFS, [5] bottom-up levels | top-down levels << 32, [6] cells reached (sum
 * over sources), [7] sources run, [8] bottom-up cells that found no hit, [9] their runs,
 * [10] bitmaps in HBM (direction-optimising), [11] tiles resolved by common runs, [12] launch
 * shape of the tile-resolved search (workgroups | threads a workgroup (256 or 1024) << 40 | frontier bitmap in
 * HBM << 56 | line-resolved summaries (else per-tile column summaries) << 57), [13] hard cells rejected by their tile-visibility row, [14] bytes of those rows read,
 * [15] runs scanned by hard cells, [16] hard cells that hit, [17] hard cells, ... [38] searches the last VGA
 * global / visual step depth call ran again in the reference's level order (vga_ordered.hip), [39] microseconds
 * the last VGA preparation spent on the symmetry scatter and its all-reduces (0 when makeGraph did it), [40] the
 * memory-dependent VGA preparation the last tile search ran with (bits: 0 scan order, 1 scan order released for
 * the partial-tile masks, 2 tile-visibility rows, 3 fully-seen rows, 4 tile-to-tile rows, 5 partial-tile masks,
 * 6 row summaries, 7 asymmetric mode), [41] bytes of tile-visibility rows held, [42] bytes of the scan order
 * held, [43] asymmetric mode: nodes whose runs differ from the reference graph (dmx_graph_set_drawing), [44] lines
 * the last through-vision call walked, [45] its pixel steps, [46] its accumulation variant (0 global atomics,
 * else the side of the LDS window), [47] makeGraph: the depths at which the map's inexact world coordinates take
 * some diagonal cell out of the diagonal bin in the reference (0: none; see dmx_makegraph), [48] VGA tile search: the
 * longest list of tiles holding an unvisited cell that a level's walks took in the launch, [49] its hard cells that
 * went through phase C's row stage (0 under DMX_VGA_CSPLIT=0 and where the stage does not apply), [50] its hard cells
 * that phase C's miss certificate rejected before their rows were read (counted in [13] and [17] as well; 0 under
 * DMX_VGA_CCERT=0, with the frontier in HBM and without the masks).  n <= 51. */
int dmx_ctx_last_stats(dmx_ctx* ctx, int64_t* out, int n);

/* The sources the last makeGraph swept a second time (graph node indices, in the order the passes listed
 * them; a source can appear once per pass): bit 62 set for a capacity overflow (gap list, block spill,
 * staging), clear for a moment-sum certificate that did not decide the float.  Writes
 * min(cap, *n) entries; *n receives the count. */
int dmx_ctx_last_mk_reruns(dmx_ctx* ctx, int64_t* nodes, int64_t cap, int64_t* n);

/* Diagnostics of the last tile-resolved VGA launch: core-clock cycles spent (workgroup leader,
 * summed over workgroups) in level 1, phase A (tile-common runs), B (head runs), C (hard cells)
 * and level bookkeeping. */
int dmx_ctx_last_phase_cycles(dmx_ctx* ctx, int64_t* out5);

/* ---- VISPREP preparation (host model) ----------------------------------------------------- */
/* MetaGraph::addNewPointMap + PointMap::setGrid(spacing, (0,0)) (salalib/pointdata.cpp:122-171),
 * with the drawing `lines` ([n][4] = x1,y1,x2,y2 as PointMap::blockLines reads them,
 * pointdata.cpp:308-320) inside `region` (= MetaGraph::getRegion(), [4] = blx,bly,trx,try). */
int dmx_pointmap_create(const double* region, double spacing, const double* lines, int64_t nlines,
                        dmx_pointmap** out);
int dmx_pointmap_free(dmx_pointmap* pm);
/* dm_runmethods::fillGraph -> PointMap::makePoints(p, FULLFILL) (depthmapXcli/runmethods.cpp:269-277,
 * salalib/pointdata.cpp:402-481).  DMX_ERR_OUTSIDE if the point is outside the region;
 * *made = 0 where makePoints returns false. */
int dmx_pointmap_fill(dmx_pointmap* pm, double x, double y, int* made);
/* The same fill computed on the context's GPU (kernels/fill.hip): PointMap::blockLines
 * (pointdata.cpp:296-357, spacepix.cpp:144-214, p2dpoly.cpp:626-667) on the first fill, then the
 * makePoints/expand flood fill (pointdata.cpp:402-514) in the reference's exact expand order, so
 * the FILLED and order-dependent EDGE bits equal the host fill's.  Same return codes and *made. */
int dmx_pointmap_fill_device(dmx_ctx* ctx, dmx_pointmap* pm, double x, double y, int* made);
/* Seconds of the last dmx_pointmap_fill_device: blockLines (0 when lines were already blocked),
 * flood fill, and the number of fill levels. */
int dmx_ctx_last_fill(dmx_ctx* ctx, double* block_s, double* fill_s, int64_t* levels);
/* PointMap::makePoints(seed, fill_type) (salalib/pointdata.cpp:402-481; MetaGraph::makePoints,
 * mgraph.cpp:237-247), the GUI's three fill modes (depthmapX/views/depthmapview/depthmapview.h:75):
 * 0 FULLFILL (Point::FILLED, what the CLI uses), 1 SEMIFILL (FILLED | CONTEXTFILLED: such cells at odd
 * PixelRefs are skipped as VGA sources and not expanded under a radius or in visual step depth), 2 AUGMENT
 * (Point::AUGMENTED without FILLED).  The reference's AUGMENT fill only ends when the seed expands nowhere
 * (expand stops at FILLED cells only, pointdata.cpp:489, so augmented neighbours re-queue each other
 * forever): that case sets the seed alone, any other returns DMX_ERR_UNSUPPORTED with no cell filled
 * (the occluders are blocked, as before any fill).
 * The _device form runs FULLFILL / SEMIFILL on the context's GPU as dmx_pointmap_fill_device does. */
int dmx_pointmap_make_points(dmx_pointmap* pm, double x, double y, int fill_type, int* made);
int dmx_pointmap_make_points_device(dmx_ctx* ctx, dmx_pointmap* pm, double x, double y, int fill_type, int* made);
/* Restore the FILLED / EDGE / CONTEXTFILLED cell states of a map saved earlier (e.g. the state
 * array of a PointMap chunk of the same grid), as PointMap::read does before makeGraph. */
int dmx_pointmap_set_state(dmx_pointmap* pm, const int32_t* state);
/* cols, rows, bottom-left cell centre, filled count. */
int dmx_pointmap_info(const dmx_pointmap* pm, int32_t* cols, int32_t* rows, double* bl_x, double* bl_y,
                      int64_t* filled);
/* Point::m_state per cell, x-major (cell = x*rows + y, ColumnMatrix order, simplematrix.h:193-218). */
int dmx_pointmap_state(const dmx_pointmap* pm, int32_t* out);
/* Cropped occluder pieces per cell after blockLines: counts[C], pieces[total][4]. */
int dmx_pointmap_cell_lines(dmx_pointmap* pm, int32_t* counts, double* pieces, int64_t* total);

/* ---- makeGraph (GPU) ---------------------------------------------------------------------- */
/* MetaGraph::makeGraph(comm, boundary, maxdist) -> PointMap::sparkGraph2 (salalib/mgraph.cpp:264-284,
 * pointdata.cpp:1246-1341).  Builds nodes [node_begin, node_end) of the filled cells in x-major
 * order (node_end < 0: all) -- a sub-range is one rank's shard.  maxdist = -1: unrestricted.
 * Known divergence, inexact world coordinates: the reference bins a visible cell by
 * whichbin(depixelate(cell) - centre) (pointdata.cpp:1466, pointdata.h:432-520), and depixelate rounds
 * bottom_left + spacing * index at every cell.  On grids where those sums are not exact (an OS-grid origin with a
 * 0.7 m spacing, say; not spacings 2.0 or 0.5 there, and no grid with unit coordinates) a diagonal cell's
 * |gy| / |gx| can fall below 1 - 1e-12, and the reference puts that cell into the sector bin next to the diagonal
 * bin.  This engine gives every diagonal cell the diagonal bin: on such a map every node's visible cells and its
 * three attributes are the reference's, while bin records, run lists and the PointMap chunk's bytes differ at those
 * cells (a diagonal bin is stored as one run from its first to its last cell, Bin::make, ngraph.cpp:243-258: where a
 * moved cell was an end of that run beyond a blocked stretch, the reference's run is shorter, and VGA, which walks
 * runs, then sees fewer cells through it).  The call does not fail; dmx_ctx_last_stats [47] is then non-zero, the same on every rank
 * (it depends on the grid alone), and DMX_VERBOSE prints a line. */
int dmx_makegraph(dmx_ctx* ctx, dmx_pointmap* pm, double maxdist, int boundary, int64_t node_begin,
                  int64_t node_end, dmx_graph** out);
/* Shard bounds for `world` ranks (no reference counterpart: the reference builds the graph on one
 * host, pointdata.cpp:1246-1341).  Sweeps every stride-th source (the middle node of each run of
 * `stride` nodes), models each source's cost from its sieve depth steps and candidate chunks, and writes
 * bounds[0..world] (bounds[0] = 0, bounds[world] = nodes) so that the contiguous ranges
 * [bounds[r], bounds[r+1]) carry equal modelled makeGraph cost.  The counts are deterministic: every rank
 * computes the same bounds without communicating.  boundary as for dmx_makegraph (applied to pm here). */
int dmx_makegraph_balance(dmx_ctx* ctx, dmx_pointmap* pm, double maxdist, int boundary, int32_t world,
                          int64_t stride, int64_t* bounds);
int dmx_graph_free(dmx_graph* g);
/* nodes in the whole map, first/last node built here, runs held. */
int dmx_graph_info(const dmx_graph* g, int64_t* nnodes, int64_t* node_begin, int64_t* node_end, int64_t* nruns);
/* Copies in reference layout (rows for the built range only, node order):
 *   attrs[n][3]  Connectivity, Point First Moment, Point Second Moment (pointdata.cpp:1494-1497)
 *   bins[n][32][4]  Bin::m_dir, m_node_count (u16), m_distance (f32 bits), runs in bin (ngraph.h:48-60)
 *   runs[R][4]   PixelVec start.x,start.y,end.x,end.y in Bin order (ngraph.cpp:234-304)
 *   gridconn[n]  Point::m_grid_connections (pointdata.cpp:1735-1768)
 * Any pointer may be NULL. */
int dmx_graph_copy(dmx_graph* g, float* attrs, int32_t* bins, int16_t* runs, uint8_t* gridconn);
/* The same for the local nodes [node_b, node_e) only (node_e < 0: to the end): bins/attrs/gridconn
 * sized for the range, runs node-ordered (capacity runs_cap entries, < 0: unchecked); *nruns_out
 * = the range's run count (runs may be NULL to query it). */
int dmx_graph_copy_range(dmx_graph* g, int64_t node_b, int64_t node_e, float* attrs, int32_t* bins, int16_t* runs,
                         int64_t runs_cap, int64_t* nruns_out, uint8_t* gridconn);

/* Shard exchange for multi-GPU runs: a graph's built range serialises into one flat blob
 * (device memory) that another rank's dmx_graph_assemble can consume. */
int dmx_graph_blob_size(dmx_graph* g, int64_t* bytes);
int dmx_graph_blob_write_device(dmx_graph* g, void* dst_device, int64_t bytes);
/* Build the whole-map graph from nshards blobs (device pointers, any order of ranges). */
int dmx_graph_assemble_device(dmx_ctx* ctx, dmx_pointmap* pm, const void* const* blobs, const int64_t* sizes,
                              int nshards, dmx_graph** out);

/* ---- VGA global (GPU) ----------------------------------------------------------------------- */
/* MetaGraph::analyseGraph(OUTPUT_VISUAL, global) -> VGAVisualGlobal(radius, gates_only).run
 * (salalib/mgraph.cpp:349-359, vgamodules/vgavisualglobal.cpp:23-216) for source nodes
 * [src_begin, src_end) (src_end < 0: all).  radius = -1 for "n".  The graph must hold every node
 * (dmx_graph_assemble_device for shards).  out: host [N][7] or device (dmx_vga_global_device), rows
 * outside the range untouched, columns in table (alphabetical) order: Visual Entropy, Visual
 * Integration [HH], [P-value], [Tekl], Visual Mean Depth, Visual Node Count, Visual Relativised
 * Entropy.  levels (optional, host [N][3]): total nodes, total depth, BFS levels.
 * The first call on a graph builds its search structures (scan order, tile-visibility rows and, when
 * they take at most a quarter of the free device memory, the partial-tile masks: about 10 GB next to
 * the 36 GB graph at 1000^2); they stay with the graph until dmx_graph_free.  Results do not depend on
 * which of them fit. */
int dmx_vga_global(dmx_ctx* ctx, dmx_graph* g, double radius, int gates_only, int64_t src_begin, int64_t src_end,
                   float* out, int64_t* levels);
int dmx_vga_global_device(dmx_ctx* ctx, dmx_graph* g, double radius, int gates_only, int64_t src_begin,
                          int64_t src_end, float* out_device);
/* The same for an arbitrary list of source nodes (host array of n node indices); rows of other
 * nodes in out_device are left untouched.  Used to interleave multi-GPU shards over the grid. */
int dmx_vga_global_device_list(dmx_ctx* ctx, dmx_graph* g, double radius, int gates_only, const int64_t* nodes,
                               int64_t n, float* out_device);
/* Diagnostics of the VGA preparation (no reference counterpart): the nodes whose visible set is not
 * symmetric (a cell in the node's runs that does not see the node back), found by 64-bit random-weight
 * range hashes and routed through exact in-set corrections.  *n in = capacity, out = count; nodes NULL:
 * only *n.  Builds the preparation on the graph's context if no VGA call has. */
int dmx_graph_special_nodes(dmx_graph* g, int32_t* nodes, int64_t* n);
/* ---- VGA metric (GPU) ----------------------------------------------------------------------- */
/* MetaGraph::analyseGraph(OUTPUT_METRIC) -> VGAMetric(radius, gates_only).run (salalib/mgraph.cpp:
 * 359-361, vgamodules/vgametric.cpp:26-136) for source nodes [src_begin, src_end) (src_end < 0:
 * all); radius < 0 for "n" (otherwise in drawing units, compared with dist * spacing).  out: host
 * [N][4] in node order, rows outside the range untouched: Metric Mean Shortest-Path Angle, Metric
 * Mean Shortest-Path Distance, Metric Mean Straight-Line Distance, Metric Node Count (-1 rows with
 * gates_only). */
int dmx_vga_metric(dmx_ctx* ctx, dmx_graph* g, double radius, int gates_only, int64_t src_begin, int64_t src_end,
                   float* out);
/* ---- VGA angular (GPU) ---------------------------------------------------------------------- */
/* MetaGraph::analyseGraph(OUTPUT_ANGULAR) -> VGAAngular(radius, gates_only).run (salalib/mgraph.cpp:
 * 362-364, vgamodules/vgaangular.cpp:26-133) for source nodes [src_begin, src_end); radius < 0 for
 * "n" (otherwise compared with the cumulative angle).  out: host [N][3] in node order: Angular Mean
 * Depth, Angular Total Depth, Angular Node Count (-1 rows with gates_only). */
int dmx_vga_angular(dmx_ctx* ctx, dmx_graph* g, double radius, int gates_only, int64_t src_begin, int64_t src_end,
                    float* out);
/* ---- VGA visual local (GPU) ----------------------------------------------------------------- */
/* MetaGraph::analyseGraph(OUTPUT_VISUAL, local) -> VGAVisualLocal(gates_only).run
 * (salalib/mgraph.cpp:349-353, vgamodules/vgavisuallocal.cpp:23-117) for source nodes
 * [src_begin, src_end) (src_end < 0: all).  out: host [N][3] in node order, rows outside the range
 * untouched: Visual Clustering Coefficient, Visual Control, Visual Controllability (-1 for skipped
 * sources and neighbourhoods of <= 1 cell).  The two tile bitmaps per source live in LDS up to ~780^2
 * cells and in per-workgroup HBM slices above that (no grid-size limit). */
int dmx_vga_local(dmx_ctx* ctx, dmx_graph* g, int gates_only, int64_t src_begin, int64_t src_end, float* out);
/* ---- VGA through vision (GPU) --------------------------------------------------------------- */
/* MetaGraph::analyseGraph(OUTPUT_THRU_VISION) -> VGAThroughVision().run (salalib/mgraph.cpp:366-368,
 * vgamodules/vgathroughvision.cpp:27-104): for every source node in [src_begin, src_end) (src_end < 0: all)
 * and every cell of the source's runs, the line from that cell to the source is walked with
 * PixelBase::quickPixelateLine (salalib/spacepix.cpp:218-270, the same sequence of FP64 adds) and every pixel
 * between its two ends counts once.  The graph must hold every node (DMX_ERR_STATE otherwise).  Unlike the
 * per-source analyses EVERY row of out (host [N], node order) is written: the count the sources of the range
 * add to that cell, as float ("Through vision").  counts (optional, host [N]) receives the same numbers as
 * integers, so the results of disjoint source ranges (one per GPU) can be summed exactly.  Merge links play no
 * part; context-filled sources are not skipped.  The reference counts in an int (Point::m_misc): a total
 * above INT32_MAX returns DMX_ERR_UNSUPPORTED instead of wrapping.  The gate-counting side branch
 * (vgathroughvision.cpp:61-74, maps with a column __Internal_Gate) is not part of this call.  Progress and
 * cancel as in dmx_vga_global. */
int dmx_vga_thruvision(dmx_ctx* ctx, dmx_graph* g, int64_t src_begin, int64_t src_end,
                       float* out /* host [N] */, int64_t* counts /* host [N], optional */);
/* ---- Connections of the visibility graph (GPU) ------------------------------------------------- */
/* Node::contents (salalib/ngraph.cpp:158-191, over Bin::first / next / cursor, :392-416) for the nodes
 * [node_begin, node_end) (node_end < 0: all): the cells of each node's runs in the reference's order -- bins 0..31,
 * the runs of a bin as stored, the cells of a run from its start along the bin's direction (a run's start is always
 * visited; a diagonal bin is one span) -- without the cells that occurred earlier in the same node's enumeration
 * (depthmapX::addIfNotExists keeps the first occurrence; a graph fresh from makeGraph has none, one read back from a
 * .graph can, ngraph.cpp:536-563).  With DMX_CONN_EXPORT the list is cut down to what
 * PointMap::outputConnectionsAsCSV (salalib/pointdata.cpp:656-681) writes for the node: the cells that are filled()
 * and are not a node at or before the source in x-major order (here: FILLED, and cell > the source's cell).
 * Divergence: a run shifted out of the grid by the format's 4-bit row shift makes the reference read points outside
 * its matrix (undefined behaviour); here cells outside the grid are dropped.
 *   off    host [n + 1] (n = nodes of the range), or NULL: the start of each node's cells in refs; off[n] = *total
 *   refs   host [cap], or NULL: PixelRefs packed as the reference packs them, (x << 16) + (y & 0xffff)
 * The capacity protocol is dmx_isovists': refs NULL or cap < *total sets off and *total only (DMX_OK); nothing is
 * half written.  An empty range: DMX_OK.  Nodes the graph does not hold (a shard): DMX_ERR_STATE.  Progress and cancel
 * as in dmx_vga_thruvision (phase DMX_PHASE_VGA, the unit is a node); on a cancel or an error no output is touched.
 * The order of the output does not depend on scheduling (count, scan, emit: kernels/connections.hip). */
#define DMX_CONN_EXPORT 1   /* apply outputConnectionsAsCSV's filter; 0: Node::contents */
int dmx_graph_connections(dmx_ctx* ctx, dmx_graph* g, int64_t node_begin, int64_t node_end, int flags,
                          int64_t* off /* [n+1] */, int32_t* refs /* [cap] or NULL */, int64_t cap, int64_t* total);
/* The edge lines of PointMap::outputConnectionsAsCSV(stream, delim) (pointdata.cpp:656-681; depthmapXcli -m EXPORT
 * -em pointmap-connections-csv, runmethods.cpp:662-669) for the nodes of the range, formatted on the device: per
 * edge "\n" + from + delim + to, both PixelRefs as the decimal of the packed int (PixelRef::operator int).  The
 * header "RefFrom" + delim + "RefTo" is the caller's; the texts of consecutive ranges, concatenated, are the text
 * of their union.  off (optional) [n + 1]: the byte at which each node's lines start; buf NULL or cap < *size: only
 * off and *size are set.  delim empty or longer than 8 bytes: DMX_ERR_ARG.  Otherwise as dmx_graph_connections. */
int dmx_graph_connections_csv(dmx_ctx* ctx, dmx_graph* g, int64_t node_begin, int64_t node_end, const char* delim,
                              int64_t* off /* [n+1] bytes, or NULL */, char* buf /* [cap] or NULL */, int64_t cap,
                              int64_t* size);
/* The last dmx_graph_connections / _csv call: kernel seconds of the counting pass with its scan and of the emitting
 * pass (0 when nothing was emitted), and out4 = {1 when the per-node bitmap lay in per-workgroup HBM slices (grids
 * whose bitmap does not fit LDS; 0: in LDS), nodes that held a duplicate, cells dropped as duplicates, cells dropped
 * outside the grid}.  Any pointer may be NULL. */
int dmx_ctx_last_connections(dmx_ctx* ctx, double* count_s, double* emit_s, int64_t* out4);
/* ---- Agent analysis: standard agents, Gate Counts (GPU) ----------------------------------------- */
/* depthmapXcli -m AGENTS with the standard look (salalib/agents/: AgentEngine::run, AgentSet, Agent; SEL_STANDARD).
 * The reference draws every agent's numbers from one global generator, so its run is one sequential stream.  Agents
 * never interact; here every agent owns a stream (the reference's 64-bit LCG, seeded as pafsrand(seed) seeds it), and
 * the AGENT is the reference's bit for bit: after pafsrand(agent_seed) a reference Agent on the same graph walks the
 * same cells to the same final location.  The ENSEMBLE (who is released when, where and with which seed) is this
 * engine's, so a run here and a run of the reference hold different, equally distributed counts.
 *
 * dmx_agent_schedule (host only) restates AgentEngine::run's release loop (agentengine.cpp:66-84) and AgentSet::init
 * (agentset.cpp:28-40) over two streams of its own.  The stream seeded `seed` gives, per timestep, the count
 * invcumpoisson(prandomr(), release_rate) and, per agent, its seed (the stream's next pafrand) and -- with release
 * cells -- pafrand() % nrelease.  Without release cells a stream seeded `locseed` repeats pickPixel(prandom())
 * (pointdata.cpp:1771-1775) until the cell is FILLED; a draw of exactly 0 is drawn again (the reference indexes
 * cell -1 there).  moves = min(lifetime, timesteps - release timestep).  Cells are x-major indices.  *nagents
 * receives the number of agents; the first cap are written (cap 0: count only).  A release cell outside the grid
 * or not FILLED: DMX_ERR_ARG; a map without FILLED cells and without release cells: DMX_ERR_STATE. */
int dmx_agent_schedule(const dmx_pointmap* pm, uint32_t seed, int32_t timesteps, double release_rate,
                       int32_t lifetime, const int32_t* release_cells, int64_t nrelease, int32_t locseed,
                       int32_t* start_cell, uint32_t* agent_seed, int32_t* moves, int64_t cap, int64_t* nagents);
/* Every agent of the table from Agent::onInit(start) through moves[i] x Agent::onMove, on the GPU.  vbin is
 * AgentProgram::m_vbin (-1: the whole isovist; runmethods.cpp:499-504 derives it from the field of view), steps
 * m_steps.  The graph must hold every node.
 *   counts      host [cols*rows], x-major: per cell, the moves that entered it from another cell while it is FILLED
 *               (what the reference adds to "Gate Counts").  Written, not added to; sums of calls over disjoint parts
 *               of a table equal the whole table's, in any order.
 *   final_cell  host [n], final_loc host [n][2], stuck host [n]: m_node, m_loc, m_stuck after the last move (optional)
 *   trail       host [ntrail][max of moves] or NULL: the cell after each move of the first ntrail agents, -1 beyond
 *               an agent's moves
 * Defined where the reference is not: an agent whose look finds no cell even in the whole isovist is stuck for good
 * and counts nothing more; a draw beyond the cells a bin's runs enumerate (re-read maps only) takes the bin's last
 * cell and is reported by dmx_ctx_last_agents.  binfromvec needs acos, whose last bit may differ between device and
 * host: an agent whose look lies within 1e-9 of a bin boundary is run again on the host (reported as well).
 * Progress and cancel as in dmx_vga_thruvision (phase DMX_PHASE_VGA; the unit is 64 agents).
 * Test and measurement hook: with the environment variable DMX_AGENTS_HOST set, the call launches no kernel and runs
 * EVERY agent through that host routine on one thread ("lazy": the run pool read a bin at a time, as for a flagged
 * agent; any other value: the whole pool downloaded first).  The results are the same; dmx_ctx_last_agents then
 * reports every agent as run again on the host.  Leave it unset in production. */
int dmx_agents(dmx_ctx* ctx, dmx_graph* g, int32_t vbin, int32_t steps, int64_t nagents,
               const int32_t* start_cell, const uint32_t* agent_seed, const int32_t* moves,
               uint32_t* counts /* [cols*rows], x-major */, int32_t* final_cell, double* final_loc /* [n][2] */,
               uint8_t* stuck, int32_t* trail /* [ntrail][max moves] or NULL */, int64_t ntrail);
/* The last dmx_agents call: kernel seconds and out4 = {moves made (Agent::onStep calls), looks, agents run again on
 * the host, bins clamped}.  Any pointer may be NULL. */
int dmx_ctx_last_agents(dmx_ctx* ctx, double* seconds, int64_t* out4);
/* More of the same call: the seconds the host routine spent on the agents run again (without the download of the
 * graph's per-node arrays that the first of them costs: cell map, grid connections, bin counts, run counts, run starts;
 * with the reads of the run pool, a bin at a time as the looks need it), and out3 =
 * {narrow looks that fell back to the whole isovist, diagonal steps taken, moves that stopped (both diagonal tries
 * refused)}.  Any pointer may be NULL. */
int dmx_ctx_last_agents_detail(dmx_ctx* ctx, double* host_seconds, int64_t* out3);
/* ---- VGA isovist analysis (GPU) -------------------------------------------------------------- */
/* MetaGraph::analyseGraph(OUTPUT_ISOVIST) -> VGAIsovist().run (salalib/mgraph.cpp:346-348,
 * vgamodules/vgaisovist.cpp:24-129; what depthmapXcli -m VGA runs without -vm): a BSP tree of the drawing lines
 * is built on the host, and for every node in [src_begin, src_end) (src_end < 0: all) the isovist polygon of the
 * cell centre is made by walking the tree front to back (Isovist::makeit, salalib/isovist.cpp).  The lines are
 * those the graph's point map was created with, or those given to dmx_graph_set_drawing (a chunk-loaded map);
 * DMX_ERR_STATE if there are none.  The graph must hold every node (DMX_ERR_STATE otherwise).
 *   out         host [N][8], node order, columns in table order: Isovist Area, Compactness, Drift Angle, Drift
 *               Magnitude, Max Radial, Min Radial, Occlusivity, Perimeter.  Only rows of the range are written, and
 *               of those not the cells the reference skips (context-filled at an odd PixelRef, vgaisovist.cpp:50-52:
 *               their rows keep what they held, -1 in a fresh table).  simple_version: only column 0 is written.
 *   occ_dist    optional, host [N][32]: Bin::m_occ_distance of every bin (rows as for out)
 *   occ_counts  optional, host [N][32]: sizes of Node::m_occlusion_bins (rows as for out)
 *   occ_pixels  optional, host [occ_cap]: the PixelRefs of the occlusion bins of the rows written, packed as the
 *               reference packs them ((x << 16) + (y & 0xffff)), by node, then bin, then the reference's push order.
 *               *occ_total (optional) receives their number; occ_pixels NULL or occ_cap < *occ_total: only
 *               *occ_total is set.
 * Results depend on the platform's acos / sin / cos in the last bit of FP64, which the rounding to float hides
 * except where the reference itself is unstable.  Per-cell lists have fixed capacities
 * (policy.hpp); a cell that exceeds one is run again with larger lists, DMX_ERR_CAPACITY only after that.
 * Progress and cancel as in dmx_vga_thruvision (phase DMX_PHASE_VGA; the unit is a tile of 8 x 8 cells). */
int dmx_vga_isovist(dmx_ctx* ctx, dmx_graph* g, int simple_version, int64_t src_begin, int64_t src_end,
                    float* out /* host [N][8] */, float* occ_dist /* host [N][32], optional */,
                    int32_t* occ_counts /* host [N][32], optional */, int32_t* occ_pixels, int64_t occ_cap,
                    int64_t* occ_total);
/* The last dmx_vga_isovist or dmx_isovists: seconds of the host BSP build and of the kernels (either may be NULL),
 * and out4 = tree nodes, tree depth, cells (points) run again for capacity, the most blocks a cell (point) held. */
int dmx_ctx_last_isovist(dmx_ctx* ctx, double* bsp_s, double* kernel_s, int64_t* out4);
/* ---- Isovists at arbitrary points (GPU) -------------------------------------------------------- */
/* MetaGraph::makeIsovist (salalib/mgraph.cpp:491-521; depthmapXcli -m ISOVIST, runmethods.cpp:635-647) for a batch of
 * n points: Isovist::makeit(root, p, region, startangle, endangle) and setData (salalib/isovist.cpp:31-120, :270-335)
 * per point, from the drawing alone -- no point map and no graph.  A BSP tree of `lines` ([nlines][4] = x1,y1,x2,y2)
 * is built on the host.
 *   region   [4] blx, bly, trx, try: what makeit takes for its tolerance (MetaGraph::m_region, the drawing's bounding
 *            box; tolerance = max(width, height) * 1e-9).  NULL: the bounding box of lines.
 *   points   [n][2].  angles [n][2] startangle, endangle in radians as makeit takes them (start == end or (0, 2 pi):
 *            full circle; start > end: a cone across angle 0), or NULL: full circles.
 *   out      host [n][8], columns in the table order of dmx_vga_isovist; simple_version: only column 0 of a row is
 *            written.
 *   poly_off / poly_xy   optional CSR in the caller's order: poly_off [n + 1], poly_xy [poly_cap][2] the polygons'
 *            vertices (Isovist::getPolygon(), m_poly order, in doubles; a cone's polygon holds its centre).
 *            *poly_total (optional) receives their number; poly_xy NULL or poly_cap < *poly_total: poly_off and
 *            *poly_total are set and no vertex is written (DMX_OK).  Where the tree cuts a wall the polygon holds a
 *            vertex on that wall, as the reference's does; the reference's cuts depend on the state of its random
 *            generator (BSPTree::makeLines), so vertex counts agree with it only after dropping those collinear
 *            vertices.
 * n == 0: DMX_OK.  No (or only zero-length) lines: DMX_ERR_STATE.  A coordinate or angle that is not finite:
 * DMX_ERR_ARG.  Per-point lists have the capacities of dmx_vga_isovist; a point that exceeds one is run again with
 * larger lists, DMX_ERR_CAPACITY only after that.  Progress and cancel as in dmx_vga_isovist (phase DMX_PHASE_VGA; the
 * unit is 64 points).  On an error or a cancel no output array is touched.  Results do not depend on the order of
 * the points. */
int dmx_isovists(dmx_ctx* ctx, const double* lines, int64_t nlines, const double* region /* [4] or NULL */,
                 const double* points /* [n][2] */, const double* angles /* [n][2] start,end or NULL: full circle */,
                 int64_t n, int simple_version, float* out /* [n][8] */,
                 int64_t* poly_off /* [n+1] or NULL */, double* poly_xy /* [poly_cap][2] or NULL */,
                 int64_t poly_cap, int64_t* poly_total /* or NULL */);
/* Multi-GPU share of the VGA preparation (no reference counterpart: the reference prepares nothing;
 * this splits our own O(runs) pre-passes).  Every rank holds the whole graph; the per-node scatters
 * (in-set hash sums, tile-visibility rows) then run over nodes [node_begin, node_end)
 * only and each partial device buffer is handed to fn, which must sum it in place over all ranks
 * (an all-reduce SUM of `count` elements of dtype DMX_I32 / DMX_I64, returning 0 on success) before
 * returning.  Every rank must call this with the same fn semantics before its first VGA call on g;
 * fn is called the same number of times, in the same order, on every rank.  fn = NULL undoes it. */
#define DMX_I32 0
#define DMX_I64 1
typedef int (*dmx_allreduce_fn)(void* device_ptr, int64_t count, int dtype, void* user);
int dmx_graph_set_prep_shard(dmx_graph* g, int64_t node_begin, int64_t node_end, dmx_allreduce_fn fn, void* user);

/* ---- VGA metric step depth (GPU) ----------------------------------------------------------- */
/* dm_runmethods::runStepDepth with -sdt metric -> MetaGraph::analyseGraph(point_depth_selection=2)
 * -> VGAMetricDepth::run (depthmapXcli/runmethods.cpp:735-778, salalib/mgraph.cpp:327-330,
 * vgamodules/vgametricdepth.cpp:23-92).  sel_cells: x-major cell indices of the selection
 * (PointMap::setCurSel keeps FILLED cells only; order and duplicates do not matter).  out: host
 * [N][3] in node order: Metric Step Shortest-Path Angle, Metric Step Shortest-Path Length,
 * Metric Straight-Line Distance (single selected cell only, else -1); unreached cells -1.
 * DMX_ERR_STATE if no filled cell is selected (the reference then skips the analysis). */
int dmx_metric_stepdepth(dmx_ctx* ctx, dmx_graph* g, const int32_t* sel_cells, int64_t nsel, float* out);
/* ---- VGA angular step depth (GPU) ---------------------------------------------------------- */
/* dm_runmethods::runStepDepth with -sdt angular -> MetaGraph::analyseGraph(point_depth_selection=3)
 * -> VGAAngularDepth::run (depthmapXcli/runmethods.cpp:770-772, salalib/mgraph.cpp:334-336,
 * vgamodules/vgaangulardepth.cpp:23-75).  sel_cells as for dmx_metric_stepdepth.  out: host [N]
 * "Angular Step Depth" in node order (unreached cells -1).  DMX_ERR_STATE if no filled cell is
 * selected. */
int dmx_angular_stepdepth(dmx_ctx* ctx, dmx_graph* g, const int32_t* sel_cells, int64_t nsel, float* out);
/* ---- VGA visual step depth (GPU) ----------------------------------------------------------- */
/* dm_runmethods::runStepDepth with -sdt visual -> MetaGraph::analyseGraph(point_depth_selection=1)
 * -> VGAVisualGlobalDepth::run (depthmapXcli/runmethods.cpp:767-769, salalib/mgraph.cpp:312-314,
 * vgamodules/vgavisualglobaldepth.cpp:23-77).  sel_cells as for dmx_metric_stepdepth.  out: host
 * [N] "Visual Step Depth" in node order (unreached cells -1).  DMX_ERR_STATE if no filled cell is
 * selected.  Grids up to 1024^2 with a symmetric graph take the tile-resolved BFS; others the
 * level-synchronous top-down search (kernels/vstep.hip). */
int dmx_visual_stepdepth(dmx_ctx* ctx, dmx_graph* g, const int32_t* sel_cells, int64_t nsel, float* out);
/* Kernel time of the last step-depth call, expanders popped, cells relaxed. */
int dmx_ctx_last_stepdepth(dmx_ctx* ctx, double* seconds, int64_t* expanders_popped, int64_t* cells_relaxed);
/* How the last metric step depth ran: out4 = {mode (0 serial, 1 batched over the whole GPU, 2 a
 * batch capacity overflowed and the serial kernel re-ran the search), batches, cells improved,
 * ambiguous cells folded sequentially}.  The batches slot has two meanings.  Mode 1: the batches
 * of the whole-GPU search.  Modes 0 and 2, angular step depth, and dmx_vga_metric /
 * dmx_vga_angular (which leave mode 0; summed over their sources and attempts): the refills of the
 * serial search's queue, i.e. how often its LDS window ran dry and was refilled from the HBM
 * overflow list. */
int dmx_ctx_last_stepdepth_detail(dmx_ctx* ctx, int64_t* out4);
/* Kernel launches of the last serial metric / angular step depth: 1, plus one for every time the
 * queue's overflow list was too small and the search ran again with a list four times as long (after
 * four launches the call fails with DMX_ERR_CAPACITY).  0 when the batched search answered.  The
 * environment variable DMX_SD_CAP sets the first list's length (a test hook, as for VGA metric /
 * angular). */
int dmx_ctx_last_stepdepth_attempts(dmx_ctx* ctx, int64_t* attempts);
/* What the folds of the last batched metric step depth met: out5 = {ambiguous cells folded by the
 * one-block-per-cell pass (relaxer lists longer than 32), the longest relaxer list folded by either
 * pass, the most ambiguous cells of one batch, the most relaxer-list entries of one batch (counted
 * past their capacity), overflow reason bits}.  Reason bits: 1 the list entries of a batch (2^22), 2
 * the ambiguous cells of a batch (2^16), 4 the relaxers of one ambiguous cell (2048); 0 when the
 * batched search answered.  In mode 2 (dmx_ctx_last_stepdepth_detail) these are the counters of the
 * batched attempt the serial kernel replaced, as are that call's cells improved and ambiguous cells;
 * all zero when no batched search was tried.  The environment variables DMX_SDB_AMB_CAP and
 * DMX_SDB_ENT_CAP shrink the two batch capacities (test hooks). */
int dmx_ctx_last_stepdepth_batched(dmx_ctx* ctx, int64_t* out5);

/* ---- .graph PointMap chunk (host) ------------------------------------------------------------ */
/* The bytes PointMap::write emits into a .graph file (salalib/pointdata.cpp:1158-1188, with
 * AttributeTable::write attributetable.cpp:427-456, Point::write point.cpp:51-73, Node/Bin/PixelVec
 * write ngraph.cpp:209-220,447-472,517-583): header, attribute table (columns alphabetical, stats
 * replayed in setValue order), every cell x-major with its run-length node (4-bit ShiftLength).
 * bins/runs/gridconn as dmx_graph_copy returns them; values [ncols][nnodes] in insertion order;
 * displayed indexes the columns.  buf NULL (or cap too small): only *size is set. */
int dmx_chunk_write(const dmx_pointmap* pm, int64_t nnodes, const int32_t* bins, const int16_t* runs, int64_t nruns,
                    const uint8_t* gridconn, int ncols, const char* const* names, const float* values,
                    const uint8_t* locked, const uint8_t* setmask, int displayed, int boundary, uint8_t* buf, int64_t cap,
                    int64_t* size);
/* setmask (optional, [ncols][nnodes]): rows the analysis called setValue on (column statistics
 * skip the others, like the reference's AttributeColumnImpl::updateStats). */
/* PointMap::read (pointdata.cpp:1073-1156, ngraph.cpp:420-445,491-563): decode a chunk; runs come
 * back with the reference's lossy 4-bit row shift applied. */
typedef struct dmx_chunk dmx_chunk;
int dmx_chunk_parse(const uint8_t* buf, int64_t size, dmx_chunk** out);
int dmx_chunk_free(dmx_chunk* c);
int dmx_chunk_info(const dmx_chunk* c, int32_t* cols, int32_t* rows, double* spacing, double* bl, int64_t* nnodes,
                   int64_t* nruns, int32_t* ncols, int32_t* displayed_sorted, int64_t* bytes_used);
int dmx_chunk_column(const dmx_chunk* c, int i, char* name, int name_cap, float* values, int* locked);
int dmx_chunk_arrays(const dmx_chunk* c, int32_t* state, int32_t* bins, int16_t* runs, uint8_t* gridconn);
/* A state-only point map (region = MetaGraph::getRegion()) and its device graph from a chunk: what
 * the reference CLI's VGA / STEPDEPTH steps analyse after loadGraph (runmethods.cpp:33). */
int dmx_chunk_load(dmx_ctx* ctx, const dmx_chunk* c, const double* region, dmx_pointmap** pm, dmx_graph** g);
/* Device graph from host node records (e.g. a graph the reference itself built or loaded). */
int dmx_graph_from_runs(dmx_ctx* ctx, dmx_pointmap* pm, int64_t nnodes, const int32_t* bins, const int16_t* runs,
                        int64_t nruns, const uint8_t* gridconn, const float* attrs, dmx_graph** out);
/* Merge links (Point::m_merge, set by the LINK mode / PointMap::mergePixels, salalib/pointdata.cpp:1653-1680):
 * n pairs (cell, partner cell) of x-major indices; a pair may be listed in both directions (as
 * PointMap::write stores it on both points); a cell belongs to at most one link (DMX_ERR_ARG otherwise).
 * dmx_chunk_load sets them from the chunk.  Every search that follows merge links in the reference
 * follows them here, with the reference's bookkeeping of the partner: VGA global (vgavisualglobal.cpp:
 * 113-122), visual step depth (vgavisualglobaldepth.cpp:55-63), metric / angular all sources
 * (vgametric.cpp:97-105, vgaangular.cpp:95-104) and metric / angular step depth (vgametricdepth.cpp:68-83,
 * vgaangulardepth.cpp:57-67).  Both ends must be filled cells of the graph (DMX_ERR_ARG at the analysis).
 * A link with one end CONTEXTFILLED at an odd PixelRef is followed exactly too: where the reference's result
 * depends on its pop order inside a level (VGA global with a radius where a source finds both ends at one
 * level; visual step depth where extracting the unexpanded end would reach a new cell) that source or search
 * is run again in the reference's own level order (kernels/vga_ordered.hip).  VGA visual local has no merge
 * logic.  The links are set on the
 * graph's point map as well (they belong to the points: a chunk written from it saves them).  A chunk
 * (dmx_chunk_merges, dmx_chunk_load) must store every link on both of its points (DMX_ERR_ARG otherwise). */
int dmx_graph_set_merges(dmx_graph* g, const int32_t* cell_pairs, int64_t n);
/* The drawing ([n][4] lines x1,y1,x2,y2, the MetaGraph's drawing layers) the graph's point map was made from.  A
 * graph read back from a .graph file is asymmetric at scale: PixelVec::write stores each run after a bin's first
 * as a 4-bit row shift (salalib/ngraph.cpp:536-583), so a jump of more than 15 rows moves every later run of the
 * bin, and Bin::write's unsigned short node count drops the runs of a bin of 65536 k cells (:447-472).  With the
 * drawing, VGA global makes the map's graph again as a symmetric reference and runs the tile search on it, the
 * nodes whose runs differ pushing their own runs (exact; DESIGN.md section 2, asymmetric mode); without it, such
 * a graph takes the top-down search.  Replaces nothing in the reference: its VGA walks the re-read runs as they
 * are (vgavisualglobal.cpp:96-128), which this reproduces.  The reference graph is made by the first VGA global
 * call and kept on the graph; a new drawing or dmx_graph_set_merges drops it (a graph with merge links does not run
 * in this mode, one cleared of them does again).  Making it leaves the context's makeGraph figures
 * (dmx_ctx_last_timing, the makeGraph counters of dmx_ctx_last_stats, dmx_ctx_last_mk_reruns) as they were. */
int dmx_graph_set_drawing(dmx_graph* g, const double* lines, int64_t nlines);
/* The same links on a point map: written into its PointMap chunk (Point::write, point.cpp:51-73) and
 * followed by the graphs made from it (dmx_makegraph, dmx_graph_assemble_device, dmx_graph_from_runs). */
int dmx_pointmap_set_merges(dmx_pointmap* pm, const int32_t* cell_pairs, int64_t n);
/* The merge links stored in a chunk, one entry per link (cell < partner cell): *n in = capacity of
 * cell_pairs ([n][2]), out = number of links; cell_pairs NULL: only *n. */
int dmx_chunk_merges(const dmx_chunk* c, int32_t* cell_pairs, int64_t* n);
/* The attribute rows of a chunk in table (key) order, for PointMap::outputSummary (pointdata.cpp:554-587): keys
 * [nrows] the rows' PixelRefs as ints, visible [nrows] what isObjectVisible(m_layers, row) gives (layermanager.h:
 * 84-87: the map's visible layers & the row's layer key).  nrows from dmx_chunk_flags; either may be NULL. */
int dmx_chunk_rows(const dmx_chunk* c, int32_t* keys, uint8_t* visible);
/* Point::m_merge as the chunk stores it, for PointMap::outputLinksAsCSV (pointdata.cpp:683-706): (cell, partner
 * cell) of EVERY point with a link, in x-major order of the cell -- a link appears once per point that stores it,
 * and nothing is checked (dmx_chunk_merges normalises and checks).  *n in = capacity of cell_pairs ([n][2]), out =
 * the number of records; cell_pairs NULL: only *n. */
int dmx_chunk_merge_records(const dmx_chunk* c, int32_t* cell_pairs, int64_t* n);
/* Editing a parsed chunk the way the reference edits a PointMap it read (PointMap::read then ::write,
 * pointdata.cpp:1073-1188): columns that are not set keep their bytes (stats, display parameters,
 * formula), point records are re-emitted with the state bits PointMap::read keeps.
 * processed / boundary flags, points with merge links, attribute rows. */
int dmx_chunk_flags(const dmx_chunk* c, int* processed, int* boundary, int64_t* merges, int64_t* nrows);
/* AttributeTable::insertOrResetColumn / insertOrResetLockedColumn (attributetable.cpp:303-326) + setValue on
 * the rows of setmask (NULL: all; values [nrows] in row = node order); make_displayed: the analysis's
 * setDisplayedAttribute.  The chunk's dmx_chunk_column / dmx_chunk_info views are not refreshed. */
int dmx_chunk_set_column(dmx_chunk* c, const char* name, const float* values, const uint8_t* setmask, int locked,
                         int make_displayed);
int dmx_chunk_set_displayed(dmx_chunk* c, int physical_column);
/* The isovist analysis's per-node data as the chunk stores it (PointMap::read reads it back, the agent engine
 * consumes it): occ_dist [N][32] Bin::m_occ_distance, occ_counts [N][32] the sizes of Node::m_occlusion_bins,
 * occ_pixels their PixelRefs packed (x << 16) + (y & 0xffff), by node, bin, stored order; any may be NULL, and
 * occ_pixels is filled only when cap holds them all.  *total: the number of PixelRefs. */
int dmx_chunk_occlusion(const dmx_chunk* c, float* occ_dist, int32_t* occ_counts, int32_t* occ_pixels, int64_t cap,
                        int64_t* total);
/* Rewrites the node records so that dmx_chunk_serialize emits this data as Node::write and Bin::write do
 * (ngraph.cpp:209-220, :447-472).  A chunk it was never called on serialises byte for byte as before. */
int dmx_chunk_set_occlusion(dmx_chunk* c, const float* occ_dist, const int32_t* occ_counts, const int32_t* occ_pixels);

int dmx_chunk_set_name(dmx_chunk* c, const char* name);
/* PointMap::setCurSel(r, add) of the STEPDEPTH selection (runmethods.cpp:745-753): Point::SELECTED on the
 * filled cells among `cells` (x-major indices); MetaGraph::write then saves it. */
int dmx_chunk_select_cells(dmx_chunk* c, const int32_t* cells, int64_t n);
/* PointMap::unmake(removeLinks) (pointdata.cpp:1343-1374): VISPREP -pu [-pl]. */
int dmx_chunk_unmake(dmx_chunk* c, int remove_links);
/* PointMap::write of the (edited) chunk; buf NULL or cap too small: only *size. */
int dmx_chunk_serialize(const dmx_chunk* c, uint8_t* buf, int64_t cap, int64_t* size);

/* ---- .graph PointMap chunk, node records on the GPU ------------------------------------------ */
/* PointMap::write of g's point map with g's nodes; bytes equal dmx_chunk_write(pm, dmx_graph_copy(g)...),
 * followed, when map_name is not NULL / "VGA Map", by what dmx_chunk_set_name + dmx_chunk_serialize give.
 * The header, the attribute table and the two flag bytes are written on the host; the Point / Node records
 * (more than 99 % of the bytes) are encoded on g's device from the graph as it lies there and copied out in
 * slabs, so neither the runs nor the chunk are held a second time.  columns as in dmx_chunk_write.
 * buf NULL or cap too small: only *size is set (from the size pass; nothing is encoded).  DMX_ERR_ARG for a
 * bin with a node count and no runs, DMX_ERR_STATE for a shard (node_begin != 0 or node_end != nnodes). */
int dmx_graph_chunk_write(dmx_graph* g, const char* map_name, int ncols, const char* const* names,
                          const float* values, const uint8_t* locked, const uint8_t* setmask, int displayed,
                          int boundary, uint8_t* buf, int64_t cap, int64_t* size);
/* Host only: walk a chunk's records without decoding them (header, attribute table, then from bin header to
 * bin header); every record's end is checked against size, DMX_ERR_ARG with dmx_chunk_parse's messages on
 * damage.  Any out pointer may be NULL. */
int dmx_chunk_scan(const uint8_t* buf, int64_t size, int32_t* cols, int32_t* rows, int64_t* nnodes,
                   int64_t* nruns, int64_t* bytes_used);
/* dmx_chunk_parse + dmx_chunk_load in one call, node records decoded on the GPU: the scan above validates the
 * chunk and keeps the cells' state, grid connections, merge links and each node's extent; the bytes are
 * uploaded in slabs and a kernel writes the graph's runs and bin records in place.  Occlusion data in the
 * chunk is skipped.  Results and errors are dmx_chunk_load's. */
int dmx_chunk_load_bytes(dmx_ctx* ctx, const uint8_t* buf, int64_t size, const double* region,
                         dmx_pointmap** pm, dmx_graph** g);

/* ---- .graph file (host) ---------------------------------------------------------------------- */
/* The MetaGraph container, METAGRAPH_VERSION 440: MetaGraph::readFromFile / readFromStream
 * (salalib/mgraph.cpp:2475-2654) and MetaGraph::write(file, 440, false) (mgraph.cpp:2656-2757, as
 * depthmapXcli calls it, runmethods.cpp:113,265,339,776).  Drawing layers (SpacePixelFile / ShapeMap /
 * SalaShape, spacepixfile.cpp:28-57, shapemap.cpp:49-76,2273-2449) are parsed and re-emitted as the
 * reference re-emits them; point maps are PointMap chunks (dmx_chunk_*); shape graphs and data maps are
 * carried through unchanged.  Older file versions need the reference's legacy mgraph440 reader:
 * DMX_ERR_UNSUPPORTED. */
typedef struct dmx_graphfile dmx_graphfile;
int dmx_graphfile_read(const char* path, dmx_graphfile** out);
int dmx_graphfile_free(dmx_graphfile* g);
int dmx_graphfile_write(const dmx_graphfile* g, const char* path);
/* MetaGraph m_state / m_view_class, m_region ([4] blx, bly, trx, try), the drawing lines PointMap::blockLines
 * reads (every shown layer, pointdata.cpp:308-320), point map count, displayed point map. */
int dmx_graphfile_info(const dmx_graphfile* g, int32_t* state, int32_t* view_class, double* region, int64_t* nlines,
                       int32_t* npointmaps, int32_t* displayed);
int dmx_graphfile_lines(const dmx_graphfile* g, double* lines /* [nlines][4] */);
int dmx_graphfile_set_view(dmx_graphfile* g, int32_t state, int32_t view_class);
/* Point map i (the pointer stays valid until the next put on the same file). */
int dmx_graphfile_pointmap(const dmx_graphfile* g, int i, const uint8_t** chunk, int64_t* size);
/* Replace point map i, or (i = -1) append it and make it the displayed one (MetaGraph::addNewPointMap). */
int dmx_graphfile_put_pointmap(dmx_graphfile* g, int i, const uint8_t* chunk, int64_t size);
/* The name addNewPointMap gives the next map ("VGA Map", then "VGA Map 1", ...; mgraph.cpp:2791-2809). */
int dmx_graphfile_new_pointmap_name(const dmx_graphfile* g, char* name, int cap);
/* MetaGraph::setViewClass(SHOWVGATOP) applied to a view class (mgraph.cpp:167-177). */
int32_t dmx_view_vga_top(int32_t view_class);

#ifdef __cplusplus
}
#endif
#endif
