// policy.hpp -- the engine's tuning and memory decisions in one place (DESIGN.md §9 "Policy").
//
// Every constant here was chosen by an A/B measurement on MI355X at BASELINE.json configs[2] (1000^2) and,
// where it matters, configs[4] (2000^2/5000); the record each one rests on is named next to it.  None of them
// changes a result: every path they choose between is exact (the parity tests run every one of them).
//
// Run-time overrides are test hooks (DMX_* environment variables, read through hook() / hook_int()).  The
// suite runs with the defaults; the hooks exist for the A/B records and to force fallbacks in tests.
#pragma once
#include <cstdint>
#include <cstdlib>

namespace dmx {
namespace policy {

// ---- makeGraph (makegraph.hip)
// sources of the pool-sizing sample pass (run when the worst-case pool would not fit)
constexpr int64_t kMkSample = 4096;
// makeGraph cost model of one source for the balanced shard ranges (dmx_makegraph_balance): chunks of 64
// candidates weigh 0.7 of a depth step (profiles/r4_balance_config*.log)
constexpr double kMkSourceCost = 0.0, kMkChunkCost = 0.7;
// (the shortest occluder-free span, MK_SPAN_MIN = 4 depths, is a kernel constant: makegraph.hip)

// ---- VGA global, tile search (vga_tile.hip)
// Beamer's alpha: a level goes top-down when the frontier's runs are fewer than the unvisited cells / alpha.
// 60 with the frontier in LDS (r5_vga1000_knobs_ab.jsonl, r6 knobs.jsonl: 30 / 60 / 120 within 3 %), 1000 with
// the frontier in HBM (grids above ~1010^2: top-down levels there cost a global pass; r5 probe_vga2000)
constexpr int kVgaTileAlpha = 60;
constexpr int kVgaTileAlphaHbm = 1000;
// tile-common runs tested in phase A (all 4: the last two save ~20 % of the phase-B cell tests)
constexpr int kVgaTileCommonRuns = 4;
// consecutive sources a workgroup takes per grab (neighbouring sources share L2 lines and hit hints)
constexpr int kVgaSourceChunk = 1;
// phase B of a bottom-up level in stages ("phase B in stages"): bit 0 tests the tile-to-tile
// rows as a stage of its own, without the per-cell loads, and hands the tiles they leave to the cell stage; bit 1
// lists the cells that miss their first heads and hints and tests their other runs a cell a lane.  0 is the fused
// loop (a wave a tile through rows, cells and extension).  Hook: DMX_VGA_BSPLIT (0..3; A/B records, tests).
constexpr int kVgaTileBSplit = 3;
// phase C of a bottom-up level in stages ("phase C in stages"): bit 0 walks the regular cells of a
// hard-list chunk in a loop of their own (c1_chunk): no store in the loop, the chunk's hints written once at its end.
// 0 keeps every cell in the chunk's one loop with the special entries and writes each hint at its hit.  Both read a
// cell's rows with the same buffer loads (crow_load) and test them with the same code (pmask_hit_rows), so the switch
// checks the loop and the hint writes, not the row read; the other searches and the tests' restatement check that.
// (Bit 1 is kept for a mask stage, which is not built: the hook masks it off.)  Like DMX_VGA_BSPLIT a correctness
// switch for tests and bisecting: timings are taken against the parent build.  Hook: DMX_VGA_CSPLIT (0 / 1).
constexpr int kVgaTileCSplit = 1;
// phase C's miss certificate ("a miss certificate in front of the rows"): a chunk of hard cells
// loads the cells' block summaries (tvblk: the cell's view by 8 x 8 blocks of tiles, 4 words a cell) in one trip and
// drops the cells none of whose blocks holds a frontier tile: certain misses, found without their rows.  0 turns the
// test off and leaves the summaries in place.  A correctness switch for tests and bisecting: timings are
// taken against the parent build.  Hook: DMX_VGA_CCERT (0 / 1), read at launch.
constexpr int kVgaTileCCert = 1;
// the tile walks of a level (phase A, the level bookkeeping, X = F & ~V) take VGA_WALK_NF tiles a thread at once, all
// their loads in flight before the first is used, and a plain source builds its level 1 in place (DESIGN.md section 2,
// "tile walks").  0 selects the loops that take a tile at a time.  A correctness switch for tests and bisecting, not
// a tuning knob: timings are taken against the parent build.  Hook: DMX_VGA_WALK (0 / 1).
constexpr int kVgaTileWalk = 1;
// ---- VGA global, direction-optimising fallback (vga_do.hip)
constexpr int kVgaDoAlpha = 15;
constexpr int kVgaDoShortList = 16;

// ---- batched metric step depth (sdb_* kernels, stepdepth.hip)
// capacities of one batch: ambiguous cells (4 bytes each in `amb` and in `ahead`) and entries of their relaxer
// lists (8 bytes in `ent`, 4 in `enext`: 48 MiB).  A batch that outgrows either gives the search to the serial
// kernel.  Hooks: DMX_SDB_AMB_CAP, DMX_SDB_ENT_CAP (tests shrink them to the edge of a run; clamped to
// [1, default]).  (The relaxers of one ambiguous cell, SDB_FOLD_CAP = 2048, size a static LDS array: a kernel
// constant.)
constexpr int kSdbAmbCap = 1 << 16;
constexpr int kSdbEntCap = 1 << 22;

// ---- VGA through vision (thruvision.hip)
// side of the LDS window of 32-bit counters around the source (variant B; 0 would select variant A, global
// atomics only).  64^2 x 4 B = 16 KiB lets eight workgroups share a CU's LDS (profiles/thruvision_ab.jsonl)
constexpr int kTvWindow = 64;
// the largest window the DMX_TV_WINDOW hook accepts (128^2 counters; next to the kernel's static 3 KiB)
constexpr int kTvWindowMaxBytes = 64 * 1024;

// ---- VGA isovist (isovist.hip)
// per-lane list capacities of the first launch: the synthetic maps up to 128^2 need at most 14 gaps and 88 blocks
// (tests/isovist/isovist_check.cpp prints both); a lane's lists take gcap * 20 + bcap * 52 bytes of HBM.  Cells
// that need more are run again with kIsoRetryFactor times as much.  Hooks: DMX_ISO_GCAP, DMX_ISO_BCAP (tests
// shrink them to force the second launch).
constexpr int kIsoGapCap = 32;
constexpr int kIsoBlockCap = 128;
constexpr int kIsoRetryFactor = 16;
constexpr int kIsoCapMax = 1 << 16;   // the largest capacity a hook or the retry may ask for
// workgroups (of one wave) per CU the persistent kernel is launched with, if the occupancy query allows: 8 is
// what the kernel's 170 VGPRs admit (2 waves a SIMD).  1000^2, columns only: 33.1 ms with 2, 23.5 ms with 4,
// 15.6 ms with 8, 15.9 ms with 16 (capped at 8 by occupancy); syn128's 289 tiles show no difference
// (profiles/isovist_ab.jsonl).  Hook: DMX_ISO_WAVES.
constexpr int kIsoWavesPerCu = 8;
// pool entries (8 bytes) per node the first launch reserves for occlusion pixels; a pool found too small is
// enlarged to what the cursor counted and the launch repeated
constexpr int kIsoPoolPerNode = 48;
// isovists at arbitrary points (isovist_points_kernel, dmx_isovists).  Polygon pool: vertices (16 bytes) a point
// the first launch reserves; a point takes 2 nb + 2 of them (syn32's points hold 30 blocks on average and reserve
// 62, the 1000^2 benchmark map's cell centres 90 vertices and reserve 92), and a pool found too small is enlarged
// to what the cursor counted and the launch repeated.  Hook: DMX_ISO_VPOOL (tests shrink it to 1).
constexpr int kIsoVertexPoolPerPoint = 128;
// workgroups (of one wave) per CU, as kIsoWavesPerCu, capped by the occupancy query: the kernel's 166 VGPRs admit
// 12 (3 waves a SIMD).  998,001 points, columns only: 23.2 ms with 4, 15.7 ms with 8, 13.5 ms with 16 (that is 12)
// (profiles/isovist_points.jsonl).  Hook: DMX_ISO_PWAVES.
constexpr int kIsoPointsWavesPerCu = 16;
// launch order of the points: by Morton code of the point over the region (1), so that a wave's 64 lanes walk
// similar paths through the tree, or the caller's order (0).  Results do not depend on it.  998,001 points in a
// random order: 110 ms in the caller's order, 13.5 ms in Morton order; in tile order 13.5 and 13.7 ms
// (profiles/isovist_points.jsonl).  Hook: DMX_ISO_ORDER (caller | morton).
constexpr int kIsoPointsMorton = 1;

// ---- .graph chunk codec (chunk_codec.hip, api/chunk.hip)
// bytes of the record stream a slab holds: two slabs in device memory and two in pinned host memory, whatever the
// size of the chunk (18.5 GB at 1000^2).  A slab is a byte range, so a record larger than it spans several.  64 MiB
// keeps the pinned allocation short next to the copy it serves.  Hook: DMX_CODEC_SLAB (bytes; tests shrink it).
constexpr int64_t kCodecSlabBytes = 64ll << 20;

// ---- connections export (connections.hip, api/connections.hip, dmxcli -m EXPORT)
// LDS the two kernels hold beside the per-node bitmap (run tile, prefix, text staging: 15.3 KiB in the emitting
// kernel): the bitmap goes to per-workgroup HBM slices when bitmap + this exceeds kLdsPassBudget (grids above
// ~1040^2 cells).  Hook: DMX_CONN_GBM (any value) forces the slices (tests).
constexpr int kConnStaticLds = 16 * 1024;
// bytes of CSV text dmxcli asks for in one dmx_graph_connections_csv call (a device buffer and a host copy of that
// size, whatever the size of the export).  Hook: DMX_CONN_BUDGET (bytes; tests shrink it to a few KB, so that a small
// map takes many ranges).  A node whose lines exceed the budget goes alone.
constexpr int64_t kConnTextBudget = 256ll << 20;

// ---- memory: optional summaries are built only within a share of the free device memory, so a graph
// that fills the GPU still runs (on the slower exact path that needs no summary)
// tile rows (tvis / ftvis) and partial-tile masks on narrow grids: a quarter of the free memory
constexpr int kMemShareDiv = 4;
// tile rows on wide grids (above 1024^2), where the scan order's place is released for them: a third
constexpr int kMemShareWideDiv = 3;
// a per-workgroup LDS budget above which a preparation pass takes its HBM variant (of the 160 KiB a CU)
constexpr int kLdsPassBudget = 150 * 1024;

// ---- test hooks
inline const char* hook(const char* name) { return std::getenv(name); }
inline int hook_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}

}  // namespace policy
}  // namespace dmx
