"""Every variant of the tile-resolved VGA search (kernels/vga_tile.hip) at the thresholds where the host picks it.

vga_tile_kernel is a family: 256 or 1024 threads (above 4,096 tiles), the frontier bitmap in the LDS or in HBM,
line summaries or per-tile summaries (tile_lds_layout, api/vga_global.hip), and, as branches on what
prepare_tiles built, narrow rows (tvw <= 256 words) or wide ones, with or without the fully-seen rows, the
tile-to-tile rows, the partial-tile masks and the row summaries -- or no rows at all above 32 GB of them.  Each
case below is the smallest grid on which the host rules give one member; the test asserts which member ran
(Context.last_stats: vga_threads, vga_frontier_hbm, vga_line_summaries, vga_prep) and compares it

  * bit for bit (levels and all 7 columns) with the direction-optimising search (DMX_VGA_KERNEL=do) on a fresh
    graph, which shares none of the tile search's certificates, and
  * with the C restatement (oracle/dmx_oracle.c) over the same drawing at 256 seeded sources plus the first and
    the last node: node counts and level sums exact, floats within 1e-6 * max(1, |want|).

The large grids hold one walled room (make_room_map), placed across a 64-tile word boundary of the tile rows
where the region allows it, so the kernel sees the whole grid while the restatement pays for the room; the strips
(make_strip_map) are 65 tiles long (two words) or 257 tiles high (wide rows) and many levels deep.  Two more
groups: eight small dense maps whose cols % 8 and rows % 8 take every residue (partial tiles at the edges), and
the preparation switches (the fallbacks the host takes by itself when memory is short), each bit-identical to the
same map's default run and each asserted to have switched.

Measured on an MI355X (profiles/vga_variants_durations.txt): the module's 73 tests take 9.7 s, the slowest 1.9 s
(C, radius n: 14,378 sources, tile search 0.74 s, second search 1.12 s).  On F and G the second search runs all 3,959
sources in 0.014 s and 0.028 s (64 of them: 4-5 ms), so it is not cut to a block; G's first call, preparation over
its 4.2 M cells included, takes 0.016 s (kernel 0.013 s), and the restatement's 258 sources 0.68 s there.
"""
import time
import types

import numpy as np
import pytest

import depthmapx_amd as dmx
from golden.gen_synthetic import make_lines, make_lines_rect, make_room_map, make_strip_map

pytestmark = pytest.mark.gpu

# vga_prep with every certificate built.  Narrow rows have no row summaries: their tvnz is compiled out (VGA_TVNZ 0
# in kernels/vga_tile.hip; DESIGN.md, "What the row words hold": it made the kernel slower), so on narrow grids
# prepare_tiles builds none and DMX_VGA_TVNZ switches nothing.
ALL = "scan+tvis+ftvis+ttvis+masks"
ALL_WIDE = "scan+tvis+ftvis+ttvis+masks+tvsum"
# every environment switch the search or its preparation reads: the default runs are made without them
SWITCH_NAMES = ["DMX_VGA_KERNEL", "DMX_VGA_TVIS", "DMX_VGA_FTVIS", "DMX_VGA_TTVIS", "DMX_VGA_PMASK", "DMX_VGA_TVNZ",
                "DMX_VGA_NOHINT2", "DMX_VGA_RB", "DMX_VGA_CRK", "DMX_VGA_CHUNK", "DMX_VGA_ALPHA", "DMX_VGA_BEXT",
                "DMX_VGA_ASYM", "DMX_VGA_NOASYM", "DMX_VSD_TOPDOWN"]

# The variant the host rules give (tile_lds_layout, prepare_tiles; LDS 159 KiB, rows of tvw = th * ceil(tw / 64)
# words):
#   A, B  65 tiles along one side: the tile-row (A) / tile-column (B) words go from 1 to 2
#   C     tvw = 257: wide rows on a grid whose frontier fits the LDS keep tvis and its summaries alone
#   D     4,356 tiles: 1024 threads; the room lies across tile column 63|64
#   E     19,044 tiles: the frontier (152,352 B) still fits the LDS, the line summaries (58 KB) no longer do
#   F     20,449 tiles: the frontier moves to HBM, the line summaries fit again; the wide-row certificates are
#         all built.  (The masks take the released scan order's place only when they do not fit next to it and
#         16 GiB: those of a 64-cell room always fit wherever the 9 GB of rows did, so the scan order stays.)
#   G     66,564 tiles: 44 GB of rows (> 32 GB) are not built; line summaries (175 KB) do not fit
# deep: a strip, more than 3 levels from some source.
CASES = {
    "A": dict(make=lambda: make_strip_map(519, 16, 6, 10, 1), threads=256, hbm=0, lines=1, wide=False, prep=ALL,
              deep=True),
    "B": dict(make=lambda: make_strip_map(16, 519, 6, 10, 2), threads=256, hbm=0, lines=1, wide=False, prep=ALL,
              deep=True),
    "C": dict(make=lambda: make_strip_map(8, 2055, 24, 10, 3), threads=256, hbm=0, lines=1, wide=True,
              prep="scan+tvis+tvsum", deep=True),
    # (a room of 48 around x = 512 would end at 536, outside the region of 520: its centre is moved to 494, so that
    # it still spans tile columns 58..64 across the word boundary at cell x = 512)
    "D": dict(make=lambda: make_room_map(520.0, 48.0, 30, 5, centre=(494.0, 256.0)), threads=1024, hbm=0, lines=1,
              wide=False, prep=ALL, deep=False),
    "E": dict(make=lambda: make_room_map(1100.0, 64.0, 60, 9, centre=(512.0, 1024.0)), threads=1024, hbm=0, lines=0,
              wide=True, prep="scan+tvis+tvsum", deep=False),
    "F": dict(make=lambda: make_room_map(1136.0, 64.0, 60, 9, centre=(512.0, 1024.0)), threads=1024, hbm=1, lines=1,
              wide=True, prep=ALL_WIDE, deep=False),
    "G": dict(make=lambda: make_room_map(2056.0, 64.0, 60, 9), threads=1024, hbm=1, lines=0, wide=True,
              prep="scan", deep=False),
}


def _clean(mp):
    for k in SWITCH_NAMES:
        mp.delenv(k, raising=False)


def _assert_close(got, want):
    want = want.astype(np.float64)
    got = got.astype(np.float64)
    bad = np.abs(got - want) > 1e-6 * np.maximum(1.0, np.abs(want))
    assert not bad.any(), "VGA mismatch at %d entries, first %s" % (bad.sum(), np.argwhere(bad)[:5].tolist())


def _assert_same(a, b):
    (out_a, lv_a), (out_b, lv_b) = a, b
    np.testing.assert_array_equal(lv_a, lv_b)
    np.testing.assert_array_equal(out_a.view(np.uint32), out_b.view(np.uint32))


def _assert_variant(st, pm, threads, hbm, lines, wide, prep):
    assert st["vga_kernel"] == "tile-resolved", st
    tw, th = (pm.cols + 7) // 8, (pm.rows + 7) // 8
    assert (th * ((tw + 63) // 64) > 256) == wide
    got = (st["vga_threads"], st["vga_frontier_hbm"], st["vga_line_summaries"], st["vga_prep"])
    assert got == (threads, hbm, lines, prep), st


@pytest.fixture(scope="module", params=list(CASES))
def case(request, ctx):
    from pyoracle import OracleMap
    spec = CASES[request.param]
    region, lines, sp = spec["make"]()
    pm = dmx.PointMap(region, lines, 1.0)
    assert pm.make_points(*sp)
    g = pm.make_graph(ctx)
    om = OracleMap(region, 1.0, lines)
    assert om.fill(*sp)
    om.make_graph(threads=8)
    N = g.info()["nnodes"]
    rng = np.random.default_rng(17)
    src = np.unique(np.concatenate([rng.choice(N, 256, replace=False), [0, N - 1]]))
    yield types.SimpleNamespace(name=request.param, spec=spec, pm=pm, g=g, om=om, N=N, src=src)
    g.close()
    pm.close()


def test_makegraph_matches_oracle(case):
    """bins and runs of the case's graph equal the restatement's (C, E and G are new shapes for makeGraph too)."""
    got, ref = case.g.copy(runs=True), case.om.graph()
    assert case.N == case.om.num_nodes > 2000
    np.testing.assert_array_equal(got["bins"], ref["bins"])
    np.testing.assert_array_equal(got["runs"], ref["runs"])


@pytest.mark.parametrize("radius", [-1, 3])
def test_variant_matches_second_search_and_oracle(case, ctx, monkeypatch, radius):
    """The default search over all sources: the variant of the table, bit-identical to the direction-optimising
    search over all sources (E-G too: its bitmaps are in HBM there; F 0.014 s, G 0.028 s) and equal to the
    restatement at the sample."""
    _clean(monkeypatch)
    spec, N, s = case.spec, case.N, case.src
    t0 = time.perf_counter()
    got, lv = case.g.vga_visual_global(radius=radius, levels=True)   # (radius -1 runs first: with the preparation)
    t1 = time.perf_counter()
    st, st_kernel = ctx.last_stats(), ctx.last_timing()[1]
    _assert_variant(st, case.pm, spec["threads"], spec["hbm"], spec["lines"], spec["wide"], spec["prep"])
    assert st["vga_sources"] == N and st["vga_bottom_up_levels"] > 0, st
    if "masks" in spec["prep"]:
        assert st["vga_pmask_cells"] > 0, st

    monkeypatch.setenv("DMX_VGA_KERNEL", "do")
    g2 = case.pm.make_graph(ctx)
    t2 = time.perf_counter()
    second = g2.vga_visual_global(radius=radius, levels=True)
    t3 = time.perf_counter()
    assert ctx.last_stats()["vga_kernel"] == "direction-optimizing"
    g2.close()
    _assert_same((got, lv), second)

    want, _, rlv = case.om.vga_global_sample(s, radius=radius, threads=8, levels=True)
    print("case %s radius %d: tile search of %d sources %.3f s (kernel %.3f s), second search of %d sources %.3f s, "
          "restatement of %d sources %.3f s" % (case.name, radius, N, t1 - t0, st_kernel, N, t3 - t2, len(s),
                                                time.perf_counter() - t3))
    np.testing.assert_array_equal(got[s, 5], want[s, 5])
    np.testing.assert_array_equal(lv[s, :2], rlv[s, :2])
    _assert_close(got[s], want[s])
    if radius == -1:
        assert (want[s, 5] == N).all()   # connected: every search crosses the whole map
        if spec["deep"]:
            assert rlv[s, 2].max() > 3


def test_visual_stepdepth_matches_oracle(case, ctx, monkeypatch):
    """Visual step depth from 1 and from 5 seeded cells: up to 16,384 tiles (A-D) the same kernel instantiation in
    seed mode, one workgroup; above (E-G) the level-synchronous top-down search."""
    _clean(monkeypatch)
    filled = np.nonzero(case.pm.state() & 2)[0]
    rng = np.random.default_rng(1)
    nt = ((case.pm.cols + 7) // 8) * ((case.pm.rows + 7) // 8)
    for nsel in (1, 5):
        cells = np.sort(rng.choice(filled, nsel, replace=False))
        got = case.g.visual_step_depth(cells=cells)
        if nt <= 16384:
            st = ctx.last_stats()
            assert (st["vga_sources"], st["vga_launch"], st["vga_threads"]) == (1, 1, case.spec["threads"]), st
            assert (st["vga_frontier_hbm"], st["vga_line_summaries"]) == (case.spec["hbm"], case.spec["lines"]), st
        want = case.om.visual_stepdepth(cells)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        assert got.min() >= 0 and got.max() >= 2


# ---- partial tiles: cols % 8 and rows % 8 take each of 0..7 once
def _residue_dims(i):
    a, b = 40 + i, 24 + (i + 4) % 8
    return (a, b) if i % 2 == 0 else (b, a)


assert sorted(_residue_dims(i)[0] % 8 for i in range(8)) == list(range(8))
assert sorted(_residue_dims(i)[1] % 8 for i in range(8)) == list(range(8))


@pytest.mark.parametrize("i", range(8))
def test_partial_tile_residues(ctx, monkeypatch, i):
    """Dense short occluders on a grid of (40 + i) x (24 + (i + 4) % 8) cells, transposed for odd i: all sources
    bit-equal to the direction-optimising search and equal to the whole restatement run."""
    from pyoracle import OracleMap
    _clean(monkeypatch)
    cols, rows = _residue_dims(i)
    region = [0.0, 0.0, cols - 1.0, rows - 1.0]
    lines = np.array(make_lines_rect(cols - 1, rows - 1, 30, seed=20 + i, lmin=0.05, lmax=0.3), dtype=np.float64)
    pm = dmx.PointMap(region, lines, 1.0)
    assert pm.make_points(0.5, 0.5)
    assert (pm.cols, pm.rows) == (cols, rows)
    g = pm.make_graph(ctx)
    N = g.info()["nnodes"]
    assert N > 600
    got = g.vga_visual_global(levels=True)
    _assert_variant(ctx.last_stats(), pm, 256, 0, 1, False, ALL)
    monkeypatch.setenv("DMX_VGA_KERNEL", "do")
    g2 = pm.make_graph(ctx)
    _assert_same(got, g2.vga_visual_global(levels=True))
    om = OracleMap(region, 1.0, lines)
    assert om.fill(0.5, 0.5)
    om.make_graph(threads=8)
    want, rlv = om.vga_global(threads=8, levels=True)
    np.testing.assert_array_equal(got[1][:, :2], rlv[:, :2])
    np.testing.assert_array_equal(got[0][:, 5], want[:, 5])
    _assert_close(got[0], want)


# ---- the preparation switches: (variable, value, expected vga_prep on the narrow maps, on case F; None: a switch
# of the narrow rows, not run on F).  The narrow maps are make_lines(96, 200, seed, 0.02, 0.3) filled from
# (0.5, 0.5).  Seed 3 fills a pocket of 80 cells that all see each other (one level a search): it checks that a
# switch changes the preparation and not the result, and nothing about the search's phases.  Seed 7 fills 1,097
# cells, up to 8 levels deep: there the phases' counters and the direction of the levels are asserted as on F.
SHALLOW = ("narrow3",)
NARROW = dict(threads=256, hbm=0, lines=1, wide=False, prep=ALL)
SWITCHES = [
    ("DMX_VGA_TVIS", "0", "scan", "scan"),
    ("DMX_VGA_FTVIS", "0", "scan+tvis", "scan+tvis+tvsum"),
    ("DMX_VGA_TTVIS", "0", "scan+tvis+ftvis+masks", "scan+tvis+ftvis+masks+tvsum"),
    ("DMX_VGA_PMASK", "0", "scan+tvis+ftvis+ttvis", "scan+tvis+ftvis+ttvis+tvsum"),
    ("DMX_VGA_TVNZ", "0", ALL, None),   # (compiled out: nothing to switch, the default preparation)
    ("DMX_VGA_NOHINT2", "1", ALL, None),
    ("DMX_VGA_RB", "0", ALL, ALL_WIDE),
    ("DMX_VGA_CRK", "0", ALL, ALL_WIDE),
    ("DMX_VGA_CHUNK", "1", ALL, ALL_WIDE),
    ("DMX_VGA_CHUNK", "7", ALL, ALL_WIDE),
    ("DMX_VGA_ALPHA", "1", ALL, ALL_WIDE),
    ("DMX_VGA_ALPHA", "1000000", ALL, ALL_WIDE),
]


@pytest.fixture(scope="module")
def base(request, ctx):
    """The map and its default run (all sources, levels)."""
    if request.param.startswith("narrow"):
        W = 96
        region = [0.0, 0.0, float(W), float(W)]
        lines = np.array(make_lines(W, 200, seed=int(request.param[6:]), lmin=0.02, lmax=0.3), dtype=np.float64)
        sp, spec = (0.5, 0.5), NARROW
    else:
        region, lines, sp = CASES["F"]["make"]()
        spec = {k: CASES["F"][k] for k in NARROW}
    pm = dmx.PointMap(region, lines, 1.0)
    assert pm.make_points(*sp)
    with pytest.MonkeyPatch.context() as mp:
        _clean(mp)
        g = pm.make_graph(ctx)
        run = g.vga_visual_global(levels=True)
        st = ctx.last_stats()
        g.close()
    yield types.SimpleNamespace(name=request.param, region=region, lines=lines, sp=sp, pm=pm, run=run, st=st, spec=spec)
    pm.close()


@pytest.mark.parametrize("base", ["narrow3", "narrow7", "F"], indirect=True)
def test_switch_baseline(base, ctx):
    """The default runs the switches are compared with: their variant, and the narrow maps' against the whole
    restatement run (case F's is test_variant_matches_second_search_and_oracle[F])."""
    from pyoracle import OracleMap
    _assert_variant(base.st, base.pm, **base.spec)
    if base.name not in SHALLOW:
        assert base.st["vga_cr_tiles"] > 0 and base.st["vga_pmask_cells"] > 0, base.st
        assert base.st["vga_top_down_levels"] > 0 and base.st["vga_bottom_up_levels"] > 0, base.st
    if base.name == "F":
        return
    om = OracleMap(base.region, 1.0, base.lines)
    assert om.fill(*base.sp)
    om.make_graph(threads=8)
    want, rlv = om.vga_global(threads=8, levels=True)
    np.testing.assert_array_equal(base.run[1][:, :2], rlv[:, :2])
    np.testing.assert_array_equal(base.run[0][:, 5], want[:, 5])
    _assert_close(base.run[0], want)


SWITCH_RUNS = [(m, var, value, prep) for k, m in ((2, "narrow3"), (2, "narrow7"), (3, "F")) for (var, value, prep) in
               ((s[0], s[1], s[k]) for s in SWITCHES) if prep is not None]


@pytest.mark.parametrize("base,var,value,prep", SWITCH_RUNS, indirect=["base"],
                         ids=["%s-%s=%s" % r[:3] for r in SWITCH_RUNS])
def test_preparation_switch(base, ctx, monkeypatch, var, value, prep):
    """One switch, a fresh graph (the switches are read at preparation): bit-identical to the default run, and the
    switch took effect (the preparation built, the summaries, the tile-common runs, the direction of the levels)."""
    _clean(monkeypatch)
    monkeypatch.setenv(var, value)
    g = base.pm.make_graph(ctx)
    run = g.vga_visual_global(levels=True)
    st = ctx.last_stats()
    g.close()
    spec = dict(base.spec, prep=prep)
    if var == "DMX_VGA_RB":
        spec["lines"] = 0
    _assert_variant(st, base.pm, **spec)
    _assert_same(run, base.run)
    N = run[0].shape[0]
    levels = base.st["vga_top_down_levels"] + base.st["vga_bottom_up_levels"]
    assert st["vga_sources"] == N and st["vga_top_down_levels"] + st["vga_bottom_up_levels"] == levels, st
    if "masks" not in prep:
        assert st["vga_pmask_cells"] == 0, st
    if var == "DMX_VGA_CRK":
        assert st["vga_cr_tiles"] == 0, st
    if base.name in SHALLOW:
        return
    if var == "DMX_VGA_ALPHA" and value == "1000000":
        # m_f * alpha > m_u at every level past the first: one top-down level (the source's own runs) a search
        assert st["vga_top_down_levels"] <= N < st["vga_bottom_up_levels"], st
    if var == "DMX_VGA_ALPHA" and value == "1":
        # bottom-up only where the frontier outnumbers the unvisited cells: more top-down levels than by default
        assert st["vga_top_down_levels"] > base.st["vga_top_down_levels"] > 0, st
        assert st["vga_bottom_up_levels"] < base.st["vga_bottom_up_levels"], st
