"""Phase B of the tile-resolved VGA search in stages (kernels/vga_tile.hip, DESIGN.md section 2 "phase B in stages").

By default a bottom-up level tests the tile-to-tile rows as a stage of its own (B1: a batch of queue entries a
grab, no per-cell loads), hands the tiles the rows leave to the cell stage through a second queue (B2) and lists the
cells that miss their first heads and hints for the extension stage (B3: a cell a lane).  DMX_VGA_BSPLIT=0 selects
the fused loop (a wave a tile through all three).  Results do not depend on it.

Each case compares, over all sources and bit for bit on the levels and the 7 columns, the default run with the run
under DMX_VGA_BSPLIT=0 and with the direction-optimising search (DMX_VGA_KERNEL=do) on a fresh graph, and compares
the default run with the C restatement (oracle/dmx_oracle.c) at up to 64 seeded sources under the tolerances of
tests/test_gpu_vga_variants.py: node counts and level columns exact, floats within 1e-6 * max(1, |want|).  Radius n
and radius 3.  The dense map's restatement graph is built once and shared.

The shapes (the row stage's batch is VGA_BB1 = 4 entries, BATCH below):
   1  a map of 3 x 3 tiles (24^2 cells): queues shorter than one batch
   2  a strip, with a source whose second level queues a number of tiles that is 1 modulo the batch: a batch with
      a single entry (found among the first sources by one-source radius-2 runs, whose vga_b_tiles is that queue)
   3  a dense 129^2 map with occluders (289 tiles, the 256-thread member): every stage, asserted from the counters
   4  a room across the 64-tile word boundary on a 521^2 grid: the 1024-thread member
   5  a room on a 1137^2 grid: the frontier in HBM, wide rows
   6  the dense map without the tile-to-tile rows (DMX_VGA_TTVIS=0): the row stage is skipped
   7  the dense map without the masks (DMX_VGA_PMASK=0): no diagonal skip in the extension stage
   8  the dense map context-filled (SEMIFILL) at radius 3, run twice (small frontiers, top-down levels in between:
      the stage counters are reset with the level counters, whose reset once raced the next level's appends)
   9  visual step depth from seeded cells on the dense map: seed mode
  10  a re-read graph in asymmetric mode (DMX_VGA_ASYM=1), built as in tests/test_asym_mode.py
"""
import types

import numpy as np
import pytest

import depthmapx_amd as dmx
from depthmapx_amd import graphio
from golden.gen_synthetic import make_lines, make_room_map, make_strip_map
from golden_io import case_input_lines, load_case

pytestmark = pytest.mark.gpu

BATCH = 4   # VGA_BB1, kernels/vga_tile.hip
SWITCH_NAMES = ["DMX_VGA_BSPLIT", "DMX_VGA_KERNEL", "DMX_VGA_TVIS", "DMX_VGA_FTVIS", "DMX_VGA_TTVIS", "DMX_VGA_PMASK",
                "DMX_VGA_TVNZ", "DMX_VGA_NOHINT2", "DMX_VGA_RB", "DMX_VGA_CRK", "DMX_VGA_CHUNK", "DMX_VGA_ALPHA",
                "DMX_VGA_BEXT", "DMX_VGA_ASYM", "DMX_VGA_NOASYM", "DMX_VSD_TOPDOWN"]
DENSE = dict(W=128, n=120, seed=5, lmin=0.02, lmax=0.12)


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


def _sample(N):
    rng = np.random.default_rng(17)
    return np.unique(np.concatenate([rng.choice(N, min(N, 62), replace=False), [0, N - 1]]))


def _oracle(region, lines, sp, fill_type=0):
    from pyoracle import OracleMap
    om = OracleMap(region, 1.0, lines)
    assert om.fill(*sp, fill_type=fill_type)
    om.make_graph(threads=8)
    return om


def _three_way(ctx, mp, g, make_second, radius, om, src, runs=1):
    """The default run of graph g (`runs` times, all equal), the fused run and the second search on make_second()'s
    graph, all sources, bit for bit; the default run against the restatement at src.  Returns the default run's
    and the fused run's counters."""
    mp.delenv("DMX_VGA_BSPLIT", raising=False)
    got = g.vga_visual_global(radius=radius, levels=True)
    st = ctx.last_stats()
    assert st["vga_kernel"] == "tile-resolved", st
    for _ in range(runs - 1):
        _assert_same(got, g.vga_visual_global(radius=radius, levels=True))
    mp.setenv("DMX_VGA_BSPLIT", "0")
    fused = g.vga_visual_global(radius=radius, levels=True)
    st0 = ctx.last_stats()
    mp.delenv("DMX_VGA_BSPLIT")
    assert st0["vga_kernel"] == "tile-resolved", st0
    _assert_same(got, fused)
    mp.setenv("DMX_VGA_KERNEL", "do")
    g2 = make_second()
    second = g2.vga_visual_global(radius=radius, levels=True)
    # (on a re-read graph the second search runs top-down only and says so)
    assert ctx.last_stats()["vga_kernel"].startswith("direction-optimizing")
    g2.close()
    mp.delenv("DMX_VGA_KERNEL")
    _assert_same(got, second)
    want, _, rlv = om.vga_global_sample(src, radius=radius, threads=8, levels=True)
    np.testing.assert_array_equal(got[0][src, 5], want[src, 5])
    np.testing.assert_array_equal(got[1][src, :2], rlv[src, :2])
    _assert_close(got[0][src], want[src])
    return st, st0


def _map_case(ctx, mp, region, lines, sp, radius, env=(), fill_type=0, om=None, runs=1):
    """A map made from its drawing under the switches `env` (read at preparation), through _three_way."""
    _clean(mp)
    for k, v in env:
        mp.setenv(k, v)
    pm = dmx.PointMap(region, lines, 1.0)
    assert pm.make_points(*sp, fill_type=fill_type)
    g = pm.make_graph(ctx)
    N = g.info()["nnodes"]
    om = om or _oracle(region, lines, sp, fill_type)
    assert om.num_nodes == N
    try:
        return _three_way(ctx, mp, g, lambda: pm.make_graph(ctx), radius, om, _sample(N), runs) + (pm, N)
    finally:
        g.close()


@pytest.fixture(scope="module")
def dense():
    """The dense map's drawing and its restatement graph (built once; the searches do not change it)."""
    W = DENSE["W"]
    region = [0.0, 0.0, float(W), float(W)]
    lines = np.array(make_lines(W, DENSE["n"], seed=DENSE["seed"], lmin=DENSE["lmin"], lmax=DENSE["lmax"]),
                     dtype=np.float64)
    sp = (0.5, 0.5)
    return types.SimpleNamespace(region=region, lines=lines, sp=sp, om=_oracle(region, lines, sp))


@pytest.mark.parametrize("radius", [-1, 3])
def test_queue_shorter_than_a_batch(ctx, monkeypatch, radius):
    """Shape 1: 24^2 cells are 9 tiles; a level's queue holds a few of them."""
    W = 23
    lines = np.array(make_lines(W, 12, seed=3, lmin=0.1, lmax=0.4), dtype=np.float64)
    st, _, pm, N = _map_case(ctx, monkeypatch, [0.0, 0.0, float(W), float(W)], lines, (0.5, 0.5), radius)
    assert (pm.cols, pm.rows) == (24, 24) and N > 300
    assert st["vga_threads"] == 256 and st["vga_bottom_up_levels"] > 0 and st["vga_b_tiles"] > 0, st
    assert st["vga_b_tiles"] < 9 * st["vga_bottom_up_levels"], st


@pytest.mark.parametrize("radius", [-1, 3])
def test_batch_with_a_single_entry(ctx, monkeypatch, radius):
    """Shape 2: a strip 65 tiles long, many levels deep; some source's second level queues 1 modulo BATCH tiles."""
    region, lines, sp = make_strip_map(519, 16, 6, 10, 1)
    st, _, pm, N = _map_case(ctx, monkeypatch, region, lines, sp, radius)
    assert st["vga_bottom_up_levels"] > 0 and st["vga_b_tiles"] > 0, st
    if radius != -1:
        return
    assert st["vga_bottom_up_levels"] > N, st   # more than one bottom-up level a source: a deep map
    g = pm.make_graph(ctx)
    found = None
    for s in range(0, min(N, 96)):
        g.vga_visual_global(radius=2, src_begin=s, src_end=s + 1)
        one = ctx.last_stats()
        if one["vga_kernel"] == "tile-resolved" and one["vga_bottom_up_levels"] == 1 and one["vga_b_tiles"] % BATCH == 1:
            found = (s, one["vga_b_tiles"])
            break
    g.close()
    assert found, "no source among the first 96 queues 1 modulo %d tiles at its second level" % BATCH


@pytest.mark.parametrize("radius", [-1, 3])
def test_dense_map_every_stage(ctx, monkeypatch, dense, radius):
    """Shape 3: the rows resolve tiles and leave tiles to the cell stage, cells reach the extension stage and the
    hard list."""
    st, st0, pm, N = _map_case(ctx, monkeypatch, dense.region, dense.lines, dense.sp, radius, om=dense.om)
    assert (pm.cols, pm.rows) == (129, 129) and N > 8000
    assert st["vga_threads"] == 256 and st["vga_frontier_hbm"] == 0, st
    assert "ttvis" in st["vga_prep"] and "masks" in st["vga_prep"], st
    for k in ("vga_tt_tiles", "vga_b_cell_tiles", "vga_b_ext_cells", "vga_hard_cells"):
        assert st[k] > 0, (k, st)
    assert st["vga_b_cell_tiles"] < st["vga_b_tiles"], st


@pytest.mark.parametrize("radius", [-1, 3])
def test_1024_thread_member(ctx, monkeypatch, radius):
    """Shape 4: 4,356 tiles, the room across tile column 63|64."""
    region, lines, sp = make_room_map(520.0, 48.0, 30, 5, centre=(494.0, 256.0))
    st, _, pm, N = _map_case(ctx, monkeypatch, region, lines, sp, radius)
    assert st["vga_threads"] == 1024 and st["vga_frontier_hbm"] == 0, st
    assert st["vga_tt_tiles"] > 0 and st["vga_b_cell_tiles"] > 0, st


@pytest.mark.parametrize("radius", [-1, 3])
def test_hbm_frontier_member(ctx, monkeypatch, radius):
    """Shape 5: 20,449 tiles: the frontier in HBM, wide rows (the row stage's loop over the row words)."""
    region, lines, sp = make_room_map(1136.0, 64.0, 60, 9, centre=(512.0, 1024.0))
    st, _, pm, N = _map_case(ctx, monkeypatch, region, lines, sp, radius)
    assert st["vga_threads"] == 1024 and st["vga_frontier_hbm"] == 1, st
    assert "ttvis" in st["vga_prep"] and st["vga_b_tiles"] > 0, st


@pytest.mark.parametrize("radius", [-1, 3])
def test_row_stage_skipped_without_rows(ctx, monkeypatch, dense, radius):
    """Shape 6: no tile-to-tile rows: the cell stage reads phase A's queue."""
    st, _, pm, N = _map_case(ctx, monkeypatch, dense.region, dense.lines, dense.sp, radius,
                             env=[("DMX_VGA_TTVIS", "0")], om=dense.om)
    assert "ttvis" not in st["vga_prep"], st
    assert st["vga_tt_tiles"] == 0 and st["vga_b_cell_tiles"] == st["vga_b_tiles"] > 0, st
    assert st["vga_b_ext_cells"] > 0, st


@pytest.mark.parametrize("radius", [-1, 3])
def test_extension_without_masks(ctx, monkeypatch, dense, radius):
    """Shape 7: no masks: the extension stage tests diagonal runs too, phase C scans the runs."""
    st, _, pm, N = _map_case(ctx, monkeypatch, dense.region, dense.lines, dense.sp, radius,
                             env=[("DMX_VGA_PMASK", "0")], om=dense.om)
    assert "masks" not in st["vga_prep"] and st["vga_pmask_cells"] == 0, st
    assert st["vga_b_ext_cells"] > 0, st


def test_contextfilled_map_radius_3_twice(ctx, monkeypatch, dense):
    """Shape 8: a SEMIFILL map at radius 3: odd cells are no sources and are not expanded, the frontiers are small
    and top-down levels come between the bottom-up ones; two runs give the same bits."""
    st, _, pm, N = _map_case(ctx, monkeypatch, dense.region, dense.lines, dense.sp, 3,
                             fill_type=dmx.PointMap.SEMIFILL, runs=2)
    assert st["vga_bottom_up_levels"] > 0 and st["vga_top_down_levels"] > 0, st
    assert st["vga_b_tiles"] > 0, st


def test_seed_mode_step_depth(ctx, monkeypatch, dense):
    """Shape 9: visual step depth from 1 and from 5 seeded cells: the same kernel in seed mode, one workgroup;
    staged, fused and the top-down search give the restatement's bits."""
    _clean(monkeypatch)
    pm = dmx.PointMap(dense.region, dense.lines, 1.0)
    assert pm.make_points(*dense.sp)
    g = pm.make_graph(ctx)
    filled = np.nonzero(pm.state() & 2)[0]
    rng = np.random.default_rng(1)
    for nsel in (1, 5):
        cells = np.sort(rng.choice(filled, nsel, replace=False))
        got = g.visual_step_depth(cells=cells)
        st = ctx.last_stats()
        assert (st["vga_sources"], st["vga_launch"]) == (1, 1) and st["vga_bottom_up_levels"] > 0, st
        monkeypatch.setenv("DMX_VGA_BSPLIT", "0")
        fused = g.visual_step_depth(cells=cells)
        monkeypatch.delenv("DMX_VGA_BSPLIT")
        monkeypatch.setenv("DMX_VSD_TOPDOWN", "1")
        topdown = g.visual_step_depth(cells=cells)
        monkeypatch.delenv("DMX_VSD_TOPDOWN")
        want = dense.om.visual_stepdepth(cells)
        np.testing.assert_array_equal(got.view(np.uint32), fused.view(np.uint32))
        np.testing.assert_array_equal(got.view(np.uint32), topdown.view(np.uint32))
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        assert got.max() >= 2
    g.close()


@pytest.mark.parametrize("radius", [-1, 3])
def test_asymmetric_mode(ctx, monkeypatch, radius):
    """Shape 10: syn128 written as a .graph chunk and read again (runs moved by the 4-bit row shifts), searched in
    asymmetric mode; the restatement walks the decoded runs."""
    from pyoracle import OracleMap
    _clean(monkeypatch)
    meta, _ = load_case("syn128")
    lines = case_input_lines(meta)
    pm = dmx.PointMap(meta["region"], lines, meta["spacing"])
    for f in meta["fills"]:
        assert pm.make_points(*f)
    g0 = pm.make_graph(ctx)
    c = g0.copy(runs=True)
    cols = [(n, c["attrs"][:, i], False)
            for i, n in enumerate(["Connectivity", "Point First Moment", "Point Second Moment"])]
    blob = graphio.write_chunk(pm, c["bins"], c["runs"], c["gridconn"], cols)
    info = graphio.read_chunk(blob)
    assert len(info["runs"]) == len(c["runs"]) and np.any(info["runs"] != c["runs"])
    om = OracleMap.from_grid(info["cols"], info["rows"], info["spacing"], info["bottom_left"], info["state"])
    om.set_graph(info["bins"], info["runs"])
    monkeypatch.setenv("DMX_VGA_ASYM", "1")
    loaded = []

    def load():
        pm2, g2 = graphio.load_chunk(ctx, blob, meta["region"], lines=lines)
        loaded.append(pm2)
        return g2
    g = load()
    N = g.info()["nnodes"]
    st, _ = _three_way(ctx, monkeypatch, g, load, radius, om, _sample(N))
    assert st["vga_asym_mode"] == 1 and st["vga_asym_nodes"] > 0 and st["vga_b_tiles"] > 0, st
    g.close()
    g0.close()
