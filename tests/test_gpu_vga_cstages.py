"""Phase C of the tile-resolved VGA search with its row stage (kernels/vga_tile.hip c1_chunk, DESIGN.md section 2
"phase C in stages").

By default a wave walks the regular entries of a hard-list chunk in a loop of their own: a cell's tile-visibility rows
are range-checked buffer loads issued back to back, the cell is reduced at once to a certain hit, a certain miss or the
mask loop, and the chunk's hints are written once, a hit cell a lane.  Special (asymmetric) entries, grids whose
frontier lives in HBM and the build without masks keep the loop that loads and tests a cell at a time, which
DMX_VGA_CSPLIT=0 selects for every cell.  Results do not depend on it.  (The mask stage of the design, bit 1 of the
switch, is not built: the hook masks the bit off, so DMX_VGA_CSPLIT=2 is the loop of 0.)  The loop of 0 reads a cell's
rows with the same buffer loads and tests them with the same code as the row stage; it differs in the loop and in where
the hints are written.  The independent checks of the row read are the direction-optimising search and the restatement.

Each case compares, over all sources and bit for bit on the levels and the 7 columns, the default run with the run
under DMX_VGA_CSPLIT=0 and with the direction-optimising search (DMX_VGA_KERNEL=do) on a fresh graph, and compares
the default run with the C restatement (oracle/dmx_oracle.c) at up to 64 seeded sources under the tolerances of
tests/test_gpu_vga_bstages.py: node counts and level columns exact, floats within 1e-6 * max(1, |want|).  Each case
asserts from the counters that the stage ran (vga_c_row_cells, the hard cells that went through it) or was absent.

The shapes (a wave takes VGA_CCH = 16 list entries a grab, CHUNK below; the stage has one cell's rows in flight, so
there are no groups of cells whose last could hold a single one):
   1  a map of 3 x 3 tiles (24^2 cells), with a source whose only bottom-up level lists fewer hard cells than a chunk
   2  the dense map, a source whose only bottom-up level lists 1 modulo CHUNK hard cells: a chunk with a single entry
      (found among the first sources by one-source radius-2 runs, whose vga_hard_cells is that list)
   3  a dense 129^2 map with occluders: certain hits, certain misses, undecided cells and mask hits, asserted from
      the counters; the same under DMX_VGA_CSPLIT=1 (the default) and =2 (mapped to 0)
   5  a room across the 64-tile word boundary on a 521^2 grid: the 1024-thread member, two row words a tile row
   6  the stage absent, counters zero, results equal: a 1137^2 room (frontier in HBM, wide rows) and the dense map
      without the masks (DMX_VGA_PMASK=0)
   7  the dense map context-filled (SEMIFILL) at radius 3, run twice
   8  visual step depth from seeded cells on the dense map: seed mode
   9  a re-read graph in asymmetric mode, and a map with asymmetric (special) nodes: special hard-list entries take
      the unchanged path next to staged regular ones
(Shape 4 of the design, the capacity of the mask stage's item list, has nothing to test without that stage.)
"""
import os
import types

import numpy as np
import pytest

import depthmapx_amd as dmx
from depthmapx_amd import graphio
from golden.gen_synthetic import make_lines, make_room_map
from golden_io import GOLDEN, case_input_lines, load_case

pytestmark = pytest.mark.gpu

CHUNK = 16   # VGA_CCH, kernels/vga_tile.hip
SWITCH_NAMES = ["DMX_VGA_CSPLIT", "DMX_VGA_BSPLIT", "DMX_VGA_WALK", "DMX_VGA_KERNEL", "DMX_VGA_TVIS", "DMX_VGA_FTVIS",
                "DMX_VGA_TTVIS", "DMX_VGA_PMASK", "DMX_VGA_TVNZ", "DMX_VGA_NOHINT2", "DMX_VGA_RB", "DMX_VGA_CRK",
                "DMX_VGA_CHUNK", "DMX_VGA_ALPHA", "DMX_VGA_BEXT", "DMX_VGA_ASYM", "DMX_VGA_NOASYM", "DMX_VSD_TOPDOWN"]
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


def _three_way(ctx, mp, g, make_second, radius, om, src, runs=1, split="0"):
    """The default run of graph g (`runs` times, all equal), the run under DMX_VGA_CSPLIT=`split` and the second search
    on make_second()'s graph, all sources, bit for bit; the default run against the restatement at src.  Returns
    the default run's and the switched run's counters."""
    mp.delenv("DMX_VGA_CSPLIT", raising=False)
    got = g.vga_visual_global(radius=radius, levels=True)
    st = ctx.last_stats()
    assert st["vga_kernel"] == "tile-resolved", st
    for _ in range(runs - 1):
        _assert_same(got, g.vga_visual_global(radius=radius, levels=True))
    mp.setenv("DMX_VGA_CSPLIT", split)
    plain = g.vga_visual_global(radius=radius, levels=True)
    st0 = ctx.last_stats()
    mp.delenv("DMX_VGA_CSPLIT")
    assert st0["vga_kernel"] == "tile-resolved", st0
    _assert_same(got, plain)
    mp.setenv("DMX_VGA_KERNEL", "do")
    g2 = make_second()
    second = g2.vga_visual_global(radius=radius, levels=True)
    assert ctx.last_stats()["vga_kernel"].startswith("direction-optimizing")
    g2.close()
    mp.delenv("DMX_VGA_KERNEL")
    _assert_same(got, second)
    want, _, rlv = om.vga_global_sample(src, radius=radius, threads=8, levels=True)
    np.testing.assert_array_equal(got[0][src, 5], want[src, 5])
    np.testing.assert_array_equal(got[1][src, :2], rlv[src, :2])
    _assert_close(got[0][src], want[src])
    return st, st0


def _map_case(ctx, mp, region, lines, sp, radius, env=(), fill_type=0, om=None, runs=1, split="0"):
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
        return _three_way(ctx, mp, g, lambda: pm.make_graph(ctx), radius, om, _sample(N), runs, split) + (pm, N)
    finally:
        g.close()


def _staged(st):
    """The row stage took every regular hard cell of the run (special entries are counted apart)."""
    return st["vga_c_row_cells"] > 0 and st["vga_c_row_cells"] == st["vga_pmask_cells"] == st["vga_hard_cells"]


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
def test_hard_list_shorter_than_a_chunk(ctx, monkeypatch, radius):
    """Shape 1: 24^2 cells are 9 tiles; some source's second level lists fewer hard cells than a chunk."""
    W = 23
    lines = np.array(make_lines(W, 12, seed=3, lmin=0.1, lmax=0.4), dtype=np.float64)
    st, st0, pm, N = _map_case(ctx, monkeypatch, [0.0, 0.0, float(W), float(W)], lines, (0.5, 0.5), radius)
    assert (pm.cols, pm.rows) == (24, 24) and N > 300
    assert st["vga_threads"] == 256 and st["vga_bottom_up_levels"] > 0, st
    assert _staged(st), st
    assert st0["vga_c_row_cells"] == 0 and st0["vga_pmask_cells"] > 0, st0
    if radius != -1:
        return
    # a source whose only bottom-up level (radius 2) lists fewer hard cells than a chunk: one wave, one partial chunk
    g = pm.make_graph(ctx)
    found = None
    for s in range(0, min(N, 96)):
        got = g.vga_visual_global(radius=2, src_begin=s, src_end=s + 1, levels=True)
        one = ctx.last_stats()
        if (one["vga_kernel"] == "tile-resolved" and one["vga_bottom_up_levels"] == 1 and one["vga_n_spec"] == 0
                and 0 < one["vga_hard_cells"] < CHUNK and one["vga_c_row_cells"] == one["vga_hard_cells"]):
            found = (s, one["vga_hard_cells"])
            monkeypatch.setenv("DMX_VGA_CSPLIT", "0")
            plain = g.vga_visual_global(radius=2, src_begin=s, src_end=s + 1, levels=True)
            monkeypatch.delenv("DMX_VGA_CSPLIT")
            assert ctx.last_stats()["vga_c_row_cells"] == 0
            _assert_same(got, plain)
            break
    g.close()
    assert found, "no source among the first 96 lists fewer than %d hard cells at its second level" % CHUNK


def test_chunk_with_a_single_entry(ctx, monkeypatch, dense):
    """Shape 2: some source's only bottom-up level (radius 2) lists 1 modulo CHUNK hard cells: its last chunk holds
    one entry.  The source's staged run equals its run under DMX_VGA_CSPLIT=0."""
    _clean(monkeypatch)
    pm = dmx.PointMap(dense.region, dense.lines, 1.0)
    assert pm.make_points(*dense.sp)
    g = pm.make_graph(ctx)
    N = g.info()["nnodes"]
    found = None
    for s in range(0, min(N, 512)):
        got = g.vga_visual_global(radius=2, src_begin=s, src_end=s + 1, levels=True)
        one = ctx.last_stats()
        if (one["vga_kernel"] == "tile-resolved" and one["vga_bottom_up_levels"] == 1 and one["vga_n_spec"] == 0
                and one["vga_hard_cells"] > CHUNK and one["vga_hard_cells"] % CHUNK == 1):
            found = (s, one["vga_hard_cells"])
            assert one["vga_c_row_cells"] == one["vga_hard_cells"], one
            monkeypatch.setenv("DMX_VGA_CSPLIT", "0")
            plain = g.vga_visual_global(radius=2, src_begin=s, src_end=s + 1, levels=True)
            monkeypatch.delenv("DMX_VGA_CSPLIT")
            assert ctx.last_stats()["vga_c_row_cells"] == 0
            _assert_same(got, plain)
            break
    g.close()
    assert found, "no source among the first 512 lists 1 modulo %d hard cells at its second level" % CHUNK


@pytest.mark.parametrize("radius,split", [(-1, "0"), (3, "0"), (-1, "1"), (-1, "2")])
def test_dense_map_every_outcome(ctx, monkeypatch, dense, radius, split):
    """Shape 3: certain hits, certain misses, undecided cells, mask loads and mask hits; DMX_VGA_CSPLIT=1 is the
    default, =2 (the mask stage alone, not built) is mapped to the loop of 0."""
    st, st0, pm, N = _map_case(ctx, monkeypatch, dense.region, dense.lines, dense.sp, radius, om=dense.om, split=split)
    assert (pm.cols, pm.rows) == (129, 129) and N > 8000
    assert st["vga_threads"] == 256 and st["vga_frontier_hbm"] == 0 and "masks" in st["vga_prep"], st
    assert _staged(st), st
    undecided = st["vga_pmask_cells"] - st["vga_hard_certain"] - st["vga_pruned_cells"]
    mask_hits = st["vga_hard_hits"] - st["vga_hard_certain"]
    assert st["vga_hard_certain"] > 0 and st["vga_pruned_cells"] > 0 and undecided > 0, st
    assert st["vga_pmask_loads"] > 0 and 0 < mask_hits <= undecided, st
    if split == "1":
        assert _staged(st0), st0
    else:
        assert st0["vga_c_row_cells"] == 0 and st0["vga_pmask_cells"] > 0, st0
    # the outcomes of a cell do not depend on the loop that tests it (hints only order the tests)
    for k in ("vga_pruned_cells",):
        assert st[k] == st0[k], (k, st, st0)


@pytest.mark.parametrize("radius", [-1, 3])
def test_1024_thread_member(ctx, monkeypatch, radius):
    """Shape 5: 4,356 tiles, the room across tile column 63|64: two row words a tile row."""
    region, lines, sp = make_room_map(520.0, 48.0, 30, 5, centre=(494.0, 256.0))
    st, st0, pm, N = _map_case(ctx, monkeypatch, region, lines, sp, radius)
    assert st["vga_threads"] == 1024 and st["vga_frontier_hbm"] == 0, st
    assert _staged(st), st
    assert st0["vga_c_row_cells"] == 0, st0


@pytest.mark.parametrize("radius", [-1, 3])
def test_absent_with_the_frontier_in_hbm(ctx, monkeypatch, radius):
    """Shape 6a: 20,449 tiles: the frontier in HBM, wide rows: the wide path, no row stage."""
    region, lines, sp = make_room_map(1136.0, 64.0, 60, 9, centre=(512.0, 1024.0))
    st, _, pm, N = _map_case(ctx, monkeypatch, region, lines, sp, radius)
    assert st["vga_threads"] == 1024 and st["vga_frontier_hbm"] == 1, st
    assert st["vga_c_row_cells"] == 0, st


@pytest.mark.parametrize("radius", [-1, 3])
def test_absent_without_masks(ctx, monkeypatch, dense, radius):
    """Shape 6b: no masks: phase C scans the runs behind its row pass."""
    st, _, pm, N = _map_case(ctx, monkeypatch, dense.region, dense.lines, dense.sp, radius,
                             env=[("DMX_VGA_PMASK", "0")], om=dense.om)
    assert "masks" not in st["vga_prep"] and st["vga_pmask_cells"] == 0, st
    assert st["vga_c_row_cells"] == 0 and st["vga_hard_cells"] > 0, st


def test_contextfilled_map_radius_3_twice(ctx, monkeypatch, dense):
    """Shape 7: a SEMIFILL map at radius 3: small frontiers, top-down levels between the bottom-up ones; two runs
    give the same bits."""
    st, _, pm, N = _map_case(ctx, monkeypatch, dense.region, dense.lines, dense.sp, 3,
                             fill_type=dmx.PointMap.SEMIFILL, runs=2)
    assert st["vga_bottom_up_levels"] > 0 and st["vga_top_down_levels"] > 0, st
    assert _staged(st), st


def test_seed_mode_step_depth(ctx, monkeypatch, dense):
    """Shape 8: visual step depth from 1 and from 5 seeded cells: the same kernel in seed mode, one workgroup."""
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
        assert _staged(st), st
        monkeypatch.setenv("DMX_VGA_CSPLIT", "0")
        plain = g.visual_step_depth(cells=cells)
        assert ctx.last_stats()["vga_c_row_cells"] == 0
        monkeypatch.delenv("DMX_VGA_CSPLIT")
        monkeypatch.setenv("DMX_VSD_TOPDOWN", "1")
        topdown = g.visual_step_depth(cells=cells)
        monkeypatch.delenv("DMX_VSD_TOPDOWN")
        want = dense.om.visual_stepdepth(cells)
        np.testing.assert_array_equal(got.view(np.uint32), plain.view(np.uint32))
        np.testing.assert_array_equal(got.view(np.uint32), topdown.view(np.uint32))
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        assert got.max() >= 2
    g.close()


@pytest.mark.parametrize("radius", [-1, 3])
def test_asymmetric_mode(ctx, monkeypatch, radius):
    """Shape 9a: syn128 written as a .graph chunk and read again (runs moved by the 4-bit row shifts), searched in
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
    st, st0 = _three_way(ctx, monkeypatch, g, load, radius, om, _sample(N))
    assert st["vga_asym_mode"] == 1 and st["vga_asym_nodes"] > 0, st
    assert st["vga_c_row_cells"] > 0 and st0["vga_c_row_cells"] == 0, (st, st0)
    g.close()
    g0.close()


def test_special_entries_next_to_staged_ones(ctx, monkeypatch):
    """Shape 9b: syn256 has 4 asymmetric nodes; around them the hard lists hold special entries (the exact in-set
    path, unchanged) and regular ones (the row stage).  Staged, unstaged and the v1 top-down kernel agree."""
    _clean(monkeypatch)
    lines = np.loadtxt(os.path.join(GOLDEN, "inputs", "syn256.csv"), delimiter=",", skiprows=1)
    pm = dmx.PointMap([0.0, 0.0, 256.0, 256.0], lines, 1.0)
    assert pm.make_points(0.5, 0.5)
    g = pm.make_graph(ctx)
    ranges = [(21900, 22100), (34000, 34200), (48050, 48200)]
    outs, nspec, nrow = [], 0, 0
    for (b, e) in ranges:
        outs.append(g.vga_visual_global(src_begin=b, src_end=e, levels=True))
        st = ctx.last_stats()
        assert st["vga_kernel"] == "tile-resolved" and st["vga_special_nodes"] == 4, st
        nspec += st["vga_n_spec"]
        nrow += st["vga_c_row_cells"]
    assert nspec > 0 and nrow > 0, (nspec, nrow)
    monkeypatch.setenv("DMX_VGA_CSPLIT", "0")
    for (b, e), (o, lv) in zip(ranges, outs):
        o0, lv0 = g.vga_visual_global(src_begin=b, src_end=e, levels=True)
        assert ctx.last_stats()["vga_c_row_cells"] == 0
        np.testing.assert_array_equal(lv[b:e], lv0[b:e])
        np.testing.assert_array_equal(o[b:e].view(np.uint32), o0[b:e].view(np.uint32))
    monkeypatch.delenv("DMX_VGA_CSPLIT")
    monkeypatch.setenv("DMX_VGA_KERNEL", "v1")
    g2 = pm.make_graph(ctx)
    for (b, e), (o, lv) in zip(ranges, outs):
        o2, lv2 = g2.vga_visual_global(src_begin=b, src_end=e, levels=True)
        np.testing.assert_array_equal(lv[b:e], lv2[b:e])
        np.testing.assert_array_equal(o[b:e].view(np.uint32), o2[b:e].view(np.uint32))
    g2.close()
    g.close()
