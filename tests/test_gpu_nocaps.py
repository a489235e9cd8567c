"""Grid sizes without LDS caps (VERDICT r1 "size caps the reference does not have"):

  * VGA visual local (VGAVisualLocal::run, salalib/vgamodules/vgavisuallocal.cpp:23-117): above
    ~780^2 cells its two tile bitmaps move from LDS to per-workgroup HBM slices;
  * visual step depth (VGAVisualGlobalDepth::run, vgavisualglobaldepth.cpp:23-77): above 1024^2, or
    on graphs too asymmetric for the tile-resolved BFS, the level-synchronous top-down search of
    kernels/vstep.hip runs instead.

Both variants are checked bit-exact against the reference fixtures (forced by DMX_VL_GBM /
DMX_VSD_TOPDOWN on the small cases) and, on grids past the old caps, against the C restatement
(oracle/dmx_oracle.c, pinned to the reference).  The large grids hold one walled room with
occluders, so the oracle builds their graphs in seconds while the kernels see the full grid.
"""
import numpy as np
import pytest

import depthmapx_amd as dmx
from golden.gen_synthetic import make_room_map as _room_map
from golden_io import case_input_lines, load_case

pytestmark = pytest.mark.gpu


def _map(meta):
    pm = dmx.PointMap(meta["region"], case_input_lines(meta), meta["spacing"])
    for f in meta["fills"]:
        assert pm.make_points(*f)
    return pm


@pytest.mark.parametrize("name", ["kat", "syn32", "syn64", "gallery"])
def test_vga_local_hbm_bitmaps_match_reference(ctx, monkeypatch, name):
    import os
    from golden_io import GOLDEN
    meta, A = load_case(name)
    g = _map(meta).make_graph(ctx)
    lds = g.vga_visual_local()
    monkeypatch.setenv("DMX_VL_GBM", "1")
    gbm = g.vga_visual_local()
    np.testing.assert_array_equal(gbm.view(np.uint32), lds.view(np.uint32))
    path = os.path.join(GOLDEN, name + "_vlocal.npy")
    if os.path.exists(path):
        np.testing.assert_array_equal(gbm.view(np.uint32), np.load(path).view(np.uint32))


def test_vga_local_above_780_matches_oracle(ctx):
    """820^2 cells (10,609 tiles: past the LDS variant's 9,600): HBM bitmaps vs the restatement."""
    from pyoracle import OracleMap
    region, lines, sp = _room_map(820.0, 56.0, 40, seed=5)
    pm = dmx.PointMap(region, lines, 1.0)
    assert pm.make_points(*sp)
    i = pm.info()
    assert ((i["cols"] + 7) // 8) * ((i["rows"] + 7) // 8) * 16 > 150 * 1024
    g = pm.make_graph(ctx)
    got = g.vga_visual_local()
    om = OracleMap(region, 1.0, lines)
    assert om.fill(*sp)
    om.make_graph(threads=8)
    np.testing.assert_array_equal(got.view(np.uint32), om.vga_local(threads=8).view(np.uint32))
    assert got.shape[0] == i["filled"] > 2000 and (got[:, 2] > 0).any()


@pytest.mark.parametrize("name", ["barnsbury", "syn128sd"])
def test_visual_stepdepth_topdown_matches_reference(ctx, monkeypatch, name):
    meta, A = load_case(name)
    if "vstepdepth" not in A:
        pytest.skip("fixture without visual step depth")
    g = _map(meta).make_graph(ctx)
    pts = [tuple(float(v) for v in p.split(",")) for p in meta["stepdepth"]]
    monkeypatch.setenv("DMX_VSD_TOPDOWN", "1")
    got = g.visual_step_depth(points=pts)
    np.testing.assert_array_equal(got.view(np.uint32), A["vstepdepth"].view(np.uint32))


@pytest.mark.parametrize("seed", [3, 7])
def test_visual_stepdepth_topdown_equals_tile(ctx, monkeypatch, seed):
    """Seeded dense maps, 1 / 4 / 32 selected cells: the top-down search == the tile BFS."""
    from golden.gen_synthetic import make_lines
    W = 96
    lines = np.array(make_lines(W, 200, seed=seed, lmin=0.02, lmax=0.3), dtype=np.float64)
    pm = dmx.PointMap([0.0, 0.0, float(W), float(W)], lines, 1.0)
    assert pm.make_points(0.5, 0.5)
    g = pm.make_graph(ctx)
    filled = np.nonzero(pm.state() & 2)[0]
    rng = np.random.default_rng(seed)
    for nsel in (1, 4, 32):
        cells = np.sort(rng.choice(filled, nsel, replace=False))
        monkeypatch.delenv("DMX_VSD_TOPDOWN", raising=False)
        a = g.visual_step_depth(cells=cells)
        monkeypatch.setenv("DMX_VSD_TOPDOWN", "1")
        b = g.visual_step_depth(cells=cells)
        np.testing.assert_array_equal(b.view(np.uint32), a.view(np.uint32))
        assert (b >= 0).sum() > len(b) // 2


def test_visual_stepdepth_above_1024_matches_oracle(ctx):
    """1100^2 cells (19,044 tiles: visual step depth takes the tile BFS in seed mode up to 16,384, api/stepdepth.hip):
    the top-down search vs the restatement."""
    from pyoracle import OracleMap
    region, lines, sp = _room_map(1100.0, 64.0, 60, seed=9)
    pm = dmx.PointMap(region, lines, 1.0)
    assert pm.make_points(*sp)
    g = pm.make_graph(ctx)
    om = OracleMap(region, 1.0, lines)
    assert om.fill(*sp)
    om.make_graph(threads=8)
    filled = np.nonzero(pm.state() & 2)[0]
    rng = np.random.default_rng(1)
    for nsel in (1, 5):
        cells = np.sort(rng.choice(filled, nsel, replace=False))
        got = g.visual_step_depth(cells=cells)
        want = om.visual_stepdepth(cells)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        assert got.max() >= 2


def test_vga_source_list_above_1024_matches_full_run(ctx):
    """dmx_vga_global_device_list at 1100^2 (19,044 tiles).  VGA global has no tile cap there: the full run and the
    source list both take the tile-resolved search, 1024 threads with the frontier (152 KB) still in the LDS, per-tile
    summaries instead of the line summaries, wide tile-visibility rows with their summaries and none of the other
    certificates (tests/test_gpu_vga_variants.py case E).  Listed rows equal the full run's, the others are
    untouched, and a block of them equals the restatement's BFS."""
    import torch
    from pyoracle import OracleMap
    region, lines, sp = _room_map(1100.0, 64.0, 60, seed=9)
    pm = dmx.PointMap(region, lines, 1.0)
    assert pm.make_points(*sp)
    g = pm.make_graph(ctx)
    full = g.vga_visual_global()
    n = full.shape[0]
    rng = np.random.default_rng(3)
    nodes = np.unique(np.concatenate([rng.choice(n, n // 4, replace=False), np.arange(100, 164)]))
    out = torch.full((n, 7), -7.0, dtype=torch.float32, device="cuda")
    variant = lambda st: (st["vga_kernel"], st["vga_threads"], st["vga_frontier_hbm"], st["vga_line_summaries"], st["vga_prep"])
    want_variant = ("tile-resolved", 1024, 0, 0, "scan+tvis+tvsum")
    assert variant(ctx.last_stats()) == want_variant and ctx.last_stats()["vga_sources"] == n
    g.vga_visual_global_device_list(out.data_ptr(), nodes)
    torch.cuda.synchronize()
    assert variant(ctx.last_stats()) == want_variant and ctx.last_stats()["vga_sources"] == len(nodes)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[nodes].view(np.uint32), full[nodes].view(np.uint32))
    assert (got[np.setdiff1d(np.arange(n), nodes)] == -7.0).all()
    om = OracleMap(region, 1.0, lines)
    assert om.fill(*sp)
    om.make_graph(threads=8)
    ref = om.vga_global(node_begin=100, node_end=164, threads=8)[100:164].astype(np.float64)
    a = got[100:164].astype(np.float64)
    np.testing.assert_array_equal(a[:, 5], ref[:, 5])
    assert (np.abs(a - ref) <= 1e-6 * np.maximum(1.0, np.abs(ref))).all()


def test_long_grid_falls_back_and_matches_oracle(ctx):
    """A strip 6001 x 13 cells: its long side is past the tile BFS's tile-common-run pass (the LDS holds
    32 B per cell of the longest side, ~4,800 cells), a capacity of the tile path -- VGA global, its
    source-list entry and visual step depth fall back to the direction-optimising / top-down searches
    instead of failing, and match the restatement over the same graph."""
    import torch
    from pyoracle import OracleMap
    W, H = 6000.0, 12.0
    rng = np.random.default_rng(11)
    walls = [[0, 0, W, 0], [W, 0, W, H], [W, H, 0, H], [0, H, 0, 0]]
    xs = rng.uniform(50.0, W - 50.0, size=12)
    walls += [[x, 0.0, x, 7.5] if i % 2 else [x + 3.0, 4.5, x + 3.0, H] for i, x in enumerate(xs)]
    lines = np.array(walls, dtype=np.float64)
    region = [0.0, 0.0, W, H]
    pm = dmx.PointMap(region, lines, 1.0)
    assert pm.make_points(0.5, 0.5)
    g = pm.make_graph(ctx)
    N = g.info()["nnodes"]
    assert max(pm.cols, pm.rows) > 4800
    om = OracleMap(region, 1.0, lines)
    assert om.fill(0.5, 0.5)
    full = g.copy(runs=True)
    om.set_graph_view(full["bins"], full["runs"])
    b, e = N // 2, N // 2 + 256
    got = g.vga_visual_global(src_begin=b, src_end=e)[b:e].astype(np.float64)
    assert ctx.last_stats()["vga_kernel"] != "tile-resolved"
    src = np.arange(b, e, 16, dtype=np.int64)
    ref, _ = om.vga_global_sample(src, threads=16)
    want = ref[src].astype(np.float64)
    mine = got[src - b]
    np.testing.assert_array_equal(mine[:, 5], want[:, 5])
    assert (np.abs(mine - want) <= 1e-6 * np.maximum(1.0, np.abs(want))).all()
    out = torch.full((N, 7), -1.0, dtype=torch.float32, device="cuda")
    g.vga_visual_global_device_list(out.data_ptr(), src)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy()[src].view(np.uint32), got[src - b].astype(np.float32).view(np.uint32))
    cell = int(np.nonzero(pm.state() & 2)[0][N // 3])
    v = g.visual_step_depth(cells=[cell])
    np.testing.assert_array_equal(v.view(np.uint32), om.visual_stepdepth([cell]).view(np.uint32))
