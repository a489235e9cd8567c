"""The tile walks of the tile-resolved VGA search (kernels/vga_tile.hip, DESIGN.md section 2 "tile walks").

By default phase A, the level bookkeeping and the X = F & ~V passes take VGA_WALK_NF = 4 tiles a thread at once (NF
below), with the loads of a batch in flight together and one list append a wave a batch, and a plain source (no seeds,
no merge links on the map, the frontier in LDS, not the asymmetric mode) builds its level 1 in place: V is written once,
by the first bookkeeping, and X not at all.  DMX_VGA_WALK=0 selects the loops that take a tile at a time.  Results do
not depend on it.

Each case compares, over all sources and bit for bit on the levels and the 7 columns, the default run with the run
under DMX_VGA_WALK=0 and with the direction-optimising search (DMX_VGA_KERNEL=do) on a fresh graph (shape 3: that
search over 8,192 of the 101,761 sources, to stay within seconds), and compares the
default run with the C restatement (oracle/dmx_oracle.c) at up to 64 seeded sources under the tolerances of
tests/test_gpu_vga_bstages.py: node counts and level columns exact, floats within 1e-6 * max(1, |want|).  The levels
run and the cells reached are equal between the default run and the DMX_VGA_WALK=0 run.  vga_tl_max is the longest tile
list a level's walks took.

The shapes (T = threads of the workgroup, a walk's batch is NF * T list entries):
   1  24^2 cells, 9 tiles: every walk is shorter than one thread-iteration
   2  dense maps of 128^2, 256^2 and 257^2 cells on the 256-thread member: 256, 1,024 and 1,089 tiles are one
      iteration, one whole batch, and a batch with a partial one; later levels list between 1 and nt tiles
   3  a room of 320^2 cells in 8 x 8 compartments on a 513^2 grid, the 1024-thread member: level 2 lists more than
      1,024 tiles (a CPU test checks that from the restatement's step depths, so that the GPU case cannot pass
      vacuously).  No room on this grid lists more than 4,096: the grid has 4,225 tiles and a room inside its border
      walls at most 63^2 = 3,969, so a second whole batch of the 1024-thread member is out of a few seconds' reach.
   4  the dense 129^2 map at radius 1, 2, 3 and n (the level loop's radius exit right after the level built in
      place), then radius 1 followed by radius n on one context against a fresh context (state left in V / X)
   5  the dense map context-filled (SEMIFILL) at radius 3, run twice: skipped odd sources between plain ones, cells
      that are not expanded, top-down levels
   6  visual step depth from seeded cells: seeded searches keep V and X initialised a source, walks batched
   7  a map with merge links, every listed cell a source with a partner: maps with links keep level 1 in X
   8  a re-read graph in asymmetric mode (DMX_VGA_ASYM=1): asym_uf in phase A, the A-cell list in the bookkeeping
   9  a room on a 1137^2 grid: the frontier in HBM
  10  an interleaved source list (dmx_vga_global_device_list), as the sharded path uses it
"""
import types

import numpy as np
import pytest

import depthmapx_amd as dmx
from depthmapx_amd import graphio
from golden.gen_synthetic import make_lines, make_room_map
from golden_io import case_input_lines, load_case

gpu = pytest.mark.gpu

NF = 4   # VGA_WALK_NF, kernels/vga_tile.hip
SWITCH_NAMES = ["DMX_VGA_WALK", "DMX_VGA_BSPLIT", "DMX_VGA_KERNEL", "DMX_VGA_TVIS", "DMX_VGA_FTVIS", "DMX_VGA_TTVIS",
                "DMX_VGA_PMASK", "DMX_VGA_TVNZ", "DMX_VGA_NOHINT2", "DMX_VGA_RB", "DMX_VGA_CRK", "DMX_VGA_CHUNK",
                "DMX_VGA_ALPHA", "DMX_VGA_BEXT", "DMX_VGA_ASYM", "DMX_VGA_NOASYM", "DMX_VSD_TOPDOWN"]
DENSE = dict(W=128, n=120, seed=5, lmin=0.02, lmax=0.12)
SAME_COUNTERS = ("vga_bottom_up_levels", "vga_top_down_levels", "vga_cells_reached", "vga_sources", "vga_threads")
THREADS = 16


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


def _sample(N, n=62):
    rng = np.random.default_rng(17)
    return np.unique(np.concatenate([rng.choice(N, min(N, n), replace=False), [0, N - 1]]))


def _dense_lines(W):
    """The DENSE recipe scaled to a W-wide region: as many occluders an area, of the same lengths in cells."""
    s = W / float(DENSE["W"])
    return np.array(make_lines(W, max(4, int(round(DENSE["n"] * s * s))), seed=DENSE["seed"], lmin=DENSE["lmin"] / s,
                               lmax=DENSE["lmax"] / s), dtype=np.float64)


def _oracle(region, lines, sp, fill_type=0):
    from pyoracle import OracleMap
    om = OracleMap(region, 1.0, lines)
    assert om.fill(*sp, fill_type=fill_type)
    om.make_graph(threads=THREADS)
    return om


def _same_counters(st, st0):
    for k in SAME_COUNTERS:
        assert st[k] == st0[k], (k, st[k], st0[k])


def _three_way(ctx, mp, g, make_second, radius, om, src, runs=1, do_range=None):
    """The default run of graph g (`runs` times, all equal), the run a tile at a time and the second search on
    make_second()'s graph, all sources, bit for bit; the default run against the restatement at src.  Returns the
    default run's and the DMX_VGA_WALK=0 run's counters.  do_range = (begin, end): the second search runs those
    sources only (shape 3, where it takes 11 s over all of them)."""
    mp.delenv("DMX_VGA_WALK", raising=False)
    got = g.vga_visual_global(radius=radius, levels=True)
    st = ctx.last_stats()
    assert st["vga_kernel"] == "tile-resolved", st
    for _ in range(runs - 1):
        _assert_same(got, g.vga_visual_global(radius=radius, levels=True))
    mp.setenv("DMX_VGA_WALK", "0")
    single = g.vga_visual_global(radius=radius, levels=True)
    st0 = ctx.last_stats()
    mp.delenv("DMX_VGA_WALK")
    assert st0["vga_kernel"] == "tile-resolved", st0
    _assert_same(got, single)
    _same_counters(st, st0)
    assert st["vga_tl_max"] == st0["vga_tl_max"], (st["vga_tl_max"], st0["vga_tl_max"])
    mp.setenv("DMX_VGA_KERNEL", "do")
    g2 = make_second()
    b, e = do_range or (0, got[0].shape[0])
    second = g2.vga_visual_global(radius=radius, levels=True, src_begin=b, src_end=e)
    # (on a re-read graph the second search runs top-down only and says so)
    assert ctx.last_stats()["vga_kernel"].startswith("direction-optimizing")
    g2.close()
    mp.delenv("DMX_VGA_KERNEL")
    _assert_same((got[0][b:e], got[1][b:e]), (second[0][b:e], second[1][b:e]))
    want, _, rlv = om.vga_global_sample(src, radius=radius, threads=THREADS, levels=True)
    np.testing.assert_array_equal(got[0][src, 5], want[src, 5])
    np.testing.assert_array_equal(got[1][src, :2], rlv[src, :2])
    _assert_close(got[0][src], want[src])
    return st, st0


def _map_case(ctx, mp, region, lines, sp, radius, fill_type=0, om=None, runs=1, nsrc=62, do_sources=None):
    """A map made from its drawing, through _three_way."""
    _clean(mp)
    pm = dmx.PointMap(region, lines, 1.0)
    assert pm.make_points(*sp, fill_type=fill_type)
    g = pm.make_graph(ctx)
    N = g.info()["nnodes"]
    om = om or _oracle(region, lines, sp, fill_type)
    assert om.num_nodes == N
    try:
        do_range = (N // 2 - do_sources // 2, N // 2 + do_sources // 2) if do_sources else None
        return _three_way(ctx, mp, g, lambda: pm.make_graph(ctx), radius, om, _sample(N, nsrc), runs, do_range) + (pm, N)
    finally:
        g.close()


@pytest.fixture(scope="module")
def dense():
    """The dense 129^2 map's drawing and its restatement graph (built once; the searches do not change it)."""
    W = DENSE["W"]
    region = [0.0, 0.0, float(W), float(W)]
    lines = _dense_lines(W)
    sp = (0.5, 0.5)
    return types.SimpleNamespace(region=region, lines=lines, sp=sp, om=_oracle(region, lines, sp))


# ---- shape 3's map: a room in compartments
ROOM = dict(W=512, room=320, pitch=40, gap=6)


def _compartment_room(W, room, pitch, gap):
    """A W x W region with a walled room of side `room` in the middle, divided into (room / pitch)^2 compartments
    by partitions that leave a door of `gap` at one end of every compartment side: a cell sees its compartment and
    slivers of others, so that most of the room's tiles keep an unvisited cell after level 1."""
    x0 = y0 = W / 2 - room / 2
    x1, y1 = x0 + room, y0 + room
    walls = [[0, 0, W, 0], [W, 0, W, W], [W, W, 0, W], [0, W, 0, 0],
             [x0, y0, x1, y0], [x1, y0, x1, y1], [x1, y1, x0, y1], [x0, y1, x0, y0]]
    n = int(round(room / pitch))
    for i in range(1, n):
        p = i * pitch + 0.37   # (off the cell corners)
        for j in range(n):
            q = j * pitch
            walls.append([x0 + p, y0 + q, x0 + p, y0 + q + pitch - gap])
            walls.append([x0 + q, y0 + p, x0 + q + pitch - gap, y0 + p])
    return [0.0, 0.0, float(W), float(W)], np.array(walls, dtype=np.float64), (x0 + 1.3, y0 + 1.3)


@pytest.fixture(scope="module")
def room():
    region, lines, sp = _compartment_room(**ROOM)
    return types.SimpleNamespace(region=region, lines=lines, sp=sp, om=_oracle(region, lines, sp))


def test_room_lists_more_than_1024_tiles_at_level_2(room):
    """CPU: from the restatement's step depths, the tiles that hold a cell deeper than level 1 -- the list the first
    bookkeeping builds for level 2 -- are more than 1,024 for a source in a corner, in the middle and at the end of
    the room, and fewer than 4,096."""
    om = room.om
    st = np.asarray(om.state())
    W = ROOM["W"] + 1
    assert len(st) == W * W
    cells = np.flatnonzero(st & 2)
    assert len(cells) == om.num_nodes and om.num_nodes >= 300 * 300
    tw = (W + 7) // 8
    for c in cells[[0, len(cells) // 2, len(cells) - 1]]:
        d = om.visual_stepdepth([int(c)])
        assert d.min() >= 0, "every cell of the room is reached"
        deep = cells[d >= 2]
        x, y = deep // W, deep % W
        ntl = len(np.unique((y >> 3) * tw + (x >> 3)))
        assert 1024 < ntl < 4096, ntl


# ---- shape 1
@gpu
@pytest.mark.parametrize("radius", [-1, 3])
def test_walks_shorter_than_one_iteration(ctx, monkeypatch, radius):
    """Shape 1: 9 tiles on 256 threads: a walk's batch holds one partial iteration."""
    W = 23
    lines = np.array(make_lines(W, 12, seed=3, lmin=0.1, lmax=0.4), dtype=np.float64)
    st, _, pm, N = _map_case(ctx, monkeypatch, [0.0, 0.0, float(W), float(W)], lines, (0.5, 0.5), radius)
    assert (pm.cols, pm.rows) == (24, 24) and N > 300
    assert st["vga_threads"] == 256 and st["vga_bottom_up_levels"] > 0, st
    assert 0 < st["vga_tl_max"] <= 9, st


# ---- shape 2
@gpu
@pytest.mark.parametrize("cells,tiles", [(128, 256), (256, 1024), (257, 1089)])
def test_dense_map_one_iteration_one_batch_and_a_partial_one(ctx, monkeypatch, cells, tiles):
    """Shape 2: 256 tiles are exactly one iteration of the 256 threads, 1,024 exactly one batch of NF, 1,089 a batch
    and a partial one; the lists of later levels hold between 1 and nt tiles."""
    W = cells - 1
    st, _, pm, N = _map_case(ctx, monkeypatch, [0.0, 0.0, float(W), float(W)], _dense_lines(W), (0.5, 0.5), -1)
    assert (pm.cols, pm.rows) == (cells, cells) and ((cells + 7) // 8) ** 2 == tiles
    assert st["vga_threads"] == 256 and st["vga_frontier_hbm"] == 0, st
    assert tiles in (256, NF * 256, NF * 256 + 65)
    assert st["vga_bottom_up_levels"] > 0 and 1 <= st["vga_tl_max"] <= tiles, st
    if tiles > 256:
        assert st["vga_tl_max"] > 256, st


# ---- shape 3
@gpu
def test_1024_thread_member_lists_more_than_1024_tiles(ctx, monkeypatch, room):
    """Shape 3: 4,225 tiles on 1024 threads; a level's list is longer than one iteration of them (and shorter than
    a whole batch of NF: see the module's note).  The default run and the run a tile at a time over all 101,761
    sources; the direction-optimising search over the 8,192 sources in the middle of the room (over all of them it
    alone takes 11 s) and the restatement at 16 sources."""
    st, _, pm, N = _map_case(ctx, monkeypatch, room.region, room.lines, room.sp, -1, om=room.om, nsrc=14,
                             do_sources=8192)
    assert (pm.cols, pm.rows) == (513, 513) and N >= 300 * 300
    assert st["vga_threads"] == 1024 and st["vga_frontier_hbm"] == 0, st
    assert 1024 < st["vga_tl_max"] < NF * 1024, st


# ---- shape 4
@gpu
@pytest.mark.parametrize("radius", [1, 2, 3, -1])
def test_dense_map_radius_exit_after_the_level_built_in_place(ctx, monkeypatch, dense, radius):
    """Shape 4: at radius 1 the level loop ends right after the first bookkeeping, at 2 and 3 after a bottom-up
    level or two."""
    st, _, pm, N = _map_case(ctx, monkeypatch, dense.region, dense.lines, dense.sp, radius, om=dense.om)
    assert (pm.cols, pm.rows) == (129, 129) and N > 8000
    assert st["vga_threads"] == 256, st
    if radius == 1:
        assert st["vga_bottom_up_levels"] == 0 and 0 < st["vga_top_down_levels"] <= N and st["vga_tl_max"] == 0, st
    else:
        assert st["vga_bottom_up_levels"] > 0 and 0 < st["vga_tl_max"] <= 289, st


@gpu
def test_radius_1_then_radius_n_on_one_context(ctx, monkeypatch, dense):
    """Shape 4: radius 1 leaves every source's V and X where its first bookkeeping put them; the radius-n run that
    follows on the same context and graph equals the one on a fresh context."""
    _clean(monkeypatch)
    pm = dmx.PointMap(dense.region, dense.lines, 1.0)
    assert pm.make_points(*dense.sp)
    g = pm.make_graph(ctx)
    first = g.vga_visual_global(radius=1, levels=True)
    then = g.vga_visual_global(radius=-1, levels=True)
    again = g.vga_visual_global(radius=1, levels=True)
    _assert_same(first, again)
    g.close()
    fresh = dmx.Context(0)
    try:
        g2 = pm.make_graph(fresh)
        _assert_same(then, g2.vga_visual_global(radius=-1, levels=True))
        assert fresh.last_stats()["vga_kernel"] == "tile-resolved"
        g2.close()
    finally:
        fresh.close()


# ---- shape 5
@gpu
def test_contextfilled_map_radius_3_twice(ctx, monkeypatch, dense):
    """Shape 5: a SEMIFILL map at radius 3: odd cells are no sources (skipped between plain ones) and are not
    expanded, top-down levels come between the bottom-up ones; two runs give the same bits."""
    st, _, pm, N = _map_case(ctx, monkeypatch, dense.region, dense.lines, dense.sp, 3,
                             fill_type=dmx.PointMap.SEMIFILL, runs=2)
    assert st["vga_bottom_up_levels"] > 0 and st["vga_top_down_levels"] > 0, st
    assert st["vga_tl_max"] > 0, st


# ---- shape 6
@gpu
def test_seed_mode_step_depth(ctx, monkeypatch, dense):
    """Shape 6: visual step depth from 1 and from 5 seeded cells: the same kernel in seed mode, one workgroup, V and
    X initialised a search and the walks batched; the run a tile at a time and the top-down search give the
    restatement's bits."""
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
        assert st["vga_tl_max"] > 0, st
        monkeypatch.setenv("DMX_VGA_WALK", "0")
        single = g.visual_step_depth(cells=cells)
        _same_counters(st, ctx.last_stats())
        monkeypatch.delenv("DMX_VGA_WALK")
        monkeypatch.setenv("DMX_VSD_TOPDOWN", "1")
        topdown = g.visual_step_depth(cells=cells)
        monkeypatch.delenv("DMX_VSD_TOPDOWN")
        want = dense.om.visual_stepdepth(cells)
        np.testing.assert_array_equal(got.view(np.uint32), single.view(np.uint32))
        np.testing.assert_array_equal(got.view(np.uint32), topdown.view(np.uint32))
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        assert got.max() >= 2
    g.close()


# ---- shape 7
@gpu
@pytest.mark.parametrize("radius", [-1, 3])
def test_merge_links_sources_with_partners(ctx, monkeypatch, radius):
    """Shape 7: 12 merge links between filled cells of a 65^2 map: 24 sources have a partner, whose bit joins V at
    level 0; the restatement over all sources."""
    from pyoracle import OracleMap
    _clean(monkeypatch)
    W = 64
    lines = np.array(make_lines(W, 60, seed=2, lmin=0.04, lmax=0.25), dtype=np.float64)
    region = [0.0, 0.0, float(W), float(W)]
    pm = dmx.PointMap(region, lines, 1.0)
    om = OracleMap(region, 1.0, lines)
    assert pm.make_points(0.5, 0.5) and om.fill(0.5, 0.5)
    filled = np.flatnonzero(pm.state() & 2)
    pairs = np.random.default_rng(2).choice(filled, size=24, replace=False).reshape(-1, 2).astype(np.int32)
    pm.set_merges(pairs)
    om.make_graph(threads=THREADS)
    om.set_merges(pairs)
    g = pm.make_graph(ctx)
    N = g.info()["nnodes"]
    st, _ = _three_way(ctx, monkeypatch, g, lambda: pm.make_graph(ctx), radius, om, np.arange(N))
    assert st["vga_bottom_up_levels"] > 0 and st["vga_tl_max"] > 0, st
    g.close()
    # the links change the result (the comparison above would hold vacuously otherwise)
    if radius == -1:
        om.set_merges(np.zeros((0, 2), dtype=np.int32))
        _, plain = om.vga_global(radius=-1, threads=THREADS, levels=True)
        g = pm.make_graph(ctx)
        _, linked = g.vga_visual_global(radius=-1, levels=True)
        g.close()
        assert (plain[:, 1] != linked[:, 1]).any()


# ---- shape 8
@gpu
@pytest.mark.parametrize("radius", [-1, 3])
def test_asymmetric_mode(ctx, monkeypatch, radius):
    """Shape 8: syn128 written as a .graph chunk and read again (runs moved by the 4-bit row shifts), searched in
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
    assert st["vga_asym_mode"] == 1 and st["vga_asym_nodes"] > 0 and st["vga_tl_max"] > 0, st
    g.close()
    g0.close()


# ---- shape 9
@gpu
@pytest.mark.parametrize("radius", [-1, 3])
def test_hbm_frontier_member(ctx, monkeypatch, radius):
    """Shape 9: 20,449 tiles: the frontier in HBM (V and X initialised a source, level 1 written to X)."""
    region, lines, sp = make_room_map(1136.0, 64.0, 60, 9, centre=(512.0, 1024.0))
    st, _, pm, N = _map_case(ctx, monkeypatch, region, lines, sp, radius)
    assert st["vga_threads"] == 1024 and st["vga_frontier_hbm"] == 1, st
    assert st["vga_bottom_up_levels"] > 0 and st["vga_tl_max"] > 0, st


# ---- shape 10
@gpu
def test_interleaved_source_list(ctx, monkeypatch, dense):
    """Shape 10: every third source through dmx_vga_global_device_list: the listed rows equal the full run's bit
    for bit, by default and a tile at a time, and every other row is left untouched."""
    import torch
    _clean(monkeypatch)
    pm = dmx.PointMap(dense.region, dense.lines, 1.0)
    assert pm.make_points(*dense.sp)
    g = pm.make_graph(ctx)
    full = g.vga_visual_global()
    n = full.shape[0]
    nodes = np.arange(1, n, 3)
    rest = np.setdiff1d(np.arange(n), nodes)
    stats = []
    for walk in (None, "0"):
        if walk is not None:
            monkeypatch.setenv("DMX_VGA_WALK", walk)
        out = torch.full((n, 7), -7.0, dtype=torch.float32, device="cuda")
        g.vga_visual_global_device_list(out.data_ptr(), nodes)
        torch.cuda.synchronize()
        st = ctx.last_stats()
        assert st["vga_kernel"] == "tile-resolved" and st["vga_sources"] == len(nodes), st
        stats.append(st)
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[nodes].view(np.uint32), full[nodes].view(np.uint32))
        assert (got[rest] == -7.0).all()
    monkeypatch.delenv("DMX_VGA_WALK")
    _same_counters(stats[0], stats[1])
    assert stats[0]["vga_tl_max"] == stats[1]["vga_tl_max"] > 0, stats[0]
    g.close()
