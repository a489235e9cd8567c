"""Phase C's miss certificate in the tile-resolved VGA search (kernels/vga_tile.hip, DESIGN.md section 2 "a miss
certificate in front of the rows").

A wave that takes a chunk of 16 hard cells loads the cells' block summaries (tvblk: 4 words a cell, a bit per 8 x 8
block of tiles the cell sees a tile of; lane 4j + k holds word k of entry j) in one trip and drops the regular cells
none of whose blocks holds a frontier tile (the same reduction of the frontier's tile summary, rebuilt by every level's
bookkeeping behind the merge pass).  Those are certain misses, counted as such
(vga_pruned_cells, vga_pmask_cells, vga_hard_cells, vga_c_row_cells) and in vga_c_cert_cells; their rows are not read.
The test is one-sided, so levels, hints and columns do not change.  DMX_VGA_CCERT=0, read at launch, turns it off.

Every case compares, over all sources and bit for bit on the levels and the 7 columns, the default run with the run
under DMX_VGA_CCERT=0 and with the direction-optimising search (DMX_VGA_KERNEL=do) on a fresh graph, and the default
run with the C restatement (oracle/dmx_oracle.c) at up to 64 seeded sources under the tolerances of
tests/test_gpu_vga_cstages.py: node counts and level columns exact, floats within 1e-6 * max(1, |want|).  Within a
run 0 <= vga_c_cert_cells <= vga_pruned_cells <= vga_hard_cells; under DMX_VGA_CCERT=0 vga_c_cert_cells == 0.

The shapes (CHUNK = VGA_CCH = 16 entries a grab):
   1  3 x 3 tiles (24^2 cells): one block, bit 0 of summary word 0 (words 1..3 of an entry are zero), and a source
      whose bottom-up level lists fewer hard cells than a chunk (entries past the list's end)
   2  the dense 129^2 map, a source whose bottom-up level lists 1 modulo 16 hard cells: a single-entry chunk behind a
      full one (whose entry 15 sits in lanes 60..63)
   3  the dense map over all sources: cells rejected, and certain hits, undecided cells and mask hits all present
   4  the dense map moved low on a 521^2 grid, to the left edge and across the 64-tile word boundary: two words a tile
      row, 9 x 9 blocks; block row 7 is bits 63..71, so summary words 0 and 1 are both set, a row word's 8 bits are
      carried across them, and the 9th column comes from a tile row's second word; 1024 threads
   5  the dense map with merge links: the frontier's summary is built after the merge pass
   6  the dense map context-filled (SEMIFILL) at radius 3, run twice: small frontiers, top-down levels past the first
   7  visual step depth from seeded cells
   8  a map with asymmetric (special) nodes, and a re-read graph in asymmetric mode: special entries are never rejected
   9  the certificate absent, counter zero, results equal: a 1137^2 room (frontier in HBM) and DMX_VGA_PMASK=0
  10  shape 3 under DMX_VGA_BSPLIT=0 and =3: phase B fused and staged next to the certificate (the row stage's
      buffer loads of the design were measured and not kept)
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
SWITCH_NAMES = ["DMX_VGA_CCERT", "DMX_VGA_CSPLIT", "DMX_VGA_BSPLIT", "DMX_VGA_WALK", "DMX_VGA_KERNEL",
                "DMX_VGA_TVIS", "DMX_VGA_FTVIS", "DMX_VGA_TTVIS", "DMX_VGA_PMASK", "DMX_VGA_NOHINT2", "DMX_VGA_RB",
                "DMX_VGA_CRK", "DMX_VGA_CHUNK", "DMX_VGA_ALPHA", "DMX_VGA_BEXT", "DMX_VGA_ASYM", "DMX_VGA_NOASYM",
                "DMX_VSD_TOPDOWN"]
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


def _ordered(st):
    assert 0 <= st["vga_c_cert_cells"] <= st["vga_pruned_cells"] <= st["vga_hard_cells"], st


def _three_way(ctx, mp, g, make_second, radius, om, src, runs=1, switch=("DMX_VGA_CCERT", "0")):
    """The default run of graph g (`runs` times, all equal), the run under `switch` and the second search on
    make_second()'s graph, all sources, bit for bit; the default run against the restatement at src.  Returns the
    default run's and the switched run's counters."""
    mp.delenv(switch[0], raising=False)
    got = g.vga_visual_global(radius=radius, levels=True)
    st = ctx.last_stats()
    assert st["vga_kernel"] == "tile-resolved", st
    print("cert / pruned / hard cells:", st["vga_c_cert_cells"], st["vga_pruned_cells"], st["vga_hard_cells"])
    _ordered(st)
    for _ in range(runs - 1):
        _assert_same(got, g.vga_visual_global(radius=radius, levels=True))
    mp.setenv(*switch)
    plain = g.vga_visual_global(radius=radius, levels=True)
    st0 = ctx.last_stats()
    mp.delenv(switch[0])
    assert st0["vga_kernel"] == "tile-resolved", st0
    _ordered(st0)
    if switch[0] == "DMX_VGA_CCERT":
        assert st0["vga_c_cert_cells"] == 0, st0
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


def _map_case(ctx, mp, region, lines, sp, radius, env=(), fill_type=0, om=None, runs=1,
              switch=("DMX_VGA_CCERT", "0")):
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
        return _three_way(ctx, mp, g, lambda: pm.make_graph(ctx), radius, om, _sample(N), runs, switch) + (pm, N)
    finally:
        g.close()


def _counted(st):
    """The certificate's cells count as the certain misses they are: the row stage's identity of
    tests/test_gpu_vga_cstages.py holds with them."""
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


def _one_source(ctx, mp, g, N, limit, want):
    """The first source below `limit` whose only bottom-up level (radius 2) lists want(n) hard cells: its default run
    against its run under DMX_VGA_CCERT=0.  Returns (source, hard cells, rejected cells) or None."""
    for s in range(0, min(N, limit)):
        got = g.vga_visual_global(radius=2, src_begin=s, src_end=s + 1, levels=True)
        one = ctx.last_stats()
        if (one["vga_kernel"] == "tile-resolved" and one["vga_bottom_up_levels"] == 1 and one["vga_n_spec"] == 0
                and want(one["vga_hard_cells"])):
            _ordered(one)
            assert one["vga_c_row_cells"] == one["vga_hard_cells"], one
            mp.setenv("DMX_VGA_CCERT", "0")
            plain = g.vga_visual_global(radius=2, src_begin=s, src_end=s + 1, levels=True)
            st0 = ctx.last_stats()
            mp.delenv("DMX_VGA_CCERT")
            assert st0["vga_c_cert_cells"] == 0 and st0["vga_hard_cells"] == one["vga_hard_cells"], (one, st0)
            assert st0["vga_pruned_cells"] == one["vga_pruned_cells"], (one, st0)
            _assert_same(got, plain)
            return s, one["vga_hard_cells"], one["vga_c_cert_cells"]
    return None


@pytest.mark.parametrize("radius", [-1, 3])
def test_one_block_and_a_short_list(ctx, monkeypatch, radius):
    """Shape 1: 9 tiles are one block: words 1..3 of every entry are zero; some source's second level lists fewer
    hard cells than a chunk, so entries are past the list's end."""
    W = 23
    lines = np.array(make_lines(W, 12, seed=3, lmin=0.1, lmax=0.4), dtype=np.float64)
    st, st0, pm, N = _map_case(ctx, monkeypatch, [0.0, 0.0, float(W), float(W)], lines, (0.5, 0.5), radius)
    assert (pm.cols, pm.rows) == (24, 24) and N > 300
    assert st["vga_threads"] == 256 and st["vga_bottom_up_levels"] > 0, st
    assert _counted(st) and _counted(st0), (st, st0)
    assert st["vga_pruned_cells"] == st0["vga_pruned_cells"], (st, st0)
    if radius != -1:
        return
    g = pm.make_graph(ctx)
    found = _one_source(ctx, monkeypatch, g, N, 96, lambda n: 0 < n < CHUNK)
    g.close()
    assert found, "no source among the first 96 lists fewer than %d hard cells at its second level" % CHUNK


def test_chunk_with_a_single_entry(ctx, monkeypatch, dense):
    """Shape 2: a source whose only bottom-up level lists 1 modulo CHUNK hard cells: the last chunk holds one entry
    (lanes 0..3), the chunk before it is full (entry 15 in lanes 60..63)."""
    _clean(monkeypatch)
    pm = dmx.PointMap(dense.region, dense.lines, 1.0)
    assert pm.make_points(*dense.sp)
    g = pm.make_graph(ctx)
    found = _one_source(ctx, monkeypatch, g, g.info()["nnodes"], 512, lambda n: n > CHUNK and n % CHUNK == 1)
    g.close()
    assert found, "no source among the first 512 lists 1 modulo %d hard cells at its second level" % CHUNK


@pytest.mark.parametrize("radius", [-1, 3])
def test_dense_map_every_outcome(ctx, monkeypatch, dense, radius):
    """Shape 3: cells rejected by the certificate next to certain hits, undecided cells and mask hits; the certain
    misses are as many with and without it."""
    st, st0, pm, N = _map_case(ctx, monkeypatch, dense.region, dense.lines, dense.sp, radius, om=dense.om)
    assert (pm.cols, pm.rows) == (129, 129) and N > 8000
    assert st["vga_threads"] == 256 and st["vga_frontier_hbm"] == 0 and "masks" in st["vga_prep"], st
    assert st["vga_tile_rows_bytes"] == st0["vga_tile_rows_bytes"] > 0, (st, st0)   # (the summaries stay in place)
    assert _counted(st) and _counted(st0), (st, st0)
    assert st["vga_c_cert_cells"] > 0, st
    undecided = st["vga_pmask_cells"] - st["vga_hard_certain"] - st["vga_pruned_cells"]
    mask_hits = st["vga_hard_hits"] - st["vga_hard_certain"]
    assert st["vga_hard_certain"] > 0 and st["vga_pruned_cells"] > st["vga_c_cert_cells"] and undecided > 0, st
    assert st["vga_pmask_loads"] > 0 and 0 < mask_hits <= undecided, st
    assert st["vga_pruned_cells"] == st0["vga_pruned_cells"], (st, st0)
    # the rows of the rejected cells are not read
    assert st["vga_tvis_bytes"] < st0["vga_tvis_bytes"], (st, st0)


_MOVED = {}


def _moved_dense(ox, oy):
    """The dense map's drawing moved by (ox, oy) into a 520 x 520 region, inside a wall of its own between the cells
    around it, and its restatement graph (built once a place)."""
    if (ox, oy) not in _MOVED:
        W = DENSE["W"]
        lines = np.array(make_lines(W, DENSE["n"], seed=DENSE["seed"], lmin=DENSE["lmin"], lmax=DENSE["lmax"]),
                         dtype=np.float64) + np.array([ox, oy, ox, oy], dtype=np.float64)
        a0, b0, a1, b1 = ox - 0.5, oy - 0.5, ox + W + 0.5, oy + W + 0.5
        box = np.array([[a0, b0, a1, b0], [a1, b0, a1, b1], [a1, b1, a0, b1], [a0, b1, a0, b0]], dtype=np.float64)
        region, lines, sp = [0.0, 0.0, 520.0, 520.0], np.concatenate([box, lines]), (ox + 0.5, oy + 0.5)
        _MOVED[(ox, oy)] = (region, lines, sp, _oracle(region, lines, sp))
    return _MOVED[(ox, oy)]


@pytest.mark.parametrize("ox", [16.0, 386.0])
@pytest.mark.parametrize("radius", [-1, 3])
def test_1024_thread_member(ctx, monkeypatch, radius, ox):
    """Shape 4: 4,356 tiles (66 x 66: two row words a tile row), 81 blocks in rows of 9 bits.  The dense map moved to
    tile rows 47..63, block rows 5..7.  Block row 7 is bits 63..71 of the summary: it starts in word 0 and goes on in
    word 1.  At ox = 16 the map covers tile columns 2..18, block columns 0..2: bits 63 | 64, 65, and the 8 bits of a
    tile row's first word are placed at bit 63, so all but the first are carried into word 1.  At ox = 386 it covers
    tile columns 48..64, across the row words' boundary 63 | 64, block columns 6..8: bits 69..71 lie in word 1, and
    column 8 comes from a tile row's second word."""
    region, lines, sp, om = _moved_dense(ox, 376.0)
    st, st0, pm, N = _map_case(ctx, monkeypatch, region, lines, sp, radius, om=om)
    assert (pm.cols, pm.rows) == (521, 521) and N > 8000
    assert st["vga_threads"] == 1024 and st["vga_frontier_hbm"] == 0, st
    assert _counted(st), st
    assert st["vga_c_cert_cells"] > 0, st
    assert st["vga_pruned_cells"] == st0["vga_pruned_cells"], (st, st0)


@pytest.mark.parametrize("radius", [-1, 3])
def test_merge_links(ctx, monkeypatch, dense, radius):
    """Shape 5: 12 merge links on the dense map (a 65^2 map is 2 x 2 blocks, and its certificate rejects nothing): the
    merge pass sets frontier bits anywhere, and the frontier's summary is built behind it.  The restatement has a graph
    of its own, since the links change it."""
    from pyoracle import OracleMap
    _clean(monkeypatch)
    pm = dmx.PointMap(dense.region, dense.lines, 1.0)
    om = OracleMap(dense.region, 1.0, dense.lines)
    assert pm.make_points(*dense.sp) and om.fill(*dense.sp)
    filled = np.flatnonzero(pm.state() & 2)
    pairs = np.random.default_rng(2).choice(filled, size=24, replace=False).reshape(-1, 2).astype(np.int32)
    pm.set_merges(pairs)
    om.make_graph(threads=8)
    om.set_merges(pairs)
    g = pm.make_graph(ctx)
    N = g.info()["nnodes"]
    st, st0 = _three_way(ctx, monkeypatch, g, lambda: pm.make_graph(ctx), radius, om, _sample(N))
    assert st["vga_bottom_up_levels"] > 0 and st["vga_hard_cells"] > 0, st
    assert st["vga_c_cert_cells"] > 0, st
    g.close()
    # the links change the result (the comparison above would hold vacuously otherwise)
    if radius == -1:
        src = _sample(N)
        with_links, _, _ = om.vga_global_sample(src, radius=radius, threads=8, levels=True)
        without, _, _ = dense.om.vga_global_sample(src, radius=radius, threads=8, levels=True)
        assert np.any(with_links[src] != without[src])


def test_contextfilled_map_radius_3_twice(ctx, monkeypatch, dense):
    """Shape 6: a SEMIFILL map at radius 3: small frontiers, top-down levels between the bottom-up ones; two runs
    give the same bits."""
    st, st0, pm, N = _map_case(ctx, monkeypatch, dense.region, dense.lines, dense.sp, 3,
                               fill_type=dmx.PointMap.SEMIFILL, runs=2)
    assert st["vga_bottom_up_levels"] > 0 and st["vga_top_down_levels"] > 0, st
    assert _counted(st), st
    assert st["vga_c_cert_cells"] > 0, st
    assert st["vga_pruned_cells"] == st0["vga_pruned_cells"], (st, st0)


def test_seed_mode_step_depth(ctx, monkeypatch, dense):
    """Shape 7: visual step depth from 1 and from 5 seeded cells: the same kernel in seed mode, one workgroup."""
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
        _ordered(st)
        monkeypatch.setenv("DMX_VGA_CCERT", "0")
        plain = g.visual_step_depth(cells=cells)
        st0 = ctx.last_stats()
        assert st0["vga_c_cert_cells"] == 0 and st0["vga_pruned_cells"] == st["vga_pruned_cells"], (st, st0)
        monkeypatch.delenv("DMX_VGA_CCERT")
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
    """Shape 8a: syn128 written as a .graph chunk and read again (runs moved by the 4-bit row shifts), searched in
    asymmetric mode: the frontier holds the cells outside A alone; the restatement walks the decoded runs."""
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
    assert st["vga_asym_mode"] == 1 and st["vga_asym_nodes"] > 0 and st["vga_hard_cells"] > 0, st
    assert st["vga_c_cert_cells"] > 0, st
    g.close()
    g0.close()


def test_special_entries_are_never_rejected(ctx, monkeypatch):
    """Shape 8b: syn256 has 4 asymmetric nodes; around them the hard lists hold special entries (their in-set includes
    Extra: never rejected) next to regular ones.  With, without the certificate and the v1 top-down kernel agree."""
    _clean(monkeypatch)
    lines = np.loadtxt(os.path.join(GOLDEN, "inputs", "syn256.csv"), delimiter=",", skiprows=1)
    pm = dmx.PointMap([0.0, 0.0, 256.0, 256.0], lines, 1.0)
    assert pm.make_points(0.5, 0.5)
    g = pm.make_graph(ctx)
    ranges = [(21900, 22100), (34000, 34200), (48050, 48200)]
    outs, stats, nspec = [], [], 0
    for (b, e) in ranges:
        outs.append(g.vga_visual_global(src_begin=b, src_end=e, levels=True))
        st = ctx.last_stats()
        assert st["vga_kernel"] == "tile-resolved" and st["vga_special_nodes"] == 4, st
        _ordered(st)
        nspec += st["vga_n_spec"]
        stats.append(st)
    assert nspec > 0, nspec
    assert sum(st["vga_c_cert_cells"] for st in stats) > 0, stats
    monkeypatch.setenv("DMX_VGA_CCERT", "0")
    for (b, e), (o, lv), st in zip(ranges, outs, stats):
        o0, lv0 = g.vga_visual_global(src_begin=b, src_end=e, levels=True)
        st0 = ctx.last_stats()
        assert st0["vga_c_cert_cells"] == 0 and st0["vga_n_spec"] == st["vga_n_spec"], (st, st0)
        np.testing.assert_array_equal(lv[b:e], lv0[b:e])
        np.testing.assert_array_equal(o[b:e].view(np.uint32), o0[b:e].view(np.uint32))
    monkeypatch.delenv("DMX_VGA_CCERT")
    monkeypatch.setenv("DMX_VGA_KERNEL", "v1")
    g2 = pm.make_graph(ctx)
    for (b, e), (o, lv) in zip(ranges, outs):
        o2, lv2 = g2.vga_visual_global(src_begin=b, src_end=e, levels=True)
        np.testing.assert_array_equal(lv[b:e], lv2[b:e])
        np.testing.assert_array_equal(o[b:e].view(np.uint32), o2[b:e].view(np.uint32))
    g2.close()
    g.close()


def test_absent_with_the_frontier_in_hbm(ctx, monkeypatch):
    """Shape 9a: 20,449 tiles: the frontier in HBM, wide rows: no certificate."""
    region, lines, sp = make_room_map(1136.0, 64.0, 60, 9, centre=(512.0, 1024.0))
    st, st0, pm, N = _map_case(ctx, monkeypatch, region, lines, sp, -1)
    assert st["vga_threads"] == 1024 and st["vga_frontier_hbm"] == 1, st
    assert st["vga_c_cert_cells"] == 0, st


def test_absent_without_masks(ctx, monkeypatch, dense):
    """Shape 9b: DMX_VGA_PMASK=0: phase C scans the runs behind its row pass: no certificate."""
    st, st0, pm, N = _map_case(ctx, monkeypatch, dense.region, dense.lines, dense.sp, -1,
                               env=[("DMX_VGA_PMASK", "0")], om=dense.om)
    assert "masks" not in st["vga_prep"] and st["vga_pmask_cells"] == 0, st
    assert st["vga_c_cert_cells"] == 0 and st["vga_hard_cells"] > 0, st


@pytest.mark.parametrize("switch", [("DMX_VGA_BSPLIT", "0"), ("DMX_VGA_BSPLIT", "3")])
def test_next_to_phase_b_fused_and_staged(ctx, monkeypatch, dense, switch):
    """Shape 10: the dense map with phase B fused and staged (the default, named): the same bits as the default run;
    the hard lists differ with the order of the tests, the certificate's outcome for a cell does not."""
    st, st0, pm, N = _map_case(ctx, monkeypatch, dense.region, dense.lines, dense.sp, -1, om=dense.om, switch=switch)
    assert st["vga_b_tiles"] > 0 and st["vga_tt_tiles"] > 0, st
    assert st["vga_c_cert_cells"] > 0 and st0["vga_c_cert_cells"] > 0, (st, st0)
