"""VGA global on a graph read back from a .graph PointMap chunk (the CLI drop-in: VISPREP writes the map, the VGA
step reads it).  PixelVec::write stores a bin's runs after the first as a 4-bit row shift (salalib/ngraph.cpp:
536-583), so a jump of more than 15 rows moves the later runs of the bin, and Bin::write drops the runs of a bin of
65536 k cells (:447-472): the re-read graph is asymmetric, at 1000^2 in 996,278 of 998,001 nodes.  The reference's
VGA walks it as it is (vgavisualglobal.cpp:96-128).

The engine's asymmetric mode (dmx_graph_set_drawing; vga_tile.hip) makes the map's graph again from the drawing as
a symmetric reference R, runs the tile search on R with the frontier limited to cells outside A (the nodes whose
re-read runs differ from R's, plus R's own asymmetric nodes) and lets A's frontier cells push their re-read runs.
Checked here on the golden maps written and re-read through the chunk codec, every source, against the oracle's
BFS over the same decoded runs (node counts exact, floats within 1e-6), at radius n and 3; the mode is forced
(DMX_VGA_ASYM) where the in-set correction lists would otherwise take the few asymmetric nodes.

The mode keeps its preparation (the reference graph, A) on the graph, so the tests below also change the graph after
it has been analysed -- links set and cleared (on a re-read and on an in-memory graph), a wrong drawing and then the
right one -- and run the mode with the frontier in HBM (a grid past the LDS frontier bitmap), over source ranges and
through the source-list entry, and check that the reference graph's makeGraph leaves the context's makeGraph figures
alone.  Where the whole-map oracle BFS would take too long, the oracle runs over a sample of sources that holds every
node the case is about (moved, linked) and a spread of the rest; two engine paths are compared bit for bit.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import depthmapx_amd as dmx
from depthmapx_amd import graphio
from golden_io import case_input_lines, load_case

pytestmark = pytest.mark.gpu

MAKEGRAPH_COLUMNS = ["Connectivity", "Point First Moment", "Point Second Moment"]
NO_LINKS = np.zeros((0, 2), dtype=np.int32)


def _reread_map(ctx, region, lines, spacing, fills, drawing=None):
    """Make the map's graph, write it as a chunk and load the chunk again (with `drawing`, default the map's lines)."""
    pm = dmx.PointMap(region, lines, spacing)
    for f in fills:
        assert pm.make_points(*f)
    g = pm.make_graph(ctx)
    c = g.copy(runs=True)
    cols = [(n, c["attrs"][:, i], False) for i, n in enumerate(MAKEGRAPH_COLUMNS)]
    blob = graphio.write_chunk(pm, c["bins"], c["runs"], c["gridconn"], cols)
    info = graphio.read_chunk(blob)
    same = len(info["runs"]) == len(c["runs"])
    moved = int(np.any(info["runs"] != c["runs"], axis=1).sum()) if same else -1
    # the nodes that own a moved run (runs are stored by node)
    node_of_run = np.repeat(np.arange(len(c["bins"])), c["bins"][:, :, 3].sum(axis=1))
    info["moved_nodes"] = np.unique(node_of_run[np.any(info["runs"] != c["runs"], axis=1)]) if same else None
    info["blob"] = blob
    pm2, g2 = graphio.load_chunk(ctx, blob, region, lines=lines if drawing is None else drawing)
    return info, g2, moved, (pm, g, pm2)


def _reread(ctx, name, drawing=None):
    meta, _ = load_case(name)
    lines = case_input_lines(meta)
    info, g2, moved, keep = _reread_map(ctx, meta["region"], lines, meta["spacing"], meta["fills"], drawing)
    return meta, info, g2, moved, keep


def _oracle(info):
    from pyoracle import OracleMap
    om = OracleMap.from_grid(info["cols"], info["rows"], info["spacing"], info["bottom_left"], info["state"])
    om.set_graph(info["bins"], info["runs"])
    return om


def _oracle_sample(om, src, radius):
    """The oracle's BFS from the listed sources: its [N][7] rows (vga_global_sample) and, for the level columns
    the sample entry does not return, {source: (node count, total depth)} of up to 48 of them."""
    ref, _ = om.vga_global_sample(src, radius=radius, threads=16)

    def one(k):
        _, lv = om.vga_global(radius=radius, node_begin=int(k), node_end=int(k) + 1, levels=True)
        return int(k), lv[k, :2].copy()
    with ThreadPoolExecutor(16) as ex:
        lv = dict(ex.map(one, src[:48]))
    return ref, lv


def _assert_equals_oracle(got, lv, ref, rlv, src):
    """The project's comparison over the sources `src`: level columns and node counts exact, floats within 1e-6."""
    for k, want in rlv.items():
        np.testing.assert_array_equal(lv[k, :2], want, err_msg="levels of source %d" % k)
    np.testing.assert_array_equal(got[src, 5], ref[src, 5])
    assert np.allclose(got[src], ref[src], rtol=1e-6, atol=1e-6), float(np.abs(got[src] - ref[src]).max())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", ["syn128", "barnsbury"])
def test_vga_on_reread_graph_asymmetric_mode_equals_oracle(ctx, monkeypatch, name):
    meta, info, g2, moved, keep = _reread(ctx, name)
    assert moved > 0, "the round trip moved no run: nothing to test"
    om = _oracle(info)
    monkeypatch.setenv("DMX_VGA_ASYM", "1")
    for radius in (-1, 3):
        got, lv = g2.vga_visual_global(radius=radius, levels=True)
        st = ctx.last_stats()
        assert st["vga_kernel"] == "tile-resolved" and st["vga_asym_mode"] == 1, st
        assert st["vga_asym_nodes"] > 0, st
        ref, rlv = om.vga_global(radius=radius, threads=16, levels=True)
        np.testing.assert_array_equal(lv[:, :2], rlv[:, :2])
        np.testing.assert_array_equal(got[:, 5], ref[:, 5])
        assert np.allclose(got, ref, rtol=1e-6, atol=1e-6)
    # the same graph without the mode (the in-set correction lists where the asymmetric nodes are few, else the
    # top-down search) gives the same bits
    asym = g2.vga_visual_global(radius=-1)
    monkeypatch.delenv("DMX_VGA_ASYM")
    monkeypatch.setenv("DMX_VGA_NOASYM", "1")
    plain = g2.vga_visual_global(radius=-1)
    assert ctx.last_stats()["vga_asym_mode"] == 0
    np.testing.assert_array_equal(asym.view(np.uint32), plain.view(np.uint32))


def _sources(*parts):
    """The parts joined, duplicates dropped, the order kept (the first 48 also get their level columns checked)."""
    s = np.concatenate([np.asarray(p, dtype=np.int64).ravel() for p in parts])
    _, first = np.unique(s, return_index=True)
    return s[np.sort(first)]


def _run(ctx, g, radius, asym):
    """VGA global with its level columns; asserts whether the asymmetric mode ran."""
    got, lv = g.vga_visual_global(radius=radius, levels=True)
    st = ctx.last_stats()
    assert st["vga_asym_mode"] == asym, st
    if asym:
        assert st["vga_kernel"] == "tile-resolved" and st["vga_asym_nodes"] > 0, st
    return got, lv


def _link_pairs(info, seed=7, nlinks=12):
    """`nlinks` disjoint pairs of filled cells: two with an end whose node's runs moved in the round trip, the
    others with both ends elsewhere.  Returns (pairs of x-major cells, the linked nodes)."""
    filled = np.flatnonzero(info["state"] & 2)   # node k <-> cell filled[k] (x-major)
    mv = info["moved_nodes"]
    rest = np.setdiff1d(np.arange(len(filled)), mv)
    rng = np.random.default_rng(seed)
    nm = min(2, len(mv))
    assert nm > 0
    ends = np.concatenate([rng.choice(mv, nm, replace=False), rng.choice(rest, 2 * nlinks - nm, replace=False)])
    # pair i < nm: (moved node, other node); the rest: both ends outside the moved nodes
    a = np.concatenate([ends[:nm], ends[2 * nm:nm + nlinks]])
    b = np.concatenate([ends[nm:2 * nm], ends[nm + nlinks:]])
    pairs_n = np.stack([a, b], axis=1)
    assert len(np.unique(pairs_n)) == 2 * nlinks
    assert np.isin(pairs_n, mv).any(axis=1).sum() == nm and (~np.isin(pairs_n, mv)).all(axis=1).any()
    return filled[pairs_n].astype(np.int32), np.sort(pairs_n.ravel())


_LINKED = {}


def _syn128_links(ctx):
    """syn128 re-read, a set of links and the oracle with those links over a sample of sources (every linked node,
    every moved node and a stride of the rest) at radius n and 3: made once, shared by the tests below, read only."""
    if not _LINKED:
        meta, info, g2, moved, keep = _reread(ctx, "syn128")
        assert moved > 0
        pairs, linked = _link_pairs(info)
        om = _oracle(info)
        om.set_merges(pairs)
        src = _sources(linked, info["moved_nodes"], np.arange(0, info["nnodes"], 127))
        _LINKED.update(meta=meta, info=info, lines=case_input_lines(meta), pairs=pairs, src=src,
                       ref={r: _oracle_sample(om, src, r) for r in (-1, 3)})
    return _LINKED


def _load(ctx, L):
    """A fresh graph from the re-read chunk, the drawing set (kept alive with its map)."""
    return graphio.load_chunk(ctx, L["info"]["blob"], L["meta"]["region"], lines=L["lines"])


def test_links_set_on_an_analysed_reread_graph(ctx, monkeypatch):
    """Links set on a re-read graph that already ran in the asymmetric mode are followed (the mode's reference graph
    has none, so the search leaves the mode), and clearing them brings the mode and the first result back."""
    monkeypatch.setenv("DMX_VGA_ASYM", "1")
    L = _syn128_links(ctx)
    pm2, g2 = _load(ctx, L)
    base = {r: _run(ctx, g2, r, asym=1) for r in (-1, 3)}
    g2.set_merges(L["pairs"])
    for r in (-1, 3):
        got, lv = g2.vga_visual_global(radius=r, levels=True)
        # the links change the result (the comparison with the oracle would hold vacuously otherwise)
        assert (lv[:, 1] != base[r][1][:, 1]).any(), "radius %d: the linked result is the unlinked one" % r
        _assert_equals_oracle(got, lv, *L["ref"][r], L["src"])
        assert ctx.last_stats()["vga_asym_mode"] == 0
    g2.set_merges(NO_LINKS)
    for r in (-1, 3):
        got, lv = _run(ctx, g2, r, asym=1)
        np.testing.assert_array_equal(_bits(got), _bits(base[r][0]))
        np.testing.assert_array_equal(lv, base[r][1])


def test_links_cleared_on_an_analysed_reread_graph(ctx, monkeypatch):
    """The opposite order: with links set before the first run the mode is refused (== the oracle with links);
    cleared, the mode runs and gives what a graph that never had links gives."""
    monkeypatch.setenv("DMX_VGA_ASYM", "1")
    L = _syn128_links(ctx)
    pm2, g2 = _load(ctx, L)
    base = {r: _run(ctx, g2, r, asym=1) for r in (-1, 3)}
    pm3, g3 = _load(ctx, L)
    g3.set_merges(L["pairs"])
    for r in (-1, 3):
        got, lv = _run(ctx, g3, r, asym=0)
        _assert_equals_oracle(got, lv, *L["ref"][r], L["src"])
    g3.set_merges(NO_LINKS)
    for r in (-1, 3):
        got, lv = _run(ctx, g3, r, asym=1)
        np.testing.assert_array_equal(_bits(got), _bits(base[r][0]))
        np.testing.assert_array_equal(lv, base[r][1])


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("kernel", ["tile", "do"])
def test_links_changed_on_an_analysed_graph(ctx, monkeypatch, seed, kernel):
    """An in-memory graph made without links and analysed, then given links (== the oracle with links, every
    source), then cleared of them (== the first result, bit for bit): the links' device state follows
    dmx_graph_set_merges across a search preparation that is already made."""
    from test_merge_links import _synthetic
    if kernel == "do":
        monkeypatch.setenv("DMX_VGA_KERNEL", "do")
    pm, om, pairs = _synthetic(seed)
    g = pm.make_graph(ctx)
    om.make_graph()
    plain = {r: g.vga_visual_global(radius=r, levels=True) for r in (-1, 3)}
    assert ctx.last_stats()["vga_kernel"] == ("tile-resolved" if kernel == "tile" else "direction-optimizing")
    g.set_merges(pairs)
    om.set_merges(pairs)
    for r in (-1, 3):
        got, lv = g.vga_visual_global(radius=r, levels=True)
        ref, rlv = om.vga_global(radius=r, threads=8, levels=True)
        np.testing.assert_array_equal(lv[:, :2], rlv[:, :2])
        np.testing.assert_array_equal(got[:, 5], ref[:, 5])
        assert np.allclose(got, ref, rtol=1e-6, atol=1e-6)
        assert (lv[:, 1] != plain[r][1][:, 1]).any()
    g.set_merges(NO_LINKS)
    for r in (-1, 3):
        got, lv = g.vga_visual_global(radius=r, levels=True)
        np.testing.assert_array_equal(_bits(got), _bits(plain[r][0]))
        np.testing.assert_array_equal(lv, plain[r][1])


def test_wrong_then_right_drawing(ctx, monkeypatch):
    """A drawing that is not the map's (its lines shifted by 0.37 of the spacing): the mode is refused and the
    fallback search answers what the oracle does; the map's own drawing set afterwards replaces the refusal, and the
    mode's result equals the fallback's bit for bit."""
    monkeypatch.setenv("DMX_VGA_ASYM", "1")
    meta, _ = load_case("syn128")
    lines = case_input_lines(meta)
    meta, info, g2, moved, keep = _reread(ctx, "syn128", drawing=lines + 0.37 * meta["spacing"])
    assert moved > 0
    fallback, flv = _run(ctx, g2, -1, asym=0)
    src = _sources(info["moved_nodes"], np.arange(0, info["nnodes"], 127))
    ref, rlv = _oracle_sample(_oracle(info), src, -1)
    _assert_equals_oracle(fallback, flv, ref, rlv, src)
    g2.set_drawing(lines)
    got, lv = _run(ctx, g2, -1, asym=1)
    np.testing.assert_array_equal(_bits(got), _bits(fallback))
    np.testing.assert_array_equal(lv, flv)


def test_asymmetric_mode_with_the_frontier_in_hbm(ctx, monkeypatch):
    """A 1137^2 grid (20,449 tiles: the frontier bitmap no longer fits the LDS beside the summaries, so it lives in
    per-workgroup HBM slices and the A cells' pushes are read back from there) with one walled room of 3,959 nodes,
    10 of them moved by the round trip: the mode against the oracle over the decoded runs on the moved nodes, their
    neighbours in node order and seeded random nodes, and a block of sources against the same graph without the
    mode."""
    from golden.gen_synthetic import make_room_map
    region, lines, sp = make_room_map(1136.0, 64.0, 60, seed=9)
    info, g2, moved, keep = _reread_map(ctx, region, lines, 1.0, [sp])
    assert moved > 0, "the round trip moved no run: nothing to test"
    N, mv = info["nnodes"], info["moved_nodes"]
    assert 0 < len(mv) <= N // 4
    # the decoded runs stay on the grid (the A cells rasterise them as they are)
    r = info["runs"]
    assert r.min() >= 0 and r[:, [0, 2]].max() < info["cols"] and r[:, [1, 3]].max() < info["rows"]
    # the engine's layout rule (tile_lds_layout): frontier bitmap + tile summaries + level histogram past the LDS
    tw, th = (info["cols"] + 7) // 8, (info["rows"] + 7) // 8
    wr, wc = (tw + 63) // 64, (th + 63) // 64
    assert tw * th * 8 + (th * wr + tw * wc) * 8 + 64 * 4 > 159 * 1024
    rng = np.random.default_rng(9)
    near = np.concatenate([np.arange(max(k - 64, 0), min(k + 65, N)) for k in mv])
    src = _sources(mv, near, rng.choice(N, 256, replace=False))
    om = _oracle(info)
    monkeypatch.setenv("DMX_VGA_ASYM", "1")
    for radius in (-1, 3):
        got, lv = _run(ctx, g2, radius, asym=1)
        assert ctx.last_stats()["vga_frontier_hbm"] == 1
        ref, rlv = _oracle_sample(om, src, radius)
        _assert_equals_oracle(got, lv, ref, rlv, src)
        if radius == -1:
            asym = got
    b = min(max(int(mv[len(mv) // 2]) - 256, 0), N - 512)
    monkeypatch.delenv("DMX_VGA_ASYM")
    monkeypatch.setenv("DMX_VGA_NOASYM", "1")
    plain = g2.vga_visual_global(radius=-1, src_begin=b, src_end=b + 512)
    st = ctx.last_stats()
    assert st["vga_asym_mode"] == 0 and st["vga_sources"] == 512, st
    np.testing.assert_array_equal(_bits(plain[b:b + 512]), _bits(asym[b:b + 512]))


def test_source_ranges_and_source_list_on_a_reread_graph(ctx, monkeypatch):
    """The mode over source ranges (exactly the range's rows written, each equal to the full run's) and the
    source-list entry on the same graph (the listed rows equal the mode's full run, the others untouched)."""
    import torch
    monkeypatch.setenv("DMX_VGA_ASYM", "1")
    meta, info, g2, moved, keep = _reread(ctx, "syn128")
    assert moved > 0
    N, mv = info["nnodes"], info["moved_nodes"]
    full, _ = _run(ctx, g2, -1, asym=1)
    m = int(mv[len(mv) // 2])
    a = (max(m - 100, 0), min(m + 201, N))              # around a moved node
    b = (N - 300, N) if a[1] <= N - 300 else (0, 300)   # an end of the node order, apart from it
    for (sb, se) in (a, b):
        part = g2.vga_visual_global(radius=-1, src_begin=sb, src_end=se)
        st = ctx.last_stats()
        assert st["vga_asym_mode"] == 1 and st["vga_sources"] == se - sb, st
        np.testing.assert_array_equal(_bits(part[sb:se]), _bits(full[sb:se]))
        assert (part[:sb] == -1.0).all() and (part[se:] == -1.0).all()
    rng = np.random.default_rng(5)
    nodes = np.unique(np.concatenate([mv[:16], np.arange(500, 564), rng.choice(N, 40, replace=False)]))
    out = torch.full((N, 7), -7.0, dtype=torch.float32, device="cuda")
    g2.vga_visual_global_device_list(out.data_ptr(), nodes)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    np.testing.assert_array_equal(_bits(got[nodes]), _bits(full[nodes]))
    assert (got[np.setdiff1d(np.arange(N), nodes)] == -7.0).all()


def test_makegraph_figures_survive_a_vga_call(ctx, monkeypatch):
    """The asymmetric mode makes its reference graph inside the VGA call: the context's makeGraph timing, counters
    and re-run list stay those of the caller's own makeGraph."""
    monkeypatch.setenv("DMX_VGA_ASYM", "1")
    meta, _ = load_case("syn128")
    lines = case_input_lines(meta)
    pm = dmx.PointMap(meta["region"], lines, meta["spacing"])
    for f in meta["fills"]:
        assert pm.make_points(*f)
    g = pm.make_graph(ctx)

    def figures():
        st = ctx.last_stats()
        return (ctx.last_timing()[0], {k: v for k, v in st.items() if k.startswith("mk_")},
                [a.tolist() for a in ctx.last_mk_reruns()])
    before = figures()
    assert before[0] > 0 and before[1]["mk_runs"] == g.info()["nruns"]
    assert sorted(before[1]) == ["mk_cells_examined", "mk_chunks", "mk_depth_steps", "mk_diag_inexact", "mk_reruns",
                                 "mk_runs", "mk_visible_pairs"]
    c = g.copy(runs=True)
    cols = [(n, c["attrs"][:, i], False) for i, n in enumerate(MAKEGRAPH_COLUMNS)]
    blob = graphio.write_chunk(pm, c["bins"], c["runs"], c["gridconn"], cols)
    pm2, g2 = graphio.load_chunk(ctx, blob, meta["region"], lines=lines)
    assert figures() == before
    _run(ctx, g2, -1, asym=1)   # (builds the reference graph)
    assert figures() == before
