"""makeGraph's two options end to end on the GPU: `maxdist` (-pr: sight blocked past a length; the MAXD variants
of makegraph_kernel and, after a capacity overflow, the generic kernel with the test read at run time) and
`boundarygraph` (-pb: every cell without the EDGE bit unfilled before the sweep).

The fixtures come from the reference built from source (tests/golden/make_golden.py OPTION_CASES): syn32 at maxdist
5.0 and gallery at 1.0 (25 cells of 0.04), both tie radii -- thousands of cell pairs lie exactly at them (3-4-5,
7-24-25) or, on gallery's inexact coordinates, within an ulp or two either side, so `>=` for `>` in the kernel's
test or a length one ulp off changes the graph (tests/test_oracle_golden.py::test_option_radii_are_tie_radii pins
that on the CPU) -- and the boundary graphs of both maps (315 of 961 and 1772 of 4332 nodes, scattered in the grid,
most of their runs single cells).  Where the probe made no fixture the C restatement (oracle/, pinned to the same
fixtures on the CPU) is the reference.

Bars as in test_gpu_parity.py: everything integer, the makeGraph attributes and the bit-exact analyses bit for bit;
VGA global floats within VGA_RTOL with the exact share asserted."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import depthmapx_amd as dmx
import thruvision_model as tvm
from depthmapx_amd import graphio
from golden_io import GOLDEN, case_input_lines, load_case, node_digests
from test_gpu_parity import _assert_stepdepth, _assert_vga_close

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OPTION_CASES = ["syn32_md5", "syn32_b", "syn32_b_md5", "gallery_md1", "gallery_b"]
ANALYSIS_CASES = ["syn32_b", "gallery_b", "syn32_md5", "gallery_md1"]
BOUNDARY_CASES = ["syn32_b", "gallery_b"]
CAPACITY_HOOKS = [{"DMX_MK_GCAP": "2", "DMX_MK_BCAP": "2"}, {"DMX_MK_GCAP": "128", "DMX_MK_BCAP": "2", "DMX_MK_SPILL": "2"}]
BIN_DIR = [4 if b in (4, 20) else 8 if b in (12, 28) else 2 if (4 < b < 12 or 20 < b < 28) else 1 for b in range(32)]

_cases, _oracles, _graphs = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _graphs.clear()
    _oracles.clear()
    _cases.clear()


def _case(name):
    if name not in _cases:
        _cases[name] = load_case(name)
    return _cases[name]


def _map(meta, ctx=None):
    """The filled map before makeGraph; with a context the fill runs on the GPU."""
    pm = dmx.PointMap(meta["region"], case_input_lines(meta), meta["spacing"])
    for f in meta["fills"]:
        assert pm.make_points(*f, ctx=ctx)
    return pm


def _make(ctx, pm, meta, **kw):
    return pm.make_graph(ctx, boundarygraph=meta["boundary"], maxdist=meta["maxdist"], **kw)


def _graph(ctx, name):
    """(map, graph) of an option case made with its options: once per module, only read by the tests."""
    if name not in _graphs:
        meta, _ = _case(name)
        pm = _map(meta)
        _graphs[name] = (pm, _make(ctx, pm, meta))
    return _graphs[name]


def _oracle_map(meta, maxdist=None, boundary=None):
    from pyoracle import OracleMap
    om = OracleMap(meta["region"], meta["spacing"], case_input_lines(meta))
    for f in meta["fills"]:
        assert om.fill(*f)
    om.make_graph(maxdist=meta.get("maxdist", -1.0) if maxdist is None else maxdist,
                  boundary=meta.get("boundary", False) if boundary is None else boundary, threads=16)
    return om


def _oracle(name):
    """The restatement's map of an option case with its graph made: once per module, only read."""
    if name not in _oracles:
        _oracles[name] = _oracle_map(_case(name)[0])
    return _oracles[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_fixture(ctx, pm, g, name):
    """The bar of (a): counts, bins, runs or digests, attributes as bits, grid connections, the map's states and
    filled count after the call."""
    meta, A = _case(name)
    info = g.info()
    assert info["nnodes"] == meta["nodes"] and info["nruns"] == meta["runs"]
    got = g.copy(runs=True)
    assert ("bins" in A) == meta["full_runs"]
    if "bins" in A:
        np.testing.assert_array_equal(got["bins"], A["bins"])
        np.testing.assert_array_equal(got["runs"], A["runs"])
    np.testing.assert_array_equal(got["bins"][:, :, 3].sum(axis=1), A["nruns"])
    np.testing.assert_array_equal(node_digests(got["bins"], got["runs"]), A["digests"])
    np.testing.assert_array_equal(_bits(got["attrs"]), _bits(A["attrs"]))
    np.testing.assert_array_equal(got["gridconn"], A["gridconn"])
    np.testing.assert_array_equal(pm.state(), A["state"])
    assert pm.info()["filled"] == meta["nodes"]
    return got


def _assert_same_graph(got, ref):
    np.testing.assert_array_equal(got["bins"], ref["bins"])
    np.testing.assert_array_equal(got["runs"], ref["runs"])
    np.testing.assert_array_equal(_bits(got["attrs"]), _bits(ref["attrs"]))
    np.testing.assert_array_equal(got["gridconn"], ref["gridconn"])


# ---------------------------------------------------------------- (a) parity with the fixtures
@pytest.mark.parametrize("name", OPTION_CASES)
def test_option_graph_matches_reference(ctx, name):
    meta, A = _case(name)
    pm = _map(meta)
    before = pm.state()
    assert meta["boundary"] == bool((before != A["state"]).any())   # FILLED cleared, and only by the boundary option
    g = _make(ctx, pm, meta)
    first = _assert_fixture(ctx, pm, g, name)
    cleared = before != A["state"]
    assert ((before[cleared] & 2) != 0).all() and (A["state"][cleared] == (before[cleared] & ~2)).all()
    # a second call on the same map (its cells are already unfilled) gives the same graph
    g2 = _make(ctx, pm, meta)
    _assert_same_graph(_assert_fixture(ctx, pm, g2, name), first)
    # and so does a map whose fill ran on the GPU
    pmd = _map(meta, ctx=ctx)
    np.testing.assert_array_equal(pmd.state(), before)
    _assert_fixture(ctx, pmd, _make(ctx, pmd, meta), name)


# ---------------------------------------------------------------- (b) one ulp either side of the tie radii
def _side(radius, side):
    return {"below": float(np.nextafter(radius, 0.0)), "at": radius, "above": float(np.nextafter(radius, np.inf))}[side]


def _assert_equals_oracle_at(ctx, meta, maxdist):
    pm = _map(meta)
    g = pm.make_graph(ctx, maxdist=maxdist)
    ref = _oracle_map(meta, maxdist=maxdist, boundary=False).graph()
    _assert_same_graph(g.copy(runs=True), ref)
    return ref


@pytest.mark.parametrize("side", ["below", "at", "above"])
@pytest.mark.parametrize("base,radius", [("syn32", 5.0), ("gallery", 1.0)])
def test_one_ulp_either_side_of_the_radius(ctx, base, radius, side):
    meta, _ = _case(base)
    _assert_equals_oracle_at(ctx, meta, _side(radius, side))


@pytest.mark.parametrize("hooks", CAPACITY_HOOKS, ids=["gcap2", "spill2"])
@pytest.mark.parametrize("side", ["below", "at", "above"])
def test_one_ulp_either_side_in_the_capacity_reruns(ctx, monkeypatch, side, hooks):
    """After a capacity overflow the sources run again in the generic kernel, which reads the maxdist test at run
    time: the place where that kernel meets a tie."""
    meta, _ = _case("syn32")
    for k, v in hooks.items():
        monkeypatch.setenv(k, v)
    _assert_equals_oracle_at(ctx, meta, _side(5.0, side))
    if hooks["DMX_MK_GCAP"] == "2":
        assert len(ctx.last_mk_reruns()[1]) > 0, "no source overflowed a capacity: the generic kernel did not run"


# ---------------------------------------------------------------- (c) every makeGraph path under maxdist
MK_PATHS = {"gcap2": CAPACITY_HOOKS[0], "spill2": CAPACITY_HOOKS[1], "exact": {"DMX_MK_EXACT": "1"},
            "sqrt_bad": {"DMX_MK_SQRT_BAD": "1"}, "nosym": {"DMX_MK_NOSYM": "1"}, "sample": {"DMX_MK_SAMPLE": "1"}}


# the sample pass needs kMkSample (4096) nodes: gallery_md1 (4332) only
@pytest.mark.parametrize("name,path", [(n, p) for n in ("syn32_md5", "gallery_md1") for p in MK_PATHS
                                       if p != "sample" or n == "gallery_md1"])
def test_makegraph_paths_under_maxdist(ctx, monkeypatch, name, path):
    meta, A = _case(name)
    assert path != "sample" or meta["nodes"] >= 4096
    for k, v in MK_PATHS[path].items():
        monkeypatch.setenv(k, v)
    pm = _map(meta)
    g = _make(ctx, pm, meta)
    _assert_fixture(ctx, pm, g, name)
    if path == "gcap2":
        assert len(ctx.last_mk_reruns()[1]) > 0, "no source overflowed a capacity: the generic kernel did not run"
    if path == "nosym":
        # the symmetry scatter is left to the VGA preparation: same result as the graph that did it in makeGraph
        monkeypatch.delenv("DMX_MK_NOSYM")
        want, wlv = _graph(ctx, name)[1].vga_visual_global(radius=3, levels=True)
        got, lv = g.vga_visual_global(radius=3, levels=True)
        np.testing.assert_array_equal(lv, wlv)
        np.testing.assert_array_equal(_bits(got), _bits(want))


def test_makegraph_profiling_kernel_under_maxdist(ctx, tmp_path):
    """DMX_VERBOSE=1 selects the kernels with per-phase clocks (under maxdist the generic one); the flag is read
    once per process, so a child process makes gallery_md1's graph and hands it back."""
    meta, A = _case("gallery_md1")
    out = str(tmp_path / "graph.npz")
    code = ("import sys; sys.path[:0] = %r\n"
            "import numpy as np\n"
            "import depthmapx_amd as dmx\n"
            "from golden_io import load_case, case_input_lines\n"
            "meta, A = load_case('gallery_md1')\n"
            "pm = dmx.PointMap(meta['region'], case_input_lines(meta), meta['spacing'])\n"
            "[pm.make_points(*f) for f in meta['fills']]\n"
            "g = pm.make_graph(dmx.Context(0), maxdist=meta['maxdist'])\n"
            "np.savez(%r, state=pm.state(), **g.copy(runs=True))\n") % ([os.path.dirname(HERE), HERE], out)
    env = dict(os.environ, DMX_VERBOSE="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "makegraph:" in r.stderr          # the verbose log: the flag was in force
    got = np.load(out)
    assert len(got["bins"]) == meta["nodes"] and len(got["runs"]) == meta["runs"]
    np.testing.assert_array_equal(node_digests(got["bins"], got["runs"]), A["digests"])
    np.testing.assert_array_equal(_bits(got["attrs"]), _bits(A["attrs"]))
    np.testing.assert_array_equal(got["gridconn"], A["gridconn"])
    np.testing.assert_array_equal(got["state"], A["state"])


@pytest.mark.parametrize("shape", [(1300, 5), (6, 1300)])
def test_far_rows_under_maxdist_match_oracle(ctx, shape):
    """MAXD x FAR: the corridors of test_far_rows_past_lds_match_oracle (rows past MK_OPEN_LDS) at maxdist 1100.0.
    On the integer grid the cell 1100 along the axis is an exact tie: seen, the one after it not."""
    from pyoracle import OracleMap
    W, H = shape
    rng = np.random.default_rng(5)
    lines = []
    for _ in range(6):
        x = rng.uniform(0.1, 0.9) * W
        y = rng.uniform(0.1, 0.9) * H
        lines.append([x, y, x + (0.7 if W > H else 0.3), y + (0.3 if W > H else 0.7)])
    lines = np.array(lines, dtype=np.float64)
    region = [0.0, 0.0, float(W), float(H)]
    pm = dmx.PointMap(region, lines, 1.0)
    om = OracleMap(region, 1.0, lines)
    assert pm.make_points(0.5, 0.5) == om.fill(0.5, 0.5)
    g = pm.make_graph(ctx, maxdist=1100.0)
    om.make_graph(maxdist=1100.0, threads=16)
    got = g.copy(runs=True)
    _assert_same_graph(got, om.graph())
    runs = got["runs"].astype(np.int64)
    a = 0 if W > H else 1                                    # the long axis
    assert 1024 < np.abs(runs[:, a] - runs[:, a + 2]).max() <= 1100
    # some source's run along its own row ends exactly 1100 cells away (the tie, seen) and none ends farther
    cells = np.flatnonzero(pm.state() & 2)
    src = np.stack([cells // pm.rows, cells % pm.rows], axis=1)[np.repeat(np.arange(len(cells)),
                                                                          got["bins"][:, :, 3].sum(axis=1))]
    reach = np.maximum(np.abs(runs[:, a] - src[:, a]), np.abs(runs[:, a + 2] - src[:, a]))
    on_axis = (runs[:, 1 - a] == src[:, 1 - a]) & (runs[:, 3 - a] == src[:, 1 - a])
    assert reach.max() == 1100 and (reach[on_axis] == 1100).any()


# ---------------------------------------------------------------- (d) ranges, shards and balance
def _assemble(ctx, pm, meta, bounds, **kw):
    import torch
    blobs = []
    for b, e in zip(bounds, bounds[1:]):
        s = pm.make_graph(ctx, node_begin=b, node_end=e, **kw)
        t = torch.empty(s.blob_size(), dtype=torch.uint8, device="cuda:0")
        s.write_blob_device(t.data_ptr(), t.numel())
        blobs.append(t)
        s.close()
    torch.cuda.synchronize()
    return pm.assemble(ctx, [t.data_ptr() for t in blobs], [t.numel() for t in blobs])


@pytest.mark.parametrize("name", ["gallery_b", "gallery_md1", "syn32_b_md5"])
def test_option_shards_assemble_to_whole_graph(ctx, name):
    meta, A = _case(name)
    pm = _map(meta)
    n = meta["nodes"]            # node ranges count the nodes of the graph the options make
    g = _assemble(ctx, pm, meta, [0, n // 3, (2 * n) // 3, n], boundarygraph=meta["boundary"], maxdist=meta["maxdist"])
    _assert_fixture(ctx, pm, g, name)


def test_shard_bounds_with_both_options(ctx):
    """dmx_makegraph_balance with boundary and maxdist on a fresh map: it unfills the cells itself, its cost sample
    takes the generic counting kernel with the maxdist test, and the bounds cover the boundary graph's nodes."""
    meta, A = _case("gallery_b")
    pm = _map(meta)
    b = pm.shard_bounds(ctx, 4, stride=7, boundarygraph=True, maxdist=1.0)
    assert len(b) == 5 and b[0] == 0 and b[-1] == meta["nodes"] == 1772
    assert all(x <= y for x, y in zip(b, b[1:])) and len(set(b)) > 2
    assert pm.shard_bounds(ctx, 4, stride=7, boundarygraph=True, maxdist=1.0) == b
    np.testing.assert_array_equal(pm.state(), A["state"])
    assert pm.info()["filled"] == meta["nodes"]
    # the shards the bounds cut, made without maxdist, are gallery_b
    g = _assemble(ctx, pm, meta, b, boundarygraph=True)
    _assert_fixture(ctx, pm, g, "gallery_b")


# ---------------------------------------------------------------- (e) every analysis on the option graphs
def _fixture_or(name, suffix, compute):
    path = os.path.join(GOLDEN, name + suffix + ".npy")
    return np.load(path) if os.path.exists(path) else compute()


@pytest.mark.parametrize("name", ANALYSIS_CASES)
def test_vga_global_on_option_graphs(ctx, name):
    meta, A = _case(name)
    pm, g = _graph(ctx, name)
    om = _oracle(name)
    for radius in (3, 2, -1):
        out, lv = g.vga_visual_global(radius=radius, levels=True)
        ref, rlv = om.vga_global(radius=radius, threads=16, levels=True)
        np.testing.assert_array_equal(lv[:, :2], rlv[:, :2])
        want = A["vga"] if radius == -1 else ref
        exact = _assert_vga_close(out, want)
        np.testing.assert_array_equal(out[:, 5], want[:, 5])
        assert exact > 0.99
    # a source range (radius n): its rows equal the full run's, the others stay untouched
    n = meta["nodes"]
    b, e = n // 3, n // 3 + 97
    part = g.vga_visual_global(src_begin=b, src_end=e)
    np.testing.assert_array_equal(_bits(part[b:e]), _bits(out[b:e]))
    assert (part[:b] == -1).all() and (part[e:] == -1).all()


@pytest.mark.parametrize("kernel", ["v1", "topdown", "do"])
def test_vga_kernels_agree_on_the_boundary_graph(ctx, kernel, monkeypatch):
    meta, A = _case("gallery_b")
    pm, g = _graph(ctx, "gallery_b")
    want, wlv = g.vga_visual_global(levels=True)
    assert ctx.last_stats()["vga_kernel"] == "tile-resolved"
    monkeypatch.setenv("DMX_VGA_KERNEL", kernel)
    g2 = pm.make_graph(ctx, boundarygraph=True)
    got, lv = g2.vga_visual_global(levels=True)
    assert ctx.last_stats()["vga_kernel"] != "tile-resolved"
    np.testing.assert_array_equal(lv, wlv)
    np.testing.assert_array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("name", ANALYSIS_CASES)
def test_vga_local_metric_angular_on_option_graphs(ctx, name):
    """Bit for bit against the reference's columns where the probe made them (syn32_md5, syn32_b, gallery_b), else
    against the restatement: gallery_md1, whose metric and angular searches from all 4332 sources take the
    restatement seconds, over a block of 96 sources in the middle of the node order."""
    meta, _ = _case(name)
    pm, g = _graph(ctx, name)
    om = _oracle(name)
    n = meta["nodes"]
    b, e = (0, n) if os.path.exists(os.path.join(GOLDEN, name + "_vmetric.npy")) else (n // 2 - 48, n // 2 + 48)
    got = g.vga_visual_local()
    np.testing.assert_array_equal(_bits(got), _bits(_fixture_or(name, "_vlocal", lambda: om.vga_local(threads=16))))
    np.testing.assert_array_equal(_bits(got), _bits(om.vga_local(threads=16)))
    assert (got[:, 0] >= 0).any()
    finite = 10.0 if name.startswith("syn32") else 0.5
    for radius, suffix in ((-1.0, "_vmetric"), (finite, "_vmetric_r%g" % finite)):
        got = g.vga_metric(radius=radius, src_begin=b, src_end=e)
        want = _fixture_or(name, suffix, lambda: om.vga_metric(radius=radius, node_begin=b, node_end=e, threads=16))
        np.testing.assert_array_equal(_bits(got[b:e]), _bits(want[b:e]))
        assert (got[b:e, 3] > 1).any() and (got[:b] == -1).all() and (got[e:] == -1).all()
    assert (got[b:e, 3] < n).any()      # the finite radius cuts
    got = g.vga_angular(src_begin=b, src_end=e)
    want = _fixture_or(name, "_vangular", lambda: om.vga_angular(node_begin=b, node_end=e, threads=16))
    np.testing.assert_array_equal(_bits(got[b:e]), _bits(want[b:e]))
    assert (got[b:e, 2] > 1).any()


def _sel_cells(meta, A):
    sel = A["stepdepth_sel"]
    return (sel >> 16) * meta["rows"] + (sel & 0xFFFF)


@pytest.mark.parametrize("name", OPTION_CASES)
def test_step_depths_on_option_graphs(ctx, name):
    meta, A = _case(name)
    pm, g = _graph(ctx, name)
    om = _oracle(name)
    pts = [tuple(float(v) for v in p.split(",")) for p in meta["stepdepth"]]
    one = _sel_cells(meta, A)
    assert len(one) == 1 and (A["state"][one] & 2).all() and pm.pixelate(*pts[0]) == one[0]
    # from the fixture's node
    _assert_stepdepth(g.metric_step_depth(points=pts), A["stepdepth"])
    np.testing.assert_array_equal(_bits(g.visual_step_depth(points=pts)), _bits(A["vstepdepth"]))
    np.testing.assert_array_equal(_bits(g.angular_step_depth(points=pts)),
                                  _bits(np.load(os.path.join(GOLDEN, name + "_astepdepth.npy"))))
    assert (A["vstepdepth"] >= 1).sum() > 1
    # from three nodes, against the restatement (cells in PixelRef order = x-major order)
    nodes = np.flatnonzero(A["state"] & 2)
    three = np.sort(nodes[[len(nodes) // 7, len(nodes) // 2, len(nodes) - 5]])
    want3 = (om.metric_stepdepth(three), om.visual_stepdepth(three), om.angular_stepdepth(three))
    _assert_stepdepth(g.metric_step_depth(cells=three), want3[0])
    np.testing.assert_array_equal(_bits(g.visual_step_depth(cells=three)), _bits(want3[1]))
    np.testing.assert_array_equal(_bits(g.angular_step_depth(cells=three)), _bits(want3[2]))
    if not meta["boundary"]:
        return
    # a selection that names cells the boundary option unfilled: they are dropped like any unfilled cell (the
    # reference's setCurSel selects filled points only); a selection of nothing else is refused
    before = _map(meta).state()
    gone = np.flatnonzero(((before & 2) != 0) & ((A["state"] & 2) == 0))
    assert len(gone) > 2
    messy = np.concatenate([gone[:1], three[::-1], gone[-2:]])
    _assert_stepdepth(g.metric_step_depth(cells=messy), want3[0])
    np.testing.assert_array_equal(_bits(g.visual_step_depth(cells=messy)), _bits(want3[1]))
    np.testing.assert_array_equal(_bits(g.angular_step_depth(cells=messy)), _bits(want3[2]))
    for run in (g.metric_step_depth, g.visual_step_depth, g.angular_step_depth):
        with pytest.raises(dmx.DmxError):
            run(cells=gone[:2])


@pytest.mark.parametrize("name", BOUNDARY_CASES)
def test_through_vision_on_boundary_graphs(ctx, name):
    """The lines cross cells that are no longer nodes; only node rows are gathered."""
    meta, A = _case(name)
    pm, g = _graph(ctx, name)
    n = meta["nodes"]
    model = tvm.through_vision(meta["cols"], meta["rows"], A["state"], A["nruns"], _graph_runs(g, A))
    out, cnt = g.vga_through_vision(counts=True)
    assert len(cnt) == n and cnt.sum() > 0
    np.testing.assert_array_equal(cnt, model)
    np.testing.assert_array_equal(out, model.astype(np.float32))
    total = np.zeros(n, np.int64)
    for b, e in [(0, n // 3), (n // 3, n)]:
        part = g.vga_through_vision(src_begin=b, src_end=e, counts=True)[1]
        assert 0 < part.sum() < cnt.sum()
        total += part
    np.testing.assert_array_equal(total, cnt)


def _graph_runs(g, A):
    """The fixture's runs where it stores them, else the graph's own (their digests are checked in (a))."""
    return A["runs"] if "runs" in A else g.copy(runs=True)["runs"]


def _expand(bins, runs, state, cols, rows, export):
    """Node::contents per node in plain Python from the bin records and runs (cells outside the grid dropped, each
    cell once, in run order), and with export only the filled cells behind the source: (off, refs)."""
    cells = np.flatnonzero(state & 2)
    off, refs, ro = [0], [], 0
    for k, src in enumerate(cells):
        seen = set()
        for b in range(32):
            d = BIN_DIR[b]
            for r in runs[ro:ro + int(bins[k, b, 3])]:
                x, y = int(r[0]), int(r[1])
                for _ in range(max((int(r[3]) - y if d == 2 else int(r[2]) - x) + 1, 1)):
                    c = x * rows + y
                    if 0 <= x < cols and 0 <= y < rows and c not in seen:
                        seen.add(c)
                        if not export or ((state[c] & 2) and c > src):
                            refs.append((x << 16) + (y & 0xffff))
                    x += 0 if d == 2 else 1
                    y += 1 if d in (2, 4) else -1 if d == 8 else 0
            ro += int(bins[k, b, 3])
        off.append(len(refs))
    return np.array(off, np.int64), np.array(refs, np.int32), cells


@pytest.mark.parametrize("name", ANALYSIS_CASES)
def test_connections_on_option_graphs(ctx, name):
    meta, A = _case(name)
    pm, g = _graph(ctx, name)
    bins = A["bins"] if "bins" in A else g.copy(runs=False)["bins"]
    runs = _graph_runs(g, A)
    for export in (False, True):
        woff, wrefs, cells = _expand(bins, runs, A["state"], meta["cols"], meta["rows"], export)
        off, refs = g.connections(export=export)
        np.testing.assert_array_equal(off, woff)
        np.testing.assert_array_equal(refs, wrefs)
    # export keeps filled cells only: none that the boundary option unfilled
    assert (A["state"][(refs >> 16) * meta["rows"] + (refs & 0xffff)] & 2).all()
    rows = meta["rows"]
    text = b"".join(b"\n%d,%d" % (((c // rows) << 16) + (c % rows), t)
                    for k, c in enumerate(cells) for t in wrefs[woff[k]:woff[k + 1]])
    n = meta["nodes"]
    assert g.connections_csv() == text
    assert g.connections_csv(0, n // 3) + g.connections_csv(n // 3, n) == text


@pytest.mark.parametrize("name", OPTION_CASES)
def test_chunk_of_option_graphs_written_and_read_back(ctx, monkeypatch, name):
    """Graph.write_chunk (boundary: the chunk's m_boundarygraph) gives the reference's PointMap::write bytes; read
    back (4-bit row shifts), VGA global equals the reference's own VGA after its round trip (vga_rt), with the
    drawing set (the asymmetric mode, forced) and without, to the bar of test_asym_mode.py."""
    meta, A = _case(name)
    pm, g = _graph(ctx, name)
    attrs = g.copy(runs=False)["attrs"]
    cols = [(c, attrs[:, j], j == 0) for j, c in enumerate(dmx.MAKEGRAPH_COLUMNS)]
    blob = g.write_chunk(cols, displayed=0, boundary=meta["boundary"])
    assert len(blob) == int(A["pm_chunk_size"][0])
    assert hashlib.sha256(blob).digest() == A["pm_chunk_sha256"].tobytes()
    if "pm_chunk" in A:
        assert blob == A["pm_chunk"].tobytes()
    info = graphio.read_chunk(blob)
    np.testing.assert_array_equal(info["state"], A["state"])
    assert info["nnodes"] == meta["nodes"]
    lines = case_input_lines(meta)
    for drawing in (None, lines):
        if drawing is not None:
            monkeypatch.setenv("DMX_VGA_ASYM", "1")
        pm2, g2 = graphio.load_chunk(ctx, blob, meta["region"], lines=drawing)
        out = g2.vga_visual_global(radius=-1)
        np.testing.assert_array_equal(out[:, 5], A["vga_rt"][:, 5])
        assert np.allclose(out, A["vga_rt"], rtol=1e-6, atol=1e-6), float(np.abs(out - A["vga_rt"]).max())
        g2.close()


def test_isovists_of_the_boundary_graphs_nodes(ctx):
    """VGA isovist depends on the drawing, not on which cells are nodes: the rows of syn32_b equal the rows of the
    same cells on the full map, bit for bit and in node order."""
    meta, A = _case("syn32_b")
    pm, g = _graph(ctx, "syn32_b")
    fmeta, FA = _case("syn32")
    fpm = _map(fmeta)
    full = fpm.make_graph(ctx).vga_isovist()
    fcells, bcells = np.flatnonzero(FA["state"] & 2), np.flatnonzero(A["state"] & 2)
    idx = np.searchsorted(fcells, bcells)
    assert (fcells[idx] == bcells).all() and len(bcells) == 315 < len(fcells)
    got = g.vga_isovist()
    assert got.shape == (315, 8) and (got[:, 0] > 0).all()
    np.testing.assert_array_equal(_bits(got), _bits(full[idx]))
