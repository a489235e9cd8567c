"""The priority queue of the serial metric / angular search (sd_run, kernels/stepdepth.hip) where it outgrows
its LDS window: refills from the HBM overflow list, the retry with a longer list, and the refill's health.

The maps are pillar halls (tests/golden/gen_synthetic.py make_pillar_hall): nearly every cell is an expander,
sight lines are long and lattice distances tie, so one search queues several times the window's 4096 keys.
Every comparison is bit for bit against the C restatement (pyoracle.OracleMap) -- the float sums depend on
the pop order, which is what a wrong refill would change -- and every "this path ran" assertion reads the
kernel's own counters (Context.last_stepdepth / last_stats), never a figure measured elsewhere."""
import functools

import numpy as np
import pytest

HALLS = {"hall64": (64, 3), "hall96": (96, 3), "hall128": (128, 4)}


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The hall's OracleMap with its graph made: built once, shared, never changed."""
    from golden.gen_synthetic import make_pillar_hall
    from pyoracle import OracleMap
    region, lines, fill = make_pillar_hall(*HALLS[name])
    om = OracleMap(region, 1.0, lines)
    assert om.fill(*fill)
    om.make_graph(threads=8)
    return om, region, lines, fill


@pytest.fixture(scope="module")
def halls(ctx):
    """halls(name) -> (PointMap, Graph) of the hall on the GPU: made once, closed with the module."""
    import depthmapx_amd as dmx
    made = {}

    def get(name):
        if name not in made:
            om, region, lines, fill = _oracle(name)
            pm = dmx.PointMap(region, lines, 1.0)
            assert pm.make_points(*fill)
            np.testing.assert_array_equal(pm.state(), om.state())
            made[name] = (pm, pm.make_graph(ctx))
        return made[name]
    yield get
    for pm, g in made.values():
        g.close()
        pm.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cell(name, x, y):
    return x * (HALLS[name][0] + 1) + y   # x-major; ascending cell index is PixelRef order


def _selections(name):
    W = HALLS[name][0]
    return {"centre": [_cell(name, W // 2, W // 2)], "corner": [_cell(name, 1, 1)],
            "three": [_cell(name, 5, 40), _cell(name, 33, 9), _cell(name, 60, 58)]}


@functools.lru_cache(maxsize=None)
def _want_metric_sd(name, sel):
    return _oracle(name)[0].metric_stepdepth(_selections(name)[sel])


@functools.lru_cache(maxsize=None)
def _want_angular_sd(name, cell):
    return _oracle(name)[0].angular_stepdepth([cell])


def _centre_node(name):
    return _oracle(name)[0].num_nodes // 2


def _node_cell(name, node):
    return int(np.flatnonzero(_oracle(name)[0].state() & 2)[node])


def test_hall128_centre_sees_more_than_one_window():
    """The premise of the angle-0 cases: in the oracle's graph the centre node of hall128 sees more cells than
    the queue's LDS window holds (4096), and an angular search queues every one of them at angle 0."""
    om = _oracle("hall128")[0]
    assert om.num_nodes == 127 * 127
    k = _centre_node("hall128")
    assert _node_cell("hall128", k) == _cell("hall128", 64, 64)
    b = om.graph()
    assert b["attrs"][k, 0] > 4096   # Connectivity
    assert b["attrs"][k, 0] == b["bins"][k, :, 1].sum()   # the cells of its 32 bins


@pytest.mark.gpu
@pytest.mark.parametrize("sel", ["centre", "corner", "three"])
def test_serial_metric_stepdepth_refills_and_matches_oracle(ctx, halls, monkeypatch, sel):
    pm, g = halls("hall64")
    monkeypatch.setenv("DMX_SD_KERNEL", "serial")
    monkeypatch.delenv("DMX_SD_CAP", raising=False)
    got = g.metric_step_depth(cells=_selections("hall64")[sel])
    sd = ctx.last_stepdepth()
    print("serial metric hall64 %s: %s" % (sel, sd))
    assert sd["mode"] == "serial" and sd["attempts"] == 1, sd
    assert sd["refills"] > 0, sd
    want = _want_metric_sd("hall64", sel)
    for col in (1, 2, 0):
        np.testing.assert_array_equal(_bits(got[:, col]), _bits(want[:, col]), err_msg="column %d" % col)
    assert (got[:, 1] >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("sel", ["centre", "corner", "three"])
def test_batched_metric_stepdepth_matches_oracle(ctx, halls, monkeypatch, sel):
    """The whole-GPU batched search on the same map against the oracle itself (elsewhere it is compared with the
    serial kernel, with which it shares the relaxation): lattice ties make cells ambiguous."""
    pm, g = halls("hall64")
    monkeypatch.delenv("DMX_SD_KERNEL", raising=False)
    got = g.metric_step_depth(cells=_selections("hall64")[sel])
    sd = ctx.last_stepdepth()
    print("batched metric hall64 %s: %s" % (sel, sd))
    assert sd["mode"] == "batched" and sd["refills"] == 0 and sd["attempts"] == 0, sd
    assert sd["ambiguous"] > 0, sd
    want = _want_metric_sd("hall64", sel)
    for col in (1, 2, 0):
        np.testing.assert_array_equal(_bits(got[:, col]), _bits(want[:, col]), err_msg="column %d" % col)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hall64", "hall128"])
def test_angular_stepdepth_refills_and_matches_oracle(ctx, halls, monkeypatch, name):
    """From the centre node: every cell it sees is queued at angle 0 (hall128: more than the window holds)."""
    pm, g = halls(name)
    monkeypatch.delenv("DMX_SD_CAP", raising=False)
    cell = _node_cell(name, _centre_node(name))
    got = g.angular_step_depth(cells=[cell])
    sd = ctx.last_stepdepth()
    print("angular step depth %s: %s" % (name, sd))
    assert sd["mode"] == "serial" and sd["refills"] > 0, sd
    want = _want_angular_sd(name, cell)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert (got >= 0).all()


@pytest.mark.gpu
def test_stepdepth_with_merge_links_refills_and_matches_oracle(ctx, monkeypatch):
    """Merge links force the serial kernel, metric included; one link joins far corners."""
    import depthmapx_amd as dmx
    from pyoracle import OracleMap
    om, region, lines, fill = _oracle("hall64")
    monkeypatch.delenv("DMX_SD_KERNEL", raising=False)
    monkeypatch.delenv("DMX_SD_CAP", raising=False)
    pairs = np.array([[_cell("hall64", 2, 2), _cell("hall64", 62, 62)],
                      [_cell("hall64", 20, 50), _cell("hall64", 41, 7)]], dtype=np.int32)
    pm = dmx.PointMap(region, lines, 1.0)
    assert pm.make_points(*fill)
    pm.set_merges(pairs)
    g = pm.make_graph(ctx)
    om2 = OracleMap.from_grid(om.cols, om.rows, 1.0, om.bottom_left, om.state())   # the shared one stays unlinked
    b = om.graph()
    om2.set_graph(b["bins"], b["runs"])
    om2.set_merges(pairs)
    sel = _selections("hall64")["corner"]
    got = g.metric_step_depth(cells=sel)
    sd = ctx.last_stepdepth()
    print("merge metric hall64: %s" % sd)
    assert sd["mode"] == "serial" and sd["refills"] > 0, sd
    want = om2.metric_stepdepth(sel)
    for col in (1, 2, 0):
        np.testing.assert_array_equal(_bits(got[:, col]), _bits(want[:, col]), err_msg="column %d" % col)
    assert not np.array_equal(_bits(want[:, 1]), _bits(_want_metric_sd("hall64", "corner")[:, 1]))   # the links matter
    gota = g.angular_step_depth(cells=sel)
    sda = ctx.last_stepdepth()
    print("merge angular hall64: %s" % sda)
    assert sda["refills"] > 0, sda
    np.testing.assert_array_equal(_bits(gota), _bits(om2.angular_stepdepth(sel)))
    g.close()


def _vga_ranges(n):
    return [(0, 16), (n // 2 - 32, n // 2 + 32), (n - 16, n)]


@functools.lru_cache(maxsize=None)
def _want_vga(kind, radius):
    om = _oracle("hall96")[0]
    run = om.vga_metric if kind == "metric" else om.vga_angular
    return [run(radius=radius, node_begin=b, node_end=e, threads=16)[b:e] for b, e in _vga_ranges(om.num_nodes)]


def _run_vga(ctx, halls, kind, radius):
    """The three source ranges on the GPU: (rows per range, refills per range, sources re-run in all)."""
    pm, g = halls("hall96")
    run = g.vga_metric if kind == "metric" else g.vga_angular
    out, refills, rerun = [], [], 0
    for b, e in _vga_ranges(g.info()["nnodes"]):
        out.append(run(radius=radius, src_begin=b, src_end=e)[b:e].copy())
        sd = ctx.last_stepdepth()
        refills.append(sd["refills"])
        rerun += ctx.last_stats()["vga_fail_cells"]
        print("vga %s r=%g [%d, %d): %s, %.3f s" % (kind, radius, b, e, sd, ctx.last_timing()[1]))
    return out, refills, rerun


VGA_FINITE = {"metric": 20.0, "angular": 1.0}   # cuts the search while keys wait in the overflow list


@pytest.mark.gpu
@pytest.mark.parametrize("kind,radius", [("metric", -1.0), ("metric", VGA_FINITE["metric"]),
                                         ("angular", -1.0), ("angular", VGA_FINITE["angular"])])
def test_vga_metric_angular_refill_and_match_oracle(ctx, halls, monkeypatch, kind, radius):
    monkeypatch.delenv("DMX_SD_CAP", raising=False)
    got, refills, rerun = _run_vga(ctx, halls, kind, radius)
    assert all(r > 0 for r in refills), refills
    for a, w in zip(got, _want_vga(kind, radius)):
        np.testing.assert_array_equal(_bits(a), _bits(w))
    n = _want_vga(kind, radius)[1][:, -1]
    assert (n > 1).all() and (radius < 0 or (n < _want_vga(kind, -1.0)[1][:, -1]).any())   # the radius cuts


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["metric", "angular"])
def test_vga_metric_angular_short_list_reruns_exactly(ctx, halls, monkeypatch, kind):
    """DMX_SD_CAP=2048: a list shorter than one window.  Sources stop, are listed and run again with longer
    lists (vga_fail_cells), for both kinds, and the bits are the oracle's."""
    monkeypatch.setenv("DMX_SD_CAP", "2048")
    got, refills, rerun = _run_vga(ctx, halls, kind, -1.0)
    assert rerun > 0
    assert all(r > 0 for r in refills), refills
    for a, w in zip(got, _want_vga(kind, -1.0)):
        np.testing.assert_array_equal(_bits(a), _bits(w))


@pytest.mark.gpu
def test_stepdepth_overflow_list_retry_and_capacity_error(ctx, halls, monkeypatch):
    """The serial step depth's own retry loop: a first list of 2048 keys is outgrown and the search runs again
    with 4x lists until one holds it (same bits as the oracle); from 64 keys the four attempts end at 4096,
    still too short, and the call fails with DMX_ERR_CAPACITY; the next call is untouched by either."""
    import depthmapx_amd as dmx
    pm, g = halls("hall64")
    sel = _selections("hall64")["corner"]
    want = _want_metric_sd("hall64", "corner")
    monkeypatch.setenv("DMX_SD_KERNEL", "serial")
    monkeypatch.setenv("DMX_SD_CAP", "2048")
    got = g.metric_step_depth(cells=sel)
    sd = ctx.last_stepdepth()
    print("cap 2048: %s" % sd)
    assert sd["mode"] == "serial" and 1 < sd["attempts"] <= 4, sd
    np.testing.assert_array_equal(_bits(got), _bits(want))
    monkeypatch.setenv("DMX_SD_CAP", "64")
    with pytest.raises(dmx.DmxError) as ei:
        g.metric_step_depth(cells=sel)
    assert ei.value.status == -3   # DMX_ERR_CAPACITY
    assert ctx.last_stepdepth()["attempts"] == 4
    monkeypatch.delenv("DMX_SD_CAP")
    got = g.metric_step_depth(cells=sel)
    sd = ctx.last_stepdepth()
    assert sd["attempts"] == 1 and sd["refills"] > 0, sd
    np.testing.assert_array_equal(_bits(got), _bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["stepdepth", "vga"])
def test_refill_brings_back_many_keys(ctx, halls, monkeypatch, what):
    """Refill health.  A refill aims at 512 keys or more (an eighth of the window; the cut's width doubles
    while it brings fewer), so pops outnumber refills by far: the bound asks for 16 pops a refill, a 32-fold
    margin.  A cut that cannot separate the keys at one distance -- here the more than 4096 cells the centre of
    hall128 sees, all queued at angle 0 -- and then brings back one key a refill misses it by that factor."""
    pm, g = halls("hall128")
    monkeypatch.delenv("DMX_SD_CAP", raising=False)
    k = _centre_node("hall128")
    if what == "stepdepth":
        cell = _node_cell("hall128", k)
        got = g.angular_step_depth(cells=[cell])
        want = _want_angular_sd("hall128", cell)
        secs = ctx.last_stepdepth()["seconds"]
    else:
        got = g.vga_angular(src_begin=k - 4, src_end=k + 4)[k - 4:k + 4]
        want = _oracle("hall128")[0].vga_angular(node_begin=k - 4, node_end=k + 4, threads=8)[k - 4:k + 4]
        secs = ctx.last_timing()[1]
    sd = ctx.last_stepdepth()
    print("refill health %s: refills %d, expanders_popped %d, kernel %.4f s" %
          (what, sd["refills"], sd["expanders_popped"], secs))
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert sd["refills"] > 0
    assert sd["refills"] * 16 <= sd["expanders_popped"], sd
