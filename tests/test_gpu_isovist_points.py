"""Isovists at arbitrary points on the GPU (dmx_isovists, Context.isovists) against the reference's own results
(tests/golden/isovist_points/, from MetaGraph::makeIsovist of the reference library; bounds and the canonical
polygon in tests/isovist_points_util.py)."""
import ctypes

import numpy as np
import pytest

import depthmapx_amd as dmx
import isovist_points_util as pu
import isovist_util as iu
from depthmapx_amd import _native as N

pytestmark = pytest.mark.gpu

_results = {}


def run(ctx, name, **kw):
    pts = pu.reference(name)[0]
    return ctx.isovists(pu.case_lines(name), pts[:, :2], pts[:, 2:], region=pu.META[name]["region"], **kw)


def result(ctx, name):
    """The default run of a fixture case with polygons, shared (read-only) by the tests that compare against it."""
    if name not in _results:
        out, off, xy = run(ctx, name, polygons=True)
        for a in (out, off, xy):
            a.setflags(write=False)
        _results[name] = (out, off, xy, ctx.last_isovist())
    return _results[name]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _results.clear()


def same(a, b):
    """Identical rows and polygons, bit for bit."""
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))


def raw(ctx, lines, points, angles, out, off=None, xy=None, total=None, region=None):
    return N.lib().dmx_isovists(ctx.h, N.ptr(lines), len(lines), N.ptr(region), N.ptr(points), N.ptr(angles), len(points),
                                0, N.ptr(out), N.ptr(off), N.ptr(xy), 0 if xy is None else len(xy),
                                None if total is None else ctypes.byref(total))


@pytest.mark.parametrize("name", ["syn32", "kat", "syn16"])
def test_matches_reference_fixture(ctx, name):
    out, off, xy, last = result(ctx, name)
    pts, want_cols, want_off, want_xy = pu.reference(name)
    assert out.dtype == np.float32 and out.shape == want_cols.shape and off.dtype == np.int64 and xy.dtype == np.float64
    print(name, "column values that differ bitwise:", int((out.view(np.uint32) != want_cols.view(np.uint32)).sum()),
          "raw vertex counts that differ:", int((np.diff(off) != np.diff(want_off)).sum()), last)
    bad = pu.column_failures(out, want_cols)
    assert not bad.any(), np.flatnonzero(bad)[:10]
    assert not pu.polygon_failures(off, xy, want_cols, want_off, want_xy)
    assert last["reruns"] == 0 and last["tree_nodes"] >= 4 and last["tree_depth"] >= 1 and 0 < last["max_blocks"] <= 128


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_wave_boundaries(ctx, n):
    full = result(ctx, "syn32")
    pts = pu.reference("syn32")[0][:n]
    got = ctx.isovists(pu.case_lines("syn32"), pts[:, :2], pts[:, 2:], region=pu.META["syn32"]["region"], polygons=True)
    same(got, (full[0][:n], full[1][:n + 1], full[2][:full[1][n]]))


def test_empty_batch(ctx):
    lines = pu.case_lines("kat")
    out = ctx.isovists(lines, np.zeros((0, 2)))
    assert out.shape == (0, 8) and out.dtype == np.float32
    out, off, xy = ctx.isovists(lines, np.zeros((0, 2)), np.zeros((0, 2)), polygons=True)
    assert out.shape == (0, 8) and off.tolist() == [0] and xy.shape == (0, 2)


def test_results_do_not_depend_on_the_order(ctx, monkeypatch):
    """The caller's order against the Morton order through the hook, and the points reversed."""
    full = result(ctx, "syn32")
    for order in ("caller", "morton"):
        monkeypatch.setenv("DMX_ISO_ORDER", order)
        same(run(ctx, "syn32", polygons=True), full)
    monkeypatch.delenv("DMX_ISO_ORDER")
    pts = pu.reference("syn32")[0][::-1]
    out, off, xy = ctx.isovists(pu.case_lines("syn32"), pts[:, :2], pts[:, 2:], region=pu.META["syn32"]["region"], polygons=True)
    assert np.array_equal(out[::-1].view(np.uint32), full[0].view(np.uint32))
    assert np.array_equal(np.diff(off)[::-1], np.diff(full[1]))
    back = np.concatenate([xy[off[k]:off[k + 1]] for k in range(len(pts) - 1, -1, -1)])
    assert np.array_equal(back.view(np.uint64), full[2].view(np.uint64))


def test_cell_centres_equal_the_vga_isovist_analysis(ctx):
    """syn16 at its cell centres with the point map's region: Graph.vga_isovist() bit for bit on the same device."""
    m = iu.META["syn16"]
    lines = iu.case_lines("syn16")
    pm = dmx.PointMap(m["region"], lines, m["spacing"])
    assert pm.make_points(*m["fill"])
    want = pm.make_graph(ctx).vga_isovist()
    i = pm.info()
    xs, ys = np.nonzero((pm.state().reshape(i["cols"], i["rows"]) & 2) != 0)   # Point::FILLED, node order
    s = m["spacing"]
    (blx, bly) = i["bottom_left"]
    pts = np.column_stack([blx + s * 1.0 * xs, bly + s * 1.0 * ys])
    grid = [blx - s / 2.0, bly - s / 2.0, blx + (i["cols"] - 1) * s + s / 2.0, bly + (i["rows"] - 1) * s + s / 2.0]
    got = ctx.isovists(lines, pts, region=grid)
    assert len(got) == m["nodes"] and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("gcap,bcap", [("6", "128"), ("32", "20"), ("5", "16")])
def test_capacity_overflow_is_run_again_not_truncated(ctx, monkeypatch, gcap, bcap):
    """DMX_ISO_GCAP / DMX_ISO_BCAP shrunk below what syn32's points need (13 gaps, 84 blocks)."""
    full = result(ctx, "syn32")
    monkeypatch.setenv("DMX_ISO_GCAP", gcap)
    monkeypatch.setenv("DMX_ISO_BCAP", bcap)
    got = run(ctx, "syn32", polygons=True)
    assert ctx.last_isovist()["reruns"] > 0
    same(got, full)


def test_capacity_error_only_after_the_retry(ctx, monkeypatch):
    pts = pu.reference("syn32")[0]
    lines = pu.case_lines("syn32")
    monkeypatch.setenv("DMX_ISO_BCAP", "1")   # the retry's 16 blocks are still too few
    p, a = np.ascontiguousarray(pts[:, :2]), np.ascontiguousarray(pts[:, 2:])
    out = np.full((len(pts), 8), 5.0, dtype=np.float32)
    off = np.full(len(pts) + 1, 7, dtype=np.int64)
    xy = np.full((64 * len(pts), 2), 3.0)
    total = ctypes.c_int64(-9)
    assert raw(ctx, lines, p, a, out, off, xy, total) == -3
    assert (out == 5.0).all() and (off == 7).all() and (xy == 3.0).all() and total.value == -9


def test_vertex_pool_is_enlarged(ctx, monkeypatch):
    full = result(ctx, "syn32")
    monkeypatch.setenv("DMX_ISO_VPOOL", "1")
    same(run(ctx, "syn32", polygons=True), full)


def test_a_poly_cap_too_small_reports_the_total_and_writes_no_vertex(ctx, monkeypatch):
    full = result(ctx, "syn32")
    pts = pu.reference("syn32")[0]
    lines = pu.case_lines("syn32")
    p, a = np.ascontiguousarray(pts[:, :2]), np.ascontiguousarray(pts[:, 2:])
    out = np.full((len(pts), 8), -1.0, dtype=np.float32)
    off = np.zeros(len(pts) + 1, dtype=np.int64)
    xy = np.full((len(full[2]) - 1, 2), 3.0)
    total = ctypes.c_int64()
    assert raw(ctx, lines, p, a, out, off, xy, total) == 0
    assert total.value == len(full[2]) and np.array_equal(off, full[1]) and (xy == 3.0).all()
    assert np.array_equal(out.view(np.uint32), full[0].view(np.uint32))
    # the Python mirror calls a second time when its guess was too small
    monkeypatch.setattr(dmx.Context, "ISOVIST_POLY_GUESS", 8)
    got = run(ctx, "syn32", polygons=True)
    assert len(got[2]) > 8 * len(pts)
    same(got, full)


def test_simple_version_writes_the_area_only(ctx):
    full = result(ctx, "syn32")[0]
    out = run(ctx, "syn32", simple=True)
    np.testing.assert_array_equal(out[:, 0], full[:, 0])
    assert (out[:, 1:] == -1).all()


def test_bad_input(ctx):
    lines = pu.case_lines("kat")
    for p, a in [([[0.5, np.nan]], None), ([[0.5, 0.5]], [[0.0, np.inf]]), ([[np.inf, 0.5]], [[0.0, 1.0]])]:
        with pytest.raises(N.DmxError) as ei:
            ctx.isovists(lines, p, a)
        assert ei.value.status == -1
    with pytest.raises(N.DmxError) as ei:
        ctx.isovists(np.zeros((0, 4)), [[0.5, 0.5]])
    assert ei.value.status == -4
    out = np.full((1, 8), 5.0, dtype=np.float32)
    assert raw(ctx, np.zeros((0, 4)), np.array([[0.5, 0.5]]), None, out) == -4 and (out == 5.0).all()


def test_pending_cancel_returns_cancelled_and_leaves_the_outputs_unwritten(ctx):
    pts = pu.reference("syn32")[0]
    lines = pu.case_lines("syn32")
    p, a = np.ascontiguousarray(pts[:, :2]), np.ascontiguousarray(pts[:, 2:])
    out = np.full((len(pts), 8), 9.0, dtype=np.float32)
    off = np.full(len(pts) + 1, 7, dtype=np.int64)
    xy = np.full((64 * len(pts), 2), 3.0)
    total = ctypes.c_int64(-9)
    ctx.cancel()
    assert raw(ctx, lines, p, a, out, off, xy, total) == -7
    assert (out == 9.0).all() and (off == 7).all() and (xy == 3.0).all() and total.value == -9
    same(run(ctx, "syn32", polygons=True), result(ctx, "syn32"))   # the request was consumed


def test_progress_posts_items_of_64_points(ctx):
    seen = []
    ctx.set_progress(lambda phase, done, total: seen.append((phase, done, total)) or 0, 0.001)
    try:
        run(ctx, "syn32")
    finally:
        ctx.set_progress(None)
    items = (pu.META["syn32"]["n"] + 63) // 64
    assert seen and seen[-1] == (2, items, items)   # DMX_PHASE_VGA
