"""VGA through vision on the GPU (dmx_vga_thruvision, Graph.vga_through_vision, dmxcli -m VGA -vm thruvision)
against the reference's own results (tests/golden/thruvision/, from VGAThroughVision::run of the reference
library).  The result is an integer count per cell, so every comparison is exact."""
import ctypes
import hashlib
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import depthmapx_amd as dmx
import thruvision_model as tvm
from depthmapx_amd import _native as N
from depthmapx_amd import graphio
from golden_io import GOLDEN, case_input_lines, load_case

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "depthmapx_amd", "_lib", "dmxcli")
TV = os.path.join(GOLDEN, "thruvision")
GF = os.path.join(GOLDEN, "graphfiles")
GF_CASES = json.load(open(os.path.join(GF, "cases.json")))
TV_CASES = json.load(open(os.path.join(TV, "cases.json")))
CORRIDORS = ["corridor256x3", "corridor3x256"]
_graphs = {}


def reference(name):
    return np.load(os.path.join(TV, name + "_thruvision.npy"), allow_pickle=False)


def graph(ctx, name):
    """The engine's graph of a fixture map, made once per session of this module."""
    if name not in _graphs:
        if name in CORRIDORS:
            z = np.load(os.path.join(TV, name + ".npz"), allow_pickle=False)
            pm = dmx.PointMap(z["region"], z["lines"], float(z["spacing"]))
            assert pm.make_points(*(float(v) for v in z["fill"]))
            np.testing.assert_array_equal(pm.state(), z["state"])
        else:
            meta, _ = load_case(name)
            pm = dmx.PointMap(meta["region"], case_input_lines(meta), meta["spacing"])
            for f in meta["fills"]:
                assert pm.make_points(*f)
        _graphs[name] = (pm, pm.make_graph(ctx))
    return _graphs[name]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _graphs.clear()


@pytest.mark.parametrize("name", ["kat", "syn16", "syn32", "syn64", "gallery"] + CORRIDORS + ["syn128"])
def test_matches_reference_fixture(ctx, name):
    """syn128 (127^2 filled cells) is wider than the LDS window in both directions."""
    pm, g = graph(ctx, name)
    out, cnt = g.vga_through_vision(counts=True)
    want = reference(name)
    assert out.dtype == np.float32 and cnt.dtype == np.int64 and out.shape == want.shape
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(cnt, out.astype(np.int64))
    np.testing.assert_array_equal(g.vga_through_vision(), want)
    st = ctx.last_stats()
    assert st["tv_lines"] > 0 or name == "kat"
    assert st["tv_pixel_steps"] >= cnt.sum() // 2


def test_disjoint_source_ranges_sum_to_the_full_run(ctx):
    pm, g = graph(ctx, "syn64")
    n = g.info()["nnodes"]
    full_f, full = g.vga_through_vision(counts=True)
    total = np.zeros(n, np.int64)
    for b, e in [(0, 7), (7, 1500), (1500, n)]:
        out, cnt = g.vga_through_vision(src_begin=b, src_end=e, counts=True)
        np.testing.assert_array_equal(cnt, out.astype(np.int64))
        assert 0 < cnt.sum() < full.sum()
        total += cnt
    np.testing.assert_array_equal(total, full)
    np.testing.assert_array_equal(full_f, reference("syn64"))
    out, cnt = g.vga_through_vision(src_begin=5, src_end=5, counts=True)
    assert not out.any() and not cnt.any() and len(out) == n
    out, cnt = g.vga_through_vision(src_begin=n - 3, src_end=-1, counts=True)   # src_end < 0: to the end
    np.testing.assert_array_equal(cnt, g.vga_through_vision(src_begin=n - 3, src_end=n, counts=True)[1])


@pytest.mark.parametrize("window", ["8", "0", "7", "100"])
@pytest.mark.parametrize("name", ["syn32"] + CORRIDORS)
def test_window_hook_tiny_window_and_global_atomics(ctx, monkeypatch, name, window):
    """DMX_TV_WINDOW: 0 forces variant (A), global atomics only; n forces an n x n window of variant (B)
    (8: most increments leave the window; 7: odd; 100: wider than the map in one or both directions)."""
    pm, g = graph(ctx, name)
    monkeypatch.setenv("DMX_TV_WINDOW", window)
    out, cnt = g.vga_through_vision(counts=True)
    assert ctx.last_stats()["tv_window"] == int(window)
    np.testing.assert_array_equal(out, reference(name))
    np.testing.assert_array_equal(cnt, reference(name).astype(np.int64))
    monkeypatch.delenv("DMX_TV_WINDOW")
    g.vga_through_vision()
    assert ctx.last_stats()["tv_window"] not in (0, int(window))   # the suite's default is variant (B)


def test_window_hook_out_of_range_is_refused(ctx, monkeypatch):
    pm, g = graph(ctx, "syn16")
    monkeypatch.setenv("DMX_TV_WINDOW", "4000")
    with pytest.raises(N.DmxError) as ei:
        g.vga_through_vision()
    assert ei.value.status == -1


def _input(tmp, name):
    dst = os.path.join(str(tmp), name)
    if not os.path.exists(dst):
        with lzma.open(os.path.join(GF, "inputs", name + ".xz")) as f, open(dst, "wb") as o:
            o.write(f.read())
    return dst


def _graphfile(path):
    """region and the displayed point map's chunk bytes of a .graph file."""
    lib = N.lib()
    h = ctypes.c_void_p()
    N.check(lib.dmx_graphfile_read(path.encode(), ctypes.byref(h)))
    try:
        region = np.zeros(4)
        npm, disp = ctypes.c_int32(), ctypes.c_int32()
        N.check(lib.dmx_graphfile_info(h, None, None, N.ptr(region), None, ctypes.byref(npm), ctypes.byref(disp)))
        buf, size = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_int64()
        N.check(lib.dmx_graphfile_pointmap(h, disp.value, ctypes.byref(buf), ctypes.byref(size)))
        return region, ctypes.string_at(buf, size.value)
    finally:
        lib.dmx_graphfile_free(h)


@pytest.mark.parametrize("name", ["gallery_connected", "mixed_link"])
def test_reread_graphs_with_shifted_runs_and_merges(ctx, tmp_path, name):
    """Graphs read back from .graph files (4-bit-shifted runs, merge links, context-filled cells) through
    dmx_chunk_load: merge links make no difference, context-filled sources are not skipped."""
    region, blob = _graphfile(_input(tmp_path, name + ".graph"))
    pm, g = graphio.load_chunk(ctx, blob, region)
    out, cnt = g.vga_through_vision(counts=True)
    want = reference("tv_" + name)
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(cnt, want.astype(np.int64))


@pytest.mark.parametrize("name", ["kat", "syn16"])
def test_model_on_the_graph_the_engine_holds(ctx, name):
    pm, g = graph(ctx, name)
    c = g.copy(runs=True)
    meta, _ = load_case(name)
    model = tvm.through_vision(meta["cols"], meta["rows"], pm.state(), c["bins"][:, :, 3].sum(axis=1), c["runs"])
    out, cnt = g.vga_through_vision(counts=True)
    np.testing.assert_array_equal(cnt, model)
    np.testing.assert_array_equal(out, reference(name))


# ---------------------------------------------------------------- CLI
def _cli(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=600)


def _chain(tmp, inp):
    """A committed input, or ("@case") the output of a chain of graphfiles/cases.json run through dmxcli."""
    if not inp.startswith("@"):
        return _input(tmp, inp)
    case = GF_CASES[inp[1:]]
    dst = os.path.join(str(tmp), inp[1:] + ".graph")
    r = _cli("-f", _chain(tmp, case["input"]), "-o", dst, *case["args"])
    assert r.returncode == 0, r.stdout + r.stderr
    return dst


@pytest.mark.parametrize("name", sorted(TV_CASES))
def test_cli_output_is_byte_identical_to_the_reference(tmp_path, name):
    m = TV_CASES[name]
    assert m["args"] == ["-m", "VGA", "-vm", "thruvision"]
    src = _chain(tmp_path, m["input"])
    dst = str(tmp_path / (name + ".graph"))
    r = _cli("-f", src, "-o", dst, *m["args"])
    assert r.returncode == 0, r.stdout + r.stderr
    b = open(dst, "rb").read()
    assert len(b) == m["size"]
    assert hashlib.sha256(b).hexdigest() == m["sha256"]


def test_cli_simple_mode_makes_no_difference(tmp_path):
    m = TV_CASES["tv_turns_remake"]
    dst = str(tmp_path / "s.graph")
    r = _cli("-s", "-f", _chain(tmp_path, m["input"]), "-o", dst, *m["args"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert hashlib.sha256(open(dst, "rb").read()).hexdigest() == m["sha256"]


def test_cli_refuses_gate_column_and_isovist(tmp_path):
    lib = N.lib()
    g1, g2 = _chain(tmp_path, "@turns_remake"), str(tmp_path / "gate.graph")
    # the same map with a column __Internal_Gate (every row -1: no gate)
    h, c = ctypes.c_void_p(), ctypes.c_void_p()
    N.check(lib.dmx_graphfile_read(g1.encode(), ctypes.byref(h)))
    try:
        npm, disp = ctypes.c_int32(), ctypes.c_int32()
        N.check(lib.dmx_graphfile_info(h, None, None, None, None, ctypes.byref(npm), ctypes.byref(disp)))
        buf, size = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_int64()
        N.check(lib.dmx_graphfile_pointmap(h, disp.value, ctypes.byref(buf), ctypes.byref(size)))
        raw = np.frombuffer(ctypes.string_at(buf, size.value), dtype=np.uint8).copy()
        N.check(lib.dmx_chunk_parse(N.ptr(raw), len(raw), ctypes.byref(c)))
        try:
            nn = ctypes.c_int64()
            N.check(lib.dmx_chunk_info(c, None, None, None, None, ctypes.byref(nn), None, None, None, None))
            gate = np.full(nn.value, -1.0, dtype=np.float32)
            N.check(lib.dmx_chunk_set_column(c, b"__Internal_Gate", N.ptr(gate), None, 0, 0))
            N.check(lib.dmx_chunk_serialize(c, None, 0, ctypes.byref(size)))
            out = np.zeros(size.value, dtype=np.uint8)
            N.check(lib.dmx_chunk_serialize(c, N.ptr(out), len(out), ctypes.byref(size)))
        finally:
            lib.dmx_chunk_free(c)
        N.check(lib.dmx_graphfile_put_pointmap(h, disp.value, N.ptr(out), len(out)))
        N.check(lib.dmx_graphfile_write(h, g2.encode()))
    finally:
        lib.dmx_graphfile_free(h)
    dst = tmp_path / "o.graph"
    r = _cli("-m", "VGA", "-f", g2, "-o", dst, "-vm", "thruvision")
    assert r.returncode != 0 and "__Internal_Gate" in r.stdout + r.stderr
    assert not dst.exists()
    r = _cli("-m", "VGA", "-f", g1, "-o", dst, "-vm", "thruvision")   # without the column it runs
    assert r.returncode == 0, r.stdout + r.stderr
    cols = {n: v for n, v, _ in graphio.read_chunk(_graphfile(str(dst))[1])["columns"]}
    np.testing.assert_array_equal(cols["Through vision"], reference("tv_turns_remake"))
    # -vm isovist stays outside; its message names the supported modes
    dst2 = tmp_path / "i.graph"
    r = _cli("-m", "VGA", "-f", g1, "-o", dst2, "-vm", "isovist")
    assert r.returncode != 0 and "thruvision" in r.stdout + r.stderr and "are part of the accelerated path" in r.stdout + r.stderr
    assert not dst2.exists()


# ---------------------------------------------------------------- cancel, state
def test_pending_cancel_stops_the_call_once(ctx):
    pm, g = graph(ctx, "syn32")
    ctx.cancel()
    with pytest.raises(N.DmxError) as ei:
        g.vga_through_vision()
    assert ei.value.status == -7
    np.testing.assert_array_equal(g.vga_through_vision(), reference("syn32"))   # the request was consumed


def test_progress_reports_and_callback_cancels(ctx):
    pm, g = graph(ctx, "syn64")
    n = g.info()["nnodes"]
    calls = []
    ctx.set_progress(lambda phase, done, total: calls.append((phase, done, total)) and False, interval_s=0.001)
    try:
        out = g.vga_through_vision()
    finally:
        ctx.set_progress(None)
    assert calls and calls[-1] == (2, n, n) and all(p == 2 and 0 <= d <= t == n for p, d, t in calls)
    np.testing.assert_array_equal(out, reference("syn64"))
    ctx.set_progress(lambda phase, done, total: True, interval_s=0.001)
    try:
        with pytest.raises(N.DmxError) as ei:
            g.vga_through_vision()
        assert ei.value.status == -7
    finally:
        ctx.set_progress(None)
    np.testing.assert_array_equal(g.vga_through_vision(), reference("syn64"))


def test_sharded_graph_and_bad_ranges_are_refused(ctx):
    pm, g = graph(ctx, "syn32")
    n = g.info()["nnodes"]
    shard = pm.make_graph(ctx, node_begin=0, node_end=n // 2)
    with pytest.raises(N.DmxError) as ei:
        shard.vga_through_vision()
    assert ei.value.status == -4
    with pytest.raises(N.DmxError) as ei:
        g.vga_through_vision(src_begin=10, src_end=5)
    assert ei.value.status == -1
