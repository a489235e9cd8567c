"""VGA isovist analysis on the GPU (dmx_vga_isovist, Graph.vga_isovist, dmx_chunk_occlusion /
dmx_chunk_set_occlusion) against the reference's own results (tests/golden/isovist/, from VGAIsovist::run of the
reference library; bounds and the treatment of the axis-aligned case in tests/isovist_util.py)."""
import ctypes
import lzma
import os

import numpy as np
import pytest

import depthmapx_amd as dmx
import isovist_util as iu
from depthmapx_amd import _native as N
from depthmapx_amd import graphio
from golden_io import GOLDEN

pytestmark = pytest.mark.gpu

GF = os.path.join(GOLDEN, "graphfiles")
_graphs = {}
_results = {}


def graph(ctx, name):
    """The engine's graph of a fixture map, made once per session of this module."""
    if name not in _graphs:
        m = iu.META[name]
        pm = dmx.PointMap(m["region"], iu.case_lines(name), m["spacing"])
        assert pm.make_points(*m["fill"], fill_type=m["fill_type"])
        assert (pm.cols, pm.rows) == (m["cols"], m["rows"])
        _graphs[name] = (pm, pm.make_graph(ctx))
        assert _graphs[name][1].info()["nnodes"] == m["nodes"]
    return _graphs[name]


def result(ctx, name):
    """The default run of a fixture map, shared (read-only) by the tests that compare against it."""
    if name not in _results:
        out, occ = graph(ctx, name)[1].vga_isovist(occlusion=True)
        for a in [out] + list(occ.values()):
            a.setflags(write=False)
        _results[name] = (out, occ, ctx.last_isovist())
    return _results[name]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _graphs.clear()
    _results.clear()


@pytest.mark.parametrize("name", ["kat", "syn16", "syn32", "syn64", "syn128"])
def test_matches_reference_fixture(ctx, name):
    """syn16: 225 cells, fewer than one workgroup a CU, partial tiles (17 x 17 grid); syn128: 16,129 cells."""
    out, occ, last = result(ctx, name)
    want_iso, want_occ = iu.reference(name)
    assert out.dtype == np.float32 and out.shape == want_iso.shape
    print(name, "values that differ bitwise:", iu.bit_differences(out, occ, want_iso, want_occ), last)
    bad = iu.failing_cells(out, occ, want_iso, want_occ)
    assert not bad.any(), np.flatnonzero(bad)[:10]
    assert last["reruns"] == 0 and last["tree_nodes"] >= 4 and last["tree_depth"] >= 1
    assert 0 < last["max_blocks"] <= 128


def test_simple_version_writes_the_area_only(ctx):
    pm, g = graph(ctx, "syn32")
    full = result(ctx, "syn32")[0]
    out = g.vga_isovist(simple=True)
    np.testing.assert_array_equal(out[:, 0], full[:, 0])
    assert (out[:, 1:] == -1).all()
    marked = np.full(full.shape, 7.0, dtype=np.float32)
    g.vga_isovist(simple=True, out=marked)
    assert (marked[:, 1:] == 7.0).all() and np.array_equal(marked[:, 0], full[:, 0])


def test_source_ranges_write_their_rows_and_add_up_to_the_whole(ctx):
    pm, g = graph(ctx, "syn32")
    full, focc, _ = result(ctx, "syn32")
    n = len(full)
    a, aocc = g.vga_isovist(src_begin=0, src_end=300, occlusion=True)
    np.testing.assert_array_equal(a[:300], full[:300])
    assert (a[300:] == -1).all() and not aocc["occ_counts"][300:].any() and not aocc["occ_dist"][300:].any()
    b, bocc = g.vga_isovist(src_begin=300, src_end=-1, occlusion=True)   # src_end < 0: to the end
    assert (b[:300] == -1).all()
    np.testing.assert_array_equal(np.where(np.arange(n)[:, None] < 300, a, b), full)
    np.testing.assert_array_equal(aocc["occ_counts"] + bocc["occ_counts"], focc["occ_counts"])
    np.testing.assert_array_equal(aocc["occ_dist"] + bocc["occ_dist"], focc["occ_dist"])
    np.testing.assert_array_equal(np.concatenate([aocc["occ_pixels"], bocc["occ_pixels"]]), focc["occ_pixels"])
    empty = g.vga_isovist(src_begin=5, src_end=5)
    assert (empty == -1).all()
    with pytest.raises(N.DmxError) as ei:
        g.vga_isovist(src_begin=n + 1, src_end=n + 2)
    assert ei.value.status == -1


def test_semifill_skips_context_filled_cells_at_odd_pixelrefs(ctx):
    pm, g = graph(ctx, "syn16semi")
    np.testing.assert_array_equal(pm.state(), np.load(os.path.join(iu.ISO, "syn16semi_state.npy")))
    out, occ, _ = result(ctx, "syn16semi")
    want_iso, want_occ = iu.reference("syn16semi")
    skipped = (want_iso == -1).all(axis=1)
    assert 0 < skipped.sum() < len(skipped)
    assert (out[skipped] == -1).all() and not occ["occ_counts"][skipped].any() and not occ["occ_dist"][skipped].any()
    assert not iu.failing_cells(out, occ, want_iso, want_occ).any()
    marked = np.full(out.shape, 3.0, dtype=np.float32)
    g.vga_isovist(out=marked)
    assert (marked[skipped] == 3.0).all() and np.array_equal(marked[~skipped], out[~skipped])


@pytest.mark.parametrize("gcap,bcap", [("6", "128"), ("32", "20"), ("5", "16")])
def test_capacity_overflow_is_run_again_not_truncated(ctx, monkeypatch, gcap, bcap):
    """DMX_ISO_GCAP / DMX_ISO_BCAP shrunk below what syn32 needs (13 gaps, 85 blocks): the flagged cells run
    again with larger lists and the results are those of the default run."""
    pm, g = graph(ctx, "syn32")
    full, focc, _ = result(ctx, "syn32")
    monkeypatch.setenv("DMX_ISO_GCAP", gcap)
    monkeypatch.setenv("DMX_ISO_BCAP", bcap)
    out, occ = g.vga_isovist(occlusion=True)
    assert ctx.last_isovist()["reruns"] > 0
    np.testing.assert_array_equal(out, full)
    for k in focc:
        np.testing.assert_array_equal(occ[k], focc[k])


def test_capacity_error_only_after_the_retry_and_hook_range(ctx, monkeypatch):
    pm, g = graph(ctx, "syn16")
    monkeypatch.setenv("DMX_ISO_BCAP", "1")   # the retry's 16 blocks are still too few
    out = np.full((g.info()["nnodes"], 8), 5.0, dtype=np.float32)
    with pytest.raises(N.DmxError) as ei:
        g.vga_isovist(out=out)
    assert ei.value.status == -3 and (out == 5.0).all()
    monkeypatch.setenv("DMX_ISO_BCAP", "0")
    with pytest.raises(N.DmxError) as ei:
        g.vga_isovist()
    assert ei.value.status == -1


def _chunk_of(ctx, name):
    pm, g = graph(ctx, name)
    c = g.copy(runs=True)
    cols = [(n, np.ascontiguousarray(c["attrs"][:, i]), False) for i, n in
            enumerate(["Connectivity", "Point First Moment", "Point Second Moment"])]
    return graphio.write_chunk(pm, c["bins"], c["runs"], c["gridconn"], cols)


def test_chunk_loaded_graph_on_an_unaligned_grid(ctx):
    """A graph read back from a PointMap chunk has no drawing of its own: with dmx_graph_set_drawing it gives the
    rows of the in-memory graph (17 x 17 grid: neither side a multiple of the 8 x 8 tile), without it
    DMX_ERR_STATE."""
    m = iu.META["syn16"]
    assert m["cols"] % 8 and m["rows"] % 8
    blob = _chunk_of(ctx, "syn16")
    full, focc, _ = result(ctx, "syn16")
    pm2, g2 = graphio.load_chunk(ctx, blob, m["region"], lines=iu.case_lines("syn16"))
    out, occ = g2.vga_isovist(occlusion=True)
    np.testing.assert_array_equal(out, full)
    for k in focc:
        np.testing.assert_array_equal(occ[k], focc[k])
    pm3, g3 = graphio.load_chunk(ctx, blob, m["region"])
    with pytest.raises(N.DmxError) as ei:
        g3.vga_isovist()
    assert ei.value.status == -4


def test_pending_cancel_returns_cancelled_and_leaves_out_unwritten(ctx):
    pm, g = graph(ctx, "syn32")
    out = np.full((g.info()["nnodes"], 8), 9.0, dtype=np.float32)
    ctx.cancel()
    with pytest.raises(N.DmxError) as ei:
        g.vga_isovist(out=out)
    assert ei.value.status == -7 and (out == 9.0).all()
    np.testing.assert_array_equal(g.vga_isovist(), result(ctx, "syn32")[0])   # the request was consumed


def test_progress_posts_tiles(ctx):
    pm, g = graph(ctx, "syn64")
    seen = []
    ctx.set_progress(lambda phase, done, total: seen.append((phase, done, total)) or 0, 0.001)
    try:
        g.vga_isovist()
    finally:
        ctx.set_progress(None)
    m = iu.META["syn64"]
    tiles = ((m["cols"] + 7) // 8) * ((m["rows"] + 7) // 8)
    assert seen and seen[-1] == (2, tiles, tiles)   # DMX_PHASE_VGA; the unit is a tile of 8 x 8 cells


def test_axis_aligned_case_on_its_stable_cells(ctx):
    out, occ, _ = result(ctx, "axis16")
    iu.check_degenerate("axis16", out, occ)


# ---------------------------------------------------------------- occlusion data in the PointMap chunk
def _pointmap_chunk(path):
    lib = N.lib()
    h = ctypes.c_void_p()
    N.check(lib.dmx_graphfile_read(path.encode(), ctypes.byref(h)))
    try:
        npm, disp = ctypes.c_int32(), ctypes.c_int32()
        N.check(lib.dmx_graphfile_info(h, None, None, None, None, ctypes.byref(npm), ctypes.byref(disp)))
        buf, size = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_int64()
        N.check(lib.dmx_graphfile_pointmap(h, disp.value, ctypes.byref(buf), ctypes.byref(size)))
        return ctypes.string_at(buf, size.value)
    finally:
        lib.dmx_graphfile_free(h)


def _unxz(src, tmp):
    dst = os.path.join(str(tmp), os.path.basename(src)[:-3])
    with lzma.open(src) as f, open(dst, "wb") as o:
        o.write(f.read())
    return dst


def test_chunk_occlusion_of_the_graph_the_reference_wrote(tmp_path):
    blob = _pointmap_chunk(_unxz(os.path.join(iu.ISO, "syn16_isovist.graph.xz"), tmp_path))
    got = graphio.chunk_occlusion(blob)
    want = iu.reference("syn16")[1]
    for k in want:
        np.testing.assert_array_equal(got[k], want[k])
    # written back through dmx_chunk_set_occlusion: the reference's own bytes
    used = graphio.read_chunk(blob)["bytes_used"]
    assert graphio.set_chunk_occlusion(blob, got["occ_dist"], got["occ_counts"], got["occ_pixels"]) == blob[:used]


def test_chunk_set_occlusion_round_trip_with_the_gpu_result(ctx):
    blob = _chunk_of(ctx, "syn16")
    out, occ, _ = result(ctx, "syn16")
    plain = graphio.chunk_occlusion(blob)
    assert not plain["occ_counts"].any() and not plain["occ_dist"].any() and len(plain["occ_pixels"]) == 0
    blob2 = graphio.set_chunk_occlusion(blob, occ["occ_dist"], occ["occ_counts"], occ["occ_pixels"])
    assert len(blob2) == len(blob) + 4 * len(occ["occ_pixels"])
    back = graphio.chunk_occlusion(blob2)
    for k in occ:
        np.testing.assert_array_equal(back[k], occ[k])
    a, b = graphio.read_chunk(blob), graphio.read_chunk(blob2)
    for k in ("state", "bins", "runs", "gridconn"):
        np.testing.assert_array_equal(a[k], b[k])
    assert graphio.set_chunk_occlusion(blob, None, None, None) == blob   # dmx_chunk_write still writes the bins empty


@pytest.mark.parametrize("name", ["gallery_connected", "mixed_link"])
def test_chunk_without_set_occlusion_serialises_as_before(tmp_path, name):
    """A chunk nobody set occlusion on: parse + serialise gives the bytes of the .graph the reference wrote, which
    is what the serialiser emitted for these fixtures before it knew about occlusion data."""
    blob = _pointmap_chunk(_unxz(os.path.join(GF, "inputs", name + ".graph.xz"), tmp_path))
    used = graphio.read_chunk(blob)["bytes_used"]
    assert graphio.set_chunk_occlusion(blob, None, None, None) == blob[:used]
