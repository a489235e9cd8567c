"""The .graph PointMap chunk's node records on the GPU: Graph.write_chunk (dmx_graph_chunk_write) against the host
writer on dmx_graph_copy's arrays and the reference's own bytes, and graphio.load_chunk_device
(dmx_chunk_load_bytes) against the parser (read_chunk) and dmx_chunk_load.  Everything is compared bit for bit: the
codec has no tolerance.

Graphs and chunks are made once per module and left unchanged.  The format-limit graphs are fabricated with
dmx_graph_from_runs on maps of a few thousand empty cells, so they stay tiny; a bin of more than 65535 runs needs
16000 cells a side and is held by review (cc_payload_bytes and the host writer both cast the run count to u16)."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import depthmapx_amd as dmx
from depthmapx_amd import _native as N
from depthmapx_amd import graphio
from depthmapx_amd._native import DmxError
from golden_io import case_input_lines, load_case

pytestmark = pytest.mark.gpu

DMX_ERR_ARG, DMX_ERR_STATE = -1, -4
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_CASES = ["kat", "syn32", "gallery", "syn64"]
_CACHE = {}


def _cols(attrs, locked_first=True):
    return [(name, attrs[:, j], locked_first and j == 0) for j, name in enumerate(dmx.MAKEGRAPH_COLUMNS)]


def _host(pm, c, cols, **kw):
    return graphio.write_chunk(pm, c["bins"], c["runs"], c["gridconn"], cols, **kw)


def _renamed(blob, name):
    """dmx_chunk_parse + dmx_chunk_set_name + dmx_chunk_serialize: what the CLI did for a map with a name of its own."""
    c = graphio._Chunk(blob)
    N.check(N.lib().dmx_chunk_set_name(c.h, name.encode()))
    size = ctypes.c_int64()
    N.check(N.lib().dmx_chunk_serialize(c.h, None, 0, ctypes.byref(size)))
    buf = np.zeros(size.value, dtype=np.uint8)
    N.check(N.lib().dmx_chunk_serialize(c.h, N.ptr(buf), size.value, ctypes.byref(size)))
    return buf.tobytes()


def _first_diff(a, b):
    if a == b:
        return None
    n = min(len(a), len(b))
    x = np.frombuffer(a, np.uint8, n) != np.frombuffer(b, np.uint8, n)
    return "lengths %d / %d, first differing byte %s" % (len(a), len(b), int(np.argmax(x)) if x.any() else n)


def _same(a, b):
    assert a == b, _first_diff(a, b)


def _case(ctx, name):
    """A golden case's map, its graph made on the GPU, the graph's host copy and the golden arrays."""
    key = ("case", name)
    if key not in _CACHE:
        meta, A = load_case(name)
        lines = case_input_lines(meta)
        pm = dmx.PointMap(meta["region"], lines, meta["spacing"])
        for f in meta["fills"]:
            assert pm.make_points(*f)
        g = pm.make_graph(ctx)
        _CACHE[key] = dict(meta=meta, A=A, lines=lines, pm=pm, g=g, c=g.copy(), region=meta["region"])
    return _CACHE[key]


# ---------------------------------------------------------------- 1: encode, reference and host writer
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_encode_equals_host_writer_and_reference(ctx, name):
    K = _case(ctx, name)
    pm, g, c = K["pm"], K["g"], K["c"]
    cols = _cols(c["attrs"])
    blob = g.write_chunk(cols)
    _same(blob, _host(pm, c, cols))
    assert len(blob) == int(K["A"]["pm_chunk_size"][0])
    assert hashlib.sha256(blob).digest() == K["A"]["pm_chunk_sha256"].tobytes()
    # the writer's options
    _same(g.write_chunk(cols, boundary=True), _host(pm, c, cols, boundary=True))
    _same(g.write_chunk(cols, displayed=-1), _host(pm, c, cols, displayed=-1))
    _same(g.write_chunk(cols, displayed=2), _host(pm, c, cols, displayed=2))
    _same(g.write_chunk([]), _host(pm, c, []))
    rng = np.random.default_rng(1)
    mask = (rng.random(len(c["attrs"])) < 0.5).astype(np.uint8)
    masked = [(n, v, lk, mask if j == 1 else None) for j, (n, v, lk) in enumerate(cols)]
    _same(g.write_chunk(masked, displayed=1), _host(pm, c, masked, displayed=1))
    # a map with a name of its own: parse + set_name + serialise of the host writer's chunk
    for disp in (0, 2, -1):
        _same(g.write_chunk(cols, displayed=disp, name="VGA Map 1"), _renamed(_host(pm, c, cols, displayed=disp), "VGA Map 1"))
    _same(g.write_chunk(cols, name="VGA Map"), blob)


# ---------------------------------------------------------------- 2: cells that are not plain filled cells
def _mixed(ctx):
    """A 41 x 41 map with occluders (blocked cells, cells the fill does not reach), a SEMIFILL fill and twelve merge
    links, one of them ending in the last cell of a column."""
    if "mixed" not in _CACHE:
        W = 40
        rng = np.random.default_rng(3)
        # a closed box the fill cannot enter, and twelve occluders; no border, so the grid's outer cells are filled
        lines = [[10.3, 10.3, 14.7, 10.3], [14.7, 10.3, 14.7, 14.7], [14.7, 14.7, 10.3, 14.7], [10.3, 14.7, 10.3, 10.3]]
        for _ in range(12):
            c, a, h = rng.uniform(4, 36, 2), rng.uniform(0, np.pi), rng.uniform(1, 4)
            lines.append([c[0] - h * np.cos(a), c[1] - h * np.sin(a), c[0] + h * np.cos(a), c[1] + h * np.sin(a)])
        lines = np.array(lines, dtype=np.float64)
        region = [0.0, 0.0, float(W), float(W)]
        pm = dmx.PointMap(region, lines, 1.0)
        assert pm.make_points(0.5, 0.5, fill_type=dmx.PointMap.SEMIFILL)
        pm.cell_lines()   # blockLines
        st = pm.state()
        rows = pm.rows
        assert (st & 8).any() and (st & 4).any() and ((st & 2) == 0).any(), "no CONTEXTFILLED / BLOCKED / unfilled cell"
        filled = np.flatnonzero(st & 2)
        top = filled[filled % rows == rows - 1]
        assert len(top), "no filled cell at the end of a column"
        rng = np.random.default_rng(3)
        others = rng.choice(np.setdiff1d(filled, top[-1:]), size=23, replace=False)
        pairs = np.concatenate([others, top[-1:]]).reshape(-1, 2).astype(np.int32)
        assert (pairs[-1, 1] % rows) == rows - 1
        pm.set_merges(pairs)
        g = pm.make_graph(ctx)
        _CACHE["mixed"] = dict(pm=pm, g=g, c=g.copy(), region=region, lines=lines, pairs=pairs)
    return _CACHE["mixed"]


def test_encode_unfilled_blocked_semifilled_and_linked_cells(ctx):
    K = _mixed(ctx)
    cols = _cols(K["c"]["attrs"])
    blob = K["g"].write_chunk(cols)
    _same(blob, _host(K["pm"], K["c"], cols))
    assert graphio.scan_chunk(blob)["nnodes"] < K["pm"].cols * K["pm"].rows


# ---------------------------------------------------------------- 3: inexact coordinates
def _os07(ctx):
    if "os07" not in _CACHE:
        from test_gpu_longsight import _room_graph, _room_inputs
        pm, g = _room_graph(ctx, "os07")
        region, lines, spacing, fill = _room_inputs("os07")
        assert spacing == 0.7
        _CACHE["os07"] = dict(pm=pm, g=g, c=g.copy(), region=region, lines=lines)
    return _CACHE["os07"]


def test_encode_locations_on_inexact_coordinates(ctx):
    """m_location is bottom left + spacing * x in FP64, one multiply and one add, at every cell: byte for byte the
    host's doubles on the os07 origin with spacing 0.7."""
    K = _os07(ctx)
    cols = _cols(K["c"]["attrs"])
    _same(K["g"].write_chunk(cols), _host(K["pm"], K["c"], cols))


# ---------------------------------------------------------------- 4: format limits on fabricated graphs
def _from_runs(ctx, pm, bins, runs, gridconn, attrs):
    bins = np.ascontiguousarray(bins, dtype=np.int32)
    runs = np.ascontiguousarray(runs, dtype=np.int16).reshape(-1, 4)
    gridconn = np.ascontiguousarray(gridconn, dtype=np.uint8)
    attrs = np.ascontiguousarray(attrs, dtype=np.float32)
    h = ctypes.c_void_p()
    N.check(N.lib().dmx_graph_from_runs(ctx.h, pm.h, len(bins), N.ptr(bins), N.ptr(runs) if len(runs) else None,
                                        len(runs), N.ptr(gridconn), N.ptr(attrs), ctypes.byref(h)))
    return dmx.Graph(h, ctx, pm)


def _empty_map(cols, rows):
    """A cols x rows grid without occluders, every cell filled."""
    region = [0.0, 0.0, float(cols - 1), float(rows - 1)]
    pm = dmx.PointMap(region, np.zeros((0, 4)), 1.0)
    assert pm.make_points(0.4, 0.4)
    assert (pm.cols, pm.rows) == (cols, rows) and pm.info()["filled"] == cols * rows
    return pm, region


def _fabricated(ctx, which):
    """which = "wide": a 4200 x 2 map whose node 0 holds a bin whose count is 65536 (with runs: the u16 is 0, no
    payload), a bin with a later run of 4150 cells (length & 0xFFF), a vertical bin with column shifts of 15, 16
    and 40, both diagonal bins, a one-run bin; node 1 a one-cell run; node 2 a bin of 1500 runs (a record longer than a
    4096-byte slab); every other node 32 empty bins.
    which = "tall": a 3 x 80 map whose node 0 holds a horizontal bin with row shifts of 15, 16 and 40."""
    key = ("fab", which)
    if key in _CACHE:
        return _CACHE[key]
    pm, region = _empty_map(4200, 2) if which == "wide" else _empty_map(3, 80)
    n = pm.info()["filled"]
    bins = np.zeros((n, 32, 4), dtype=np.int32)
    runs = []

    def put(k, b, count, rr, dist):
        bins[k, b, 1] = count
        bins[k, b, 2] = np.float32(dist).view(np.int32)
        bins[k, b, 3] = len(rr)
        runs.extend(rr)
    if which == "wide":
        put(0, 0, 65536, [(1, 0, 30, 0), (1, 1, 40, 1)], 39.5)                     # count wraps to 0
        put(0, 1, 4193, [(5, 0, 45, 0), (40, 1, 4190, 1)], 4190.25)                # a later run of 4150 cells
        put(0, 4, 2, [(0, 0, 1, 1)], 1.4142135)                                     # DIR_PD
        put(0, 6, 8, [(0, 0, 0, 1), (15, 0, 15, 1), (31, 0, 31, 1), (71, 1, 71, 1)], 71.0)   # column shifts 15, 16, 40
        put(0, 12, 2, [(0, 1, 1, 0)], 1.4142135)                                    # DIR_ND
        put(0, 17, 4200, [(0, 0, 4199, 0)], 4199.0)                                 # one run, longer than 4095
        put(1, 31, 1, [(7, 1, 7, 1)], 6.0)
        put(2, 3, 3000, [(i % 50, i & 1, i % 50 + 1, i & 1) for i in range(1500)], 50.0)   # a record of 6 KB
    else:
        put(0, 2, 12, [(0, 0, 2, 0), (0, 15, 2, 15), (1, 31, 2, 31), (0, 71, 1, 71)], 71.5)   # row shifts 15, 16, 40
        put(0, 20, 3, [(0, 77, 2, 79)], 2.8)
    rng = np.random.default_rng(4)
    gridconn = rng.integers(0, 256, n).astype(np.uint8)
    attrs = rng.random((n, 3), dtype=np.float32)
    runs = np.array(runs, dtype=np.int16).reshape(-1, 4)
    g = _from_runs(ctx, pm, bins, runs, gridconn, attrs)
    _CACHE[key] = dict(pm=pm, g=g, c=g.copy(), region=region, lines=np.zeros((0, 4)))
    return _CACHE[key]


@pytest.mark.parametrize("which", ["wide", "tall"])
def test_encode_format_limits(ctx, which):
    K = _fabricated(ctx, which)
    c = K["c"]
    assert (c["bins"][:, :, 3].sum(axis=1) == 0).sum() >= len(c["bins"]) - 3, "the other nodes hold 32 empty bins"
    cols = _cols(c["attrs"])
    blob = K["g"].write_chunk(cols)
    _same(blob, _host(K["pm"], c, cols))
    doc = graphio.read_chunk(blob)
    if which == "wide":
        assert c["bins"][0, 0, 1] == 0 and c["bins"][0, 0, 3] == 2   # the count wrapped, the runs are not written
        assert doc["bins"][0, 0, 3] == 0
        assert doc["runs"][1, 2] - doc["runs"][1, 0] == 4150 & 0xFFF   # the long later run comes back cut
        np.testing.assert_array_equal(doc["runs"][3:7, 0], [0, 15, 15 + (16 & 15), 15 + (16 & 15) + (40 & 15)])
    else:
        np.testing.assert_array_equal(doc["runs"][:4, 1], [0, 15, 15 + (16 & 15), 15 + (16 & 15) + (40 & 15)])


def test_encode_refuses_a_count_without_runs(ctx):
    pm, _ = _empty_map(6, 5)
    n = 30
    bins = np.zeros((n, 32, 4), dtype=np.int32)
    bins[3, 9, 1] = 5
    g = _from_runs(ctx, pm, bins, np.zeros((0, 4), np.int16), np.zeros(n, np.uint8), np.zeros((n, 3), np.float32))
    c = g.copy()
    with pytest.raises(DmxError) as host:
        _host(pm, c, [])
    with pytest.raises(DmxError) as dev:
        g.write_chunk([])
    assert dev.value.status == host.value.status == DMX_ERR_ARG
    assert str(dev.value) == str(host.value) and "bin with a node count but no runs" in str(dev.value)


def test_encode_refuses_a_shard(ctx):
    K = _case(ctx, "kat")
    n = K["g"].info()["nnodes"]
    shard = K["pm"].make_graph(ctx, node_begin=0, node_end=n // 2)
    with pytest.raises(DmxError) as e:
        shard.write_chunk([])
    assert e.value.status == DMX_ERR_STATE


# ---------------------------------------------------------------- the chunks the decoder is run on
def _record_bytes(bins):
    """Bytes of each node's Point record, from the parsed bins (the sizes the encoder's size pass computes)."""
    count, nr, d = bins[:, :, 1] & 0xFFFF, bins[:, :, 3] & 0xFFFF, bins[:, :, 0]
    pay = np.where(count == 0, 0, np.where((d & 12) != 0, 6, 8 + 4 * np.maximum(nr - 1, 0)))
    return 34 + 32 * 11 + 128 + pay.sum(axis=1)


def _with_occlusion(blob, seed=3):
    n = graphio.read_chunk(blob)["nnodes"]
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 4, size=(n, 32)).astype(np.int32)
    pix = rng.integers(0, 1 << 20, size=int(counts.sum())).astype(np.int32)
    return graphio.set_chunk_occlusion(blob, rng.random((n, 32), dtype=np.float32), counts, pix)


def _chunk(ctx, name):
    """(chunk bytes, region, drawing lines) of a decode case; made once."""
    key = ("chunk", name)
    if key not in _CACHE:
        if name in GOLDEN_CASES or name == "syn128":
            K = _case(ctx, name)
        elif name == "occlusion":
            K = _case(ctx, "syn32")
        elif name == "mixed":
            K = _mixed(ctx)
        elif name == "os07":
            K = _os07(ctx)
        else:
            K = _fabricated(ctx, name)
        blob = K["g"].write_chunk(_cols(K["c"]["attrs"]))
        if name == "occlusion":
            plain, blob = blob, _with_occlusion(blob)
            assert len(blob) > len(plain)
        _CACHE[key] = (blob, K["region"], K["lines"])
    return _CACHE[key]


DECODE_CASES = GOLDEN_CASES + ["mixed", "os07", "wide", "tall", "occlusion", "syn128"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_decoded(ctx, blob, region, pm2, g2):
    """(pm2, g2) from load_chunk_device against the parser and dmx_chunk_load."""
    doc = graphio.read_chunk(blob)
    c2 = g2.copy()
    np.testing.assert_array_equal(c2["runs"], doc["runs"])
    np.testing.assert_array_equal(c2["bins"][:, :, 1:], doc["bins"][:, :, 1:])
    has = doc["bins"][:, :, 3] > 0   # (a graph keeps no direction for a bin without runs)
    np.testing.assert_array_equal(c2["bins"][:, :, 0][has], doc["bins"][:, :, 0][has])
    np.testing.assert_array_equal(c2["gridconn"], doc["gridconn"])
    by_name = {n: v for (n, v, _) in doc["columns"]}
    for j, n in enumerate(dmx.MAKEGRAPH_COLUMNS):
        np.testing.assert_array_equal(_bits(c2["attrs"][:, j]), _bits(by_name[n]))
    np.testing.assert_array_equal(pm2.state(), doc["state"])
    assert pm2.spacing == doc["spacing"]
    pm1, g1 = graphio.load_chunk(ctx, blob, region)
    c1 = g1.copy()
    for k in ("bins", "runs", "gridconn"):
        np.testing.assert_array_equal(c2[k], c1[k])
    np.testing.assert_array_equal(_bits(c2["attrs"]), _bits(c1["attrs"]))
    assert g2.info() == g1.info()
    # the host writer over either map gives the same bytes: the merge links are the chunk's
    cols = [(n, v, lk) for (n, v, lk) in doc["columns"]]
    again = _host(pm2, doc, cols)
    _same(again, _host(pm1, doc, cols))
    # and the encoder on the decoded graph equals the host writer on the decoded arrays (the quirk is idempotent)
    # (the graph's own arrays: a bin the file gives a direction but no runs has none in a graph)
    _same(g2.write_chunk(cols), _host(pm2, c2, cols))
    return doc, c2


# ---------------------------------------------------------------- 5: slabs
def _assert_slabbed(ctx, monkeypatch, K, name, slabs, longer_than):
    """Encode and decode with the slab shrunk to each of `slabs` bytes are bit-identical to the default; at least one
    node record is longer than `longer_than` bytes (sizes from the parsed bins, as the encoder's size pass has them)."""
    blob, region, _ = _chunk(ctx, name)
    doc = graphio.read_chunk(blob)
    assert _record_bytes(doc["bins"]).max() > longer_than, "no node record is longer than the slab"
    _, g0 = graphio.load_chunk_device(ctx, blob, region)
    c0 = g0.copy()
    for slab in slabs:
        monkeypatch.setenv("DMX_CODEC_SLAB", str(slab))
        _same(K["g"].write_chunk(_cols(K["c"]["attrs"])), blob)
        pm2, g2 = graphio.load_chunk_device(ctx, blob, region)
        c2 = g2.copy()
        for k in ("bins", "runs", "gridconn"):
            np.testing.assert_array_equal(c2[k], c0[k])
        np.testing.assert_array_equal(_bits(c2["attrs"]), _bits(c0["attrs"]))
        np.testing.assert_array_equal(c2["runs"], doc["runs"])
        np.testing.assert_array_equal(pm2.state(), doc["state"])


def test_slabs_on_syn64(ctx, monkeypatch):
    """DMX_CODEC_SLAB=4096 on syn64; its longest record has 2270 bytes, so also 1024 (records span slabs) and a slab
    that is no multiple of four bytes."""
    _assert_slabbed(ctx, monkeypatch, _case(ctx, "syn64"), "syn64", (4096, 1024, 1499), longer_than=1499)


def test_slab_of_4096_bytes_and_a_longer_record(ctx, monkeypatch):
    _assert_slabbed(ctx, monkeypatch, _fabricated(ctx, "wide"), "wide", (4096, 4099), longer_than=4099)


# ---------------------------------------------------------------- 6: decode
@pytest.mark.parametrize("name", DECODE_CASES)
def test_decode_equals_parser(ctx, name):
    blob, region, _ = _chunk(ctx, name)
    pm2, g2 = graphio.load_chunk_device(ctx, blob, region)
    doc, c2 = _assert_decoded(ctx, blob, region, pm2, g2)
    if name == "syn128":
        c = _case(ctx, name)["c"]
        moved = int(np.any(doc["runs"] != c["runs"], axis=1).sum())
        assert moved > 0, "the round trip moved no run"
    if name == "occlusion":   # skipped, not lost: the graph is the one of the chunk without it
        plain, _, _ = _chunk(ctx, "syn32")
        _, g3 = graphio.load_chunk_device(ctx, plain, region)
        c3 = g3.copy()
        for k in ("bins", "runs", "gridconn"):
            np.testing.assert_array_equal(c2[k], c3[k])
    if name == "mixed":   # cells without a node, and the links on the decoded map
        assert len(doc["state"]) > doc["nnodes"]
        st2 = pm2.state()
        assert (st2 & 8).any() and ((st2 & 2) == 0).any()


def test_decode_refuses_an_unprocessed_map_and_damage(ctx):
    good, region, _ = _chunk(ctx, "kat")
    with pytest.raises(DmxError) as e:
        graphio.load_chunk_device(ctx, good[:-1], region)
    assert e.value.status == DMX_ERR_ARG
    flags = bytearray(good)
    flags[-2] = 0   # m_processed
    with pytest.raises(DmxError) as e:
        graphio.load_chunk_device(ctx, bytes(flags), region)
    assert e.value.status == DMX_ERR_STATE
    with pytest.raises(DmxError) as h:
        graphio.load_chunk(ctx, bytes(flags), region)
    assert str(h.value) == str(e.value)


# ---------------------------------------------------------------- 7: one analysis on top
def test_vga_on_the_device_loaded_graph(ctx):
    import torch
    K = _case(ctx, "syn128")
    blob, region, lines = _chunk(ctx, "syn128")
    n = K["g"].info()["nnodes"]
    nodes = np.linspace(0, n - 1, 32).astype(np.int64)

    def run(loader, drawing):
        pm, g = loader(ctx, blob, region, lines=lines if drawing else None)
        out = torch.full((n, 7), -7.0, dtype=torch.float32, device="cuda")
        g.vga_visual_global_device_list(out.data_ptr(), nodes)
        torch.cuda.synchronize()
        return out.cpu().numpy()[nodes]
    for drawing in (False, True):
        got, want = run(graphio.load_chunk_device, drawing), run(graphio.load_chunk, drawing)
        assert (want[:, 5] > 0).all()
        np.testing.assert_array_equal(_bits(got), _bits(want))


# ---------------------------------------------------------------- 8: the CLI's VISPREP -pm
def test_cli_second_named_map_bytes(ctx, tmp_path):
    """dmxcli VISPREP adding a second map ("VGA Map 1") with its graph to a file that has one: the new map's chunk is
    parse / set_name / serialise of the host writer's chunk, as before the CLI wrote it from the device graph."""
    import lzma
    import graphfile_util as gu
    cli = os.path.join(os.path.dirname(HERE), "depthmapx_amd", "_lib", "dmxcli")
    src = str(tmp_path / "gallery_empty.graph")
    with lzma.open(os.path.join(HERE, "golden", "graphfiles", "inputs", "gallery_empty.graph.xz")) as f, open(src, "wb") as o:
        o.write(f.read())
    one, two = str(tmp_path / "one.graph"), str(tmp_path / "two.graph")
    for (a, b, grid) in ((src, one, "0.08"), (one, two, "0.1")):
        r = subprocess.run([cli, "-f", a, "-o", b, "-m", "VISPREP", "-pg", grid, "-pp", "1.32,7.24", "-pm"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    lib = N.lib()
    h = ctypes.c_void_p()
    N.check(lib.dmx_graphfile_read(two.encode(), ctypes.byref(h)))
    try:
        region = np.zeros(4)
        nl, npm, disp = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        N.check(lib.dmx_graphfile_info(h, None, None, N.ptr(region), ctypes.byref(nl), ctypes.byref(npm), ctypes.byref(disp)))
        assert (npm.value, disp.value) == (2, 1)
        lines = np.zeros((nl.value, 4))
        N.check(lib.dmx_graphfile_lines(h, N.ptr(lines)))
        buf, size = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_int64()
        N.check(lib.dmx_graphfile_pointmap(h, 1, ctypes.byref(buf), ctypes.byref(size)))
        got = ctypes.string_at(buf, size.value)
    finally:
        lib.dmx_graphfile_free(h)
    assert got[4:13] == b"VGA Map 1"
    pm = dmx.PointMap(region, lines, 0.1)
    assert pm.make_points(1.32, 7.24)
    g = pm.make_graph(ctx)
    c = g.copy()
    _same(got, _renamed(_host(pm, c, _cols(c["attrs"])), "VGA Map 1"))
    assert gu.parse(open(two, "rb").read())["maps"][0]["name"] == "VGA Map"
