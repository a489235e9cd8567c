"""dmx_chunk_scan (graphio.scan_chunk): the walk over a PointMap chunk's records that decodes nothing -- header,
attribute table, then from bin header to bin header -- and is the only code in front of the GPU decoder that
trusts nothing.  Host calls on host memory (no GPU): it must agree with the parser (read_chunk) on every chunk,
with and without occlusion data, and refuse every truncated or overrunning chunk with DMX_ERR_ARG."""
import struct

import numpy as np
import pytest

from depthmapx_amd import graphio
from depthmapx_amd._native import DmxError
from golden_io import load_case
from test_graph_chunk import _chunk, _maps

DMX_ERR_ARG = -1
_CHUNKS = {}


def _made(name):
    """The chunk of a golden case written by the host writer (as tests/test_graph_chunk.py makes it); once."""
    if name not in _CHUNKS:
        meta, _ = load_case(name)
        pm, g = _maps(meta)
        _CHUNKS[name] = _chunk(pm, g)
    return _CHUNKS[name]


def _with_occlusion(blob, seed=3):
    """The chunk with seeded isovist data in its node records: 0..3 pixels a bin, a distance a bin."""
    n = graphio.read_chunk(blob)["nnodes"]
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 4, size=(n, 32)).astype(np.int32)
    pix = rng.integers(0, 1 << 20, size=int(counts.sum())).astype(np.int32)
    return graphio.set_chunk_occlusion(blob, rng.random((n, 32), dtype=np.float32), counts, pix)


def _golden_bytes(name):
    _, A = load_case(name)
    return A["pm_chunk"].tobytes() if "pm_chunk" in A else None


def _agrees(blob):
    doc, sc = graphio.read_chunk(blob), graphio.scan_chunk(blob)
    for key in ("cols", "rows", "nnodes", "bytes_used"):
        assert sc[key] == doc[key], key
    assert sc["nruns"] == len(doc["runs"])
    assert sc["spacing"] == doc["spacing"] and tuple(sc["bottom_left"]) == tuple(doc["bottom_left"])
    assert sc["bytes_used"] == len(blob)


@pytest.mark.parametrize("name", ["kat", "syn16", "syn32"])
def test_scan_agrees_with_the_parser_on_golden_bytes(name):
    """The reference's own bytes where the fixture carries them (the host writer's equal them: test_graph_chunk)."""
    blob = _golden_bytes(name)
    if blob is None:
        blob = _made(name)
    _agrees(blob)


@pytest.mark.parametrize("name", ["gallery", "syn64"])
def test_scan_agrees_with_the_parser_on_written_chunks(name):
    _agrees(_made(name))


def test_scan_skips_occlusion_data():
    plain = _made("syn32")
    occ = _with_occlusion(plain)
    assert len(occ) > len(plain)
    _agrees(occ)
    a, b = graphio.scan_chunk(plain), graphio.scan_chunk(occ)
    assert (a["nnodes"], a["nruns"]) == (b["nnodes"], b["nruns"])


def test_scan_ignores_bytes_behind_the_chunk():
    blob = _made("kat")
    assert graphio.scan_chunk(blob + b"\x07" * 19)["bytes_used"] == len(blob)


def _refused(blob):
    with pytest.raises(DmxError) as e:
        graphio.scan_chunk(blob)
    assert e.value.status == DMX_ERR_ARG, e.value
    return str(e.value)


def test_every_prefix_of_kat_is_refused():
    blob = _golden_bytes("kat") or _made("kat")
    for n in range(1, len(blob)):
        _refused(blob[:n])


def test_seeded_prefixes_of_syn16_are_refused():
    blob = _made("syn16")
    rng = np.random.default_rng(16)
    cuts = np.unique(np.concatenate([rng.integers(1, len(blob), 300), [len(blob) - 1, len(blob) - 2, len(blob) - 3]]))
    for n in cuts:
        _refused(blob[:int(n)])


def _first_hv_payload(blob):
    """Offset of the u16 run count of the first H / V bin with runs, found by walking the first node's bins."""
    o = 4 + struct.unpack_from("<I", blob, 0)[0] + 8 + 12 + 16 + 4      # name, spacing, rows/cols/filled, bl, displayed
    o += 8 + 8
    nlayers, = struct.unpack_from("<i", blob, o)
    o += 4
    for _ in range(nlayers):
        o += 8
        o += 4 + struct.unpack_from("<I", blob, o)[0]
    ncols, = struct.unpack_from("<i", blob, o)
    o += 4
    for _ in range(ncols):
        o += 4 + struct.unpack_from("<I", blob, o)[0]
        o += 4 + 4 + 8 + 4 + 1 + 1 + 12
        o += 4 + struct.unpack_from("<I", blob, o)[0]
    nrows, = struct.unpack_from("<i", blob, o)
    o += 4
    for _ in range(nrows):
        o += 12
        o += 4 + 4 * struct.unpack_from("<I", blob, o)[0]
    o += 12
    while True:                      # cells up to the first node
        node = blob[o + 17]
        o += 18
        if node:
            break
        o += 16
    for _ in range(32):
        d, count = blob[o], struct.unpack_from("<H", blob, o + 1)[0]
        o += 11
        if count and not d & 12:
            return o
        if count:
            o += 6
    raise AssertionError("no H / V bin with runs in the first node")


def test_run_count_past_the_end_is_refused():
    """A bin whose stated run count reaches past the end of the chunk: 65535 runs are 262 KB, more than all of syn16's
    chunk has behind that bin."""
    blob = bytearray(_made("syn16"))
    o = _first_hv_payload(bytes(blob))
    assert 1 <= struct.unpack_from("<H", blob, o)[0] < 65535
    assert len(blob) - o < 8 + 4 * 65534
    struct.pack_into("<H", blob, o, 65535)
    assert "truncated" in _refused(bytes(blob))
    # the parser refuses it the same way
    with pytest.raises(DmxError) as e:
        graphio.read_chunk(bytes(blob))
    assert e.value.status == DMX_ERR_ARG
