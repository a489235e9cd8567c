"""The PointMap chunk of a depthmapX .graph file (PointMap::write / PointMap::read,
salalib/pointdata.cpp:1073-1188), byte-exact, through the C ABI (include/dmx.h dmx_chunk_*).

    blob = write_chunk(pm, graph_arrays, columns, displayed=0)   # bytes
    doc = read_chunk(blob)                                        # dict of numpy arrays
    pm2, g2 = load_chunk(ctx, blob, region)                       # state-only map + device graph
"""
import ctypes

import numpy as np

from . import _native as N


def _column_args(columns, n):
    """The column arguments of dmx_chunk_write / dmx_graph_chunk_write: (ncols, names, values, locked, setmask);
    the arrays are kept alive by the tuple."""
    names = (ctypes.c_char_p * max(len(columns), 1))(*[c[0].encode() for c in columns])
    vals = np.ascontiguousarray(np.stack([np.asarray(c[1], dtype=np.float32) for c in columns]) if columns
                                else np.zeros((0, n), np.float32))
    locked = np.ascontiguousarray([1 if (len(c) > 2 and c[2]) else 0 for c in columns] or [0], dtype=np.uint8)
    masks = None
    if any(len(c) > 3 and c[3] is not None for c in columns):
        masks = np.ascontiguousarray(np.stack([np.asarray(c[3], dtype=np.uint8) if (len(c) > 3 and c[3] is not None)
                                               else np.ones(n, np.uint8) for c in columns]))
    return len(columns), names, vals, locked, masks


def write_chunk_device(g, columns, displayed=0, boundary=False, name=None):
    """PointMap::write of the graph's map with its nodes, the node records encoded on the GPU
    (dmx_graph_chunk_write): the bytes of write_chunk(pm, *g.copy()...), without the copy.  name: the map's
    name where it is not "VGA Map"."""
    n = g.info()["nnodes"]
    nc, names, vals, locked, masks = _column_args(columns, n)
    size = ctypes.c_int64()
    args = [g.h, None if name is None else name.encode(), nc, names, N.ptr(vals), N.ptr(locked), N.ptr(masks),
            int(displayed), int(bool(boundary))]
    N.check(N.lib().dmx_graph_chunk_write(*args, None, 0, ctypes.byref(size)))
    buf = np.empty(size.value, dtype=np.uint8)
    N.check(N.lib().dmx_graph_chunk_write(*args, N.ptr(buf), size.value, ctypes.byref(size)))
    return buf.tobytes()


def write_chunk(pm, bins, runs, gridconn, columns, displayed=0, boundary=False):
    """columns: list of (name, values[N] float32, locked[, setmask[N]]) in insertion order
    (MAKEGRAPH_COLUMNS after VISPREP, then the VGA columns); displayed indexes that list."""
    bins = np.ascontiguousarray(bins, dtype=np.int32)
    runs = np.ascontiguousarray(runs, dtype=np.int16).reshape(-1, 4)
    gridconn = np.ascontiguousarray(gridconn, dtype=np.uint8)
    n = bins.shape[0]
    nc, names, vals, locked, masks = _column_args(columns, n)
    size = ctypes.c_int64()
    args = [pm.h, n, N.ptr(bins), N.ptr(runs), len(runs), N.ptr(gridconn), nc, names, N.ptr(vals),
            N.ptr(locked), N.ptr(masks), int(displayed), int(bool(boundary))]
    N.check(N.lib().dmx_chunk_write(*args, None, 0, ctypes.byref(size)))
    buf = np.zeros(size.value, dtype=np.uint8)
    N.check(N.lib().dmx_chunk_write(*args, N.ptr(buf), size.value, ctypes.byref(size)))
    return buf.tobytes()


class _Chunk:
    def __init__(self, blob):
        self.buf = np.frombuffer(blob, dtype=np.uint8).copy()
        h = ctypes.c_void_p()
        N.check(N.lib().dmx_chunk_parse(N.ptr(self.buf), len(self.buf), ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            N.lib().dmx_chunk_free(self.h)
            self.h = None

    __del__ = close


def read_chunk(blob):
    c = _Chunk(blob)
    cols, rows, nc, disp = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    sp = ctypes.c_double()
    bl = np.zeros(2)
    nn, nr, used = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    N.check(N.lib().dmx_chunk_info(c.h, ctypes.byref(cols), ctypes.byref(rows), ctypes.byref(sp), N.ptr(bl),
                                   ctypes.byref(nn), ctypes.byref(nr), ctypes.byref(nc), ctypes.byref(disp),
                                   ctypes.byref(used)))
    n = nn.value
    state = np.zeros(cols.value * rows.value, dtype=np.int32)
    bins = np.zeros((n, 32, 4), dtype=np.int32)
    runs = np.zeros((max(nr.value, 1), 4), dtype=np.int16)
    gc = np.zeros(n, dtype=np.uint8)
    N.check(N.lib().dmx_chunk_arrays(c.h, N.ptr(state), N.ptr(bins), N.ptr(runs), N.ptr(gc)))
    columns = []
    for i in range(nc.value):
        name = ctypes.create_string_buffer(512)
        vals = np.zeros(n, dtype=np.float32)
        lk = ctypes.c_int()
        N.check(N.lib().dmx_chunk_column(c.h, i, name, 512, N.ptr(vals), ctypes.byref(lk)))
        columns.append((name.value.decode(), vals, bool(lk.value)))
    return dict(cols=cols.value, rows=rows.value, spacing=sp.value, bottom_left=tuple(bl), nnodes=n,
                state=state, bins=bins, runs=runs[:nr.value], gridconn=gc, columns=columns,
                displayed_sorted=disp.value, bytes_used=used.value)


def load_chunk(ctx, blob, region, lines=None):
    """(PointMap-like handle, Graph) analysing what the reference CLI's VGA / STEPDEPTH step would
    after loading the .graph (the run-length graph as decoded, 4-bit shift quirk included).  lines: the
    document's drawing, for VGA global's asymmetric mode (Graph.set_drawing)."""
    from .engine import Graph, PointMap
    c = _Chunk(blob)
    reg = np.ascontiguousarray(region, dtype=np.float64)
    hp, hg = ctypes.c_void_p(), ctypes.c_void_p()
    N.check(N.lib().dmx_chunk_load(ctx.h, c.h, N.ptr(reg), ctypes.byref(hp), ctypes.byref(hg)))
    pm = PointMap.__new__(PointMap)
    pm._region = reg
    pm._lines = np.zeros((0, 4))
    pm.h = hp
    info = read_chunk(blob)
    pm.spacing = info["spacing"]
    g = Graph(hg, ctx, pm)
    if lines is not None:
        g.set_drawing(lines)
    return pm, g


def scan_chunk(blob):
    """A walk over the chunk's records without decoding them (dmx_chunk_scan; host only): cols, rows, nnodes, nruns
    and bytes_used as read_chunk gives them, and the header's spacing and bottom_left.  DmxError(DMX_ERR_ARG) on a
    damaged chunk."""
    buf = np.frombuffer(blob, dtype=np.uint8)
    cols, rows = ctypes.c_int32(), ctypes.c_int32()
    nn, nr, used = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    N.check(N.lib().dmx_chunk_scan(N.ptr(buf), len(buf), ctypes.byref(cols), ctypes.byref(rows), ctypes.byref(nn),
                                   ctypes.byref(nr), ctypes.byref(used)))
    spacing, bl = _header_geometry(blob)
    return dict(cols=cols.value, rows=rows.value, nnodes=nn.value, nruns=nr.value, bytes_used=used.value,
                spacing=spacing, bottom_left=bl)


def _header_geometry(blob):
    """(spacing, bottom left) from the header of a chunk a scan has walked: name, spacing, rows, cols, filled,
    bottom left."""
    import struct
    o = 4 + struct.unpack_from("<I", blob, 0)[0]
    return struct.unpack_from("<d", blob, o)[0], struct.unpack_from("<dd", blob, o + 20)


def load_chunk_device(ctx, blob, region, lines=None):
    """load_chunk with the node records decoded on the GPU (dmx_chunk_load_bytes): the chunk is scanned, not
    parsed, and its bytes go to the device as they are."""
    from .engine import Graph, PointMap
    buf = np.frombuffer(blob, dtype=np.uint8)
    reg = np.ascontiguousarray(region, dtype=np.float64)
    hp, hg = ctypes.c_void_p(), ctypes.c_void_p()
    N.check(N.lib().dmx_chunk_load_bytes(ctx.h, N.ptr(buf), len(buf), N.ptr(reg), ctypes.byref(hp), ctypes.byref(hg)))
    pm = PointMap.__new__(PointMap)
    pm._region = reg
    pm._lines = np.zeros((0, 4))
    pm.h = hp
    pm.spacing = _header_geometry(blob)[0]   # (dmx_chunk_load_bytes has scanned the chunk)
    g = Graph(hg, ctx, pm)
    if lines is not None:
        g.set_drawing(lines)
    return pm, g


def chunk_occlusion(blob):
    """The isovist analysis's per-node data a chunk stores (dmx_chunk_occlusion): occ_dist float32 [N][32],
    occ_counts int32 [N][32], occ_pixels int32 [total] (packed PixelRefs by node, bin, stored order)."""
    c = _Chunk(blob)
    n = read_chunk(blob)["nnodes"]
    dist = np.zeros((n, 32), dtype=np.float32)
    counts = np.zeros((n, 32), dtype=np.int32)
    total = ctypes.c_int64()
    N.check(N.lib().dmx_chunk_occlusion(c.h, N.ptr(dist), N.ptr(counts), None, 0, ctypes.byref(total)))
    pix = np.zeros(max(total.value, 1), dtype=np.int32)
    N.check(N.lib().dmx_chunk_occlusion(c.h, None, None, N.ptr(pix), total.value, ctypes.byref(total)))
    return dict(occ_dist=dist, occ_counts=counts, occ_pixels=pix[:total.value])


def set_chunk_occlusion(blob, occ_dist, occ_counts, occ_pixels):
    """The chunk's bytes with this per-node isovist data in its node records (dmx_chunk_set_occlusion, then
    dmx_chunk_serialize); occ_dist None: the chunk serialised as it is."""
    c = _Chunk(blob)
    if occ_dist is not None:
        d = np.ascontiguousarray(occ_dist, dtype=np.float32)
        k = np.ascontiguousarray(occ_counts, dtype=np.int32)
        p = np.ascontiguousarray(occ_pixels, dtype=np.int32)
        assert k.sum() == len(p)
        N.check(N.lib().dmx_chunk_set_occlusion(c.h, N.ptr(d), N.ptr(k), N.ptr(p) if len(p) else None))
    size = ctypes.c_int64()
    N.check(N.lib().dmx_chunk_serialize(c.h, None, 0, ctypes.byref(size)))
    buf = np.zeros(size.value, dtype=np.uint8)
    N.check(N.lib().dmx_chunk_serialize(c.h, N.ptr(buf), size.value, ctypes.byref(size)))
    return buf.tobytes()
