"""Shared by the tests of isovists at arbitrary points: the fixtures of tests/golden/isovist_points/ (from the real
reference, see tests/golden/make_golden_isovist_points.py) and the comparison both the host and the GPU tests apply.

Bounds (none of them derived from the code under test):
  columns    those of tests/isovist_util.py: 1e-6 relative on Area, Compactness, Max Radial, Min Radial, Occlusivity
             and Perimeter; drift as a vector within 1e-6 x the isovist's Max Radial
  vertices   every vertex within 1e-6 x the isovist's Max Radial of the reference's (the drift bound applied to a
             point), vertex counts exactly -- on the canonical polygon, see below

The canonical polygon.  The reference's m_poly holds, next to the isovist's corners, one vertex wherever its BSP
tree happened to cut a wall the isovist sees: two adjacent blocks of one wall share an end, and makeit pushes every
block's endpoint.  Where the tree cuts depends on the state of the reference's global random generator
(BSPTree::makeLines picks pafrand() % size), so its vertex COUNT is not a function of the input: on syn32 16 runs of
the reference that differ only in the pafsrand seed agree on the count of 49 of 256 isovists, while agreeing
bitwise on all eight columns of all of them.  This engine's tree (host/bsptree.hpp) takes the first line where the
reference draws, so it is one more such variant.  What all of them share is the polygon as a set of points; its
canonical vertex list drops every vertex that lies on the segment between its kept predecessor and its successor
(within 1e-9 x Max Radial, the scale of makeit's own approxeq tolerance; a cut point is collinear to ~1e-15).
Counts and positions are compared on that list, and every raw vertex must lie on the reference polygon's boundary
within the vertex bound.
"""
import json
import os

import numpy as np

import isovist_util as iu
from golden_io import GOLDEN

ISOP = os.path.join(GOLDEN, "isovist_points")
META = json.load(open(os.path.join(ISOP, "meta.json"))) if os.path.exists(os.path.join(ISOP, "meta.json")) else {}
VERTEX_BOUND = 1e-6     # x Max Radial
COLLINEAR = 1e-9        # x Max Radial
_cache = {}


def case_lines(name):
    return np.loadtxt(os.path.join(GOLDEN, META[name]["lines"]), delimiter=",", skiprows=1, dtype=np.float64).reshape(-1, 4)


def reference(name):
    """(points [n][4], columns [n][8], off [n+1], xy [total][2]); loaded once, returned read-only."""
    if name not in _cache:
        pts = np.load(os.path.join(ISOP, name + "_points.npy"), allow_pickle=False)
        cols = np.load(os.path.join(ISOP, name + "_cols.npy"), allow_pickle=False)
        z = np.load(os.path.join(ISOP, name + "_poly.npz"), allow_pickle=False)
        r = (pts, cols, z["off"], z["xy"])
        for a in r:
            a.setflags(write=False)
        _cache[name] = r
    return _cache[name]


def _dist_seg(p, a, b):
    """Distances of the points p [k][2] to the segments a [m][2] -> b [m][2]: [k][m]."""
    d = b - a
    L2 = (d * d).sum(axis=-1)
    t = ((p[:, None, :] - a[None]) * d[None]).sum(axis=-1) / np.where(L2 > 0, L2, 1.0)
    t = np.clip(np.where(L2 > 0, t, 0.0), 0.0, 1.0)
    q = a[None] + t[..., None] * d[None]
    return np.hypot(p[:, None, 0] - q[..., 0], p[:, None, 1] - q[..., 1])


def canonical(poly, tol):
    """The closed polygon's vertex list without the vertices that lie on the segment between their kept predecessor
    and their successor (cut points of a wall, repeated points), in the list's own order."""
    pts = [tuple(p) for p in np.asarray(poly, dtype=np.float64)]
    changed = True
    while changed and len(pts) > 2:
        changed = False
        out = []
        m = len(pts)
        for i in range(m):
            prev = out[-1] if out else pts[-1]
            nxt = pts[(i + 1) % m]
            d = _dist_seg(np.array([pts[i]]), np.array([prev]), np.array([nxt]))[0, 0]
            if d <= tol:
                changed = True
                continue
            out.append(pts[i])
        pts = out
    return np.array(pts, dtype=np.float64).reshape(-1, 2)


def column_failures(cols, want):
    """bool [n]: rows whose columns miss the bounds of isovist_util (plain columns relative, drift as a vector)."""
    assert cols.shape == want.shape and cols.dtype == np.float32
    bad = ~iu._close(cols[:, iu.PLAIN], want[:, iu.PLAIN]).all(axis=1)
    ga, gm = np.deg2rad(cols[:, 2].astype(np.float64)), cols[:, 3].astype(np.float64)
    wa, wm = np.deg2rad(want[:, 2].astype(np.float64)), want[:, 3].astype(np.float64)
    d = np.hypot(gm * np.cos(ga) - wm * np.cos(wa), gm * np.sin(ga) - wm * np.sin(wa))
    return bad | ~(d <= iu.REL * want[:, 4].astype(np.float64))


def polygon_failures(off, xy, want_cols, want_off, want_xy):
    """[(row, reason)]: isovists whose polygon misses the vertex checks above."""
    assert off.dtype == np.int64 and xy.dtype == np.float64 and len(off) == len(want_off) and off[0] == 0
    assert off[-1] == len(xy)
    bad = []
    for k in range(len(off) - 1):
        r = float(want_cols[k, 4])
        got, want = xy[off[k]:off[k + 1]], want_xy[want_off[k]:want_off[k + 1]]
        cg, cw = canonical(got, COLLINEAR * r), canonical(want, COLLINEAR * r)
        if len(cg) != len(cw):
            bad.append((k, "canonical vertex count %d, reference %d" % (len(cg), len(cw))))
            continue
        d = np.hypot(*(cg - cw).T).max()
        if not d <= VERTEX_BOUND * r:
            bad.append((k, "vertex off by %.3g x Max Radial" % (d / r)))
            continue
        e = _dist_seg(got, want, np.roll(want, -1, axis=0)).min(axis=1).max()
        if not e <= VERTEX_BOUND * r:
            bad.append((k, "raw vertex %.3g x Max Radial off the reference's boundary" % (e / r)))
    return bad
