"""Fixtures for isovists at arbitrary points (dmx_isovists) from the real reference.  Run by hand where the
reference library exists (oracle/_ref/libsalaref.a, made by oracle/Makefile); never by build(), by a test or on a
GPU machine.

The driver tests/golden/ref_isovist_points.cpp (our own code over the reference's public classes) is compiled into
a temporary directory with the REFFLAGS of oracle/Makefile plus -fno-builtin, and calls MetaGraph::makeIsovist(comm,
p, start, end, false) per point in K = 16 variants of the reference (pafsrand seeds; acos / sin / cos nudged by 0
or +-1 ulp).  Cases (drawings of tests/golden/inputs; axis16 is left out: the reference's own result is unstable
there):

  syn32   256 points drawn with a fixed seed uniformly inside the outer boundary.  Angle pairs by quarter of the
          index: full circles given as (0, 0), (a, a) and (0, 2 pi); start < end with widths from 1 to 350 degrees;
          start > end (a cone across angle 0); cones from isovist_cone / isovist_path_cones of
          depthmapx_amd.engine, some with a view angle >= 2 pi
  kat     128 points, the same mix
  syn16   the depixelated centres of its 225 filled cells, full circle

and stores under tests/golden/isovist_points/
  <case>_points.npy   float64 [n][4]  x, y, startangle, endangle as passed to makeit
  <case>_cols.npy     float32 [n][8]  the columns in table order (Isovist Area, Compactness, Drift Angle, Drift
                                      Magnitude, Max Radial, Min Radial, Occlusivity, Perimeter)
  <case>_poly.npz     off int64 [n+1], xy float64 [total][2]: the shapes' m_points
  meta.json           per case: lines, region (MetaGraph::m_region), n, variants, the reference's seconds, the
                      points replaced, and the largest spread of a vertex across the variants as a fraction of
                      that isovist's Max Radial

Conditions asserted here, so that the reference alone stays inside the tests' bounds: every kept point has at
least 3 vertices in every variant; all variants agree bitwise on the eight columns and on the vertex count of the
canonical polygon; the spread of a canonical vertex across the variants is at most a tenth of the tests' vertex
bound (1e-6 x Max Radial).  A point that fails one is replaced by the next draw of the same stream; at most 2 % of
a case's points may be replaced.  The canonical polygon (tests/isovist_points_util.py) is m_points without the
vertices the BSP tree's cuts of a wall leave on it: the raw vertex count changes with the pafsrand seed alone
(the variants agree on it for 49 of syn32's 256 first draws), so it is no property of the input.

    python tests/golden/make_golden_isovist_points.py [case ...]
"""
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REPO)
from make_golden_isovist import K, REF_LIB, ref_flags  # noqa: E402
from depthmapx_amd.engine import PointMap, isovist_cone, isovist_path_cones  # noqa: E402
from isovist_points_util import COLLINEAR, VERTEX_BOUND, canonical  # noqa: E402

OUT = os.path.join(HERE, "isovist_points")
# name: (lines csv, points or None for the cell centres, seed, spacing of the cell-centre case)
CASES = {"syn32": ("inputs/syn32.csv", 256, 3201, None), "kat": ("inputs/kat_square.csv", 128, 1501, None),
         "syn16": ("inputs/syn16.csv", None, 0, 1.0)}
VIEW_DEG = [30.0, 90.0, 120.0, 180.0, 270.0, 360.0, 400.0]
FOV = [math.pi / 3, math.pi / 2, math.pi, 2 * math.pi, 7.0]


def build_driver(tmp):
    exe = os.path.join(tmp, "ref_isovist_points")
    cmd = [os.environ.get("CXX", "g++")] + ref_flags() + ["-fno-builtin", os.path.join(HERE, "ref_isovist_points.cpp"),
                                                        "-o", exe, "-Wl,--start-group", REF_LIB, "-Wl,--end-group", "-ldl"]
    print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return exe


def read_lines(src):
    return np.loadtxt(os.path.join(HERE, src), delimiter=",", skiprows=1, dtype=np.float64).reshape(-1, 4)


def draw(rng, box, k, n):
    """Point k of n from the stream: position uniform inside the bounding box (its outermost 1 % aside), angles by
    the quarter k falls into."""
    u = rng.random(3)
    w, h = box[2] - box[0], box[3] - box[1]
    x, y = box[0] + w * (0.01 + 0.98 * u[0]), box[1] + h * (0.01 + 0.98 * rng.random())
    q, cnt = (4 * k) // n, n // 4
    j = k - q * cnt
    if q == 0:
        a = u[1] * 2 * math.pi
        s, e = [(0.0, 0.0), (a, a), (0.0, 2 * math.pi)][j % 3]
    elif q == 1:
        wd = math.radians(1.0 + 349.0 * j / (cnt - 1))
        s = u[1] * (2 * math.pi - wd)
        e = s + wd
    elif q == 2:
        wd = math.radians(5.0 + 295.0 * u[2])
        f = 0.05 + 0.9 * u[1]
        s, e = 2 * math.pi - wd * f, wd * (1.0 - f)
        assert s > e > 0
    elif j % 2 == 0:
        s, e = isovist_cone(u[1] * 360.0, VIEW_DEG[(j // 2) % len(VIEW_DEG)], degrees=True)
    else:
        t = u[1] * 2 * math.pi
        p, a = isovist_path_cones([(x, y), (x + math.cos(t), y + math.sin(t))], FOV[(j // 2) % len(FOV)])
        (x, y), (s, e) = p[0], a[0]
    return [x, y, s, e]


def run_ref(exe, src, pts, tmp, tag):
    d = os.path.join(tmp, tag)
    os.makedirs(d)
    pts.tofile(os.path.join(d, "points.bin"))
    cmd = [exe, "--lines", os.path.join(HERE, src), "--points", os.path.join(d, "points.bin"), "--n", str(len(pts)),
           "--variants", str(K), "--out", d]
    subprocess.check_call(cmd)
    n = len(pts)
    cols, cnt, xy = [], [], []
    for v in range(K):
        rd = lambda f, dt: np.fromfile(os.path.join(d, "v%d_%s.bin" % (v, f)), dtype=dt)
        cols.append(rd("cols", np.float32).reshape(n, 8))
        cnt.append(rd("cnt", np.int32))
        xy.append(rd("xy", np.float64).reshape(-1, 2))
    info = dict(l.split(None, 1) for l in open(os.path.join(d, "info.txt")))
    return cols, cnt, xy, info


def judge(cols, cnt, xy):
    """(bool [n] the points that meet the conditions, float [n] vertex spread / Max Radial)."""
    n = len(cnt[0])
    ok = np.ones(n, dtype=bool)
    spread = np.zeros(n)
    off = [np.concatenate([[0], np.cumsum(c)]) for c in cnt]
    for v in range(K):
        ok &= (cols[v].view(np.uint32) == cols[0].view(np.uint32)).all(axis=1) & (cnt[v] >= 3)
    for k in np.flatnonzero(ok):
        r = float(cols[0][k, 4])
        a = canonical(xy[0][off[0][k]:off[0][k + 1]], COLLINEAR * r)
        for v in range(1, K):
            b = canonical(xy[v][off[v][k]:off[v][k + 1]], COLLINEAR * r)
            if len(a) != len(b):
                ok[k] = False
                break
            spread[k] = max(spread[k], np.hypot(*(a - b).T).max() / r)
    ok &= spread <= 0.1 * VERTEX_BOUND
    ok &= np.isfinite(cols[0]).all(axis=1)
    return ok, spread


def run_case(exe, name, tmp):
    src, n, seed, spacing = CASES[name]
    lines = read_lines(src)
    box = [lines[:, [0, 2]].min(), lines[:, [1, 3]].min(), lines[:, [0, 2]].max(), lines[:, [1, 3]].max()]
    replaced = 0
    if n is None:
        pm = PointMap(box, lines, spacing)
        assert pm.make_points(0.5, 0.5)
        i = pm.info()
        st = pm.state().reshape(i["cols"], i["rows"])
        xs, ys = np.nonzero(st & 2)   # Point::FILLED, x-major node order
        assert len(xs) == 225
        pts = np.zeros((len(xs), 4))
        pts[:, 0] = i["bottom_left"][0] + spacing * 1.0 * xs
        pts[:, 1] = i["bottom_left"][1] + spacing * 1.0 * ys
        cols, cnt, xy, info = run_ref(exe, src, pts, tmp, name)
        ok, spread = judge(cols, cnt, xy)
        assert ok.all(), (name, np.flatnonzero(~ok))
    else:
        rng = np.random.default_rng(seed)
        pts = np.array([draw(rng, box, k, n) for k in range(n)])
        for attempt in range(8):
            cols, cnt, xy, info = run_ref(exe, src, pts, tmp, "%s_%d" % (name, attempt))
            ok, spread = judge(cols, cnt, xy)
            if ok.all():
                break
            for k in np.flatnonzero(~ok):
                pts[k] = draw(rng, box, int(k), n)
                replaced += 1
        assert ok.all() and replaced <= 0.02 * n, (name, replaced)
    region = [float(v) for v in info["region"].split()]
    assert region == [float(v) for v in box]
    os.makedirs(OUT, exist_ok=True)
    np.save(os.path.join(OUT, name + "_points.npy"), pts)
    np.save(os.path.join(OUT, name + "_cols.npy"), cols[0])
    np.savez_compressed(os.path.join(OUT, name + "_poly.npz"), off=np.concatenate([[0], np.cumsum(cnt[0])]).astype(np.int64),
                        xy=xy[0])
    path = os.path.join(OUT, "meta.json")
    meta = json.load(open(path)) if os.path.exists(path) else {}
    meta[name] = {"lines": src, "region": region, "n": len(pts), "variants": K, "ref_seconds": float(info["t_isovists"]),
                  "ref_first_seconds": float(info["t_first"]), "replaced": replaced, "max_vertex_spread": float(spread.max()),
                  "vertices": int(cnt[0].sum())}
    if spacing:
        meta[name]["spacing"] = spacing
    json.dump(meta, open(path, "w"), indent=1, sort_keys=True)
    print(name, len(pts), "points,", replaced, "replaced, spread %.3g, %d vertices" % (spread.max(), cnt[0].sum()), flush=True)


def main(names):
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for n in names:
            run_case(exe, n, tmp)


if __name__ == "__main__":
    main(sys.argv[1:] or list(CASES))
