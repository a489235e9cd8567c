"""Isovists at arbitrary points on the host: the per-point routine the HIP kernel is built from (isovist_point of
csrc/kernels/isovist_cell.hpp) over the BSP builder, compiled with plain g++ and -ffp-contract=off into the
stand-alone program tests/isovist/isovist_points_check.cpp and compared with the reference's own results
(tests/golden/isovist_points/; bounds and the canonical polygon in tests/isovist_points_util.py), and the angle
helpers of depthmapx_amd.engine.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import isovist_points_util as pu
import isovist_util as iu
from depthmapx_amd.engine import isovist_cone, isovist_path_cones

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "depthmapx_amd", "csrc")
SOURCES = [os.path.join(HERE, "isovist", "isovist_points_check.cpp"), os.path.join(CSRC, "host", "bsptree.cpp"),
           os.path.join(CSRC, "host", "pointmap.cpp")]
PI = math.pi


def _build(path, extra):
    subprocess.check_call(["g++", "-O1" if extra else "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-Wall"] + extra +
                          SOURCES + ["-o", path])
    return path


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("isovist_points") / "isovist_points_check"), [])


def _run(exe, lines, region, pts, tmp, caps=()):
    d = str(tmp)
    lines.tofile(os.path.join(d, "lines.bin"))
    np.ascontiguousarray(pts, dtype=np.float64).tofile(os.path.join(d, "points.bin"))
    cmd = [exe, "points", os.path.join(d, "lines.bin"), str(len(lines)), os.path.join(d, "points.bin"), str(len(pts))] + \
          [repr(float(v)) for v in region] + [d] + [str(c) for c in caps]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return r, None, None, None, None
    rd = lambda f, dt: np.fromfile(os.path.join(d, f), dtype=dt)
    cols = rd("cols.bin", np.float32).reshape(len(pts), 8)
    off = np.concatenate([[0], np.cumsum(rd("cnt.bin", np.int32))]).astype(np.int64)
    xy = rd("xy.bin", np.float64).reshape(-1, 2)
    info = {k: int(v) for k, v in (l.split() for l in open(os.path.join(d, "info.txt")))}
    return r, cols, off, xy, info


def _case(exe, name, tmp):
    pts = pu.reference(name)[0]
    r, cols, off, xy, info = _run(exe, pu.case_lines(name), pu.META[name]["region"], pts, tmp)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    return cols, off, xy, info


@pytest.mark.parametrize("name", ["syn32", "kat", "syn16"])
def test_fixtures(exe, tmp_path, name):
    """Columns within the bounds of isovist_util, canonical vertex counts exactly, every vertex within 1e-6 x Max
    Radial; the sink's bound 2 nb + 2 holds every push."""
    pts, want_cols, want_off, want_xy = pu.reference(name)
    m = pu.META[name]
    assert m["replaced"] <= 0.02 * m["n"] and m["max_vertex_spread"] <= 0.1 * pu.VERTEX_BOUND and m["variants"] == 16
    cols, off, xy, info = _case(exe, name, tmp_path)
    print(name, "column values that differ bitwise:", int((cols.view(np.uint32) != want_cols.view(np.uint32)).sum()),
          "raw vertex counts that differ:", int((np.diff(off) != np.diff(want_off)).sum()), info)
    bad = pu.column_failures(cols, want_cols)
    assert not bad.any(), np.flatnonzero(bad)[:10]
    assert not pu.polygon_failures(off, xy, want_cols, want_off, want_xy)
    assert info["over"] == 0 and info["max_upper"] == 2 * info["max_blocks"] + 2


def test_the_fixture_holds_every_kind_of_cone():
    p = pu.reference("syn32")[0]
    s, e = p[:, 2], p[:, 3]
    assert ((s == 0) & (e == 0)).sum() >= 20 and ((s == e) & (s != 0)).sum() >= 20 and ((s == 0) & (e == 2 * PI)).sum() >= 20
    assert ((s < e) & ~((s == 0) & (e == 2 * PI))).sum() >= 64 and (s > e).sum() >= 64
    w = np.rad2deg((e - s)[64:128])
    assert abs(w.min() - 1.0) < 1e-9 and abs(w.max() - 350.0) < 1e-9


def test_three_ways_of_asking_for_a_full_circle_give_identical_bits(exe, tmp_path):
    p = pu.reference("syn32")[0][:64, :2]
    runs = []
    for k, (s, e) in enumerate([(0.0, 0.0), (1.25, 1.25), (0.0, 2 * PI)]):
        pts = np.column_stack([p, np.full(len(p), s), np.full(len(p), e)])
        d = tmp_path / str(k)
        d.mkdir()
        r, cols, off, xy, _ = _run(exe, pu.case_lines("syn32"), pu.META["syn32"]["region"], pts, d)
        assert r.returncode == 0
        runs.append((cols, off, xy))
    for cols, off, xy in runs[1:]:
        assert np.array_equal(cols.view(np.uint32), runs[0][0].view(np.uint32))
        assert np.array_equal(off, runs[0][1]) and np.array_equal(xy.view(np.uint64), runs[0][2].view(np.uint64))


def test_a_cone_starts_or_ends_at_its_centre(exe, tmp_path):
    """start < end: the centre is the last vertex but (at most) the closing one; start > end: it is pushed once,
    in the middle.  An edge that starts at the centre gives Min Radial 0, as in the reference."""
    pts, want_cols = pu.reference("syn32")[:2]
    cols, off, xy, _ = _case(exe, "syn32", tmp_path)
    for k in range(64, 192):
        poly = xy[off[k]:off[k + 1]]
        at = np.flatnonzero((poly == pts[k, :2]).all(axis=1))
        assert len(at) == 1
        if k < 128:
            assert at[0] >= len(poly) - 2
        assert cols[k, 5] == 0.0 and want_cols[k, 5] == 0.0


@pytest.mark.parametrize("name", ["syn16", "syn32"])
def test_cell_centres_give_the_bits_of_isovist_cell(exe, tmp_path, name):
    m = iu.META[name]
    lines = iu.case_lines(name)
    lines.tofile(str(tmp_path / "lines.bin"))
    cmd = [exe, "cells", str(tmp_path / "lines.bin"), str(len(lines))] + [repr(float(v)) for v in m["region"]] + \
          [repr(float(m["spacing"]))] + [repr(float(v)) for v in m["fill"]]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert r.stdout.split() == ["cells", str(m["nodes"]), "mismatches", "0"]


def test_small_capacity_is_reported_not_truncated(exe, tmp_path):
    pts = pu.reference("syn32")[0]
    r = _run(exe, pu.case_lines("syn32"), pu.META["syn32"]["region"], pts, tmp_path, caps=(4, 8))[0]
    assert r.returncode == 3 and "capacity error" in r.stderr
    # a cone across angle 0 starts with two gaps: one entry does not hold them
    r = _run(exe, pu.case_lines("syn32"), pu.META["syn32"]["region"], pts[128:130], tmp_path, caps=(1, 1024))[0]
    assert r.returncode == 3 and "capacity error 1" in r.stderr


def test_isovist_cone_against_isovistdef():
    """Values worked by hand from IsovistDefinition::getLeftAngle / getRightAngle (isovistdef.h:38-54)."""
    assert isovist_cone(1.0, 0.5) == (0.75, 1.25)
    # wrap below 0: 0.1 - 0.5 = -0.4 -> -0.4 + 2 pi
    assert isovist_cone(0.1, 1.0) == (0.1 - 0.5 + 2 * PI, 0.1 + 0.5)
    # wrap above 2 pi: 6.2 + 0.5 = 6.7 -> 6.7 - 2 pi
    assert isovist_cone(6.2, 1.0) == (6.2 - 0.5, 6.2 + 0.5 - 2 * PI)
    left, right = isovist_cone(6.2, 1.0)
    assert left > right   # the cone spans angle 0
    # a view angle of at least 2 pi is the full circle whatever the direction
    assert isovist_cone(2.0, 2 * PI) == (0.0, 0.0) and isovist_cone(2.0, 7.0) == (0.0, 0.0)
    assert isovist_cone(2.0, math.nextafter(2 * PI, 0.0)) != (0.0, 0.0)
    # degrees as parseIsovist converts them: v / 180.0 * M_PI
    assert isovist_cone(90.0, 90.0, degrees=True) == (90.0 / 180.0 * PI - 0.5 * (90.0 / 180.0 * PI),
                                                     90.0 / 180.0 * PI + 0.5 * (90.0 / 180.0 * PI))
    assert isovist_cone(10.0, 360.0, degrees=True) == (0.0, 0.0)
    assert isovist_cone(0.0, 90.0, degrees=True) == (-0.25 * PI + 2 * PI, 0.25 * PI)


def test_isovist_path_cones_against_startendangle():
    """mgraph.cpp:523-535 per segment, from the segment's start point."""
    path = [(0.0, 0.0), (1.0, 0.0), (1.0, 2.0), (0.0, 2.0), (0.0, 1.0)]   # east, north, west, south
    pts, ang = isovist_path_cones(path, PI / 2)
    assert np.array_equal(pts, np.array(path[:-1]))
    a = [0.0, math.acos(0.0), math.acos(-1.0), 2 * PI - math.acos(0.0)]
    assert tuple(ang[0]) == (a[0] - PI / 4 + 2 * PI, a[0] + PI / 4)     # wrap below 0
    assert tuple(ang[1]) == (a[1] - PI / 4, a[1] + PI / 4)
    assert tuple(ang[2]) == (a[2] - PI / 4, a[2] + PI / 4)
    assert tuple(ang[3]) == (a[3] - PI / 4, a[3] + PI / 4)
    # wrap above 2 pi: heading south-east-ish with a wide cone
    pts, ang = isovist_path_cones([(0.0, 0.0), (3.0, -4.0)], PI)
    h = 2 * PI - math.acos(3.0 * (1.0 / 5.0))
    assert tuple(ang[0]) == (h - PI / 2, h + PI / 2 - 2 * PI) and ang[0, 0] > ang[0, 1]
    # fov >= 2 pi: makeIsovistPath leaves (0, 0), the full circle
    for fov in (2 * PI, 7.0):
        pts, ang = isovist_path_cones(path, fov)
        assert len(pts) == 4 and not ang.any()


def test_sanitized_build_runs_clean(tmp_path):
    """Address and undefined-behaviour sanitizers on the stand-alone program (never on code loaded into Python)."""
    exe = _build(str(tmp_path / "isovist_points_check_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    want_cols = pu.reference("syn32")[1]
    cols, off, xy, info = _case(exe, "syn32", tmp_path)
    assert not pu.column_failures(cols, want_cols).any() and info["over"] == 0
