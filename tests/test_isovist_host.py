"""The isovist analysis on the host: the BSP builder (csrc/host/bsptree.cpp) and the per-cell routine the HIP
kernel is built from (csrc/kernels/isovist_cell.hpp), compiled with plain g++ and -ffp-contract=off into the
stand-alone program tests/isovist/isovist_check.cpp and compared with the reference's own results
(tests/golden/isovist/).  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import isovist_util as iu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "depthmapx_amd", "csrc")
SOURCES = [os.path.join(HERE, "isovist", "isovist_check.cpp"), os.path.join(CSRC, "host", "bsptree.cpp"),
           os.path.join(CSRC, "host", "pointmap.cpp")]


def _build(path, extra):
    subprocess.check_call(["g++", "-O1" if extra else "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-Wall"] + extra +
                          SOURCES + ["-o", path])
    return path


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("isovist") / "isovist_check"), [])


def _run(exe, name, tmp, caps=()):
    m = iu.META[name]
    lines = iu.case_lines(name)
    d = os.path.join(str(tmp), name)
    os.makedirs(d, exist_ok=True)
    lines.tofile(os.path.join(d, "lines.bin"))
    cmd = [exe, os.path.join(d, "lines.bin"), str(len(lines))] + [repr(float(v)) for v in m["region"]] + \
          [repr(float(m["spacing"]))] + [repr(float(v)) for v in m["fill"]] + [str(m["fill_type"]), d] + [str(c) for c in caps]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    rd = lambda f, dt: np.fromfile(os.path.join(d, f), dtype=dt)
    n = m["nodes"]
    iso = rd("isovist.bin", np.float32).reshape(n, 8)
    occ = dict(occ_dist=rd("occ_dist.bin", np.float32).reshape(n, 32), occ_counts=rd("occ_counts.bin", np.int32).reshape(n, 32),
               occ_pixels=rd("occ_pixels.bin", np.int32))
    tree = dict(seg=rd("tree_seg.bin", np.float64).reshape(-1, 4), links=rd("tree_links.bin", np.int32).reshape(-1, 4))
    info = dict(l.split() for l in open(os.path.join(d, "info.txt")))
    return iso, occ, tree, {k: int(v) for k, v in info.items()}


@pytest.mark.parametrize("name", ["syn16", "syn32", "axis16", "kat"])
def test_tree_covers_every_line_and_keeps_its_sides(exe, tmp_path, name):
    _, _, tree, info = _run(exe, name, tmp_path)
    seg, links = tree["seg"], tree["links"]
    tag, left, right, parent = links.T
    lines = iu.case_lines(name)
    scale = np.abs(lines).max()
    assert info["tree_nodes"] == len(seg) >= (np.hypot(lines[:, 2] - lines[:, 0], lines[:, 3] - lines[:, 1]) > 0).sum()
    # every input line is covered by the pieces that carry its tag: they lie on it and their lengths add up
    plen = np.hypot(seg[:, 2] - seg[:, 0], seg[:, 3] - seg[:, 1])
    assert (plen > 0).all()
    for k, (x1, y1, x2, y2) in enumerate(lines):
        L = np.hypot(x2 - x1, y2 - y1)
        if L == 0:
            assert not (tag == k).any()
            continue
        mine = tag == k
        assert mine.any()
        for px, py in [(seg[mine, 0], seg[mine, 1]), (seg[mine, 2], seg[mine, 3])]:
            t = ((px - x1) * (x2 - x1) + (py - y1) * (y2 - y1)) / (L * L)
            off = np.abs((px - x1) * (y2 - y1) - (py - y1) * (x2 - x1)) / L
            assert (off <= 1e-9 * scale).all() and (t >= -1e-9).all() and (t <= 1 + 1e-9).all()
        assert abs(plen[mine].sum() - L) <= 1e-9 * scale
    # every node below a node's left (right) child lies left (right) of its line; links are consistent
    depth = 0
    for k in range(len(seg)):
        c, d = k, 1
        while parent[c] >= 0:
            a = parent[c]
            assert c in (left[a], right[a]) and left[a] != right[a]
            side = 1.0 if c == left[a] else -1.0
            v0 = seg[a, 2:] - seg[a, :2]
            for p in (seg[k, :2], seg[k, 2:]):
                v1 = p - seg[a, :2]
                assert side * (v0[0] * v1[1] - v0[1] * v1[0]) >= -1e-9 * scale * scale
            c = a
            d += 1
        depth = max(depth, d)
    assert (parent < 0).sum() == 1 and parent[0] < 0
    assert info["depth"] == depth


@pytest.mark.parametrize("name", ["syn16", "syn32", "syn16semi", "kat"])
def test_generic_fixtures(exe, tmp_path, name):
    """Columns within 1e-6 relative, occlusion lists exactly, occ distances within 1e-6.  With glibc on both
    sides no value differs bitwise (printed; DESIGN.md records it)."""
    iso, occ, _, info = _run(exe, name, tmp_path)
    want_iso, want_occ = iu.reference(name)
    print(name, "values that differ bitwise:", iu.bit_differences(iso, occ, want_iso, want_occ), info)
    assert not iu.failing_cells(iso, occ, want_iso, want_occ).any()
    if name == "syn16semi":
        assert (want_iso == -1).all(axis=1).sum() > 0   # the case does hold skipped cells


def test_axis_aligned_case_on_its_stable_cells(exe, tmp_path):
    iso, occ, _, _ = _run(exe, "axis16", tmp_path)
    iu.check_degenerate("axis16", iso, occ)


def test_small_capacity_is_reported_not_truncated(exe, tmp_path):
    m = iu.META["syn16"]
    lines = iu.case_lines("syn16")
    lines.tofile(str(tmp_path / "lines.bin"))
    cmd = [exe, str(tmp_path / "lines.bin"), str(len(lines))] + [repr(float(v)) for v in m["region"]] + \
          [repr(float(m["spacing"]))] + [repr(float(v)) for v in m["fill"]] + ["0", str(tmp_path), "4", "8"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 3 and "capacity error" in r.stderr


def test_sanitized_build_runs_clean(tmp_path):
    """Address and undefined-behaviour sanitizers on the stand-alone program (never on code loaded into Python)."""
    exe = _build(str(tmp_path / "isovist_check_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    iso, occ, _, _ = _run(exe, "syn16", tmp_path)
    want_iso, want_occ = iu.reference("syn16")
    assert not iu.failing_cells(iso, occ, want_iso, want_occ).any()
