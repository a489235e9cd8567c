"""Shared by the isovist tests: the fixtures of tests/golden/isovist/ (from the real reference, see
tests/golden/make_golden_isovist.py) and the per-cell comparison both the host and the GPU tests apply.

Bounds (none of them derived from the code under test):
  columns      1e-6 relative, the project's VGA float bound (README), for Area, Compactness, Max Radial, Min
               Radial, Occlusivity and Perimeter
  drift        compared as a vector: mag * (cos, sin) may differ by 1e-6 x the cell's Max Radial (the angle alone
               is ill-conditioned where the magnitude is near 0, and wraps at 360)
  occlusion    counts and pixels exactly, occ distances 1e-6 relative
"""
import csv
import json
import os

import numpy as np

from golden_io import GOLDEN

ISO = os.path.join(GOLDEN, "isovist")
META = json.load(open(os.path.join(ISO, "meta.json")))
REL = 1e-6
PLAIN = [0, 1, 4, 5, 6, 7]   # Area, Compactness, Max Radial, Min Radial, Occlusivity, Perimeter
_cache = {}


def case_lines(name):
    with open(os.path.join(GOLDEN, META[name]["lines"])) as f:
        rows = list(csv.reader(f))[1:]
    return np.array(rows, dtype=np.float64).reshape(-1, 4)


def reference(name):
    """(columns [N][8], dict occ_dist / occ_counts / occ_pixels); loaded once, returned read-only."""
    if name not in _cache:
        iso = np.load(os.path.join(ISO, name + "_isovist.npy"), allow_pickle=False)
        z = np.load(os.path.join(ISO, name + "_occ.npz"), allow_pickle=False)
        occ = {k: z[k] for k in ("occ_dist", "occ_counts", "occ_pixels")}
        for a in [iso] + list(occ.values()):
            a.setflags(write=False)
        _cache[name] = (iso, occ)
    return _cache[name]


def _close(g, w):
    return np.abs(g.astype(np.float64) - w.astype(np.float64)) <= REL * np.abs(w.astype(np.float64))


def failing_cells(iso, occ, want_iso, want_occ):
    """bool [N]: the cells whose columns, occlusion lists or occ distances miss the bounds above."""
    assert iso.shape == want_iso.shape and iso.dtype == np.float32
    bad = ~_close(iso[:, PLAIN], want_iso[:, PLAIN]).all(axis=1)
    ga, gm = np.deg2rad(iso[:, 2].astype(np.float64)), iso[:, 3].astype(np.float64)
    wa, wm = np.deg2rad(want_iso[:, 2].astype(np.float64)), want_iso[:, 3].astype(np.float64)
    d = np.hypot(gm * np.cos(ga) - wm * np.cos(wa), gm * np.sin(ga) - wm * np.sin(wa))
    skipped = (want_iso == -1).all(axis=1)   # rows of cells the reference skips: every column -1, compared exactly
    bad |= ~skipped & ~(d <= REL * want_iso[:, 4].astype(np.float64))
    bad |= skipped & (iso != -1).any(axis=1)
    bad |= ~_close(occ["occ_dist"], want_occ["occ_dist"]).all(axis=1)
    bad |= (occ["occ_counts"] != want_occ["occ_counts"]).any(axis=1)
    gs = np.concatenate([[0], np.cumsum(occ["occ_counts"].sum(axis=1))])
    ws = np.concatenate([[0], np.cumsum(want_occ["occ_counts"].sum(axis=1))])
    assert gs[-1] == len(occ["occ_pixels"]) and ws[-1] == len(want_occ["occ_pixels"])
    for k in range(len(iso)):
        if not bad[k] and not np.array_equal(occ["occ_pixels"][gs[k]:gs[k + 1]], want_occ["occ_pixels"][ws[k]:ws[k + 1]]):
            bad[k] = True
    return bad


def bit_differences(iso, occ, want_iso, want_occ):
    """Values (columns and occ distances) that differ bitwise."""
    return int((iso.view(np.uint32) != want_iso.view(np.uint32)).sum() +
               (occ["occ_dist"].view(np.uint32) != want_occ["occ_dist"].view(np.uint32)).sum())


def check_degenerate(name, iso, occ):
    """The axis-aligned case: the reference itself is unstable on some cells (its result changes with its RNG
    state and with the last bit of libm).  The stable share must be at least 75 %; on the stable cells the
    comparison is the generic one, and at most 2 S + 2 of them may fail (S from meta.json: the most cells a
    single variant of the reference changed alone; this implementation's libm is one more draw from that
    population, the factor 2 the margin for it).  Returns the number of failing stable cells."""
    stable = np.load(os.path.join(ISO, name + "_stable.npy"), allow_pickle=False)
    assert stable.mean() >= 0.75
    want_iso, want_occ = reference(name)
    bad = failing_cells(iso, occ, want_iso, want_occ)
    n = int((bad & stable).sum())
    print("%s: %d of %d stable cells fail (allowed %d); %d of %d unstable cells differ" %
          (name, n, int(stable.sum()), 2 * META[name]["S"] + 2, int((bad & ~stable).sum()), int((~stable).sum())))
    assert n <= 2 * META[name]["S"] + 2
    return n
