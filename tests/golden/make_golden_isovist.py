"""Fixtures for the VGA isovist analysis (-vm isovist) from the real reference.  Run by hand where the reference
library exists (oracle/_ref/libsalaref.a, made by oracle/Makefile); never by build(), by a test or on a GPU
machine.

The driver tests/golden/ref_isovist.cpp (our own code over the reference's public classes) is compiled into a
temporary directory with the REFFLAGS of oracle/Makefile plus -fno-builtin, and run with K = 16 variants of the
reference (pafsrand seeds; acos / sin / cos nudged by 0 or +-1 ulp) on

  generic cases   syn16, syn32, syn64, syn128, kat (spacing and fill of tests/golden/cases.json) and syn16semi
                  (syn16 filled with SEMIFILL: context-filled cells at odd PixelRefs are skipped)
  axis16          inputs/axis16.csv at spacing 0.5: axis-aligned walls whose ends are collinear with cell
                  centres, where the reference's own result depends on its RNG state and on libm's last bit

and stores under tests/golden/isovist/
  <case>_isovist.npy    float32 [N][8], the columns in table order (Isovist Area, Compactness, Drift Angle, Drift
                        Magnitude, Max Radial, Min Radial, Occlusivity, Perimeter), row (node) order
  <case>_occ.npz        occ_dist float32 [N][32], occ_counts int32 [N][32], occ_pixels int32 [total]
  syn16semi_state.npy   Point::m_state of the SEMIFILL map (x-major)
  axis16_stable.npy     bool [N]: all K variants agree bitwise on the cell's columns, lists and distances
  syn16_isovist.graph.xz  the .graph the reference writes after the analysis
  meta.json             per case: nodes, grid, the reference's wall time, unstable cells and S, the largest number
                        of cells that a single variant changed and no other did

It asserts zero unstable cells for every generic case and at most 25 % for axis16.

    python tests/golden/make_golden_isovist.py [case ...]
"""
import json
import lzma
import os
import re
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REPO)
from make_golden import CASES as MAP_CASES, parse_grid  # noqa: E402

OUT = os.path.join(HERE, "isovist")
REF_LIB = os.path.join(REPO, "oracle", "_ref", "libsalaref.a")
K = 16
# name: (lines csv, spacing, fill, fill type, write the .graph)
CASES = {n: (MAP_CASES[n][0], MAP_CASES[n][1], MAP_CASES[n][2][0], 0, n == "syn16")
         for n in ["kat", "syn16", "syn32", "syn64", "syn128"]}
CASES["syn16semi"] = (MAP_CASES["syn16"][0], 1.0, "0.5,0.5", 1, False)
CASES["axis16"] = ("inputs/axis16.csv", 0.5, "0.5,0.5", 0, False)
DEGENERATE = {"axis16": 0.25}   # the cap on the unstable share


def ref_flags():
    mk = open(os.path.join(REPO, "oracle", "Makefile")).read()
    ref = re.search(r"^REF\s*\?=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^REFFLAGS\s*:=\s*(.*)$", mk, re.M).group(1)
    return flags.replace("$(REF)", ref).split()


def build_driver(tmp):
    exe = os.path.join(tmp, "ref_isovist")
    cmd = [os.environ.get("CXX", "g++")] + ref_flags() + ["-fno-builtin", os.path.join(HERE, "ref_isovist.cpp"), "-o", exe,
                                                        "-Wl,--start-group", REF_LIB, "-Wl,--end-group", "-ldl"]
    print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return exe


def save_npz(path, **arrays):
    """An .npz with LZMA members (numpy.load reads it): syn128's occ distances stay under the size limit of a
    committed file, which deflate misses."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_LZMA) as z:
        for k, a in arrays.items():
            with z.open(k + ".npy", "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.ascontiguousarray(a), allow_pickle=False)


def run_case(exe, name, tmp):
    src, spacing, fill, filltype, write = CASES[name]
    d = os.path.join(tmp, name)
    os.makedirs(d)
    cmd = [exe, "--lines", os.path.join(HERE, src), "--spacing", str(spacing), "--fill", fill, "--filltype",
           str(filltype), "--variants", str(K), "--out", d]
    if write:
        cmd += ["--write", os.path.join(OUT, name + "_isovist.graph")]
    print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    g = parse_grid(os.path.join(d, "grid.txt"))
    n = int(g["nodes"])
    rd = lambda f, dt: np.fromfile(os.path.join(d, f), dtype=dt)
    iso = rd("isovist.bin", np.float32).reshape(n, 8)
    occ_dist = rd("occ_dist.bin", np.float32).reshape(n, 32)
    occ_counts = rd("occ_counts.bin", np.int32).reshape(n, 32)
    occ_pixels = rd("occ_pixels.bin", np.int32)
    assert occ_counts.sum() == len(occ_pixels)
    h = rd("hashes.bin", np.uint64).reshape(K, n)
    stable = (h == h[0]).all(axis=0)
    unstable = int((~stable).sum())
    # S: cells where exactly one variant deviates from the K - 1 others, which agree; the most for one variant
    S = 0
    for v in range(K):
        others = np.delete(h, v, axis=0)
        alone = (others == others[0]).all(axis=0) & (h[v] != others[0])
        S = max(S, int(alone.sum()))
    if name in DEGENERATE:
        assert unstable <= DEGENERATE[name] * n, (name, unstable, n)
        np.save(os.path.join(OUT, name + "_stable.npy"), stable)
    else:
        assert unstable == 0, (name, unstable)
    np.save(os.path.join(OUT, name + "_isovist.npy"), iso)
    save_npz(os.path.join(OUT, name + "_occ.npz"), occ_dist=occ_dist, occ_counts=occ_counts, occ_pixels=occ_pixels)
    if write:
        path = os.path.join(OUT, name + "_isovist.graph")
        with open(path, "rb") as f, lzma.open(path + ".xz", "w") as o:
            o.write(f.read())
        os.remove(path)
    if filltype:
        np.save(os.path.join(OUT, name + "_state.npy"), rd("state.bin", np.int32))
    path = os.path.join(OUT, "meta.json")
    meta = json.load(open(path)) if os.path.exists(path) else {}
    meta[name] = {"nodes": n, "ref_seconds": float(g["t_isovist"]), "variants": K, "unstable": unstable, "S": S,
                  "lines": src, "spacing": spacing, "fill": [float(v) for v in fill.split(",")], "fill_type": filltype,
                  "cols": int(g["cols"]), "rows": int(g["rows"]), "region": list(g["region"])}
    json.dump(meta, open(path, "w"), indent=1, sort_keys=True)
    print(name, n, "nodes,", unstable, "unstable, S", S, "%.3f s" % g["t_isovist"], flush=True)


def main(names):
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for n in names:
            run_case(exe, n, tmp)


if __name__ == "__main__":
    main(sys.argv[1:] or list(CASES))
