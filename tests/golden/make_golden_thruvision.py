"""Fixtures for VGA through vision (-vm thruvision) from the real reference.  Run by hand where the reference
library exists (oracle/_ref/libsalaref.a, made by oracle/Makefile); never by build(), by a test or on a GPU
machine.

The driver tests/golden/ref_thruvision.cpp (our own code over the reference's public classes) is compiled into a
temporary directory with the REFFLAGS of oracle/Makefile and run on

  in-memory cases   lines -> grid -> fill -> makeGraph -> analyseGraph(OUTPUT_THRU_VISION):
                    kat, syn16, syn32, syn64, gallery, syn128 (the maps of tests/golden/cases.json) and two
                    corridors of 256 x 3 and 3 x 256 filled cells (inputs/corridor256x3.csv, corridor3x256.csv:
                    long lines in both major directions, many half-way points, coordinates up to 257)
  .graph cases      readFromFile -> analyseGraph -> write, as depthmapXcli -m VGA -vm thruvision does: the
                    outputs of the chains gallery_one_op and turns_remake of graphfiles/cases.json, and the
                    re-read graphs gallery_connected.graph and mixed_link.graph (4-bit-shifted runs, merge links)

and stores under tests/golden/thruvision/
  <case>_thruvision.npy   float32 [N], the "Through vision" column in row (node) order
  <corridor>.npz          the corridor maps: state, nruns, runs, lines, cols, rows, region, spacing, fill
  cases.json              the .graph cases: input, args, sha256 + size of the reference's output, columns
  meta.json               per case: nodes and the reference's wall time (single thread)

    python tests/golden/make_golden_thruvision.py [case ...]
"""
import hashlib
import json
import lzma
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REPO)
import graphfile_util as gu  # noqa: E402
from make_golden import CASES as MAP_CASES, parse_grid  # noqa: E402

OUT = os.path.join(HERE, "thruvision")
REF_LIB = os.path.join(REPO, "oracle", "_ref", "libsalaref.a")
REF_CLI = os.path.join(REPO, "oracle", "_ref", "ref_cli")
GF = os.path.join(HERE, "graphfiles")
GF_CASES = json.load(open(os.path.join(GF, "cases.json")))

# corridors: walls around [0, W] x [0, H] at spacing 1; the wall cells are blocked, the cells inside are filled
CORRIDORS = {"corridor256x3": (257, 4), "corridor3x256": (4, 257)}
MEMORY = ["kat", "syn16", "syn32", "syn64", "gallery", "syn128"] + list(CORRIDORS)
GRAPH = {
    "tv_gallery_one_op": "@gallery_one_op",
    "tv_turns_remake": "@turns_remake",
    "tv_gallery_connected": "gallery_connected.graph",
    "tv_mixed_link": "mixed_link.graph",
}
ARGS = ["-m", "VGA", "-vm", "thruvision"]


def ref_flags():
    mk = open(os.path.join(REPO, "oracle", "Makefile")).read()
    ref = re.search(r"^REF\s*\?=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^REFFLAGS\s*:=\s*(.*)$", mk, re.M).group(1)
    return flags.replace("$(REF)", ref).split()


def build_driver(tmp):
    exe = os.path.join(tmp, "ref_thruvision")
    cmd = [os.environ.get("CXX", "g++")] + ref_flags() + [os.path.join(HERE, "ref_thruvision.cpp"), "-o", exe,
                                                        "-Wl,--start-group", REF_LIB, "-Wl,--end-group"]
    print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return exe


def write_corridor_csv(name):
    W, H = CORRIDORS[name]
    path = os.path.join(HERE, "inputs", name + ".csv")
    with open(path, "w") as f:
        f.write("x1,y1,x2,y2\n")
        for l in [(0, 0, W, 0), (W, 0, W, H), (W, H, 0, H), (0, H, 0, 0)]:
            f.write("%.6f,%.6f,%.6f,%.6f\n" % tuple(float(v) for v in l))
    return path


def save_meta(name, nodes, seconds):
    path = os.path.join(OUT, "meta.json")
    meta = json.load(open(path)) if os.path.exists(path) else {}
    meta[name] = {"nodes": int(nodes), "ref_seconds": float(seconds)}
    json.dump(meta, open(path, "w"), indent=1, sort_keys=True)


def run_memory(exe, name, tmp):
    d = os.path.join(tmp, name)
    os.makedirs(d)
    if name in CORRIDORS:
        src, spacing, fills = write_corridor_csv(name), 1.0, ["1.5,1.5"]
    else:
        src, spacing, fills = MAP_CASES[name][:3]
        src = src if os.path.isabs(src) else os.path.join(HERE, src)
    cmd = [exe, "--drawing" if src.endswith(".graph") else "--lines", src, "--spacing", str(spacing), "--out", d]
    for p in fills:
        cmd += ["--fill", p]
    print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    g = parse_grid(os.path.join(d, "grid.txt"))
    tv = np.fromfile(os.path.join(d, "thruvision.bin"), dtype=np.float32)
    assert len(tv) == int(g["nodes"])
    np.save(os.path.join(OUT, name + "_thruvision.npy"), tv)
    if name in CORRIDORS:
        rd = lambda f, dt: np.fromfile(os.path.join(d, f), dtype=dt)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), state=rd("state.bin", np.int32),
                            nruns=rd("nruns.bin", np.int32), runs=rd("runs.bin", np.int16).reshape(-1, 4),
                            lines=rd("lines.bin", np.float64).reshape(-1, 4), cols=np.int32(g["cols"]),
                            rows=np.int32(g["rows"]), region=np.array(g["region"]), spacing=np.float64(spacing),
                            fill=np.array([float(v) for v in fills[0].split(",")]))
    save_meta(name, g["nodes"], g["t_thruvision"])
    print(name, len(tv), "nodes, max", tv.max(), "%.2f s" % g["t_thruvision"], flush=True)


def graph_input(name, tmp, made):
    """A committed input (graphfiles/inputs/*.xz) or the reference CLI's output of a chain of graphfiles/cases.json."""
    if not name.startswith("@"):
        dst = os.path.join(tmp, name)
        if not os.path.exists(dst):
            with lzma.open(os.path.join(GF, "inputs", name + ".xz")) as f, open(dst, "wb") as o:
                o.write(f.read())
        return dst
    case = name[1:]
    if case not in made:
        src = graph_input(GF_CASES[case]["input"], tmp, made)
        dst = os.path.join(tmp, case + ".graph")
        subprocess.check_call([REF_CLI, "-f", src, "-o", dst] + GF_CASES[case]["args"], stdout=subprocess.DEVNULL)
        b = open(dst, "rb").read()
        assert hashlib.sha256(b).hexdigest() == GF_CASES[case]["sha256"], case
        made[case] = dst
    return made[case]


def run_graph(exe, name, tmp, made):
    d = os.path.join(tmp, name)
    os.makedirs(d)
    src = graph_input(GRAPH[name], tmp, made)
    dst = os.path.join(d, "out.graph")
    subprocess.check_call([exe, "--analyse", src, "--write", dst, "--out", d])
    g = parse_grid(os.path.join(d, "grid.txt"))
    b = open(dst, "rb").read()
    tv = np.fromfile(os.path.join(d, "thruvision.bin"), dtype=np.float32)
    col = gu.columns(b, ["Through vision"])["Through vision"]
    assert np.array_equal(col, tv)
    np.save(os.path.join(OUT, name + "_thruvision.npy"), tv)
    path = os.path.join(OUT, "cases.json")
    cases = json.load(open(path)) if os.path.exists(path) else {}
    cases[name] = {"input": GRAPH[name], "args": ARGS, "gpu": True, "regression": "(VGA through vision)",
                   "size": len(b), "sha256": hashlib.sha256(b).hexdigest(), "columns": ["Through vision"],
                   "masked_sha256": gu.masked_digest(b, ["Through vision"])}
    json.dump(cases, open(path, "w"), indent=1, sort_keys=True)
    save_meta(name, g["nodes"], g["t_thruvision"])
    print(name, len(b), cases[name]["sha256"][:16], "%.2f s" % g["t_thruvision"], flush=True)


def main(names):
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        made = {}
        for n in names:
            if n in GRAPH:
                run_graph(exe, n, tmp, made)
            else:
                run_memory(exe, n, tmp)


if __name__ == "__main__":
    main(sys.argv[1:] or MEMORY + list(GRAPH))
