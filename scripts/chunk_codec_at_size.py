#!/usr/bin/env python
"""The .graph PointMap chunk of the benchmark map (bench.py's synthetic 1000^2) written and read both ways in one
process, on one GPU: the host codec over the graph's host copy against the GPU codec.

    write, parent path   Graph.copy() + graphio.write_chunk
    write, new path      Graph.write_chunk                       (dmx_graph_chunk_write)
    read, parent path    dmx_chunk_parse + dmx_chunk_load
    read, new path       graphio.load_chunk_device               (dmx_chunk_load_bytes)

The two written chunks are compared by SHA-256 (one blob in memory at a time); the two loaded graphs by their bin
records and 64 spread node ranges of runs.  The new paths run first, so the peak resident set recorded after them
is theirs; the process's final peak is the parent paths'.  Writes the record (seconds, bytes, peak RSS) as JSON.

    python scripts/chunk_codec_at_size.py [--grid 1000] [--out profiles/chunk_codec_1000.json]
"""
import argparse
import ctypes
import hashlib
import json
import os
import resource
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (the benchmark's map)
import depthmapx_amd as dmx  # noqa: E402
from depthmapx_amd import _native as N  # noqa: E402
from depthmapx_amd import graphio  # noqa: E402


def peak_rss_gb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1048576.0


def note(rec, key):
    print("[chunk_codec] %s = %s" % (key, rec[key]), file=sys.stderr, flush=True)


def sample(g, ranges):
    return g.copy(runs=False)["bins"], [g.copy_range(b, e)["runs"] for (b, e) in ranges]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--occluders", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W = args.grid
    out = args.out or os.path.join(REPO, "profiles", "chunk_codec_%d.json" % W)
    region = [0.0, 0.0, float(W), float(W)]
    lines = bench.load_lines(W, args.occluders)
    ctx = dmx.Context(0)
    pm = dmx.PointMap(region, lines, 1.0)
    assert pm.make_points(0.5, 0.5)
    t = time.time()
    g = pm.make_graph(ctx)
    rec = {"grid": W, "nodes": g.info()["nnodes"], "runs": g.info()["nruns"], "makegraph_s": time.time() - t}
    note(rec, "makegraph_s")
    attrs = g.copy(runs=False)["attrs"]
    cols = [(name, attrs[:, j].copy(), j == 0) for j, name in enumerate(dmx.MAKEGRAPH_COLUMNS)]
    n = rec["nodes"]
    ranges = [(int(b), min(int(b) + 16, n)) for b in np.linspace(0, max(n - 16, 0), 64)]

    # ---- new paths
    t = time.time()
    blob = g.write_chunk(cols)
    rec["write_new_s"] = time.time() - t
    note(rec, "write_new_s")
    rec["chunk_bytes"] = len(blob)
    sha_new = hashlib.sha256(blob).hexdigest()
    t = time.time()
    sc = graphio.scan_chunk(blob)
    rec["scan_s"] = time.time() - t          # the host bin-header walk alone (part of read_new_s)
    note(rec, "scan_s")
    assert sc["nnodes"] == n
    t = time.time()
    pm2, g2 = graphio.load_chunk_device(ctx, blob, region)
    rec["read_new_s"] = time.time() - t
    note(rec, "read_new_s")
    rec["peak_rss_new_gb"] = peak_rss_gb()
    bins_new, runs_new = sample(g2, ranges)
    g2.close()
    pm2.close()

    # ---- parent paths
    t = time.time()
    c = graphio._Chunk(blob)
    hp, hg = ctypes.c_void_p(), ctypes.c_void_p()
    reg = np.ascontiguousarray(region, dtype=np.float64)
    N.check(N.lib().dmx_chunk_load(ctx.h, c.h, N.ptr(reg), ctypes.byref(hp), ctypes.byref(hg)))
    rec["read_parent_s"] = time.time() - t
    note(rec, "read_parent_s")
    pm1 = dmx.PointMap.__new__(dmx.PointMap)
    pm1.h, pm1.spacing = hp, 1.0
    g1 = dmx.Graph(hg, ctx, pm1)
    bins_par, runs_par = sample(g1, ranges)
    g1.close()
    pm1.close()
    c.close()
    rec["read_equal"] = bool(np.array_equal(bins_new, bins_par) and
                             all(np.array_equal(a, b) for a, b in zip(runs_new, runs_par)))
    del blob, c, bins_new, bins_par
    t = time.time()
    h = g.copy()
    rec["copy_parent_s"] = time.time() - t
    note(rec, "copy_parent_s")
    blob = graphio.write_chunk(pm, h["bins"], h["runs"], h["gridconn"], cols)
    rec["write_parent_s"] = time.time() - t  # Graph.copy() + graphio.write_chunk
    note(rec, "write_parent_s")
    rec["write_equal"] = hashlib.sha256(blob).hexdigest() == sha_new
    rec["sha256"] = sha_new
    rec["peak_rss_gb"] = peak_rss_gb()
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0 if rec["read_equal"] and rec["write_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
