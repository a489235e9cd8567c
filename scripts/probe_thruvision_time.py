"""VGA through vision kernel time, once per accumulation variant: (A) global atomics (DMX_TV_WINDOW=0) and (B)
the LDS window (the default side, policy::kTvWindow), on syn128 (the fixture map, checked against the
reference's result), the 256^2 synthetic map and the 1000^2 benchmark map.  One JSON line per run: seconds,
lines per second, pixel steps per second.

    python scripts/probe_thruvision_time.py [--maps syn128,256,1000] [--budget 60] [--out profiles/thruvision_ab.jsonl]

A map whose full run would exceed --budget seconds (estimated from a first range of sources) is measured on a
source range only; the record then says "partial": true and the rates are those of the range.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import depthmapx_amd as dmx  # noqa: E402
from bench import load_lines  # noqa: E402


def make_map(name):
    if name == "syn128":
        from golden_io import case_input_lines, load_case
        meta, _ = load_case("syn128")
        pm = dmx.PointMap(meta["region"], case_input_lines(meta), meta["spacing"])
        for f in meta["fills"]:
            assert pm.make_points(*f)
        return pm
    W = int(name)
    pm = dmx.PointMap([0.0, 0.0, float(W), float(W)], load_lines(W, 50), 1.0)
    assert pm.make_points(0.5, 0.5)
    return pm


def run(ctx, g, name, variant, window, budget, n):
    if window is None:
        os.environ.pop("DMX_TV_WINDOW", None)
    else:
        os.environ["DMX_TV_WINDOW"] = str(window)
    # a first range of sources in the middle of the map sizes the run
    probe = max(1, min(n, 64))
    b0 = (n - probe) // 2
    t0 = time.time()
    g.vga_through_vision(src_begin=b0, src_end=b0 + probe)
    s_probe = ctx.last_timing()[1]
    est = s_probe / probe * n
    rec = {"map": name, "nodes": n, "variant": variant, "estimate_s": est}
    if est <= budget:
        b, e = 0, n
    else:
        k = max(probe, int(n * budget / est))
        b, e = (n - k) // 2, (n - k) // 2 + k
    t0 = time.time()
    out, cnt = g.vga_through_vision(src_begin=b, src_end=e, counts=True)
    wall = time.time() - t0
    s = ctx.last_timing()[1]
    st = ctx.last_stats()
    rec.update({"partial": (b, e) != (0, n), "src_begin": b, "src_end": e, "seconds": s, "wall_s": wall,
                "lines": st["tv_lines"], "pixel_steps": st["tv_pixel_steps"], "window": st["tv_window"],
                "lines_per_s": st["tv_lines"] / s if s else 0.0,
                "pixel_steps_per_s": st["tv_pixel_steps"] / s if s else 0.0,
                "max_count": int(cnt.max()) if len(cnt) else 0, "sum_count": int(cnt.sum()),
                "digest": hashlib.sha256(cnt.tobytes()).hexdigest()[:16]})
    if name == "syn128" and not rec["partial"]:
        ref = np.load(os.path.join(REPO, "tests", "golden", "thruvision", "syn128_thruvision.npy"))
        meta = json.load(open(os.path.join(REPO, "tests", "golden", "thruvision", "meta.json")))["syn128"]
        rec["equals_reference"] = bool(np.array_equal(out, ref))
        rec["ref_seconds"] = meta["ref_seconds"]
        rec["speedup_vs_reference"] = meta["ref_seconds"] / s if s else 0.0
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="syn128,256,1000")
    ap.add_argument("--budget", type=float, default=60.0, help="seconds of kernel time per run before a range is used")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "thruvision_ab.jsonl"))
    a = ap.parse_args()
    ctx = dmx.Context(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for name in a.maps.split(","):
            pm = make_map(name)
            g = pm.make_graph(ctx)
            n = g.info()["nnodes"]
            for variant, window in (("A", 0), ("B", None)):
                rec = run(ctx, g, name, variant, window, a.budget, n)
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
            g.close()


if __name__ == "__main__":
    main()
