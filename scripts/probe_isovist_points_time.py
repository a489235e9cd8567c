"""Time of isovists at arbitrary points (dmx_isovists, isovist_points_kernel): HIP-event kernel time and the
call's wall time on the 1000^2 benchmark map's 50 lines, the points being the map's 998,001 cell centres.  One JSON
line per run; every configuration is run --repeats times after one warm-up run (which also pays the allocations).

    python scripts/probe_isovist_points_time.py --runs yardstick,order,waves [--out profiles/isovist_points.jsonl]
    python scripts/probe_isovist_points_time.py --runs polygons,cones

  yardstick  the centres in the tile order of isovist_kernel (8 x 8 tiles, row-major inside a tile), columns only,
             both launch orders (DMX_ISO_ORDER): what scripts/probe_isovist_time.py --maps 1000 measures for
             isovist_kernel, columns only
  order      the same centres in a seeded random order, the caller's order against the Morton order
  waves      the yardstick with DMX_ISO_PWAVES = 4, 8, 16 one-wave workgroups a CU
  polygons   the yardstick with polygons (vertices a point, kernel time of the last call, wall time of the whole
             Context.isovists, which calls twice when its guess was too small)
  cones      the yardstick with 90 degree cones in seeded random directions
"""
import argparse
import hashlib
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import depthmapx_amd as dmx  # noqa: E402
from bench import load_lines  # noqa: E402

W = 1000


def centres_in_tile_order(lines):
    pm = dmx.PointMap([0.0, 0.0, float(W), float(W)], lines, 1.0)
    assert pm.make_points(0.5, 0.5)
    i = pm.info()
    filled = (pm.state().reshape(i["cols"], i["rows"]) & 2) != 0   # [x][y]
    xs, ys = np.nonzero(filled)
    key = ((ys >> 3) * ((i["cols"] + 7) // 8) + (xs >> 3)) * 64 + (ys & 7) * 8 + (xs & 7)
    o = np.argsort(key, kind="stable")
    blx, bly = i["bottom_left"]
    return np.column_stack([blx + 1.0 * xs[o], bly + 1.0 * ys[o]]), [blx - 0.5, bly - 0.5, blx + i["cols"] - 0.5, bly + i["rows"] - 0.5]


def run(ctx, f, tag, lines, pts, region, repeats, angles=None, polygons=False, env=None):
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        for rep in range(-1, repeats):
            t0 = time.time()
            res = ctx.isovists(lines, pts, angles, region=region, polygons=polygons)
            wall = time.time() - t0
            if rep < 0:
                continue
            out = res[0] if polygons else res
            last = ctx.last_isovist()
            rec = {"run": tag, "points": len(pts), "repeat": rep, "wall_s": wall, "points_per_s": len(pts) / last["kernel_seconds"],
                   "digest": hashlib.sha256(out.tobytes()).hexdigest()[:16]}
            rec.update(last)
            rec.update(env or {})
            if polygons:
                rec["vertices"] = int(len(res[2]))
                rec["vertices_per_point"] = len(res[2]) / len(pts)
                rec["calls"] = 2 if len(res[2]) > ctx.ISOVIST_POLY_GUESS * len(pts) else 1
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
    finally:
        for k in (env or {}):
            os.environ.pop(k, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="yardstick,order,waves,polygons,cones")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "isovist_points.jsonl"))
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    lines = np.ascontiguousarray(load_lines(W, 50), dtype=np.float64).reshape(-1, 4)
    pts, region = centres_in_tile_order(lines)
    ctx = dmx.Context(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    rng = np.random.default_rng(1000)
    with open(a.out, "a") as f:
        for name in a.runs.split(","):
            if name == "yardstick":
                for order in ("caller", "morton"):
                    run(ctx, f, "tile order", lines, pts, region, a.repeats, env={"DMX_ISO_ORDER": order})
            elif name == "order":
                shuffled = np.ascontiguousarray(pts[rng.permutation(len(pts))])
                for order in ("caller", "morton"):
                    run(ctx, f, "random order", lines, shuffled, region, a.repeats, env={"DMX_ISO_ORDER": order})
            elif name == "waves":
                for waves in ("4", "8", "16"):
                    run(ctx, f, "tile order", lines, pts, region, a.repeats, env={"DMX_ISO_PWAVES": waves})
            elif name == "polygons":
                run(ctx, f, "tile order, polygons", lines, pts, region, a.repeats, polygons=True)
            elif name == "cones":
                ang = np.array([dmx.isovist_cone(d, math.pi / 2) for d in rng.random(len(pts)) * 2 * math.pi])
                run(ctx, f, "tile order, 90 degree cones", lines, pts, region, a.repeats, angles=ang)
            else:
                raise SystemExit("unknown run " + name)


if __name__ == "__main__":
    main()
