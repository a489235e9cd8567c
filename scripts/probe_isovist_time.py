"""VGA isovist analysis time: the host BSP build and the kernels (HIP events), columns only and with the
occlusion data, on syn128 (the fixture map, checked against the reference's result) and the 1000^2 benchmark map.
One JSON line per run.

    python scripts/probe_isovist_time.py [--maps syn128,1000] [--out profiles/isovist_time.jsonl] [--waves 4,8,16]

--waves runs every map once per value of DMX_ISO_WAVES (one-wave workgroups a CU; the A/B record
profiles/isovist_ab.jsonl); without it the default of policy.hpp is measured.
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


def run(ctx, g, name, occlusion, n):
    t0 = time.time()
    res = g.vga_isovist(occlusion=occlusion)
    wall = time.time() - t0
    out, occ = res if occlusion else (res, None)
    last = ctx.last_isovist()
    rec = {"map": name, "nodes": n, "occlusion": occlusion, "wall_s": wall, "cells_per_s": n / last["kernel_seconds"]}
    rec.update(last)
    rec["digest"] = hashlib.sha256(out.tobytes()).hexdigest()[:16]
    if occlusion:
        rec["occ_pixels"] = int(len(occ["occ_pixels"]))
    if name == "syn128":
        import isovist_util as iu
        want_iso, want_occ = iu.reference("syn128")
        rec["ref_seconds"] = iu.META["syn128"]["ref_seconds"]
        rec["speedup_vs_reference"] = rec["ref_seconds"] / (last["kernel_seconds"] + last["bsp_seconds"])
        rec["bitwise_equal_columns"] = bool(np.array_equal(out.view(np.uint32), want_iso.view(np.uint32)))
        if occlusion:
            rec["failing_cells"] = int(iu.failing_cells(out, occ, want_iso, want_occ).sum())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="syn128,1000")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "isovist_time.jsonl"))
    ap.add_argument("--waves", default="")
    a = ap.parse_args()
    ctx = dmx.Context(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for name in a.maps.split(","):
            pm = make_map(name)
            g = pm.make_graph(ctx)
            n = g.info()["nnodes"]
            for waves in (a.waves.split(",") if a.waves else [None]):
                if waves is None:
                    os.environ.pop("DMX_ISO_WAVES", None)
                else:
                    os.environ["DMX_ISO_WAVES"] = waves
                for occlusion in (False, True, False):   # the first run also pays the scratch allocation (wall_s)
                    rec = run(ctx, g, name, occlusion, n)
                    if waves is not None:
                        rec["waves_per_cu"] = int(waves)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()
            g.close()


if __name__ == "__main__":
    main()
