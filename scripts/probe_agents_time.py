"""Agent analysis throughput on the bench's 1000^2 map: 65,536 agents x 1,000 moves at fov 15, steps 3, on the GPU
and (a slice of the same table) through the host routine on one thread (the DMX_AGENTS_HOST hook; the
download of the graph's arrays it needs is in the wall time, not in the rate).  Also 100 agents,
about the reference's default live population.  Prints one JSON line and writes it to argv[1] (default
profiles/agents.json).

    python scripts/probe_agents_time.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
import depthmapx_amd as dmx  # noqa: E402

W = int(os.environ.get("AG_W", "1000"))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "agents.json")
out = {}
lines = bench.load_lines(W, 50)
ctx = dmx.Context(0)
pm = dmx.PointMap([0.0, 0.0, float(W), float(W)], lines, 1.0)
assert pm.make_points(0.5, 0.5)
t0 = time.time()
g = pm.make_graph(ctx)
out["makegraph_wall_s"] = time.time() - t0
out["nodes"], out["nruns"] = g.info()["nnodes"], g.info()["nruns"]
table = pm.agent_schedule(seed=1, timesteps=2100, release_rate=64.0, lifetime=1000, locseed=1)[:65536]
assert len(table) == 65536 and (table[:, 2] == 1000).all()
print("map ready", out, flush=True)


def timed(tab, reps=3, steps=3):
    best = None
    for _ in range(reps):
        t = time.time()
        g.agents(tab, fov=15, steps=steps)
        wall = time.time() - t
        st = ctx.last_agents()
        if best is None or wall < best["wall_s"]:
            best = dict(st, wall_s=wall)
    # under the hook every agent is a host re-run: the host routine's seconds; else the kernel's
    t = best["host_seconds"] if best["host_reruns"] == len(tab) else best["seconds"]
    best["moves_per_s"] = best["moves"] / t
    best["moves_per_s_wall"] = best["moves"] / best["wall_s"]
    return best


out["gpu_65536x1000"] = timed(table)
print(out["gpu_65536x1000"], flush=True)
# the look / step split: the same table with a look at every move (steps 1); t = a * moves + b * looks
out["gpu_65536x1000_steps1"] = timed(table, steps=1)
print(out["gpu_65536x1000_steps1"], flush=True)
out["gpu_100x1000"] = timed(table[:100])
print(out["gpu_100x1000"], flush=True)
json.dump(out, open(OUT, "w"), indent=1)
# t = a * moves + b * looks over the two step settings
m1, l1, t1 = (out["gpu_65536x1000"][k] for k in ("moves", "looks", "seconds"))
m2, l2, t2 = (out["gpu_65536x1000_steps1"][k] for k in ("moves", "looks", "seconds"))
det = m1 * l2 - m2 * l1
if det:
    out["gpu_seconds_per_move"] = (t1 * l2 - t2 * l1) / det
    out["gpu_seconds_per_look"] = (m1 * t2 - m2 * t1) / det
if os.environ.get("AG_SKIP_HOST"):
    json.dump(out, open(OUT, "w"), indent=1)
    print(json.dumps(out), flush=True)
    sys.exit(0)
# host routine, one thread: the first 2048 agents of the same table (and the same 100)
os.environ["DMX_AGENTS_HOST"] = "1"
out["host_2048x1000"] = timed(table[:2048], reps=1)
print(out["host_2048x1000"], flush=True)
out["host_100x1000"] = timed(table[:100], reps=1)
del os.environ["DMX_AGENTS_HOST"]
json.dump(out, open(OUT, "w"), indent=1)
print(json.dumps(out), flush=True)
