"""Fixtures for the agent analysis (standard agents, Gate Counts) from the real reference.  Run by hand where the
reference library exists (oracle/_ref/libsalaref.a, made by oracle/Makefile); never by build(), by a test or on a
GPU machine.

The driver tests/golden/ref_agents.cpp (our own code over the reference's classes) is compiled into a temporary
directory with the REFFLAGS of oracle/Makefile.  Per case it makes the map's graph, produces the agent table with
the reference's own pafrand / invcumpoisson / pickPixel under the engine's two-stream rule, and runs every agent
of the table as a reference Agent after pafsrand(seed).  Stored under tests/golden/agents/

  <case>.npz   table int32 [n][3] (start cell, seed, moves), counts uint32 [cols*rows], final_cell int32 [n],
               final_loc float64 [n][2], stuck uint8 [n], trails int32 [8][lifetime] (-1 beyond an agent's moves)
  cases.json   per case: the map (a case of tests/golden/cases.json), fov, steps, seeds, timesteps, rate,
               lifetime, release cells, and what it exercised: moves, looks, fallbacks (narrow looks that fell
               back to the whole isovist), diag_taken, stopped (diagonal steps refused: the move stopped)

The counters come from the host routine (tests/agents/agents_check.cpp over kernels/agent_step.hpp), which is first
held to the reference's outputs exactly; moves, looks and stopped are also observed on the reference's agents from
outside and must agree.  No case may flag an agent (a look within 1e-9 of a bin boundary) or clamp a bin: a case
that does gets another seed here.

    python tests/golden/make_golden_agents.py [case ...]
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REPO)
from agents_util import run_host_check  # noqa: E402
from make_golden import CASES as MAP_CASES  # noqa: E402
from make_golden_thruvision import REF_LIB, ref_flags  # noqa: E402

OUT = os.path.join(HERE, "agents")
NAGENTS, TIMESTEPS, LIFETIME, RATE, NTRAIL = 256, 400, 200, 1.0, 8

# name -> (map, fov, steps, seed, locseed, release cells (x, y))
CASES = {
    "kat_f15_s3": ("kat", 15, 3, 1, 11, []),
    "syn16_f32_s3": ("syn16", 32, 3, 2, 12, []),
    "syn32_f15_s3": ("syn32", 15, 3, 3, 13, []),
    "syn32_f15_s1": ("syn32", 15, 1, 4, 14, []),
    "syn32_f1_s3": ("syn32", 1, 3, 5, 15, []),
    "syn32_f15_s3_rel": ("syn32", 15, 3, 6, 16, [(3, 3), (16, 16), (29, 5)]),
    "gallery_f15_s3": ("gallery", 15, 3, 7, 17, []),
}
STATS = ["moves", "looks", "fallbacks", "diag_taken", "stopped"]


def build_driver(tmp):
    exe = os.path.join(tmp, "ref_agents")
    cmd = [os.environ.get("CXX", "g++")] + ref_flags() + [os.path.join(HERE, "ref_agents.cpp"), "-o", exe,
                                                        "-Wl,--start-group", REF_LIB, "-Wl,--end-group"]
    print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return exe


def run_case(exe, name, tmp):
    mp, fov, steps, seed, locseed, release = CASES[name]
    src, spacing, fills = MAP_CASES[mp][:3]
    src = src if os.path.isabs(src) else os.path.join(HERE, src)
    d = os.path.join(tmp, name)
    os.makedirs(d)
    cmd = [exe, "--drawing" if src.endswith(".graph") else "--lines", src, "--spacing", str(spacing), "--out", d,
           "--fov", str(fov), "--steps", str(steps), "--seed", str(seed), "--locseed", str(locseed),
           "--timesteps", str(TIMESTEPS), "--rate", str(RATE), "--lifetime", str(LIFETIME), "--nagents", str(NAGENTS)]
    for p in fills:
        cmd += ["--fill", p]
    for x, y in release:
        cmd += ["--release", "%d,%d" % (x, y)]
    print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    rd = lambda f, dt: np.fromfile(os.path.join(d, f), dtype=dt)
    ref = dict(table=rd("table.bin", np.int32).reshape(-1, 3), counts=rd("counts.bin", np.uint32),
               final_cell=rd("final_cell.bin", np.int32), final_loc=rd("final_loc.bin", np.float64).reshape(-1, 2),
               stuck=rd("stuck.bin", np.uint8), trails=rd("trails.bin", np.int32).reshape(NTRAIL, LIFETIME))
    seen = dict(l.split() for l in open(os.path.join(d, "stats.txt")))
    case = dict(map=mp, fov=fov, steps=steps, seed=seed, locseed=locseed, release=[list(r) for r in release],
                timesteps=TIMESTEPS, rate=RATE, lifetime=LIFETIME, nagents=NAGENTS, ntrail=NTRAIL)
    got, stats = run_host_check(case, os.path.join(tmp, name + "_host"))
    for k in ref:
        a, b = ref[k], got[k]
        if k == "final_loc":
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), (name, k, "the host routine differs from the reference")
    assert stats["flagged"] == 0 and stats["clamps"] == 0, (name, stats, "choose another seed")
    for k in ("moves", "looks", "stopped"):
        assert stats[k] == int(seen[k]), (name, k, stats[k], seen[k])
    case.update({k: stats[k] for k in STATS})
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **ref)
    print(name, {k: case[k] for k in STATS}, "stuck", int(ref["stuck"].sum()), "cells counted",
          int((ref["counts"] > 0).sum()), flush=True)
    return case


def main(names):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "cases.json")
    cases = json.load(open(path)) if os.path.exists(path) else {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for n in names:
            cases[n] = run_case(exe, n, tmp)
    for k in STATS:
        assert any(c[k] > 0 for c in cases.values()), k + " is not exercised by any case"
    json.dump(cases, open(path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv[1:] or list(CASES))
