"""Helpers for the agent-analysis tests: the fixtures of tests/golden/agents/ and the stand-alone host program
tests/agents/agents_check.cpp (kernels/agent_step.hpp on one thread)."""
import json
import os
import subprocess
import tempfile

import numpy as np

from golden_io import GOLDEN, load_case

HERE = os.path.dirname(os.path.abspath(__file__))
AGENTS = os.path.join(GOLDEN, "agents")
CHECK_SRC = os.path.join(HERE, "agents", "agents_check.cpp")
FIELDS = ["table", "counts", "final_cell", "final_loc", "stuck", "trails"]
_built = {}


def cases():
    with open(os.path.join(AGENTS, "cases.json")) as f:
        return json.load(f)


def load_fixture(name):
    z = np.load(os.path.join(AGENTS, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def vbin_of(fov):
    """runmethods.cpp:499-504"""
    return -1 if fov == 32 else (fov - 1) // 2


def build_check(flags=()):
    """agents_check compiled with g++ -ffp-contract=off (+ flags), once per set of flags."""
    key = tuple(flags)
    if key not in _built:
        d = tempfile.mkdtemp(prefix="agents_check_")
        exe = os.path.join(d, "agents_check")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-ffp-contract=off"] +
                              list(flags) + [CHECK_SRC, "-o", exe])
        _built[key] = exe
    return _built[key]


def release_cells(case, rows):
    return np.array([x * rows + y for x, y in case["release"]], dtype=np.int32)


def run_host_check(case, workdir, flags=()):
    """Run agents_check on a case of cases.json -> (outputs by FIELDS name, counters)."""
    meta, A = load_case(case["map"])
    os.makedirs(workdir, exist_ok=True)
    rows = int(meta["rows"])
    rel = release_cells(case, rows)
    A["state"].astype(np.int32).tofile(os.path.join(workdir, "state.bin"))
    A["bins"].astype(np.int32).tofile(os.path.join(workdir, "bins.bin"))
    A["runs"].astype(np.int16).tofile(os.path.join(workdir, "runs.bin"))
    A["gridconn"].astype(np.uint8).tofile(os.path.join(workdir, "gridconn.bin"))
    rel.tofile(os.path.join(workdir, "release.bin"))
    kv = dict(cols=meta["cols"], rows=rows, spacing=meta["spacing"], blx=meta["bottom_left"][0],
              bly=meta["bottom_left"][1], nodes=len(A["gridconn"]), nruns=len(A["runs"]), fov=case["fov"],
              steps=case["steps"], seed=case["seed"], locseed=case["locseed"], timesteps=case["timesteps"],
              rate=case["rate"], lifetime=case["lifetime"], nagents=case["nagents"], ntrail=case["ntrail"],
              nrelease=len(rel))
    with open(os.path.join(workdir, "meta.txt"), "w") as f:
        for k, v in kv.items():
            f.write("%s %.17g\n" % (k, float(v)))
    subprocess.check_call([build_check(flags), workdir])
    rd = lambda f, dt: np.fromfile(os.path.join(workdir, f), dtype=dt)
    out = dict(table=rd("out_table.bin", np.int32).reshape(-1, 3), counts=rd("out_counts.bin", np.uint32),
               final_cell=rd("out_final_cell.bin", np.int32),
               final_loc=rd("out_final_loc.bin", np.float64).reshape(-1, 2), stuck=rd("out_stuck.bin", np.uint8),
               trails=rd("out_trails.bin", np.int32).reshape(case["ntrail"], case["lifetime"]))
    out["counts_split"] = rd("out_counts_split.bin", np.uint32)
    stats = {k: int(v) for k, v in (l.split() for l in open(os.path.join(workdir, "out_stats.txt")))}
    return out, stats


def assert_same(got, ref, fields=FIELDS, what=""):
    for k in fields:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        if k == "final_loc":
            a, b = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
        assert a.shape == b.shape and np.array_equal(a, b), "%s %s differs" % (what, k)
