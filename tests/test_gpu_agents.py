"""The agent analysis on the GPU (dmx_agents, Graph.agents, Context.last_agents) against the fixtures made from the
reference's own Agent class (tests/golden/agents/, make_golden_agents.py).  Every comparison is exact: counts, final
cells, final locations as bit patterns, stuck flags and trails.  256 agents x 200 moves a case; the largest grid is
115 x 76."""
import ctypes

import numpy as np
import pytest

import agents_util as au
import depthmapx_amd as dmx
from depthmapx_amd import _native as N
from depthmapx_amd import graphio
from golden_io import case_input_lines, load_case

pytestmark = pytest.mark.gpu

CASES = au.cases()
OUT_FIELDS = ["counts", "final_cell", "final_loc", "stuck", "trails"]
_graphs = {}


def graph(ctx, name):
    """The engine's graph of a fixture map, made once per session of this module."""
    if name not in _graphs:
        meta, _ = load_case(name)
        pm = dmx.PointMap(meta["region"], case_input_lines(meta), meta["spacing"])
        for f in meta["fills"]:
            assert pm.make_points(*f)
        _graphs[name] = (pm, pm.make_graph(ctx))
    return _graphs[name]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _graphs.clear()


def run(g, case, table, trails=0):
    return g.agents(table, fov=case["fov"], steps=case["steps"], trails=trails)


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_reference_fixture(ctx, name):
    case, ref = CASES[name], au.load_fixture(name)
    pm, g = graph(ctx, case["map"])
    got = run(g, case, ref["table"], trails=case["ntrail"])
    au.assert_same(got, ref, fields=OUT_FIELDS, what=name)
    st = ctx.last_agents()
    assert st["host_reruns"] == 0 and st["clamped"] == 0
    for k in ("moves", "looks", "fallbacks", "diag_taken", "stopped"):
        assert st[k] == case[k], k
    assert st["seconds"] > 0 and st["host_seconds"] == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_schedule_equals_fixture_table(name):
    """dmx_agent_schedule (host only, but part of the library) gives the reference driver's table."""
    case, ref = CASES[name], au.load_fixture(name)
    meta, _ = load_case(case["map"])
    pm = dmx.PointMap(meta["region"], case_input_lines(meta), meta["spacing"])
    for f in meta["fills"]:
        assert pm.make_points(*f)
    t = pm.agent_schedule(seed=case["seed"], timesteps=case["timesteps"], release_rate=case["rate"],
                          lifetime=case["lifetime"], release_cells=au.release_cells(case, meta["rows"]),
                          locseed=case["locseed"])
    assert len(t) >= case["nagents"]
    np.testing.assert_array_equal(t[:case["nagents"]], ref["table"])
    with pytest.raises(N.DmxError) as ei:
        pm.agent_schedule(release_cells=[0])   # cell (0, 0) of these maps is not filled
    assert ei.value.status == -1
    with pytest.raises(N.DmxError) as ei:
        pm.agent_schedule(release_cells=[meta["cols"] * meta["rows"]])
    assert ei.value.status == -1


def test_counts_do_not_depend_on_order_or_split(ctx):
    name = "syn32_f15_s3"
    case, ref = CASES[name], au.load_fixture(name)
    pm, g = graph(ctx, case["map"])
    t = ref["table"]
    rev = run(g, case, t[::-1])
    np.testing.assert_array_equal(rev["counts"], ref["counts"])
    np.testing.assert_array_equal(rev["final_cell"][::-1], ref["final_cell"])
    a, b = run(g, case, t[:100]), run(g, case, t[100:])
    np.testing.assert_array_equal(a["counts"] + b["counts"], ref["counts"])
    np.testing.assert_array_equal(np.concatenate([a["final_cell"], b["final_cell"]]), ref["final_cell"])


def test_agents_sharing_a_start_cell(ctx):
    """64 agents released on one cell (atomic adds on the same entries): the sum of 64 calls of one agent each."""
    name = "syn16_f32_s3"
    case, ref = CASES[name], au.load_fixture(name)
    pm, g = graph(ctx, case["map"])
    t = ref["table"][:64].copy()
    t[:, 0] = t[0, 0]
    t[:, 2] = 40
    together = run(g, case, t)
    alone = sum(run(g, case, t[i:i + 1])["counts"].astype(np.int64) for i in range(64))
    np.testing.assert_array_equal(together["counts"], alone)
    assert together["counts"].max() > 1


def test_node_without_bins_leaves_its_agent_stuck(ctx):
    """syn16's arrays with one node's bins emptied (dmx_graph_from_runs): an agent started there is stuck and counts
    nothing; the agents that never look from that node are unchanged."""
    name = "syn16_f32_s3"
    case, ref = CASES[name], au.load_fixture(name)
    meta, A = load_case(case["map"])
    pm, g0 = graph(ctx, case["map"])
    cell_of = np.flatnonzero(pm.state() & 2)
    # a node no agent of the fixture ever stands on would prove nothing about the others: take the least visited
    # one and keep, as "the others", the agents that do not enter it
    k = int(np.argmin(ref["counts"][cell_of] + 1000 * (np.isin(cell_of, ref["table"][:, 0]))))
    bins = A["bins"].astype(np.int32).copy()
    starts = np.concatenate([[0], np.cumsum(bins[:, :, 3].sum(axis=1))])
    runs = np.concatenate([A["runs"][:starts[k]], A["runs"][starts[k + 1]:]]).astype(np.int16)
    bins[k, :, 1] = 0
    bins[k, :, 3] = 0
    gc = np.ascontiguousarray(A["gridconn"], dtype=np.uint8)
    h = ctypes.c_void_p()
    N.check(N.lib().dmx_graph_from_runs(ctx.h, pm.h, len(bins), N.ptr(bins), N.ptr(runs), len(runs), N.ptr(gc), None,
                                        ctypes.byref(h)))
    g = dmx.Graph(h, ctx, pm)
    lone = np.array([[cell_of[k], 12345, 50]], dtype=np.int32)
    got = run(g, case, lone, trails=1)
    assert got["stuck"][0] == 1 and got["counts"].sum() == 0 and got["final_cell"][0] == cell_of[k]
    assert (got["trails"][0, :50] == cell_of[k]).all()
    assert ctx.last_agents()["moves"] == 0 and ctx.last_agents()["looks"] == 1
    # agents of the fixture whose whole walk avoids node k behave as on the full graph
    full = run(g0, case, ref["table"], trails=0)
    per_agent = [run(g0, case, ref["table"][i:i + 1], trails=1) for i in range(16)]
    keep = [i for i in range(16) if cell_of[k] not in per_agent[i]["trails"][0] and ref["table"][i, 0] != cell_of[k]]
    assert len(keep) >= 8
    t = ref["table"][keep]
    a, b = run(g, case, t), run(g0, case, t)
    au.assert_same(a, b, fields=["counts", "final_cell", "final_loc", "stuck"], what="others")
    np.testing.assert_array_equal(full["counts"], ref["counts"])


def test_reread_map_gives_the_same_counts(ctx):
    name = "syn32_f15_s3"
    case, ref = CASES[name], au.load_fixture(name)
    meta, _ = load_case(case["map"])
    pm, g = graph(ctx, case["map"])
    blob = g.write_chunk([])
    pm2, g2 = graphio.load_chunk_device(ctx, blob, meta["region"])
    got = run(g2, case, ref["table"], trails=case["ntrail"])
    au.assert_same(got, ref, fields=OUT_FIELDS, what="re-read " + name)
    assert ctx.last_agents()["clamped"] == 0


@pytest.mark.parametrize("name,how", [("syn32_f1_s3", "lazy"), ("gallery_f15_s3", "lazy"), ("gallery_f15_s3", "1")])
def test_host_rerun_path_through_the_hook(ctx, monkeypatch, name, how):
    """DMX_AGENTS_HOST launches no kernel and sends every agent through the API's host re-run (the graph's per-node
    arrays downloaded, counts, final state and trails written by ag_run_host): the same results, and the call says
    so.  "lazy" reads the run pool a bin at a time, as the re-run of a flagged agent does; "1" downloads it whole."""
    case, ref = CASES[name], au.load_fixture(name)
    pm, g = graph(ctx, case["map"])
    monkeypatch.setenv("DMX_AGENTS_HOST", how)
    got = run(g, case, ref["table"], trails=case["ntrail"])
    au.assert_same(got, ref, fields=OUT_FIELDS, what="host " + name)
    st = ctx.last_agents()
    assert st["host_reruns"] == case["nagents"] and st["host_seconds"] > 0 and st["clamped"] == 0
    for k in ("moves", "looks", "fallbacks", "diag_taken", "stopped"):
        assert st[k] == case[k], k
    monkeypatch.delenv("DMX_AGENTS_HOST")
    run(g, case, ref["table"])
    assert ctx.last_agents()["host_reruns"] == 0 and ctx.last_agents()["host_seconds"] == 0


def test_pending_cancel_stops_the_call_once(ctx):
    name = "syn32_f15_s3"
    case, ref = CASES[name], au.load_fixture(name)
    pm, g = graph(ctx, case["map"])
    ctx.cancel()
    with pytest.raises(N.DmxError) as ei:
        run(g, case, ref["table"])
    assert ei.value.status == -7
    np.testing.assert_array_equal(run(g, case, ref["table"])["counts"], ref["counts"])   # the request was consumed


def test_bad_arguments_are_refused(ctx):
    name = "syn32_f15_s3"
    case, ref = CASES[name], au.load_fixture(name)
    pm, g = graph(ctx, case["map"])
    bad = ref["table"][:4].copy()
    bad[1, 0] = 0   # cell (0, 0) is not filled
    with pytest.raises(N.DmxError) as ei:
        run(g, case, bad)
    assert ei.value.status == -1
    with pytest.raises(N.DmxError) as ei:
        g.agents(ref["table"][:4], fov=15, steps=0)
    assert ei.value.status == -1
    n = g.info()["nnodes"]
    shard = pm.make_graph(ctx, node_begin=0, node_end=n // 2)
    with pytest.raises(N.DmxError) as ei:
        run(shard, case, ref["table"][:4])
    assert ei.value.status == -4
    empty = run(g, case, np.zeros((0, 3), dtype=np.int32))
    assert empty["counts"].sum() == 0 and len(empty["final_cell"]) == 0
