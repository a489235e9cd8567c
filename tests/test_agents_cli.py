"""dmxcli -m AGENTS: the depthmapXcli agent parser (depthmapXcli/agentparser.cpp:30-346) -- every flag, every "can
only be used once", the required-argument messages -- on the CPU, and on the GPU the run on a .graph file: the
"Gate Counts" column equals Graph.agents over PointMap.agent_schedule with the same arguments, it is the displayed
attribute, a second run accumulates (AttributeRow::incrValue), and -ot gatecounts is the data export of the written
graph."""
import ctypes
import lzma
import os
import subprocess

import numpy as np
import pytest

import graphfile_util as gu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "depthmapx_amd", "_lib", "dmxcli")
GF_INPUTS = os.path.join(REPO, "tests", "golden", "graphfiles", "inputs")
BASE = ["-m", "AGENTS", "-f", "a", "-o", "b"]
FULL = ["-ats", "60", "-arr", "1.5", "-afov", "15", "-asteps", "3", "-alife", "40", "-alocseed", "1"]
TAIL = "Type 'depthmapXcli -h' for help"


def run(*args):
    p = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True)
    return p.returncode, p.stdout


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        from depthmapx_amd import build
        build.build()


def without(flag):
    """FULL without a flag and its value."""
    i = FULL.index(flag)
    return FULL[:i] + FULL[i + 2:]


@pytest.mark.parametrize("args,message", [
    (["-am", "standard", "-am", "occ-any"], "-am can only be used once, modes are mutually exclusive"),
    (["-am"], "-am requires an argument"),
    (["-am", "sideways"], "Invalid AGENTS mode: sideways"),
    (["-ats", "5", "-ats", "6"], "-ats can only be used once"),
    (["-ats"], "-ats requires an argument"),
    (["-ats", "5x"], "-ats must be a number >0, got 5x"),
    (["-ats", "0"], "-ats must be a number >0, got 0"),
    (["-arr", "1", "-arr", "2"], "-arr can only be used once"),
    (["-arr"], "-arr requires an argument"),
    (["-arr", "x"], "-arr must be a number >0, got x"),
    (["-arr", "0"], "-arr must be a number >0, got 0"),
    (["-atrails", "1", "-atrails", "2"], "-atrails can only be used once"),
    (["-atrails"], "-atrails requires an argument"),
    (["-atrails", "x"], "-atrails must be a number >=1 or 0 for all (max possible = 50), got x"),
    (["-afov", "3", "-afov", "4"], "-afov can only be used once"),
    (["-afov"], "-afov requires an argument"),
    (["-afov", "x"], "-afov must be a number between 1 and 32, got x"),
    (["-afov", "33"], "-afov must be a number between 1 and 32, got 33"),
    (["-afov", "0"], "-afov must be a number between 1 and 32, got 0"),
    (["-asteps", "3", "-asteps", "4"], "-asteps can only be used once"),
    (["-asteps"], "-asteps requires an argument"),
    (["-asteps", "0"], "-asteps must be a number >0, got 0"),
    (["-alife", "3", "-alife", "4"], "-alife can only be used once"),
    (["-alife"], "-alife requires an argument"),
    (["-alife", "y"], "-alife must be a number >0, got y"),
    (["-aseed", "3", "-aseed", "4"], "-aseed can only be used once"),
    (["-aseed"], "-aseed requires an argument"),
    (["-aseed", "4294967296"], "-aseed must be a number between 0 and 4294967295, got 4294967296"),
    (["-alocfile", "p", "-alocseed", "1"], "-alocseed cannot be used together with -alocfile"),
    (["-aloc", "1,2", "-alocseed", "1"], "-alocseed cannot be used together with -aloc"),
    (["-alocseed"], "-alocseed requires an argument"),
    (["-alocseed", "1.5"], "Invalid starting location seed provided (1.5). Should only contain digits"),
    (["-alocseed", "11"], "-alocseed must be a number between 0 and 10, got 11"),
    (["-aloc", "1,2", "-alocfile", "p"], "-alocfile cannot be used together with -aloc"),
    (["-alocseed", "1", "-alocfile", "p"], "-alocfile cannot be used together with -alocseed"),
    (["-alocfile"], "-alocfile requires an argument"),
    (["-alocfile", "p", "-aloc", "1,2"], "-aloc cannot be used together with -alocfile"),
    (["-alocseed", "1", "-aloc", "1,2"], "-aloc cannot be used together with -alocseed"),
    (["-aloc"], "-aloc requires an argument"),
    (["-aloc", "a,b"], "Invalid starting point provided (a,b). Should only contain digits dots and commas"),
    (["-ot"], "-ot requires an argument"),
    (["-ot", "graph", "-ot", "graph"], "Same output type argument (graph) provided twice"),
    (["-ot", "gatecounts", "-ot", "gatecounts"], "Same output type argument (gatecounts) provided twice"),
    (["-ot", "trails", "-ot", "trails"], "Same output type argument (trails) provided twice"),
    (without("-ats"), "Total number of timesteps (-ats <timesteps>) is required"),
    (without("-arr"), "Release rate (-arr <rate>) is required"),
    (without("-afov"), "Agent field-of-view (-afov <bins>) is required"),
    (without("-asteps"), "Agent number of steps before turn decision (-asteps <steps>) is required"),
    (without("-alife"), "Agent life in timesteps (-alife <timesteps>) is required"),
    (without("-alocseed"), "Either -aloc, -alocfile or -alocseed must be given"),
])
def test_agent_parser_messages_like_depthmapxcli(args, message):
    rc, out = run(*(BASE + args))
    assert rc == 255, out   # main returns -1
    assert out.splitlines() == [message, TAIL]


def test_missing_point_file_and_help(tmp_path):
    rc, out = run(*(BASE + without("-alocseed") + ["-alocfile", tmp_path / "none.tsv"]))
    assert rc == 255 and out.startswith("Failed to load file " + str(tmp_path / "none.tsv") + ", error ")
    rc, out = run("-h")
    assert rc == 0 and "AGENTS" in out and "-aseed" in out


def graph_input(tmp_path, name="gallery_connected.graph"):
    dst = tmp_path / name
    with lzma.open(os.path.join(GF_INPUTS, name + ".xz")) as f:
        dst.write_bytes(f.read())
    return str(dst)


@pytest.mark.parametrize("extra,needle", [
    (["-am", "los-length"], "Agent mode los-length is not part of the accelerated path"),
    (["-am", "occ-length"], "occ-length"), (["-am", "occ-any"], "occ-any"), (["-am", "occ-group-45"], "occ-group-45"),
    (["-am", "occ-group-60"], "occ-group-60"), (["-am", "occ-furthest"], "occ-furthest"),
    (["-am", "bin-far-dist"], "bin-far-dist"), (["-am", "bin-angle"], "bin-angle"),
    (["-am", "bin-far-dist-angle"], "bin-far-dist-angle"), (["-am", "bin-memory"], "bin-memory"),
    (["-ot", "trails"], "Agent trails"), (["-atrails", "5"], "Agent trails"),
])
def test_other_modes_and_trails_parse_and_are_refused(tmp_path, extra, needle):
    """Like the shapegraph-* exports: the parser takes them, the run refuses them after loading, no GPU opened."""
    out = tmp_path / "o.graph"
    rc, msg = run("-m", "AGENTS", "-f", graph_input(tmp_path), "-o", out, *FULL, *extra)
    assert rc == 255 and needle in msg and "not part of the accelerated path" in msg and msg.splitlines()[-1] == TAIL
    assert not out.exists()
    rc, msg = run("-m", "AGENTS", "-f", tmp_path / "none.graph", "-o", out, *FULL, *extra)
    assert rc == 255 and "Failed to load graph from file" in msg


# ---------------------------------------------------------------- on the GPU
def _load(ctx, path):
    import depthmapx_amd  # noqa: F401
    from depthmapx_amd import _native as N
    from depthmapx_amd import graphio
    lib = N.lib()
    h = ctypes.c_void_p()
    N.check(lib.dmx_graphfile_read(str(path).encode(), ctypes.byref(h)))
    try:
        region = np.zeros(4)
        npm, disp = ctypes.c_int32(), ctypes.c_int32()
        N.check(lib.dmx_graphfile_info(h, None, None, N.ptr(region), None, ctypes.byref(npm), ctypes.byref(disp)))
        buf, size = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_int64()
        N.check(lib.dmx_graphfile_pointmap(h, disp.value, ctypes.byref(buf), ctypes.byref(size)))
        blob = ctypes.string_at(buf, size.value)
    finally:
        lib.dmx_graphfile_free(h)
    return graphio.load_chunk(ctx, blob, region)


@pytest.mark.gpu
def test_cli_gate_counts_on_a_graph_file(ctx, tmp_path):
    src = graph_input(tmp_path)
    o1, o2, csv, exp, tcsv = (tmp_path / n for n in ("o1.graph", "o2.graph", "gc.csv", "exp.csv", "t.csv"))
    args = ["-ats", "60", "-arr", "1.5", "-afov", "15", "-asteps", "3", "-alife", "40", "-alocseed", "1", "-aseed", "9"]
    rc, msg = run("-m", "AGENTS", "-f", src, "-o", o1, "-t", tcsv, *args)
    assert rc == 0, msg
    assert "Running agent analysis... " in msg and "Writing out result..." in msg
    assert [l.split(",")[0] for l in open(tcsv).read().splitlines()] == [
        '"action"', '"Load graph file"', '"Running agent analysis"', '"Writing graph"']
    # the same run through the Python API
    pm, g = _load(ctx, src)
    table = pm.agent_schedule(seed=9, timesteps=60, release_rate=1.5, lifetime=40, locseed=1)
    assert len(table) > 30
    res = g.agents(table, fov=15, steps=3)
    cnt = res["counts"][np.flatnonzero(pm.state() & 2)].astype(np.float32)
    assert cnt.sum() > 0
    b1 = open(o1, "rb").read()
    col = gu.columns(b1, ["Gate Counts"])["Gate Counts"]
    np.testing.assert_array_equal(col, np.where(cnt > 0, cnt, np.float32(-1)))
    # the displayed attribute (the chunk stores its index among the columns sorted by name)
    names = gu.column_names(b1)
    assert "Gate Counts" in names and "Gate Counts" not in gu.column_names(open(src, "rb").read())
    assert sorted(names)[gu.parse(b1)["maps"][0]["displayed_sorted"]] == "Gate Counts"
    # a second run accumulates on the existing column
    rc, msg = run("-m", "AGENTS", "-f", o1, "-o", o2, *args)
    assert rc == 0, msg
    col2 = gu.columns(open(o2, "rb").read(), ["Gate Counts"])["Gate Counts"]
    np.testing.assert_array_equal(col2, np.where(cnt > 0, 2 * cnt, np.float32(-1)))
    # -ot gatecounts: outputSummary of the map the graph output holds
    rc, msg = run("-m", "AGENTS", "-f", src, "-o", csv, "-ot", "gatecounts", "-t", tcsv, *args)
    assert rc == 0, msg
    assert open(tcsv).read().splitlines()[-1].startswith('"Writing gatecounts"')
    rc, msg = run("-m", "EXPORT", "-f", o1, "-o", exp, "-em", "pointmap-data-csv")
    assert rc == 0, msg
    assert open(csv, "rb").read() == open(exp, "rb").read()
    assert b"Gate Counts" in open(csv, "rb").read().split(b"\n")[0]
    # both outputs at once: the reference's suffixes
    rc, msg = run("-m", "AGENTS", "-f", src, "-o", tmp_path / "both", "-ot", "graph", "-ot", "gatecounts", *args)
    assert rc == 0, msg
    assert open(str(tmp_path / "both") + ".graph", "rb").read() == b1
    assert open(str(tmp_path / "both") + "_gatecounts.csv", "rb").read() == open(csv, "rb").read()


@pytest.mark.gpu
def test_cli_release_points(ctx, tmp_path):
    """-aloc points become release cells through pixelate; a point on a cell that is not filled is an error."""
    src = graph_input(tmp_path)
    pm, g = _load(ctx, src)
    i = pm.info()
    filled = np.flatnonzero(pm.state() & 2)
    cell = int(filled[len(filled) // 2])
    x, y = cell // i["rows"], cell % i["rows"]
    px, py = i["bottom_left"][0] + pm.spacing * x, i["bottom_left"][1] + pm.spacing * y
    args = ["-ats", "30", "-arr", "2", "-afov", "32", "-asteps", "2", "-alife", "20", "-aseed", "3"]
    out = tmp_path / "o.graph"
    rc, msg = run("-m", "AGENTS", "-f", src, "-o", out, "-aloc", "%.6f,%.6f" % (px, py), *args)
    assert rc == 0, msg
    table = pm.agent_schedule(seed=3, timesteps=30, release_rate=2, lifetime=20, release_cells=[cell])
    assert (table[:, 0] == cell).all()
    cnt = g.agents(table, fov=32, steps=2)["counts"][filled].astype(np.float32)
    col = gu.columns(open(out, "rb").read(), ["Gate Counts"])["Gate Counts"]
    np.testing.assert_array_equal(col, np.where(cnt > 0, cnt, np.float32(-1)))
    empty = int(np.flatnonzero((pm.state() & 2) == 0)[0])
    ex, ey = empty // i["rows"], empty % i["rows"]
    bad = tmp_path / "bad.graph"
    rc, msg = run("-m", "AGENTS", "-f", src, "-o", bad, "-aloc",
                  "%.6f,%.6f" % (i["bottom_left"][0] + pm.spacing * ex, i["bottom_left"][1] + pm.spacing * ey), *args)
    assert rc == 255 and "release cell" in msg and not bad.exists()
