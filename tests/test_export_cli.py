"""dmxcli -m EXPORT: the depthmapXcli export parser (depthmapXcli/exportparser.cpp:25-80) and the two host-only
exports of the displayed point map, -em pointmap-data-csv (PointMap::outputSummary, salalib/pointdata.cpp:554-587)
and -em pointmap-links-csv (PointMap::outputLinksAsCSV, :683-706), byte for byte against the reference's own files
(tests/golden/export, written by make_golden_export.py).  No test here needs a GPU: the two modes open none, which
the last tests check by hiding every device from the child process."""
import json
import lzma
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "depthmapx_amd", "_lib", "dmxcli")
GOLDEN = os.path.join(REPO, "tests", "golden")
EXPORT = os.path.join(GOLDEN, "export")
CASES = json.load(open(os.path.join(EXPORT, "cases.json")))
HOST_CASES = ["kat", "gallery_connected", "mixed_link", "turns_connected"]


def run(*args, env=None):
    p = subprocess.run([CLI] + list(args), capture_output=True, text=True, env=env)
    return p.returncode, p.stdout


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        from depthmapx_amd import build
        build.build()


def case_input(case, tmp_path):
    """The case's .graph, unpacked: export/<case>.graph.xz or graphfiles/inputs/<name>.xz."""
    src = CASES[case]["input"]
    path = os.path.join(GOLDEN, src) if src.startswith("export/") else os.path.join(GOLDEN, "graphfiles", "inputs", src + ".xz")
    dst = tmp_path / (case + ".graph")
    with lzma.open(path) as f:
        dst.write_bytes(f.read())
    return str(dst)


def expected(case, kind):
    with lzma.open(os.path.join(EXPORT, CASES[case]["exports"][kind]["file"])) as f:
        return f.read()


@pytest.mark.parametrize("args,message", [
    (["-m", "EXPORT", "-f", "a", "-o", "b", "-em", "pointmap-data-csv", "-em", "pointmap-links-csv"],
     "-em can only be used once, modes are mutually exclusive"),
    (["-m", "EXPORT", "-f", "a", "-o", "b", "-em", "pointmap-net"], "Invalid EXPORT mode: pointmap-net"),
    (["-m", "EXPORT", "-f", "a", "-o", "b", "-em"], "-em requires an argument"),
    (["-m", "EXPORT", "-f", "a", "-o", "b", "-em", "-x"], "-em requires an argument"),
    (["-m", "EXPORT", "-o", "b", "-em", "pointmap-data-csv"], "-f for input file is required"),
])
def test_export_parser_messages_like_depthmapxcli(args, message):
    rc, out = run(*args)
    assert rc == 255, out   # main returns -1
    assert out.splitlines() == [message, "Type 'depthmapXcli -h' for help"]


def test_help_lists_export():
    rc, out = run("-h")
    assert rc == 0 and "EXPORT" in out and "pointmap-connections-csv" in out


def test_export_without_em_is_refused_after_loading(tmp_path):
    """Without -em the reference's mode stays NONE: exportData loads the graph, then its switch throws (runmethods.cpp:
    651, :728-731).  A missing file therefore fails as a load, an existing one with the switch's message."""
    out = tmp_path / "o.csv"
    rc, msg = run("-m", "EXPORT", "-f", str(tmp_path / "none.graph"), "-o", str(out))
    assert rc == 255 and "Failed to load graph from file" in msg
    rc, msg = run("-m", "EXPORT", "-f", case_input("kat", tmp_path), "-o", str(out))
    assert rc == 255 and msg.splitlines() == ["Error, unsupported export mode", "Type 'depthmapXcli -h' for help"]
    assert not out.exists()


@pytest.mark.parametrize("mode", ["shapegraph-map-csv", "shapegraph-map-mif", "shapegraph-connections-csv",
                                  "shapegraph-links-unlinks-csv"])
def test_shapegraph_modes_parse_and_are_refused(tmp_path, mode):
    out = tmp_path / "o.csv"
    rc, msg = run("-m", "EXPORT", "-f", case_input("kat", tmp_path), "-o", str(out), "-em", mode)
    assert rc == 255 and msg.splitlines()[0] == ("Export mode %s needs a shape graph: only the pointmap-* export "
                                                 "modes are part of the accelerated path" % mode)
    assert not out.exists()


@pytest.mark.parametrize("case", HOST_CASES)
@pytest.mark.parametrize("kind", ["data", "links"])
def test_host_exports_equal_the_reference(tmp_path, case, kind):
    out = tmp_path / "out.csv"
    times = tmp_path / "t.csv"
    rc, msg = run("-m", "EXPORT", "-f", case_input(case, tmp_path), "-o", str(out), "-em", "pointmap-%s-csv" % kind,
                  "-t", str(times))
    assert rc == 0, msg
    got, ref = out.read_bytes(), expected(case, kind)
    assert len(got) == CASES[case]["exports"][kind]["size"]
    assert got == ref
    # the reference's timing actions: the links go by the connections' name (runmethods.cpp:658, :674)
    actions = [l.split(",")[0] for l in times.read_text().splitlines()]
    assert actions == ['"action"', '"Load graph file"',
                       '"Writing pointmap data"' if kind == "data" else '"Writing pointmap connections"']


def test_kat_links_are_the_reference_tests_lines(tmp_path):
    """salaTest/testpointmap.cpp:362-380."""
    assert expected("kat", "links").decode().split("\n") == ["RefFrom,RefTo", "65537,131074", "65538,131073"]


def test_every_fixture_row_is_visible():
    """The fixtures exercise PointMap::outputSummary's row test only with visible rows: one data row a node."""
    for case in HOST_CASES:
        assert CASES[case]["exports"]["data"]["lines"] == CASES[case]["nodes"] + 1


def _no_device_env():
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["ROCR_VISIBLE_DEVICES"] = ""
    return env


@pytest.mark.parametrize("kind", ["data", "links"])
def test_host_exports_run_without_a_device(tmp_path, kind):
    out = tmp_path / "out.csv"
    rc, msg = run("-m", "EXPORT", "-f", case_input("turns_connected", tmp_path), "-o", str(out), "-em",
                  "pointmap-%s-csv" % kind, env=_no_device_env())
    assert rc == 0, msg
    assert out.read_bytes() == expected("turns_connected", kind)


def test_connections_of_a_map_without_a_graph_need_no_device(tmp_path):
    """A grid and a fill but no graph: no point has its node, the reference writes the header alone -- and so does
    dmxcli, before it would open the GPU.  The map is made here by VISPREP's host steps."""
    src = tmp_path / "gallery_empty.graph"
    with lzma.open(os.path.join(GOLDEN, "graphfiles", "inputs", "gallery_empty.graph.xz")) as f:
        src.write_bytes(f.read())
    filled = tmp_path / "filled.graph"
    rc, msg = run("-m", "VISPREP", "-f", str(src), "-o", str(filled), "-pg", "0.04", "-pp", "1.32,7.24")
    assert rc == 0, msg
    out = tmp_path / "out.csv"
    rc, msg = run("-m", "EXPORT", "-f", str(filled), "-o", str(out), "-em", "pointmap-connections-csv",
                  env=_no_device_env())
    assert rc == 0, msg
    assert out.read_bytes() == expected("nograph", "connections") == b"RefFrom,RefTo"
