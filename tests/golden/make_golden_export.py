"""Fixtures for the EXPORT mode (-em pointmap-data-csv, pointmap-links-csv, pointmap-connections-csv) from the
real reference.  Run by hand where the reference library exists (oracle/_ref/libsalaref.a, made by oracle/Makefile);
never by build(), by a test or on a GPU machine.

The driver tests/golden/ref_export.cpp (our own code over the reference's public classes) is compiled into a
temporary directory with the REFFLAGS of oracle/Makefile and writes, for the displayed point map of a .graph, what
depthmapXcli -m EXPORT writes.  Cases:

  kat                the 2 x 2 map of salaTest/testpointmap.cpp:313-398 made in memory (inputs/kat_square.csv, the
                     two merge links of its outputLinksAsCSV section); the reference also writes it as kat.graph
  gallery_one_op,    the reference CLI's outputs of these chains of graphfiles/cases.json (fresh graphs after one
  turns_remake       write / read): connections
  gallery_connected, committed inputs with analysis columns and merge links: data, links, connections
  mixed_link, turns_connected
  nograph            the chain gallery_fill (a grid and a fill, no graph): connections, the header alone
  overlap            a hand-made graph on the 26 x 26 grid (576 filled cells) of rect1x1.graph at spacing 0.04 whose
                     runs make a cell recur within one bin, across two bins and inside a diagonal span, with a
                     single-cell run, a node without a neighbourhood, neighbourhoods longer than one 256-position
                     chunk and runs over cells that are not filled.  Written with the project's host writer
                     (dmx_chunk_write + the graph-file API), exported by the reference; the arrays a reader of the
                     file sees are overlap.npz.

Stored under tests/golden/export/: <case>_<kind>.csv.xz when the xz is at most 500 KB, else only the entry of
cases.json (size, lines, sha256); an export with the bytes of another case's is stored once.  cases.json also keeps, per case, nodes, the cells Node::first()..next() visit,
how many of them deduplication dropped, and the reference's wall time for the connections.

    python tests/golden/make_golden_export.py [case ...]
"""
import ctypes
import hashlib
import json
import lzma
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
from make_golden_thruvision import REF_LIB, graph_input, ref_flags  # noqa: E402

OUT = os.path.join(HERE, "export")
XZ_LIMIT = 500 * 1000
KAT_MERGES = [(65537, 131074), (131073, 65538)]
KAT_LINES = ["RefFrom,RefTo", "65537,131073", "65537,131074", "65537,65538", "65538,131074", "65538,131073",
             "131073,131074"]
ALL = ("data", "links", "connections")
CASES = {
    "kat": (None, ALL),
    "gallery_one_op": ("@gallery_one_op", ("connections",)),
    "turns_remake": ("@turns_remake", ("connections",)),
    "gallery_connected": ("gallery_connected.graph", ALL),
    "mixed_link": ("mixed_link.graph", ALL),
    "turns_connected": ("turns_connected.graph", ALL),
    "nograph": ("@gallery_fill", ("connections",)),
    "overlap": (None, ("connections",)),
}
BIN_DIR = [4 if b in (4, 20) else 8 if b in (12, 28) else 2 if (4 < b < 12 or 20 < b < 28) else 1 for b in range(32)]


def build_driver(tmp):
    exe = os.path.join(tmp, "ref_export")
    cmd = [os.environ.get("CXX", "g++")] + ref_flags() + [os.path.join(HERE, "ref_export.cpp"), "-o", exe,
                                                        "-Wl,--start-group", REF_LIB, "-Wl,--end-group"]
    print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return exe


def enumerate_node(bins, runs):
    """Node::first()..next() of one node (ngraph.cpp:158-172, :392-406): [(bin, x, y)] in order."""
    out, ro = [], 0
    for b in range(32):
        d = BIN_DIR[b]
        for r in runs[ro:ro + int(bins[b, 3])]:
            x, y = int(r[0]), int(r[1])
            n = (int(r[3]) - y if d == 2 else int(r[2]) - x) + 1
            for _ in range(max(n, 1)):
                out.append((b, x, y))
                x += 0 if d == 2 else 1
                y += 1 if d in (2, 4) else -1 if d == 8 else 0
        ro += int(bins[b, 3])
    return out


def overlap_graph(state, cols, rows):
    """The hand-made neighbourhoods: (bins [N][32][4], runs [R][4]) for the filled cells of the grid, x-major."""
    cells = [(c // rows, c % rows) for c in range(cols * rows) if state[c] & 2]
    xs, ys = [c[0] for c in cells], [c[1] for c in cells]
    x0, x1, y0, y1 = min(xs), max(xs), min(ys), max(ys)
    bins = np.zeros((len(cells), 32, 4), dtype=np.int32)
    runs = []

    def put(k, b, rr):
        for r in rr:
            assert 0 <= min(r) and max(r[0], r[2]) < cols and max(r[1], r[3]) < rows
        n = sum(max((r[3] - r[1] if BIN_DIR[b] == 2 else r[2] - r[0]) + 1, 1) for r in rr)
        bins[k, b] = (BIN_DIR[b], n, np.float32(1.0).view(np.int32), len(rr))
        runs.extend(rr)

    for k, (x, y) in enumerate(cells):
        if k == 0:
            continue                                           # a node without a neighbourhood
        if k == 1:                                             # two runs of one bin share cells; a single-cell run
            put(k, 0, [(x0 + 2, y0 + 4, x0 + 7, y0 + 4), (x0 + 5, y0 + 4, x0 + 9, y0 + 4), (x0 + 9, y0 + 9, x0 + 9, y0 + 9)])
            continue
        if k == 2:
            # every row over the whole width (unfilled border cells included: more than two chunks of 256), rows
            # y0 + 3 .. y0 + 6 again in the next bin, and a falling diagonal through them
            put(k, 0, [(0, yy, cols - 1, yy) for yy in range(rows)])
            put(k, 1, [(x0 + 1, yy, x1 - 1, yy) for yy in range(y0 + 3, y0 + 7)])
            put(k, 12, [(x0, y1, x0 + (y1 - y0), y0)])
            continue
        if k % 2:                                              # no duplicates: the row and the column behind the cell
            if x < x1:
                put(k, 0, [(x + 1, y, x1, y)])
            if y < y1:
                put(k, 8, [(x, y + 1, x, y1)])
            continue
        d = min(x1 - x, y1 - y)                                # the cell itself in three bins, one of them diagonal
        put(k, 0, [(x0, y, x1, y)])
        put(k, 4, [(x, y, x + d, y + d)])
        put(k, 8, [(x, y0, x, y1)])
    return bins, np.array(runs, dtype=np.int16).reshape(-1, 4)


def duplicate_kinds(bins, runs):
    """How many cells of each kind deduplication drops: the earlier occurrence in the same bin, in another bin, and
    the dropped cell inside a diagonal span."""
    same = other = diag = 0
    ro = 0
    for k in range(len(bins)):
        nr = int(bins[k, :, 3].sum())
        seen = {}
        for b, x, y in enumerate_node(bins[k], runs[ro:ro + nr]):
            if (x, y) in seen:
                same += seen[(x, y)] == b
                other += seen[(x, y)] != b
                diag += BIN_DIR[b] in (4, 8)
            else:
                seen[(x, y)] = b
        ro += nr
    return same, other, diag


class GraphFile:
    def __init__(self, path):
        from depthmapx_amd import _native as N
        self.N, self.lib, self.h = N, N.lib(), ctypes.c_void_p()
        N.check(self.lib.dmx_graphfile_read(path.encode(), ctypes.byref(self.h)))
        self.region = np.zeros(4)
        nl = ctypes.c_int64()
        N.check(self.lib.dmx_graphfile_info(self.h, None, None, N.ptr(self.region), ctypes.byref(nl), None, None))
        self.lines = np.zeros((nl.value, 4))
        N.check(self.lib.dmx_graphfile_lines(self.h, N.ptr(self.lines)))

    def add_pointmap(self, blob, path):
        """MetaGraph::addNewPointMap + the state VISPREP leaves (POINTMAPS | ANGULARGRAPH, SHOWVGATOP), written."""
        N, lib = self.N, self.lib
        buf = np.frombuffer(blob, dtype=np.uint8).copy()
        N.check(lib.dmx_graphfile_put_pointmap(self.h, -1, N.ptr(buf), len(buf)))
        st, vw = ctypes.c_int32(), ctypes.c_int32()
        N.check(lib.dmx_graphfile_info(self.h, ctypes.byref(st), ctypes.byref(vw), None, None, None, None))
        N.check(lib.dmx_graphfile_set_view(self.h, st.value | 0x0002 | 0x0010, lib.dmx_view_vga_top(vw.value)))
        N.check(lib.dmx_graphfile_write(self.h, path.encode()))


def make_overlap(tmp):
    import depthmapx_amd as dmx
    from depthmapx_amd import graphio
    import graphfile_util as gu
    gf = GraphFile(graph_input("rect1x1.graph", tmp, {}))
    spacing, fill = 0.04, (0.5, 0.5)
    pm = dmx.PointMap(gf.region, gf.lines, spacing)
    assert pm.make_points(*fill)
    state, cols, rows = pm.state(), pm.cols, pm.rows
    bins, runs = overlap_graph(state, cols, rows)
    n = len(bins)
    conn = np.array([bins[k, :, 1].sum() for k in range(n)], dtype=np.float32)
    blob = graphio.write_chunk(pm, bins, runs, np.zeros(n, np.uint8),
                               [("Connectivity", conn, True), ("Point First Moment", np.zeros(n, np.float32), False),
                                ("Point Second Moment", np.zeros(n, np.float32), False)])
    path = os.path.join(tmp, "overlap.graph")
    gf.add_pointmap(blob, path)
    back = gu.load_pointmap(path)   # what a reader of the file sees (4-bit shifts applied)
    assert np.array_equal(back["bins"][:, :, 3], bins[:, :, 3]) and np.array_equal(back["runs"], runs), \
        "the hand-made runs must survive the format's shift encoding"
    same, other, diag = duplicate_kinds(back["bins"], back["runs"])
    assert same > 0 and other > 0 and diag > 0, (same, other, diag)
    assert any((r[0] == r[2] and r[1] == r[3]) for r in runs) and not bins[0, :, 3].any()
    np.savez_compressed(os.path.join(OUT, "overlap.npz"), bins=back["bins"], runs=back["runs"], state=state,
                        cols=np.int32(cols), rows=np.int32(rows), region=gf.region, lines=gf.lines,
                        spacing=np.float64(spacing), fill=np.array(fill), dropped=np.int64(same + other))
    with open(path, "rb") as f, lzma.open(os.path.join(OUT, "overlap.graph.xz"), "wb", preset=9) as o:
        o.write(f.read())
    return path, same + other


def parse_info(path):
    return {k: float(v) if "." in v else int(v) for k, v in (l.split() for l in open(path))}


def store(case, kind, text, entry):
    rec = {"size": len(text), "lines": text.count(b"\n") + (0 if text.endswith(b"\n") or not text else 1),
           "sha256": hashlib.sha256(text).hexdigest(), "file": None}
    xz = lzma.compress(text, preset=9 | lzma.PRESET_EXTREME)
    name = "%s_%s.csv.xz" % (case, kind)
    path = os.path.join(OUT, "cases.json")
    same = [e["exports"][kind]["file"] for c, e in (json.load(open(path)) if os.path.exists(path) else {}).items()
            if c != case and e["exports"].get(kind, {}).get("sha256") == rec["sha256"]
            and e["exports"][kind]["file"] not in (None, name)]
    if same:   # the same bytes as another case's export (the gallery graphs share their connections): stored once
        rec["file"] = same[0]
        if os.path.exists(os.path.join(OUT, name)):
            os.remove(os.path.join(OUT, name))
    elif len(xz) <= XZ_LIMIT:
        open(os.path.join(OUT, name), "wb").write(xz)
        rec["file"] = name
    elif os.path.exists(os.path.join(OUT, name)):
        os.remove(os.path.join(OUT, name))
    entry["exports"][kind] = rec


def run_case(exe, case, tmp, made):
    src, kinds = CASES[case]
    d = os.path.join(tmp, case)
    os.makedirs(d)
    entry = {"exports": {}}
    if case == "kat":
        kat = os.path.join(tmp, "kat.graph")
        cmd = [exe, "--lines", os.path.join(HERE, "inputs", "kat_square.csv"), "--spacing", "0.5", "--fill", "0.25,0.25",
               "--write", kat, "--contents", "--out", d]
        for a, b in KAT_MERGES:
            cmd += ["--merge", "%d,%d" % (a, b)]
        subprocess.check_call(cmd)
        assert open(os.path.join(d, "connections.csv")).read().split("\n") == KAT_LINES
        with open(kat, "rb") as f, lzma.open(os.path.join(OUT, "kat.graph.xz"), "wb", preset=9) as o:
            o.write(f.read())
        raw = np.fromfile(os.path.join(d, "contents.bin"), dtype=np.int32)
        off, refs, i = [0], [], 0
        while i < len(raw):
            refs.extend(raw[i + 1:i + 1 + raw[i]])
            off.append(len(refs))
            i += 1 + raw[i]
        np.savez(os.path.join(OUT, "kat_contents.npz"), off=np.array(off, np.int64), refs=np.array(refs, np.int32))
        entry["input"] = "export/kat.graph.xz"
    else:
        if case == "overlap":
            path, dropped = make_overlap(tmp)
            entry["input"] = "export/overlap.graph.xz"
        else:
            path = graph_input(src, tmp, made)
            entry["input"] = src
        subprocess.check_call([exe, "--graph", path, "--out", d])
    info = parse_info(os.path.join(d, "info.txt"))
    assert info["outside"] == 0, "a fixture must not hold a cell outside the grid (the reference reads out of bounds)"
    if case == "overlap":
        assert info["dropped"] == dropped, (info["dropped"], dropped)
    if case == "nograph":
        assert open(os.path.join(d, "connections.csv")).read() == "RefFrom,RefTo" and info["nodes"] == 0
    for kind in kinds:
        store(case, kind, open(os.path.join(d, kind + ".csv"), "rb").read(), entry)
    entry.update(nodes=info["nodes"], enumerated=info["enumerated"], dropped=info["dropped"],
                 ref_seconds=info["t_connections"])
    path = os.path.join(OUT, "cases.json")
    cases = json.load(open(path)) if os.path.exists(path) else {}
    cases[case] = entry
    json.dump(cases, open(path, "w"), indent=1, sort_keys=True)
    print(case, {k: (v["size"], v["file"]) for k, v in entry["exports"].items()}, "dropped", info["dropped"],
          "%.3f s" % info["t_connections"], flush=True)


def main(names):
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        made = {}
        for n in names:
            run_case(exe, n, tmp, made)


if __name__ == "__main__":
    main(sys.argv[1:] or list(CASES))
