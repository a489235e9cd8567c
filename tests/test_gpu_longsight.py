"""makeGraph on inexact world coordinates and on long open sight lines, against the oracle and the reference.

Two regimes the other makeGraph tests do not reach:

  * Rooms whose world coordinates are not exact in FP64 (tests/golden/gen_synthetic.py NOISY_ROOMS: os07, with a
    fixture from the reference itself, and neg01).  The reference bins a visible cell with
    whichbin(depixelate(cell) - centre) (pointdata.cpp:1466, pointdata.h:432-520); on these grids some diagonal
    cells' |gy| / |gx| falls below 1 - 1e-12 and they go to the sector bin next to the diagonal bin
    (tests/test_noisy_rooms.py holds the precondition).  The kernel gives every diagonal cell the diagonal bin --
    the known divergence of DESIGN.md section 2, "Inexact world coordinates" -- so the bit-exact comparisons of
    bins, runs, grid connections and digests are marked xfail(strict) here, while each node's visible cells, its
    attributes and the VGA measures must hold, in every makeGraph mode.
  * A 1400^2 plaza (make_plaza_map): sight lines up to 1400 cells.  The float-margin bin decision (makegraph.hip
    chunk loop, span.hpp cell_bin / class_last) is ambiguous, for depth <= 2048, only at the (depth, ind) cells
    (780, 209), (989, 571), (1351, 362), (1351, 780), (1560, 418), (1713, 989), (1922, 515), (1978, 1142); the
    first four fit the plaza and must be visible in all 8 octants.  Rows past MK_OPEN_LDS = 1024 keep their open
    runs in scratch memory, in the chunk loop and in the spans.  Blocks of 4 sources near the four corners, bit for
    bit against the oracle in the modes default, DMX_MK_NOSPAN, DMX_MK_SPAN=1, DMX_MK_NOFIXED.
"""
import numpy as np
import pytest

import depthmapx_amd as dmx
from golden.gen_synthetic import NOISY_ROOMS, make_noisy_room, make_plaza_map
from golden_io import case_input_lines, load_case, node_digests

pytestmark = pytest.mark.gpu

VGA_RTOL = 1e-6   # tests/test_gpu_parity.py
KNOWN = "known divergence (DESIGN.md section 2, 'Inexact world coordinates'): every diagonal cell takes the diagonal bin"

MODES = {"default": {}, "nospan": {"DMX_MK_NOSPAN": "1"}, "span1": {"DMX_MK_SPAN": "1"},
         "nofixed": {"DMX_MK_NOFIXED": "1"}, "exact": {"DMX_MK_EXACT": "1"}}
PLAZA_MODES = ["default", "nospan", "span1", "nofixed"]
D_H, D_V, D_PD, D_ND = 1, 2, 4, 8   # Bin::m_dir (ngraph.h)


def _set_mode(monkeypatch, mode):
    for env in MODES.values():
        for k in env:
            monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


def _run_cells(runs, dirs, rows):
    """The x-major cells of each run, walked as the Bin cursor does (ngraph.cpp:395-416): (run index, cell) pairs."""
    r = runs.astype(np.int64)
    n = np.where(dirs == D_V, r[:, 3] - r[:, 1], r[:, 2] - r[:, 0]) + 1
    idx = np.repeat(np.arange(len(r)), n)
    t = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    d = dirs[idx]
    x = r[idx, 0] + np.where(d == D_V, 0, t)
    y = r[idx, 1] + np.where((d == D_V) | (d == D_PD), t, np.where(d == D_ND, -t, 0))
    return idx, x * rows + y


def _node_cells(bins, runs, rows, ncells=None):
    """Per node, the sorted distinct x-major cells its runs cover."""
    nr = bins[:, :, 3].astype(np.int64)
    assert int(nr.sum()) == len(runs)
    dirs = np.repeat(bins[:, :, 0].ravel(), nr.ravel())
    idx, cells = _run_cells(runs, dirs, rows)
    C = ncells or (int(cells.max()) + 1 if len(cells) else 1)
    cut = np.searchsorted(idx, np.concatenate([[0], np.cumsum(nr.sum(axis=1))]))   # runs are in node order
    out = []
    for k in range(len(bins)):
        mask = np.zeros(C, dtype=bool)
        mask[cells[cut[k]:cut[k + 1]]] = True
        out.append(np.flatnonzero(mask))
    return out


def _gridconn(bins, runs, node_cells, rows):
    """addGridConnections (pointdata.cpp:1735-1768) per node: bit i / 4 is set when bin i (0, 4, ..., 28) holds the
    i / 4-th cell of the walk around the node that starts at its right-hand neighbour."""
    mv = [(0, 1), (-1, 0), (-1, 0), (0, -1), (0, -1), (1, 0), (1, 0), (0, 0)]
    out = np.zeros(len(bins), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum(bins[:, :, 3].ravel())]).reshape(-1)
    for k in range(len(bins)):
        cx, cy = divmod(int(node_cells[k]), rows)
        nx, ny = cx + 1, cy
        for i in range(0, 32, 4):
            rr = runs[off[32 * k + i]:off[32 * k + i + 1]]
            if len(rr):
                _, cells = _run_cells(rr, np.full(len(rr), bins[k, i, 0]), rows)
                if (nx * rows + ny) in cells:
                    out[k] |= 1 << (i // 4)
            nx, ny = nx + mv[i // 4][0], ny + mv[i // 4][1]
    return out


def _assert_same_cells(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), "%s: node %d sees %d cells, the oracle %d" % (what, k, len(a), len(b))


def _assert_close(got, want, int_cols, what):
    got, want = got.astype(np.float64), want.astype(np.float64)
    for c in int_cols:
        np.testing.assert_array_equal(got[:, c], want[:, c], err_msg="%s column %d" % (what, c))
    both_nan = np.isnan(got) & np.isnan(want)
    bad = ~both_nan & ~(np.abs(got - want) <= VGA_RTOL * np.maximum(1.0, np.abs(want)))
    assert not bad.any(), "%s: %d values differ, first %s" % (what, bad.sum(), np.argwhere(bad)[:5].tolist())


# ---------------------------------------------------------------- B1: the rooms, whole maps
def _room_inputs(name):
    origin, spacing, n, seed = NOISY_ROOMS[name]
    region, lines, fill = make_noisy_room(origin, spacing, n, seed)
    return region, lines, spacing, fill


@pytest.fixture(scope="module")
def rooms():
    """Per room: the oracle's graph (computed once, left unchanged), its cells per node, the reference fixture."""
    from pyoracle import OracleMap
    out = {}
    for name in NOISY_ROOMS:
        region, lines, spacing, fill = _room_inputs(name)
        om = OracleMap(region, spacing, lines)
        assert om.fill(*fill)
        om.make_graph(threads=8)
        ref = om.graph()
        st = om.state()
        node_cells = np.nonzero(st & 2)[0]
        fixture = load_case(name)[1] if name == "os07" else None
        out[name] = dict(om=om, ref=ref, state=st, rows=om.rows, node_cells=node_cells, fixture=fixture,
                         cells=_node_cells(ref["bins"], ref["runs"], om.rows))
        # the test-side addGridConnections is the oracle's
        np.testing.assert_array_equal(_gridconn(ref["bins"], ref["runs"], node_cells, om.rows), ref["gridconn"])
    return out


def _room_graph(ctx, name):
    region, lines, spacing, fill = _room_inputs(name)
    pm = dmx.PointMap(region, lines, spacing)
    assert pm.make_points(*fill)
    return pm, pm.make_graph(ctx)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", sorted(NOISY_ROOMS))
def test_room_visible_cells_and_attributes_match_oracle(ctx, monkeypatch, rooms, name, mode):
    """Every node's visible cells (the cells its runs cover) and the three attributes, bit for bit, against the
    oracle and (os07) the reference's own dump; the graph is the default mode's, bit for bit, in every mode; and
    the engine reports the coordinate condition (mk_diag_inexact)."""
    R = rooms[name]
    _set_mode(monkeypatch, mode)
    pm, g = _room_graph(ctx, name)
    st = ctx.last_stats()
    got = g.copy(runs=True)
    np.testing.assert_array_equal(pm.state(), R["state"])
    assert g.info()["nnodes"] == len(R["ref"]["bins"])
    np.testing.assert_array_equal(got["attrs"].view(np.uint32), R["ref"]["attrs"].view(np.uint32))
    if R["fixture"] is not None:
        np.testing.assert_array_equal(got["attrs"].view(np.uint32), R["fixture"]["attrs"].view(np.uint32))
    _assert_same_cells(_node_cells(got["bins"], got["runs"], R["rows"]), R["cells"], "%s, mode %s" % (name, mode))
    # each visible cell is in exactly one bin (the reference lists a moved diagonal cell in its sector bin only)
    assert int(got["bins"][:, :, 1].sum()) == int(R["ref"]["bins"][:, :, 1].sum()) == st["mk_visible_pairs"]
    np.testing.assert_array_equal(_gridconn(got["bins"], got["runs"], R["node_cells"], R["rows"]), got["gridconn"])
    assert st["mk_diag_inexact"] > 0
    if mode != "default":
        _set_mode(monkeypatch, "default")
        base = _room_graph(ctx, name)[1].copy(runs=True)
        for k in ("bins", "runs", "gridconn"):
            np.testing.assert_array_equal(got[k], base[k], err_msg="%s in mode %s against the default mode" % (k, mode))
        np.testing.assert_array_equal(got["attrs"].view(np.uint32), base["attrs"].view(np.uint32))


@pytest.mark.xfail(strict=True, reason=KNOWN)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", sorted(NOISY_ROOMS))
def test_room_bins_runs_gridconn_digests_match_oracle_bit_for_bit(ctx, monkeypatch, rooms, name, mode):
    """Bin records, run lists, grid connections and node digests against the oracle and (os07) the reference's dump.
    Measured on the MI355X: every case fails at its first assertion, the bin records, with "Mismatched elements:
    11438 / 73728 (15.5%)" on os07 and "3598 / 115200 (3.12%)" on neg01.  os07 holds 3,350 pairs in the diagonal
    bins 4 / 12 / 20 / 28 in the reference (68,795 runs), neg01 32,340 (134,411 runs); the engine returns the bins of
    the same rooms with unit coordinates (15,904 and 33,440 pairs; 66,268 runs on os07)."""
    R = rooms[name]
    _set_mode(monkeypatch, mode)
    pm, g = _room_graph(ctx, name)
    got = g.copy(runs=True)
    for want in (R["ref"], R["fixture"]):
        if want is None:
            continue
        np.testing.assert_array_equal(got["bins"], want["bins"])
        np.testing.assert_array_equal(got["runs"], want["runs"])
        np.testing.assert_array_equal(got["gridconn"], want["gridconn"])
        np.testing.assert_array_equal(node_digests(got["bins"], got["runs"]),
                                      want["digests"] if "digests" in want else node_digests(want["bins"], want["runs"]))


@pytest.mark.parametrize("name", sorted(NOISY_ROOMS))
def test_room_vga_matches_oracle_on_the_same_graph(ctx, rooms, name):
    """VGA global (radius n and 3), local, metric, angular and through vision on the engine's graph of the room,
    against the oracle's searches over that same graph (through vision: tests/thruvision_model.py): integer columns
    exact, floats within VGA_RTOL.  os07's global measures also against the reference's own (its graph covers the
    same cells)."""
    import thruvision_model as tvm
    from pyoracle import OracleMap
    R = rooms[name]
    region, lines, spacing, fill = _room_inputs(name)
    pm, g = _room_graph(ctx, name)
    c = g.copy(runs=True)
    om = OracleMap(region, spacing, lines)
    assert om.fill(*fill)
    om.make_graph(threads=8)
    om.set_graph(c["bins"], c["runs"])
    for radius in (-1.0, 3.0):
        _assert_close(g.vga_visual_global(radius=radius), om.vga_global(radius=radius, threads=8), [5],
                      "%s VGA global radius %g" % (name, radius))
    if R["fixture"] is not None:
        _assert_close(g.vga_visual_global(radius=-1), R["fixture"]["vga"], [5], "%s VGA global against the reference" % name)
    _assert_close(g.vga_visual_local(), om.vga_local(threads=8), [], "%s VGA local" % name)
    _assert_close(g.vga_metric(), om.vga_metric(threads=8), [3], "%s VGA metric" % name)
    _assert_close(g.vga_angular(), om.vga_angular(threads=8), [2], "%s VGA angular" % name)
    out, cnt = g.vga_through_vision(counts=True)
    model = tvm.through_vision(om.cols, om.rows, R["state"], c["bins"][:, :, 3].sum(axis=1), c["runs"])
    np.testing.assert_array_equal(cnt, model)
    np.testing.assert_array_equal(out, model.astype(np.float32))
    assert model.sum() > 0


# ---------------------------------------------------------------- B2 / B3: the plaza
W = 1400
MARGIN_CELLS = [(780, 209), (989, 571), (1351, 362), (1351, 780)]   # (depth, ind): the float test's ambiguous cells
CORNER_OFFSETS = [1, 8, 20, 40]


class Plaza:
    def __init__(self, origin, spacing):
        from pyoracle import OracleMap
        self.region, self.lines, self.fill = make_plaza_map(W, origin=origin, spacing=spacing)
        self.pm = dmx.PointMap(self.region, self.lines, spacing)
        assert self.pm.make_points(*self.fill)
        self.om = OracleMap(self.region, spacing, self.lines)
        assert self.om.fill(*self.fill)
        self.state = self.pm.state()
        np.testing.assert_array_equal(self.state, self.om.state())
        self.rows, self.cols = self.pm.rows, self.pm.cols
        assert self.rows == self.cols == W + 1
        self.filled = np.nonzero(self.state & 2)[0]
        self._ref = {}

    def blocks(self, offsets):
        """Per offset c and corner: the 4 consecutive nodes (x-major: up the column) starting at the cell (c, c),
        (W - c, c), (c, W - c), (W - c, W - c)."""
        out = []
        for c in offsets:
            for (x, y) in ((c, c), (W - c, c), (c, W - c), (W - c, W - c)):
                cell = x * self.rows + y
                k = int(np.searchsorted(self.filled, cell))
                assert self.filled[k] == cell, "source cell (%d, %d) is not filled" % (x, y)
                k = min(k, len(self.filled) - 4)   # (W - 1, W - 1) is the map's last node: the block ends there
                out.append((c, (x, y), k, k + 4))
        return out

    def oracle(self, blocks):
        """The oracle's graph of each block (sparkPixel2 of its 4 sources), computed once and kept."""
        todo = [(b, e) for (_, _, b, e) in blocks if (b, e) not in self._ref]
        if todo:
            self.om.make_graph_sample(np.concatenate([np.arange(b, e) for (b, e) in todo]), threads=16)
            for (b, e) in todo:
                r = self.om.graph_range(b, e)
                r["gridconn"] = _gridconn(r["bins"], r["runs"], self.filled[b:e], self.rows)
                self._ref[(b, e)] = r
        return [self._ref[(b, e)] for (_, _, b, e) in blocks]


@pytest.fixture(scope="module")
def plaza(ctx):
    p = Plaza((0.0, 0.0), 1.0)
    yield p
    p.pm.close()


@pytest.fixture(scope="module")
def plaza07(ctx):
    p = Plaza(NOISY_ROOMS["os07"][0], 0.7)
    yield p
    p.pm.close()


@pytest.mark.parametrize("c", CORNER_OFFSETS)
def test_plaza_blocks_match_oracle_in_every_mode(ctx, monkeypatch, plaza, c):
    """Blocks of 4 sources c cells from each corner of the plaza: bins, runs, attributes and grid connections bit
    for bit against the oracle in each mode, with the same cells examined and visible pairs in every mode and the
    oracle's pair count."""
    blocks = plaza.blocks([c])
    for (_, xy, b, e), ref in zip(blocks, plaza.oracle(blocks)):
        stats = {}
        for mode in PLAZA_MODES:
            _set_mode(monkeypatch, mode)
            g = plaza.pm.make_graph(ctx, node_begin=b, node_end=e)
            st = ctx.last_stats()
            stats[mode] = (st["mk_cells_examined"], st["mk_visible_pairs"])
            got = g.copy(runs=True)
            g.close()
            what = "source block at %s, mode %s" % (xy, mode)
            np.testing.assert_array_equal(got["bins"], ref["bins"], err_msg="bins, " + what)
            np.testing.assert_array_equal(got["runs"], ref["runs"], err_msg="runs, " + what)
            np.testing.assert_array_equal(got["attrs"].view(np.uint32), ref["attrs"].view(np.uint32), err_msg="attributes, " + what)
            np.testing.assert_array_equal(got["gridconn"], ref["gridconn"], err_msg="grid connections, " + what)
            assert st["mk_diag_inexact"] == 0
        assert len(set(stats.values())) == 1, "examined cells / visible pairs differ between modes at %s: %s" % (xy, stats)
        # (Connectivity: the bin records' own counts are 16-bit)
        assert stats["default"][1] == int(ref["attrs"][:, 0].astype(np.int64).sum()) > 0


def _octant_of(dx, dy):
    """The sieve's octant (sparksieve2.cpp:134-141) of a cell off the axes and diagonals."""
    if abs(dx) > abs(dy):
        return (0 if dx < 0 else 1) + (0 if dy > 0 else 2)
    return {(-1, -1): 4, (1, -1): 5, (-1, 1): 6, (1, 1): 7}[(int(np.sign(dx)), int(np.sign(dy)))]


def test_plaza_sample_reaches_the_margin_cells_and_far_rows(plaza):
    """What the blocks above must exercise, from the oracle's runs: each of the float test's ambiguous (depth, ind)
    cells is visible from some sampled source in each of the 8 octants, and every octant has visible cells whose
    minor offset (the row, ind) is >= 1024 -- rows whose open runs live in scratch memory."""
    blocks = plaza.blocks(CORNER_OFFSETS)
    seen = set()
    far = np.zeros(8, dtype=np.int64)
    rows = plaza.rows
    for (_, _, b, e), ref in zip(blocks, plaza.oracle(blocks)):
        cells = _node_cells(ref["bins"], ref["runs"], rows, plaza.cols * rows)
        for k in range(e - b):
            sx, sy = divmod(int(plaza.filled[b + k]), rows)
            mask = np.zeros((plaza.cols, rows), dtype=bool)
            mask.ravel()[cells[k]] = True
            for (d, i) in MARGIN_CELLS:
                for (dx, dy) in ((d, i), (-d, i), (d, -i), (-d, -i), (i, d), (-i, d), (i, -d), (-i, -d)):
                    x, y = sx + dx, sy + dy
                    if 0 <= x < plaza.cols and 0 <= y < rows and mask[x, y]:
                        seen.add(((d, i), _octant_of(dx, dy)))
            # both offsets >= 1024: at most a (W - 1024)^2 corner of the map per quadrant
            for (qx, qy) in ((-1, 1), (1, 1), (-1, -1), (1, -1)):
                xs = np.arange(sx + 1024, plaza.cols) if qx > 0 else np.arange(0, max(sx - 1023, 0))
                ys = np.arange(sy + 1024, rows) if qy > 0 else np.arange(0, max(sy - 1023, 0))
                if len(xs) == 0 or len(ys) == 0:
                    continue
                sub = mask[xs[0]:xs[-1] + 1, ys[0]:ys[-1] + 1]
                adx, ady = np.abs(xs - sx)[:, None], np.abs(ys - sy)[None, :]
                far[_octant_of(2 * qx, qy)] += int((sub & (adx > ady)).sum())
                far[_octant_of(qx, 2 * qy)] += int((sub & (adx < ady)).sum())
    missing = [(c, q) for c in MARGIN_CELLS for q in range(8) if (c, q) not in seen]
    print("margin cells seen: %d of 32 (cell, octant) pairs; visible cells with a row >= 1024 per octant: %s" %
          (32 - len(missing), far.tolist()))
    assert not missing, missing
    assert (far > 0).all(), far.tolist()


def _plaza07_blocks(ctx, plaza07):
    blocks = plaza07.blocks([20])
    out = []
    for (_, xy, b, e), ref in zip(blocks, plaza07.oracle(blocks)):
        g = plaza07.pm.make_graph(ctx, node_begin=b, node_end=e)
        st = ctx.last_stats()
        out.append((xy, g.copy(runs=True), ref, st))
        g.close()
    return out


def test_plaza_inexact_coordinates_visible_cells_and_attributes(ctx, monkeypatch, plaza07):
    """The plaza on os07's origin with spacing 0.7 (the margin branch's FP64 whichbin under coordinate noise), the
    blocks 20 cells from each corner, default mode: visible cells, attributes and pair counts against the oracle."""
    _set_mode(monkeypatch, "default")
    for xy, got, ref, st in _plaza07_blocks(ctx, plaza07):
        np.testing.assert_array_equal(got["attrs"].view(np.uint32), ref["attrs"].view(np.uint32), err_msg="block at %s" % (xy,))
        _assert_same_cells(_node_cells(got["bins"], got["runs"], plaza07.rows), _node_cells(ref["bins"], ref["runs"], plaza07.rows),
                           "block at %s" % (xy,))
        assert st["mk_visible_pairs"] == int(ref["attrs"][:, 0].astype(np.int64).sum()) > 0
        assert st["mk_diag_inexact"] > 0
        # off the diagonal bins and the two sector bins next to each, the bin records are the reference's
        near = sorted(set(b % 32 for d in (4, 12, 20, 28) for b in (d - 1, d, d + 1)))
        keep = [b for b in range(32) if b not in near]
        np.testing.assert_array_equal(got["bins"][:, keep], ref["bins"][:, keep], err_msg="block at %s" % (xy,))


@pytest.mark.xfail(strict=True, reason=KNOWN)
def test_plaza_inexact_coordinates_bins_runs_bit_for_bit(ctx, monkeypatch, plaza07):
    """The same blocks' bin records, runs and grid connections bit for bit.  Measured on the MI355X: the first block,
    at (20, 20), fails at its bin records with "Mismatched elements: 69 / 512 (13.5%)" (diagonal cells the reference
    moved to bins 3 / 5, 11 / 13, 19 / 21, 27 / 29)."""
    _set_mode(monkeypatch, "default")
    for xy, got, ref, st in _plaza07_blocks(ctx, plaza07):
        np.testing.assert_array_equal(got["bins"], ref["bins"], err_msg="bins, block at %s" % (xy,))
        np.testing.assert_array_equal(got["runs"], ref["runs"], err_msg="runs, block at %s" % (xy,))
        np.testing.assert_array_equal(got["gridconn"], ref["gridconn"], err_msg="grid connections, block at %s" % (xy,))
