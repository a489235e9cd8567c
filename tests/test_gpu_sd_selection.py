"""Step depth from a selected region: the batched metric search (sdb_* kernels, kernels/stepdepth.hip) where one
batch holds hundreds or thousands of expanders -- the block pass of its fold (relaxer lists longer than 32), its
three capacities and the serial fallback behind them -- and the serial queue with more than one window of keys at
distance 0, with visual step depth from the same selections as a companion.

The maps are open rooms (tests/golden/gen_synthetic.py make_open_room): every filled cell sees every other, so the
first batch is the selection, and the relaxer list of every unselected cell whose nearest selected cells tie is the
whole selection.  The CPU tests assert that premise and the tie counts from the oracle's graph and with numpy.  In
such a room every relaxer of the first batch carries angle 0 and no last pixel and all ties are exact, so the order
of a fold there cannot show in the output; the pillar hall (hall64 of test_gpu_sd_queue.py) adds the cases whose
long lists come from later batches, whose relaxers differ in angle.

Every result is compared with the C restatement (pyoracle.OracleMap; path length and straight-line distance bit
for bit, the angle as test_gpu_parity._assert_stepdepth does) and bit for bit on all three columns with the serial
kernel on the GPU.  Every "this path ran" assertion reads the kernel's own counters (Context.last_stepdepth)."""
import functools

import numpy as np
import pytest

import test_gpu_sd_queue as Q   # hall64: its oracle, selections and references, shared

ROOMS = {"room40": 40, "room96": 96}
W_REL = 2.0 ** -20   # the batched search's ambiguity window (sdb_w): rivals within s * 2^-20 of the smallest s
SDB_FOLD_CAP = 2048  # relaxers of one ambiguous cell (kernels/stepdepth.hip)
SD_WIN = 4096        # keys in the serial queue's LDS window


# ---------------------------------------------------------------- maps and selections
@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The room's OracleMap with its graph made: built once, shared, never changed."""
    if name == "hall64":
        return Q._oracle(name)
    from golden.gen_synthetic import make_open_room
    from pyoracle import OracleMap
    region, lines, fill = make_open_room(ROOMS[name])
    om = OracleMap(region, 1.0, lines)
    assert om.fill(*fill)
    om.make_graph(threads=8)
    return om, region, lines, fill


def _rows(name):
    return (64 if name == "hall64" else ROOMS[name]) + 1


def _cells(name, xy):
    """(x, y) pairs as x-major cells in ascending order, which is PixelRef order."""
    return sorted(x * _rows(name) + y for x, y in xy)


ROW33 = [(x, 5) for x in range(3, 34)] + [(20, 15), (20, 25)]
COLS96 = [(x, y) for x in range(2, 65, 3) for y in range(1, 96) if (x, y) != (32, 48)]   # 21 columns less one cell


@functools.lru_cache(maxsize=None)
def _selection(sel):
    """(map, cells in PixelRef order).
    s33: a row of 31 cells and two cells above its middle; s32: the same less the row's last cell.
    s2048 / s2049: full-height columns at an x pitch of 3 (no tie among them: every other cell has one nearest
    column cell), one cell taken out of a column (which ties its two neighbours in the column for that cell and
    the two beside it) and the start of a 22nd column, 54 or 55 cells long.
    s5000: a fixed-seed random choice of 5,000 of the 9,025 cells.
    block: the filled cells of a 10 x 10 block of the pillar hall; three: three far cells of it."""
    if sel == "s33":
        return "room40", tuple(_cells("room40", ROW33))
    if sel == "s32":
        return "room40", tuple(_cells("room40", [c for c in ROW33 if c != (33, 5)]))
    if sel in ("s2048", "s2049"):
        n = int(sel[1:])
        return "room96", tuple(_cells("room96", COLS96 + [(65, y) for y in range(1, 1 + n - len(COLS96))]))
    if sel == "s5000":
        filled = np.flatnonzero(_oracle("room96")[0].state() & 2)
        return "room96", tuple(int(c) for c in np.sort(np.random.default_rng(5000).choice(filled, 5000, replace=False)))
    if sel == "three":   # test_gpu_sd_queue's three far cells of the pillar hall
        return "hall64", tuple(_cells("hall64", [(5, 40), (33, 9), (60, 58)]))
    assert sel == "block"
    st = _oracle("hall64")[0].state()
    return "hall64", tuple(c for c in _cells("hall64", [(x, y) for x in range(20, 30) for y in range(20, 30)])
                           if st[c] & 2)


def _first_batch_ties(sel):
    """The unselected filled cells whose nearest selected cells tie within a relative 2^-20: the first batch's
    ambiguous cells in a room where every cell sees every other.  [n][2] (x, y)."""
    name, cells = _selection(sel)
    rows = _rows(name)
    filled = np.flatnonzero(_oracle(name)[0].state() & 2)
    rest = np.setdiff1d(filled, np.array(cells))
    s = np.array(cells)
    sx, sy = (s // rows).astype(np.float64), (s % rows).astype(np.float64)
    out = []
    for i in range(0, len(rest), 256):
        c = rest[i:i + 256]
        d = np.sqrt((c[:, None] // rows - sx[None, :]) ** 2 + (c[:, None] % rows - sy[None, :]) ** 2)
        near = d <= d.min(axis=1)[:, None] * (1.0 + W_REL)
        out.append(c[near.sum(axis=1) >= 2])
    t = np.concatenate(out)
    return np.stack([t // rows, t % rows], axis=1)


@functools.lru_cache(maxsize=None)
def _want_metric(sel):
    name, cells = _selection(sel)
    return _oracle(name)[0].metric_stepdepth(list(cells))


@functools.lru_cache(maxsize=None)
def _want_angular(sel):
    name, cells = _selection(sel)
    return _oracle(name)[0].angular_stepdepth(list(cells))


@functools.lru_cache(maxsize=None)
def _want_visual(sel):
    name, cells = _selection(sel)
    return _oracle(name)[0].visual_stepdepth(list(cells))


@pytest.fixture(scope="module")
def maps(ctx):
    """maps(name) -> (PointMap, Graph) on the GPU: made once, closed with the module."""
    import depthmapx_amd as dmx
    made = {}

    def get(name):
        if name not in made:
            om, region, lines, fill = _oracle(name)
            pm = dmx.PointMap(region, lines, 1.0)
            assert pm.make_points(*fill)
            np.testing.assert_array_equal(pm.state(), om.state())
            made[name] = (pm, pm.make_graph(ctx))
        return made[name]
    yield get
    for pm, g in made.values():
        g.close()
        pm.close()


HOOKS = ["DMX_SD_KERNEL", "DMX_SD_CAP", "DMX_SDB_AMB_CAP", "DMX_SDB_ENT_CAP", "DMX_VSD_TOPDOWN"]

_serial = {}   # (map, cells) -> the serial kernel's result on the GPU: run once, shared, never changed


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _metric(ctx, maps, monkeypatch, name, cells, label, **env):
    """One metric step depth with the default hooks but `env`: (result, last_stepdepth())."""
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    got = maps(name)[1].metric_step_depth(cells=np.array(cells, dtype=np.int32))
    sd = ctx.last_stepdepth()
    print("%s: %s" % (label, sd))
    return got, sd


def _check_metric(ctx, maps, monkeypatch, name, cells, got, want):
    """got against the oracle's `want` and against the serial kernel on the GPU."""
    from test_gpu_parity import _assert_stepdepth
    _assert_stepdepth(got, want)
    key = (name, tuple(cells))
    if key not in _serial:
        ser, sd = _metric(ctx, maps, monkeypatch, name, cells, "  serial kernel, %d cells" % len(cells),
                          DMX_SD_KERNEL="serial")
        assert sd["mode"] == "serial" and sd["overflow"] is None and sd["fold_long"] == 0, sd
        _assert_stepdepth(ser, want)
        ser.setflags(write=False)
        _serial[key] = ser
    np.testing.assert_array_equal(_bits(got), _bits(_serial[key]))
    assert (got[:, 1] >= 0).all()


# ---------------------------------------------------------------- CPU: the premises
@pytest.mark.parametrize("name", ["room40", "room96"])
def test_open_room_every_cell_sees_every_other(name):
    """The oracle's graph of an open room: (W - 1)^2 nodes, each connected to all the others, so an expander
    relaxes every cell and a tied cell's relaxer list in the first batch is the whole selection."""
    om = _oracle(name)[0]
    n = (ROOMS[name] - 1) ** 2
    assert om.num_nodes == n == int((om.state() & 2).astype(bool).sum())
    b = om.graph()
    assert (b["attrs"][:, 0] == n - 1).all()                  # Connectivity
    assert (b["bins"][:, :, 1].sum(axis=1) == n - 1).all()    # the cells of each node's 32 bins


def test_selection_sizes_and_first_batch_ties():
    """What the GPU cases rely on, counted with numpy."""
    size = {s: len(_selection(s)[1]) for s in ("s32", "s33", "s2048", "s2049", "s5000", "block")}
    assert size == {"s32": 32, "s33": 33, "s2048": 2048, "s2049": 2049, "s5000": 5000, "block": size["block"]}
    assert 33 < size["block"] <= 100
    assert list(_selection("three")[1]) == sorted(Q._selections("hall64")["three"])
    for s in size:   # selected cells are filled and distinct
        name, cells = _selection(s)
        assert len(set(cells)) == len(cells) and (_oracle(name)[0].state()[list(cells)] & 2).all()
    assert set(_selection("s2048")[1]) < set(_selection("s2049")[1])
    assert len(_first_batch_ties("s33")) == 32
    assert len(_first_batch_ties("s32")) > 0
    for s in ("s2048", "s2049"):
        t = _first_batch_ties(s)
        # few enough that one thread's insertion sort of each list stays short and that ties x list length is
        # far below the 2^22 list entries of a batch: the fold list is the first capacity reached
        assert 1 <= len(t) <= 16, t
        assert {(31, 48), (32, 48), (33, 48)} <= set(map(tuple, t.tolist()))
        assert len(t) * size[s] * 64 < 1 << 22
    # 5,000 of 9,025 cells: ties everywhere, and each tied cell lists 5,000 relaxers
    t = _first_batch_ties("s5000")
    assert len(t) > 1000 and size["s5000"] > SDB_FOLD_CAP and size["s5000"] > SD_WIN
    assert len(t) * size["s5000"] > 1 << 22


# ---------------------------------------------------------------- GPU: the fold's two passes
@pytest.mark.gpu
def test_fold_32_relaxers_thread_pass(ctx, maps, monkeypatch):
    name, cells = _selection("s32")
    got, sd = _metric(ctx, maps, monkeypatch, name, cells, "fold 32, room40")
    assert sd["mode"] == "batched" and sd["overflow"] is None and sd["attempts"] == 0, sd
    assert sd["fold_long"] == 0 and sd["list_max"] == 32 and sd["ambiguous"] > 0, sd
    _check_metric(ctx, maps, monkeypatch, name, cells, got, _want_metric("s32"))


@pytest.mark.gpu
def test_fold_33_relaxers_block_pass(ctx, maps, monkeypatch):
    name, cells = _selection("s33")
    got, sd = _metric(ctx, maps, monkeypatch, name, cells, "fold 33, room40")
    assert sd["mode"] == "batched" and sd["overflow"] is None and sd["attempts"] == 0, sd
    assert sd["fold_long"] >= 1 and sd["list_max"] == 33, sd
    assert sd["ambiguous"] >= len(_first_batch_ties("s33")), sd
    assert sd["amb_max"] >= len(_first_batch_ties("s33")) and sd["ent_max"] >= 33 * len(_first_batch_ties("s33")), sd
    _check_metric(ctx, maps, monkeypatch, name, cells, got, _want_metric("s33"))
    # the host sorts into PixelRef order, drops duplicates and unfilled cells (the walls' cells)
    rng = np.random.default_rng(33)
    rows = _rows(name)
    walls = [0, 7, 40 * rows + 40, 13 * rows, 40 * rows + 9, 22 * rows + 40]
    assert not (_oracle(name)[0].state()[walls] & 2).any()
    messy = rng.permutation(np.concatenate([np.array(cells), np.array(cells)[::3], np.array(walls)]))
    again, sd2 = _metric(ctx, maps, monkeypatch, name, messy, "fold 33 shuffled, room40")
    np.testing.assert_array_equal(_bits(again), _bits(got))
    assert (sd2["fold_long"], sd2["list_max"], sd2["expanders_popped"]) == \
        (sd["fold_long"], sd["list_max"], sd["expanders_popped"])


@pytest.mark.gpu
@pytest.mark.parametrize("sel", ["three", "block"])
def test_fold_long_lists_of_later_batches_pillar_hall(ctx, maps, monkeypatch, sel):
    """The pillar hall, where nearly every cell is an expander: the batches after the first hold more than 32
    expanders that differ in angle and last pixel, and lattice ties give cells long lists of them.  From the
    three far cells the order of the block pass's fold decides angles of the result (with the comparison of its
    insertion sort reversed this case fails on column 0); the block of 100 cells is the same from a region."""
    name, cells = _selection(sel)
    got, sd = _metric(ctx, maps, monkeypatch, name, cells, "%s, hall64" % sel)
    assert sd["mode"] == "batched" and sd["overflow"] is None, sd
    assert sd["fold_long"] >= 1 and sd["list_max"] > 32 and sd["batches"] > 1, sd
    _check_metric(ctx, maps, monkeypatch, name, cells, got, _want_metric(sel))
    assert got[:, 0].max() > 0


# ---------------------------------------------------------------- GPU: the fold list's capacity
@pytest.mark.gpu
def test_fold_capacity_2048_relaxers(ctx, maps, monkeypatch):
    name, cells = _selection("s2048")
    got, sd = _metric(ctx, maps, monkeypatch, name, cells, "fold 2048, room96")
    print("fold 2048, room96: %.4f s" % sd["seconds"])
    assert sd["mode"] == "batched" and sd["overflow"] is None and sd["attempts"] == 0, sd
    assert sd["list_max"] == SDB_FOLD_CAP and sd["fold_long"] >= 1, sd
    _check_metric(ctx, maps, monkeypatch, name, cells, got, _want_metric("s2048"))


@pytest.mark.gpu
def test_fold_capacity_2049_relaxers_serial_fallback(ctx, maps, monkeypatch):
    name, cells = _selection("s2049")
    got, sd = _metric(ctx, maps, monkeypatch, name, cells, "fold 2049, room96")
    print("fold 2049, room96: %.4f s" % sd["seconds"])
    assert sd["mode"] == "batched-overflow-serial" and sd["overflow"] == "fold" and sd["attempts"] >= 1, sd
    _check_metric(ctx, maps, monkeypatch, name, cells, got, _want_metric("s2049"))
    # the next call starts clean
    name, cells = _selection("s33")
    got, sd = _metric(ctx, maps, monkeypatch, name, cells, "fold 33 after an overflow, room40")
    assert sd["mode"] == "batched" and sd["overflow"] is None and sd["attempts"] == 0, sd
    _check_metric(ctx, maps, monkeypatch, name, cells, got, _want_metric("s33"))


# ---------------------------------------------------------------- GPU: the two batch capacities at their edge
def _hook_case(case):
    sel = {"room40-s33": "s33", "hall64-three": "three"}[case]
    name, cells = _selection(sel)
    return name, cells, _want_metric(sel)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["room40-s33", "hall64-three"])
@pytest.mark.parametrize("hook,counter,reason", [("DMX_SDB_AMB_CAP", "amb_max", "amb"),
                                                 ("DMX_SDB_ENT_CAP", "ent_max", "ent")])
def test_batch_capacity_hooks_at_their_edge(ctx, maps, monkeypatch, case, hook, counter, reason):
    """The counter only finds the edge; both sides of it are asserted, so a wrong counter fails one of the runs."""
    name, cells, want = _hook_case(case)
    got, sd = _metric(ctx, maps, monkeypatch, name, cells, "%s defaults" % case)
    assert sd["mode"] == "batched" and sd["overflow"] is None, sd
    assert sd["amb_max"] > 1 and sd["ent_max"] > 1, sd
    _check_metric(ctx, maps, monkeypatch, name, cells, got, want)
    edge = sd[counter]
    at, sda = _metric(ctx, maps, monkeypatch, name, cells, "%s %s=%d" % (case, hook, edge), **{hook: edge})
    assert sda["mode"] == "batched" and sda["overflow"] is None and sda["attempts"] == 0, sda
    assert sda[counter] == edge, sda
    np.testing.assert_array_equal(_bits(at), _bits(got))
    below, sdb = _metric(ctx, maps, monkeypatch, name, cells, "%s %s=%d" % (case, hook, edge - 1), **{hook: edge - 1})
    assert sdb["mode"] == "batched-overflow-serial" and sdb["overflow"] == reason and sdb["attempts"] >= 1, sdb
    np.testing.assert_array_equal(_bits(below), _bits(got))


# ---------------------------------------------------------------- GPU: more than a window of keys at distance 0
def _assert_refill_health(sd):
    # test_gpu_sd_queue.test_refill_brings_back_many_keys: 16 pops a refill, a 32-fold margin on the 512 keys a
    # refill aims at; a cut that cannot separate the keys at one distance brings back one key a refill
    assert sd["refills"] > 0, sd
    assert sd["refills"] * 16 <= sd["expanders_popped"], sd


@pytest.mark.gpu
def test_5000_cells_serial_metric_refills(ctx, maps, monkeypatch):
    name, cells = _selection("s5000")
    got, sd = _metric(ctx, maps, monkeypatch, name, cells, "5000 cells serial metric, room96", DMX_SD_KERNEL="serial")
    assert sd["mode"] == "serial" and sd["attempts"] == 1 and sd["overflow"] is None, sd
    _assert_refill_health(sd)
    _check_metric(ctx, maps, monkeypatch, name, cells, got, _want_metric("s5000"))


@pytest.mark.gpu
def test_5000_cells_angular_refills(ctx, maps, monkeypatch):
    name, cells = _selection("s5000")
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    got = maps(name)[1].angular_step_depth(cells=np.array(cells, dtype=np.int32))
    sd = ctx.last_stepdepth()
    print("5000 cells angular, room96: %s" % sd)
    assert sd["mode"] == "serial" and sd["attempts"] == 1 and sd["overflow"] is None, sd
    _assert_refill_health(sd)
    np.testing.assert_array_equal(_bits(got), _bits(_want_angular("s5000")))
    assert (got >= 0).all()


@pytest.mark.gpu
def test_5000_cells_batched_overflows_to_serial(ctx, maps, monkeypatch):
    name, cells = _selection("s5000")
    got, sd = _metric(ctx, maps, monkeypatch, name, cells, "5000 cells default metric, room96")
    assert sd["mode"] == "batched-overflow-serial" and sd["overflow"] is not None and sd["attempts"] == 1, sd
    assert sd["refills"] > 0, sd
    _check_metric(ctx, maps, monkeypatch, name, cells, got, _want_metric("s5000"))


# ---------------------------------------------------------------- GPU: visual step depth from the same selections
@pytest.mark.gpu
@pytest.mark.parametrize("sel", ["s33", "s2049", "s5000", "block"])
def test_visual_step_depth_from_selection(ctx, maps, monkeypatch, sel):
    """More than 32 seeds: the tile search in seed mode (one workgroup) and the top-down search."""
    name, cells = _selection(sel)
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    g = maps(name)[1]
    c = np.array(cells, dtype=np.int32)
    got = g.visual_step_depth(cells=c)
    st = ctx.last_stats()
    assert st["vga_kernel"] == "tile-resolved" and (st["vga_sources"], st["vga_launch"]) == (1, 1), st
    monkeypatch.setenv("DMX_VSD_TOPDOWN", "1")
    topdown = g.visual_step_depth(cells=c)
    want = _want_visual(sel)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    np.testing.assert_array_equal(_bits(topdown), _bits(want))
    assert (want == 0).sum() == len(cells) and want.max() >= 1
