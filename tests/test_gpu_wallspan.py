"""makeGraph's depth spans along the map's outer wall (makegraph.hip wall mode, span.hpp) on whole small maps.

A drawing with a border line leaves the outermost line of grid cells not FILLED, one piece of the border a cell.
Spans used to stop at that wall; now the clean distances ignore it, a span below the wall ends before the front
reaches it, and a span along it replays the wall cells' blocks a depth a lane.  Every map here is swept from
every filled cell in the modes default, DMX_MK_NOWALL (the behaviour of before), DMX_MK_NOSPAN (cell by cell) and
DMX_MK_SPAN=1 (spans of every length): bins, runs, attribute bits, grid connections, cells examined and visible
pairs must be equal in all four and equal to the CPU oracle's graph.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import depthmapx_amd as dmx

pytestmark = pytest.mark.gpu

MODES = {"default": {}, "nowall": {"DMX_MK_NOWALL": "1"}, "nospan": {"DMX_MK_NOSPAN": "1"},
         "span1": {"DMX_MK_SPAN": "1"}}


def _box(x0, y0, x1, y1):
    return [[x0, y0, x1, y0], [x1, y0, x1, y1], [x1, y1, x0, y1], [x0, y1, x0, y0]]


def _room(w, h, extra=(), top=None):
    """Region [0, w] x [0, h] with unit spacing (cell centres on the integers, the border through the centres of
    the outermost cells) and the border lines; `top` replaces the top wall's line(s)."""
    lines = _box(0.0, 0.0, float(w), float(h))
    if top is not None:
        lines = [lines[0], lines[1], lines[3]] + [list(t) for t in top]
    lines += [list(e) for e in extra]
    return [0.0, 0.0, float(w), float(h)], np.array(lines, dtype=np.float64), 1.0, (5.2, 5.2)


def _offset_room():
    """The border is not on cell centres: the region is the lines' bounding box, the grid's cells stay centred on
    multiples of the spacing, and each outermost cell holds an off-centre piece."""
    lines = np.array(_box(0.3, 0.2, 90.6, 40.7), dtype=np.float64)
    return [0.3, 0.2, 90.6, 40.7], lines, 1.0, (5.2, 5.2)


def _offset_room_07():
    """The same on a 0.7 grid: world coordinates that are not exact in FP64."""
    s = 0.7
    lines = np.round(np.array(_box(0.3 * s, 0.2 * s, 90.6 * s, 40.7 * s), dtype=np.float64), 6)
    region = [float(lines[:, [0, 2]].min()), float(lines[:, [1, 3]].min()), float(lines[:, [0, 2]].max()),
              float(lines[:, [1, 3]].max())]
    return region, lines, s, (5.2 * s, 5.2 * s)


MAPS = {
    # fronts run along a wall for more than 64 depths, on both major axes; every source next to a wall and in
    # the four corners (wall row 1) is in the sweep
    "room150x40": lambda: _room(150, 40),
    "room40x150": lambda: _room(40, 150),
    "offset": _offset_room,
    "offset07": _offset_room_07,
    # an occluder that ends on the top wall: one ring cell holds two pieces
    "touching": lambda: _room(120, 40, extra=[(30.2, 37.6, 31.4, 40.0), (80.3, 0.0, 80.9, 2.7)]),
    # an occluder in the cells next to the wall
    "oneoff": lambda: _room(120, 40, extra=[(50.2, 38.8, 51.3, 39.3), (0.8, 20.2, 1.4, 21.1)]),
    # the top wall has a hole over the cells (70, 40) and (71, 40), which are FILLED: that side is not closed; the
    # wall's pieces end inside the cells (69, 40) and (72, 40)
    "hole": lambda: _room(120, 40, top=[(0.0, 40.0, 69.4, 40.0), (71.6, 40.0, 120.0, 40.0)]),
    # an occluder's shadow keeps the front below the top wall for some depths; it reaches the wall mid-way
    "shadow": lambda: _room(150, 40, extra=[(20.3, 24.2, 20.8, 31.4), (100.2, 8.1, 104.7, 8.6)]),
}


def _set_mode(monkeypatch, mode):
    for env in MODES.values():
        for k in env:
            monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def oracle_graphs():
    """The oracle's graph of each map, computed once on first use and left unchanged."""
    from pyoracle import OracleMap
    cache = {}

    def get(name):
        if name not in cache:
            region, lines, spacing, fill = MAPS[name]()
            om = OracleMap(region, spacing, lines)
            assert om.fill(*fill)
            om.make_graph(threads=16)
            cache[name] = (om.state(), om.graph())
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(MAPS))
def test_wall_spans_equal_every_mode_and_the_oracle(ctx, monkeypatch, oracle_graphs, name):
    state, ref = oracle_graphs(name)
    region, lines, spacing, fill = MAPS[name]()
    pm = dmx.PointMap(region, lines, spacing)
    assert pm.make_points(*fill)
    np.testing.assert_array_equal(pm.state(), state)
    rows, cols = pm.rows, pm.cols
    st2 = state.reshape(cols, rows) & 2
    if name == "hole":
        assert st2[70, rows - 1] and st2[71, rows - 1] and not st2[69, rows - 1] and not st2[72, rows - 1]
    else:   # all four sides are closed
        assert not st2[1:-1, 0].any() and not st2[1:-1, -1].any() and not st2[0, 1:-1].any() and not st2[-1, 1:-1].any()
    stats = {}
    for mode in MODES:
        _set_mode(monkeypatch, mode)
        g = pm.make_graph(ctx)
        st = ctx.last_stats()
        stats[mode] = (st["mk_cells_examined"], st["mk_visible_pairs"])
        got = g.copy(runs=True)
        g.close()
        what = "%s, mode %s" % (name, mode)
        np.testing.assert_array_equal(got["bins"], ref["bins"], err_msg="bins, " + what)
        np.testing.assert_array_equal(got["runs"], ref["runs"], err_msg="runs, " + what)
        np.testing.assert_array_equal(got["attrs"].view(np.uint32), ref["attrs"].view(np.uint32),
                                      err_msg="attributes, " + what)
        np.testing.assert_array_equal(got["gridconn"], ref["gridconn"], err_msg="grid connections, " + what)
    pm.close()
    assert len(set(stats.values())) == 1, "cells examined / visible pairs differ between the modes: %s" % stats
    assert stats["default"][1] == int(ref["attrs"][:, 0].astype(np.int64).sum()) > 0


_VERBOSE_RUN = """
import sys
sys.path[:0] = %r
import numpy as np
import depthmapx_amd as dmx
ctx = dmx.Context(0)
lines = np.array([[0, 0, 150, 0], [150, 0, 150, 40], [150, 40, 0, 40], [0, 40, 0, 0]], dtype=np.float64)
pm = dmx.PointMap([0.0, 0.0, 150.0, 40.0], lines, 1.0)
assert pm.make_points(5.2, 5.2)
pm.make_graph(ctx).close()
"""


def _verbose_span_line(extra_env):
    env = dict(os.environ, DMX_VERBOSE="1", **extra_env)
    for k in ("DMX_MK_NOWALL", "DMX_MK_NOSPAN", "DMX_MK_SPAN"):
        if k not in extra_env:
            env.pop(k, None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _VERBOSE_RUN % ([root],)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    m = re.search(r"makegraph spans: .* (\d+) of (\d+) visible cells \(([0-9.]+)%\); (\d+) wall spans over (\d+) depths",
                  p.stdout + p.stderr)
    assert m, (p.stdout + p.stderr)[-2000:]
    return dict(span_cells=int(m.group(1)), visible=int(m.group(2)), wall_spans=int(m.group(4)),
                wall_depths=int(m.group(5)))


def test_wall_spans_are_taken_and_raise_the_span_share():
    """DMX_VERBOSE's span line on the 150 x 40 room: wall spans are taken, and the spans' share of the visible cells
    is strictly larger than with DMX_MK_NOWALL."""
    new = _verbose_span_line({})
    old = _verbose_span_line({"DMX_MK_NOWALL": "1"})
    print("span cells with the wall spans %d, without %d, of %d visible; %d wall spans over %d depths" %
          (new["span_cells"], old["span_cells"], new["visible"], new["wall_spans"], new["wall_depths"]))
    assert new["visible"] == old["visible"] > 0
    assert new["wall_spans"] > 0 and new["wall_depths"] > 0
    assert old["wall_spans"] == 0
    assert new["span_cells"] > old["span_cells"]
