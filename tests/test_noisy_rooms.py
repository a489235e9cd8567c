"""Preconditions of the inexact-coordinate makeGraph tests (tests/test_gpu_longsight.py), on the CPU oracle.

whichbin (pointdata.h:432-520) bins a visible cell by depixelate(cell) - centre, and depixelate is
bottom_left + spacing * index with every sum rounded.  Where those sums are inexact a diagonal cell's
|gy| / |gx| can fall below 1 - 1e-12, and the cell goes to the sector bin next to the diagonal bin.  The rooms
of gen_synthetic.NOISY_ROOMS are there to reach that case: each must hold fewer pairs in the diagonal bins
4 / 12 / 20 / 28 than the same layout with unit coordinates, over the same visible set -- otherwise the GPU
tests on them would say nothing about it.
"""
import numpy as np
import pytest

from golden.gen_synthetic import NOISY_ROOMS, make_noisy_room
from golden_io import case_input_lines, load_case
from pyoracle import OracleMap

DIAG_BINS = [4, 12, 20, 28]


def _graph(origin, spacing, n, seed):
    region, lines, fill = make_noisy_room(origin, spacing, n, seed)
    om = OracleMap(region, spacing, lines)
    assert om.fill(*fill)
    om.make_graph(threads=8)
    return om, om.graph()


@pytest.mark.parametrize("name", sorted(NOISY_ROOMS))
def test_noisy_room_moves_diagonal_cells_out_of_the_diagonal_bins(name):
    origin, spacing, n, seed = NOISY_ROOMS[name]
    om, g = _graph(origin, spacing, n, seed)
    om1, g1 = _graph((0.0, 0.0), 1.0, n, seed)
    assert (om.cols, om.rows, om.num_nodes) == (om1.cols, om1.rows, om1.num_nodes) == (n, n, n * n)
    np.testing.assert_array_equal(om.state(), om1.state())
    # the same visible pairs (bin counts: column 1 of the bin records) ...
    assert int(g["bins"][:, :, 1].sum()) == int(g1["bins"][:, :, 1].sum()) > 0
    np.testing.assert_array_equal(g["attrs"][:, 0], g1["attrs"][:, 0])
    # ... fewer of them in the diagonal bins
    noisy, unit = int(g["bins"][:, DIAG_BINS, 1].sum()), int(g1["bins"][:, DIAG_BINS, 1].sum())
    print("%s: %d visible pairs, diagonal bins %d (unit coordinates: %d), runs %d (%d)" %
          (name, int(g["bins"][:, :, 1].sum()), noisy, unit, len(g["runs"]), len(g1["runs"])))
    assert noisy < unit
    assert not np.array_equal(g["bins"], g1["bins"])


def test_os07_fixture_is_the_generated_room():
    """The committed reference fixture (tests/golden/make_golden.py os07) was made from this generator's room."""
    meta, A = load_case("os07")
    origin, spacing, n, seed = NOISY_ROOMS["os07"]
    region, lines, fill = make_noisy_room(origin, spacing, n, seed)
    np.testing.assert_array_equal(case_input_lines(meta), lines)
    assert meta["region"] == region and meta["spacing"] == spacing and meta["fills"] == [list(fill)]
    assert (meta["cols"], meta["rows"], meta["nodes"]) == (n, n, n * n)
    assert int(A["bins"][:, DIAG_BINS, 1].sum()) < int(A["bins"][:, :, 1].sum())
