"""The numpy restatement of VGA through vision (tests/thruvision_model.py) against the reference's own results
(tests/golden/thruvision/, written by tests/golden/make_golden_thruvision.py from the reference library): bit
for bit on the fixture graphs' runs.  The GPU tests use the model on the graphs the engine holds."""
import os

import numpy as np
import pytest

import thruvision_model as tvm
from golden_io import GOLDEN, load_case

TV = os.path.join(GOLDEN, "thruvision")
CORRIDORS = ["corridor256x3", "corridor3x256"]


def fixture_graph(name):
    """cols, rows, state, nruns, runs of a fixture map with its reference runs."""
    if name in CORRIDORS:
        z = np.load(os.path.join(TV, name + ".npz"), allow_pickle=False)
        return int(z["cols"]), int(z["rows"]), z["state"], z["nruns"], z["runs"]
    meta, A = load_case(name)
    return meta["cols"], meta["rows"], A["state"], A["nruns"], A["runs"]


def reference(name):
    return np.load(os.path.join(TV, name + "_thruvision.npy"), allow_pickle=False)


@pytest.mark.parametrize("name", ["kat", "syn16", "syn32"] + CORRIDORS)
def test_model_matches_reference_bit_for_bit(name):
    cols, rows, state, nruns, runs = fixture_graph(name)
    got = tvm.through_vision(cols, rows, state, nruns, runs)
    want = reference(name)
    assert want.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(got.astype(np.float32), want)
    assert (got < 2 ** 24).all()   # the fixture's floats hold these counts exactly
    np.testing.assert_array_equal(got, want.astype(np.int64))


def test_corridor_fixtures_are_256_by_3_filled_cells():
    for name, shape in zip(CORRIDORS, [(256, 3), (3, 256)]):
        cols, rows, state, nruns, runs = fixture_graph(name)
        filled = (state.reshape(cols, rows) & 2) != 0
        xs, ys = np.nonzero(filled)
        assert (xs.max() - xs.min() + 1, ys.max() - ys.min() + 1) == shape and filled.sum() == 768
        assert reference(name).max() > 0


def test_half_way_point_just_below_the_integer_emits_one_pixel():
    """(0,0) -> (6,1): at i = 3 the true y is exactly 1.0, the accumulated FP64 value is 0.9999999999999999, so
    floor gives 0, the 1e-9 test fails and ONE pixel (3, 0) is emitted, not the two of a half-way point."""
    w = tvm.walk((0, 0), (6, 1))
    assert len(w) == 7
    assert w[3] == [(3, 0)]
    assert [len(e) for e in w] == [1] * 7
    # the same slope walked the other way lands on the integer side: two pixels
    assert any(len(e) == 2 for e in tvm.walk((0, 0), (2, 1)))
    assert tvm.walk((0, 0), (2, 1))[1] == [(1, 1), (1, 0)]
    cnt = tvm.line_counts(7, 2, [(6, 1)], [(0, 0)]).reshape(7, 2)
    assert cnt.sum() == 5 and cnt[3, 0] == 1 and cnt[3, 1] == 0


@pytest.mark.parametrize("q", [(5, 5), (5, -5), (-3, 3), (0, 0)])
def test_diagonal_emits_nothing(q):
    p = (7, 7)
    qq = (p[0] + q[0], p[1] + q[1])
    assert tvm.walk(p, qq) == [[p]]
    assert tvm.line_counts(16, 16, [qq], [p]).sum() == 0


def test_major_y_is_symmetric():
    a = tvm.line_counts(8, 8, [(6, 1)], [(0, 0)]).reshape(8, 8)
    b = tvm.line_counts(8, 8, [(1, 6)], [(0, 0)]).reshape(8, 8)
    np.testing.assert_array_equal(a, b.T)
