"""makeGraph's occluder-free spans (depthmapx_amd/csrc/kernels/span.hpp) against the sieve's per-cell rules.

The kernel processes a span of depths row by row: each row's visible depths per gap as one interval, and its
ratio-class boundaries from two evaluations of the per-cell bin decision.  tests/span/span_check.cpp compiles
span.hpp on the host (g++, -ffp-contract=off, as the kernel) and compares, for random gap lists (including
exact quarters and 1/k ends), depth windows and octants, every row's intervals with a cell-by-cell replay of
PointMap::sieve2 (salalib/pointdata.cpp:1512-1565: visit ranges with `firstind`, `centregap`) and every class
boundary with the per-cell bins (whichbin, pointdata.h:432-520).  The GPU side is pinned by the bit-exact
makeGraph tests (tests/test_gpu_parity.py, the whole-map digests in tests/test_gpu_scale.py).
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp):
    exe = str(tmp / "span_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-include", "algorithm",
                           os.path.join(HERE, "span", "span_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def bins_out(tmp_path_factory):
    """`span_check bins` (2 s): the per-cell bin decision alone, see the two tests below."""
    out = subprocess.run([_build(tmp_path_factory.mktemp("span")), "bins"], capture_output=True, text=True)
    print(out.stdout)
    return out


def test_cell_bins_equal_exact_classes_and_fp64_whichbin_off_the_diagonal(bins_out):
    """span.hpp cell_bin (the makeGraph chunk loop's decision, verbatim):
      * unit coordinates, every (depth <= 4096, ind <= depth), 8 octants: the class from exact integer predicates
        (ind = 0 axis, ind = depth diagonal, 3 ind^2 >= depth^2 for tan 30, (2 depth - ind)^2 <= 3 depth^2 for tan 15);
      * inexact coordinates (the rooms os07 and neg01 of gen_synthetic.py, (5.3e5, 1.8e5) with spacing 0.04, and two
        exact sets), 12 sources over a 1400^2 grid, every in-grid cell: plain FP64 whichbin(depixelate - centre)
        (pointdata.h:432-520) on every cell that is not a diagonal cell;
      * diag_offbin_depths (the host's per-map precheck, dmx_ctx_last_stats mk_diag_inexact) is 0 only where no
        sampled diagonal cell differs, and equals a count over every source of a 48^2 grid."""
    out = bins_out
    assert out.returncode in (0, 2), out.stdout + out.stderr[-2000:]
    assert "exact classes: cells 67158016, mismatches 0" in out.stdout, out.stdout
    assert "noisy off-diagonal mismatches 0" in out.stdout, out.stdout
    assert "precheck mismatches 0" in out.stdout, out.stdout
    assert "unit (bottom-left 0 0, spacing 1): cells 23574246, off-diagonal mismatches 0, diagonal mismatches 0; depths with " \
           "a diagonal cell off its bin: 0 of" in out.stdout, out.stdout


@pytest.mark.xfail(strict=True, reason="known divergence (DESIGN.md section 2, 'Inexact world coordinates'): cell_bin "
                   "gives every diagonal cell the diagonal bin")
def test_cell_bins_equal_fp64_whichbin_on_diagonal_cells(bins_out):
    """The same sample's diagonal cells (ind == depth).  Measured: 29,900 of them differ -- os07 3,030 (116 of 1,399
    depths can differ somewhere on a 1400^2 grid), neg01 60 (2 depths), (5.3e5, 1.8e5, 0.04) 26,810 (1,339 depths); none
    with unit coordinates or with the barnsbury origin and spacing 2.  whichbin sends those cells to the sector bin
    next to the diagonal bin; the kernel does not (it reports the map's count as mk_diag_inexact)."""
    assert "noisy diagonal mismatches 0" in bins_out.stdout, bins_out.stdout


def test_span_rows_and_classes_equal_the_per_cell_sieve(tmp_path):
    exe = _build(tmp_path)
    for seed in (11, 12):
        out = subprocess.run([exe, "400", str(seed)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr[-2000:]
        assert "mismatches 0" in out.stdout, out.stdout
