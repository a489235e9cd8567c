"""makeGraph's spans along the outer wall: the depth-lane recurrence (depthmapx_amd/csrc/kernels/span.hpp
wall_merge_ok / wall_visit_ok) against the sieve walked one depth at a time.

Along a closed side the outermost cell line holds one border piece a cell.  Each depth's last gap visits the wall
cell of its depth, whose block trims that gap's end: e_d = min(e_{d-1}, kx_d).  The kernel replays a span of such
depths with a depth a lane (a prefix minimum) and checks, per depth, that the sequential walk takes exactly that
branch.  tests/span/wall_check.cpp compiles span.hpp on the host (g++, -ffp-contract=off, as the kernel) and
compares the recurrence -- e_d, the cells examined per depth, the last gap's visible rows, the depth at which it is
cut -- with a restatement of PointMap::sieve2's visit ranges and sparkSieve2::collectgarbage, for walls at rows 1, 2,
7, 63, 64, 65 and 300, entry depths B .. 4B, pieces through the cell centres, off them and slanted, a wall that
ends, and a piece that ends inside its cell (the next piece then starts inside its cell, and the walk creates a gap
instead of trimming one).  The GPU side is tests/test_gpu_wallspan.py.
"""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_wall_recurrence_equals_the_sequential_walk(tmp_path):
    exe = str(tmp_path / "wall_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off",
                           os.path.join(HERE, "span", "wall_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    m = re.search(r"wall depths checked (\d+), cuts (\d+), mismatches 0", out.stdout)
    assert m, out.stdout
    # the cases reach long replays (several 64-depth batches) and cuts
    assert int(m.group(1)) > 10000 and int(m.group(2)) > 100
