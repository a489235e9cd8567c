"""The agent routine of kernels/agent_step.hpp and the release schedule on the host, against the fixtures made from
the reference itself (tests/golden/agents/, make_golden_agents.py): tests/agents/agents_check.cpp, a stand-alone
program built with g++ -ffp-contract=off, walks every agent of every case on one thread.  Everything is compared
exactly: the schedule's table, the counts, the final cells, the final locations as bit patterns, the stuck flags
and the trails of the first 8 agents.  No fixture may use an escape hatch (an agent flagged at an ambiguous look,
a clamped bin).  A second build with -fsanitize=address,undefined runs one case clean."""
import numpy as np
import pytest

import agents_util as au

CASES = au.cases()


def test_case_table():
    """The set of cases the issue names, and each of the paths it wants exercised somewhere in the set."""
    want = {("kat", 15, 3, 0), ("syn16", 32, 3, 0), ("syn32", 15, 3, 0), ("syn32", 15, 1, 0), ("syn32", 1, 3, 0),
            ("syn32", 15, 3, 3), ("gallery", 15, 3, 0)}
    have = {(c["map"], c["fov"], c["steps"], len(c["release"])) for c in CASES.values()}
    assert have == want
    for c in CASES.values():
        assert (c["nagents"], c["timesteps"], c["lifetime"], c["ntrail"]) == (256, 400, 200, 8)
    for k in ("looks", "fallbacks", "diag_taken", "stopped", "moves"):
        assert any(c[k] > 0 for c in CASES.values()), k
    narrow = [c for c in CASES.values() if c["map"] == "syn32" and c["fov"] == 1]
    assert narrow[0]["fallbacks"] > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_routine_equals_reference(name, tmp_path):
    case = CASES[name]
    got, stats = au.run_host_check(case, str(tmp_path))
    au.assert_same(got, au.load_fixture(name), what=name)
    # a re-run that counts from move k on top of the first k moves' counts (the API's path for a flagged agent)
    assert np.array_equal(got["counts_split"], got["counts"])
    assert stats["flagged"] == 0 and stats["clamps"] == 0
    for k in ("moves", "looks", "fallbacks", "diag_taken", "stopped"):
        assert stats[k] == case[k], k


def test_host_routine_sanitized(tmp_path):
    """AddressSanitizer + UBSan over the same stand-alone program (host code only), one case."""
    name = "syn32_f15_s3_rel"
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    got, stats = au.run_host_check(CASES[name], str(tmp_path), flags=flags)
    au.assert_same(got, au.load_fixture(name), what=name)
    assert stats["flagged"] == 0 and stats["clamps"] == 0
