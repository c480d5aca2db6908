"""The members of tests/sparse_solve_group_cases.py behave as stated there — pinned with the CPU oracle alone, so that tests/test_gpu_sparse_solve_group.py and the
lockstep replay of tests/test_sparse_solve_group_host_cpu.py stand on inputs nobody derived from the code under test.  The oracle's stats() do not count line-search
trials: they are recorded here from the flags of its evaluation callbacks (a run of candidate evaluations is one step's first candidate and its trials)."""
import numpy as np
import pytest

import sparse_kkt_cases as kc
import sparse_solve_group_cases as gc


@pytest.fixture(scope="module")
def solves(oracle_mod):
    """the oracle's cold solves with the default options, once each: (problem, result, line-search trials per accepted step)"""
    cache = {}

    def get(shape, pid):
        if (shape, pid) not in cache:
            cache[(shape, pid)] = gc.oracle_solve_counting(oracle_mod, shape, pid)
        return cache[(shape, pid)]
    return get


@pytest.mark.parametrize("shape", [gc.SMALL, gc.LIMIT, gc.TREE, gc.WIDE], ids=["small", "limit", "tree", "wide"])
def test_the_members_solve_or_fail_as_stated(solves, shape):
    pids = sorted(set(gc.SOLVED[shape]) | set(gc.FAILING.get(shape, {})))
    assert pids == list(range(8))
    for pid in pids:
        prob, ref, trials = solves(shape, pid)
        assert prob.nx + 2 * prob.ne + 3 * prob.nc == gc.SIZES[shape]
        print(shape, pid, "status", ref["status"], "accepted", ref["accepted"], "outer", ref["outer"], "rounds", ref["max_refinement_rounds"], "fallbacks", ref["lu_fallbacks"],
              "first after", ref["first_lu_fallback_row"], "trials", trials)
        assert len(trials) == ref["accepted"] and trials == [0] * ref["accepted"]      # cold, no member takes a line-search trial in any step
        if pid in gc.SOLVED[shape]:
            assert ref["status"] == 1 and ref["lu_fallbacks"] == 0 and ref["accepted"] == gc.SOLVED[shape][pid]
        else:
            rows = gc.FAILING[shape][pid]
            assert ref["lu_fallbacks"] >= 1 and (rows is None or (ref["first_lu_fallback_row"] == rows))
    if shape == gc.SMALL:
        assert solves(shape, 0)[1]["lu_fallbacks"] == 1
    if shape == gc.TREE:
        for pid in gc.TREE_OUTER:
            ref = solves(shape, pid)[1]
            assert ref["outer"] == gc.TREE_OUTER[pid] and ref["max_refinement_rounds"] <= gc.TREE_ROUNDS_AT_MOST[pid]


def test_the_groups_hold_these_members_and_share_one_pattern(oracle_mod, solves):
    for shape, pids in (gc.GROUP_SMALL_SOLVED, gc.GROUP_SMALL_WITH_FAILURE, gc.GROUP_TREE, gc.GROUP_WIDE, gc.GROUP_LIMIT, gc.LINE_SEARCH_GROUP[:2]):
        assert all(p in gc.SOLVED[shape] or p in gc.FAILING.get(shape, {}) for p in pids)
    assert gc.GROUP_SMALL_SOLVED[1] == sorted(gc.SOLVED[gc.SMALL]) and len(gc.GROUP_LIMIT[1]) == 128
    assert [p for p in gc.GROUP_SMALL_WITH_FAILURE[1] if p in gc.FAILING[gc.SMALL]] == [0] and [p for p in gc.GROUP_WIDE[1] if p in gc.FAILING[gc.WIDE]] == [0]
    assert len(set(gc.SOLVED[gc.TREE][p] for p in gc.GROUP_TREE[1])) > 1 and len(set(gc.TREE_OUTER.values())) > 1      # they leave at different ticks
    for shape in (gc.SMALL, gc.LIMIT):
        first = kc.sparse_inputs(solves(shape, 0)[0])
        for pid in range(1, 8):
            for A, B in zip(kc.sparse_inputs(solves(shape, pid)[0]), first):
                assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    other = kc.sparse_inputs(solves(gc.SMALL, 1)[0])[0]
    assert other.shape != kc.sparse_inputs(solves(gc.LIMIT, 0)[0])[0].shape                       # what SparseConicQPGroup refuses: a member of another pattern


def test_line_search_trials_with_the_oracle(oracle_mod, solves):
    """scaling_line_search = 0.9 changes no member's trial count either; the one member the oracle shows with trials; the device group's neighbours take none"""
    for pid in range(8):
        _, ref, trials = gc.oracle_solve_counting(oracle_mod, gc.LIMIT, pid, options=dict(scaling_line_search=0.9))
        assert ref["status"] == 1 and trials == [0] * ref["accepted"]
    case = gc.LINE_SEARCH_ORACLE
    _, warm, trials = gc.oracle_solve_counting(oracle_mod, case["shape"], case["pid"], start=gc.line_search_start(oracle_mod))
    print("warm-started from a perturbed point:", warm["status"], warm["accepted"], warm["lu_fallbacks"], warm["first_lu_fallback_row"], trials)
    assert trials == case["trials"] and warm["first_lu_fallback_row"] == case["first_fallback_row"] and warm["status"] == 1
    shape, pids, who, options = gc.LINE_SEARCH_GROUP
    assert who in gc.FAILING[shape] and options == dict(continue_after_refinement_failure=1)
    for pid in pids:
        if pid != who:
            _, ref, trials = solves(shape, pid)
            assert ref["lu_fallbacks"] == 0 and max(trials) == 0
