"""GPU (run with -m gpu on an MI355X): solve! for groups of same-pattern sparse conic QPs in lockstep — SparseKKTGroup.attach_qp / initialize / solve / get / trace and
SparseConicQPGroup (csrc/sparse_solve_group.hip) — held, member by member, against a single SparseKKT on the same data BIT FOR BIT (status, counts, scalars, every
trace row, the point) and against the CPU oracle with the tolerances of tests/test_gpu_sparse_solve.py (accepted iterates 1e-8 relative, counts exact).  The members
are those of tests/sparse_solve_group_cases.py, which tests/test_sparse_solve_group_inputs_cpu.py pins with the oracle alone.  Single handles and oracle solves are
computed once per module and left unchanged."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")      # (one HIP runtime per process: torch first, then the library)

import sparse_kkt_cases as kc
import sparse_solve_cases as sc
import sparse_solve_group_cases as gc
from helpers import load_pkg

pytestmark = pytest.mark.gpu

TRACE_ROWS = 32
COUNTS = ("total_iterations", "outer_iterations", "accepted_iterates", "factorizations", "max_refinement_rounds", "refinement_failures", "worst_warning", "host_waits",
          "line_search_trials")                                            # info[0:9]
SCALARS = ("central_path", "penalty", "primal_regularization_last")       # info[9:12]


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()) if np.asarray(b).size else 0.0


def frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def problems(oracle_mod):
    cache = {}

    def get(shape, pid):
        if (shape, pid) not in cache:
            cache[(shape, pid)] = sc.problem(oracle_mod.splitmix_uniform, shape, pid)
        return cache[(shape, pid)]
    return get


@pytest.fixture(scope="module")
def oracles(oracle_mod, problems):
    """the oracle's whole solves from x0 = 0 with the default options"""
    cache = {}

    def get(shape, pid):
        if (shape, pid) not in cache:
            cache[(shape, pid)] = frozen(sc.oracle_solve(oracle_mod, problems(shape, pid)))
        return cache[(shape, pid)]
    return get


@pytest.fixture(scope="module")
def singles(problems):
    """a single SparseKKT's whole solve: dict(status, info, trace, solution, dual), by (shape, pid, options, start)"""
    cache = {}

    def get(shape, pid, options=(), start=None):
        key = (shape, pid, tuple(options), None if start is None else start.tobytes())
        if key not in cache:
            prob = problems(shape, pid)
            q, dims = kc.cone_layout(prob)
            Lxx, gx, hx = kc.sparse_inputs(prob)
            s = load_pkg().SparseKKT(Lxx, gx, hx, n_nonnegative=q, second_order_dims=dims, options=dict(options))
            s.set_values(Lxx, gx, hx)
            s.attach_qp(prob.q, prob.b, prob.h)
            s.keep_trace(TRACE_ROWS)
            if start is None:
                s.initialize(np.zeros(prob.nx))
            else:
                s.set("solution", start)
            status, info = s.solve()
            cache[key] = frozen(dict(status=status, info=info, trace=s.trace().copy(), solution=s.get("solution"), dual=s.get("dual")))
        return cache[key]
    return get


def make_group(problems, shape, pids, options=None):
    probs = [problems(shape, p) for p in pids]
    q, dims = kc.cone_layout(probs[0])
    g = load_pkg().SparseConicQPGroup([(p.Psym, p.q, p.A, p.b, p.G, p.h) for p in probs], n_nonnegative=q, second_order_dims=dims, options=options)
    g.keep_trace(TRACE_ROWS)
    return g, probs


def cold_solve(g, probs):
    g.initialize(np.zeros((len(probs), probs[0].nx)))
    return g.solve()


def assert_member_is_its_single_handle(g, m, statuses, infos, one):
    """bit for bit: status, info[0:9], the final scalars, every trace row, the point and the dual"""
    assert statuses[m] == one["status"] == infos[m]["status"], (m, statuses[m], one["status"])
    assert [infos[m][k] for k in COUNTS] == [one["info"][k] for k in COUNTS], (m, infos[m], one["info"])
    assert [infos[m][k] for k in SCALARS] == [one["info"][k] for k in SCALARS], (m, infos[m], one["info"])
    tr = g.trace(m)
    assert tr.shape == one["trace"].shape, (m, tr.shape, one["trace"].shape)
    for r in range(tr.shape[0]):
        assert np.array_equal(tr[r], one["trace"][r]), (m, r, np.abs(tr[r] - one["trace"][r]).max())
    assert np.array_equal(g.get("solution", m), one["solution"]) and np.array_equal(g.get("dual", m), one["dual"]), m


def assert_member_is_the_oracles(g, m, statuses, infos, ref):
    """as test_gpu_sparse_solve.check_whole_solve: counts exact, accepted iterates within 1e-8"""
    assert statuses[m] == ref["status"] == 1
    assert (infos[m]["total_iterations"], infos[m]["outer_iterations"], infos[m]["accepted_iterates"]) == (ref["total_iterations"], ref["outer"], ref["accepted"])
    tr = g.trace(m)
    assert tr.shape == ref["trace"].shape
    for r in range(tr.shape[0]):
        assert rel(tr[r], ref["trace"][r]) <= 1e-8, (m, r, rel(tr[r], ref["trace"][r]))
    assert rel(g.get("solution", m), ref["w"]) <= 1e-8 and rel(g.get("dual", m), ref["dual"]) <= 1e-8
    assert abs(infos[m]["central_path"] - ref["kappa"]) <= 1e-15 and abs(infos[m]["penalty"] - ref["rho"]) <= 1e-9
    assert infos[m]["refinement_failures"] == 0


# ---- 1. a group of solving members ---------------------------------------------------------------------------------------------------------------------------------
def test_small_group_of_solving_members(problems, singles, oracles):
    shape, pids = gc.GROUP_SMALL_SOLVED
    g, probs = make_group(problems, shape, pids)
    statuses, infos, report = cold_solve(g, probs)
    print("report", report)
    assert g.status == 1 and statuses == [1] * len(pids)
    for m, pid in enumerate(pids):
        assert_member_is_its_single_handle(g, m, statuses, infos, singles(shape, pid))
        assert_member_is_the_oracles(g, m, statuses, infos, oracles(shape, pid))
        assert infos[m]["accepted_iterates"] == gc.SOLVED[shape][pid]


# ---- 2. a member whose refinement fails does not disturb the others -------------------------------------------------------------------------------------------------
def check_group_with_a_failing_member(problems, singles, oracles, shape, pids, failing):
    g, probs = make_group(problems, shape, pids)
    statuses, infos, report = cold_solve(g, probs)
    print("default:", statuses, report)
    rows = gc.FAILING[shape][failing]
    m = pids.index(failing)
    assert g.status == -102 and statuses[m] == -102 and "no `H \\ residual` fallback" in g._error_text()
    ref = oracles(shape, failing)
    assert ref["first_lu_fallback_row"] == rows
    tr = g.trace(m)
    assert tr.shape[0] == rows == infos[m]["accepted_iterates"] and infos[m]["refinement_failures"] == 1
    for r in range(rows):
        assert rel(tr[r], ref["trace"][r]) <= 1e-8
    assert np.array_equal(g.get("solution", m), tr[rows - 1])                  # the point is the last accepted iterate
    assert_member_is_its_single_handle(g, m, statuses, infos, singles(shape, failing))
    for k, pid in enumerate(pids):
        if pid != failing:
            assert_member_is_its_single_handle(g, k, statuses, infos, singles(shape, pid))
            assert_member_is_the_oracles(g, k, statuses, infos, oracles(shape, pid))
    # ... and past the failure when told to: every member is its single handle's with the same option (the oracle is not the yardstick there)
    option = dict(continue_after_refinement_failure=1)
    c, probs = make_group(problems, shape, pids, options=option)
    statuses, infos, report = cold_solve(c, probs)
    print("continue_after_refinement_failure:", statuses, report)
    assert infos[m]["refinement_failures"] >= 1 and statuses[m] in (0, 1)
    for k, pid in enumerate(pids):
        assert_member_is_its_single_handle(c, k, statuses, infos, singles(shape, pid, options=tuple(option.items())))


def test_small_group_with_a_failing_member(problems, singles, oracles):
    shape, pids = gc.GROUP_SMALL_WITH_FAILURE
    check_group_with_a_failing_member(problems, singles, oracles, shape, pids, failing=0)


# ---- 3. several tree levels, cone rows across workgroups, members that leave at different ticks -------------------------------------------------------------------
def test_tree_group(problems, singles, oracles):
    shape, pids = gc.GROUP_TREE
    g, probs = make_group(problems, shape, pids)
    statuses, infos, report = cold_solve(g, probs)
    print("report", report)
    assert statuses == [1] * len(pids)
    for m, pid in enumerate(pids):
        assert_member_is_its_single_handle(g, m, statuses, infos, singles(shape, pid))
        assert_member_is_the_oracles(g, m, statuses, infos, oracles(shape, pid))
        assert infos[m]["outer_iterations"] == gc.TREE_OUTER[pid]
    assert len(set(infos[m]["accepted_iterates"] for m in range(len(pids)))) > 1


# ---- 4. a wavefront per cone in group form ------------------------------------------------------------------------------------------------------------------------
def test_wide_cone_group(problems, singles, oracles):
    shape, pids = gc.GROUP_WIDE
    check_group_with_a_failing_member(problems, singles, oracles, shape, pids, failing=0)


# ---- 5. the largest group -------------------------------------------------------------------------------------------------------------------------------------------
def test_group_of_128(problems, singles, oracles):
    shape, pids = gc.GROUP_LIMIT
    g, probs = make_group(problems, shape, pids)
    statuses, infos, report = cold_solve(g, probs)
    print("report", report)
    assert statuses == [1] * 128
    for m, pid in enumerate(pids):
        assert_member_is_its_single_handle(g, m, statuses, infos, singles(shape, pid))
    for m in (0, 61, 127):
        assert_member_is_the_oracles(g, m, statuses, infos, oracles(shape, pids[m]))


# ---- 6. a member's result does not depend on its place or the group's size; waits and launches do not grow with identical members ------------------------------------
def test_place_and_size_independence(problems, singles):
    shape, pid = gc.SMALL, gc.PLACES_PID
    one = singles(shape, pid)
    reports = {}
    for name, pids, place in (("alone", [pid], 0), ("first of 3", [pid, 5, 7], 0), ("last of 3", [4, 6, pid], 2), ("8 identical", [pid] * 8, 5)):
        g, probs = make_group(problems, shape, pids)
        statuses, infos, reports[name] = cold_solve(g, probs)
        assert_member_is_its_single_handle(g, place, statuses, infos, one)
        print(name, reports[name])
    for k in ("solve_launches", "solve_host_waits", "ticks"):
        assert reports["8 identical"][k] == reports["alone"][k], k
    # the mixed group of test 1: its host waits are at least those of its slowest member alone and less than the sum
    shape, pids = gc.GROUP_SMALL_SOLVED
    g, probs = make_group(problems, shape, pids)
    _, _, mixed = cold_solve(g, probs)
    alone = []
    for p in pids:
        g, probs = make_group(problems, shape, [p])
        alone.append(cold_solve(g, probs)[2]["solve_host_waits"])
    print("host waits: mixed", mixed["solve_host_waits"], "alone", alone)
    assert max(alone) <= mixed["solve_host_waits"] < sum(alone)


# ---- 7. a member that takes a line-search trial in a step where its neighbours take none ----------------------------------------------------------------------------
def test_member_with_an_extra_line_search_trial(problems, singles):
    shape, pids, who, options = gc.LINE_SEARCH_GROUP
    g, probs = make_group(problems, shape, pids, options=options)
    statuses, infos, report = cold_solve(g, probs)
    print(statuses, [i["line_search_trials"] for i in infos], report)
    for m, pid in enumerate(pids):
        assert_member_is_its_single_handle(g, m, statuses, infos, singles(shape, pid, options=tuple(options.items())))
    trials = [i["line_search_trials"] for i in infos]
    assert trials[pids.index(who)] > 0 and min(trials) == 0 and report["line_search_trial_rounds"] == max(trials)


# ---- 8. solve again; warm start --------------------------------------------------------------------------------------------------------------------------------------
def test_solve_twice_and_warm_start(problems, singles):
    shape, pids = gc.SMALL, [1, 2, 3]
    g, probs = make_group(problems, shape, pids)
    statuses, infos, _ = cold_solve(g, probs)
    first = [g.trace(m).copy() for m in range(3)]
    points = np.stack([g.get("solution", m) for m in range(3)])
    again, infos2, _ = cold_solve(g, probs)
    assert again == statuses
    for m in range(3):
        assert np.array_equal(g.trace(m), first[m]) and np.array_equal(g.get("solution", m), points[m])
        assert [infos2[m][k] for k in COUNTS + SCALARS] == [infos[m][k] for k in COUNTS + SCALARS]
    g.set_option("warmstart", 1)
    statuses, infos, _ = g.solve()                                          # from the solved points
    for m, pid in enumerate(pids):
        assert_member_is_its_single_handle(g, m, statuses, infos, singles(shape, pid, options=(("warmstart", 1),), start=points[m]))
    sol = g.solution_device()
    assert sol.is_cuda and sol.shape == (3, g.N) and np.array_equal(sol.cpu().numpy(), np.stack([g.get("solution", m) for m in range(3)]))


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(problems, singles):
    pkg = load_pkg()
    from calipso_jl_amd._lib import lib
    shape, pids = gc.LIMIT, [0, 1]
    probs = [problems(shape, p) for p in pids]
    q, dims = kc.cone_layout(probs[0])
    mats = [kc.sparse_inputs(p) for p in probs]
    g = pkg.SparseKKTGroup(mats[0][0], mats[0][1], mats[0][2], 2, n_nonnegative=q, second_order_dims=dims)

    def refused(call, *texts):
        with pytest.raises(pkg.CalipsoHipError) as e:
            call()
        assert "(-4)" in str(e.value) and all(t in str(e.value) for t in texts), str(e.value)

    refused(g.solve, "calipso_hip_sparse_kkt_group_solve: no Lxx resident")
    g.set_values([m[0] for m in mats], [m[1] for m in mats], [m[2] for m in mats])
    refused(g.solve, "calipso_hip_sparse_kkt_group_solve: no q, b, hvec resident (calipso_hip_sparse_kkt_group_qp_attach first)")
    refused(lambda: g.initialize(np.zeros((2, probs[0].nx))), "calipso_hip_sparse_kkt_group_initialize: no q, b, hvec resident")
    L = lib()
    assert L.calipso_hip_sparse_kkt_group_qp_attach(g._h, None, None, None, None) == -4 and "calipso_hip_sparse_kkt_group_qp_attach: q is NULL" in g._error_text()
    g.attach_qp([p.q for p in probs], [p.b for p in probs], [p.h for p in probs])
    refused(g.solve, "calipso_hip_sparse_kkt_group_solve: no point resident")
    assert L.calipso_hip_sparse_kkt_group_initialize(g._h, None) == -4 and "x0 is NULL" in g._error_text()
    assert L.calipso_hip_sparse_kkt_group_solve(g._h, None, None, None) == -4 and "status is NULL" in g._error_text()
    refused(lambda: g.get("solution", 2), "calipso_hip_sparse_kkt_group_get: member: 2 is not in 0 .. 1")
    refused(lambda: g.get("solution", -1), "member: -1 is not in 0 .. 1")
    refused(lambda: g.get("differentiate_slacks", 0), "no resident vector of a group member called differentiate_slacks")
    g.keep_trace(4)
    refused(lambda: g.trace(2), "calipso_hip_sparse_kkt_group_trace: member: 2 is not in 0 .. 1")
    refused(lambda: g.keep_trace(0), "calipso_hip_sparse_kkt_group_keep_trace: rows")
    refused(lambda: g.set_option("krylov_fallback", 1), "not built for groups")
    refused(lambda: g.set_option("no_such_option", 1.0), "unknown option")
    refused(lambda: g.initialize(torch.zeros(2, probs[0].nx, dtype=torch.float64)), "calipso_hip_sparse_kkt_group_initialize_device: x0 is not device memory")
    other = problems(gc.SMALL, 1)
    with pytest.raises(pkg.CalipsoHipError) as e:
        pkg.SparseConicQPGroup([(p.Psym, p.q, p.A, p.b, p.G, p.h) for p in probs + [other]], n_nonnegative=q, second_order_dims=dims)
    assert "member 2" in str(e.value) and "pattern" in str(e.value)
    # ... and the group works afterwards
    g.keep_trace(TRACE_ROWS)
    statuses, infos, _ = cold_solve(g, probs)
    for m, pid in enumerate(pids):
        assert_member_is_its_single_handle(g, m, statuses, infos, singles(shape, pid))
