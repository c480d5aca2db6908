"""GPU: the `H \\ residual` fallback (search_direction.jl:22,106-119; csrc/fallback.hip) where it is actually taken — the pivoted LU at the edges of its
panels against a refined reference, a whole Newton step of one handle whose refinement fails (under every schedule of the step), group members that fall
back next to members that do not, structured handles, and whole solves whose fallback counts are the oracle's.  Every input is pinned on the CPU by
tests/test_fallback_inputs_cpu.py: the oracle decides clearly on it.  Figures measured on an MI355X: profiles/fallback_paths_tests.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest

import problems as pr
from helpers import (CONE_SEARCH_LIMIT, LU_EDGE_SHAPES, MIXED_GROUPS, NAN_GROUP, SINGLE_HANDLE, SOLVE_GROUPS, SOLVES, STRUCTURED_ID, STRUCTURED_SHAPE, cone_search_halvings, load_pkg, lu_edge_case,
                     lu_strided_case, make_pair, oracle_cold_solve, oracle_newton_state, refined_solve, staged_step_case, synthetic_step_case)
from test_gpu_group import build, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, float(np.abs(np.asarray(b)).max())))


# ---- 1. the LU against a refined reference ---------------------------------------------------------------------------------------------------------------------
# e_gpu <= C_LU * max(e_lapack, N 2^-53): the device's LU and LAPACK's are both partially pivoted with the same tie rule (first largest) and differ in the summation
# order of the trailing update only.  The largest ratio measured over the cases below was 0.45 (profiles/fallback_paths_tests.txt); C_LU is the smallest power of ten
# with at least 10x headroom over it.
C_LU = 10.0


def lu_system(oracle_mod, prob, pt, lam):
    o, g = make_pair(oracle_mod, prob, pt, lam, ep=0.0, ed=0.0)
    o.cone(product=True, jacobian=True, target=True, barrier=True, barrier_gradient=True)
    g.cone(product=True, jacobian=True, target=True, barrier=True, barrier_gradient=True)
    o.residual(); g.residual()
    o.residual_jacobian_variables()
    return g, o.H_dense(), np.array(o.buf("residual"))


def check_lu(tag, g, H, R):
    N = H.shape[0]
    x, x_lapack = refined_solve(H, R)
    before = g.stats()["fallbacks"]
    assert g.search_direction_nonsymmetric() == 0
    step = g.data("step").all.copy()
    assert g.stats()["fallbacks"] == before + 1
    scale = max(1.0, float(np.abs(x).max()))
    e_gpu = float(np.abs(step.astype(np.longdouble) - x).max() / scale)
    e_lapack = float(np.abs(x_lapack.astype(np.longdouble) - x).max() / scale)
    floor = max(e_lapack, N * 2.0 ** -53)
    print("FBP lu %s N=%d e_gpu=%.3e e_lapack=%.3e ratio=%.2f" % (tag, N, e_gpu, e_lapack, e_gpu / floor))
    assert e_gpu <= 1e-9
    assert np.abs(H @ step - R).max() <= 1e-9 * max(1.0, np.abs(R).max())
    assert e_gpu <= C_LU * floor
    # Hdense and lu_ipiv are reused by the next call on the handle: same bits
    assert g.search_direction_nonsymmetric() == 0
    assert same(g.data("step").all, step) and g.stats()["fallbacks"] == before + 2


@pytest.mark.parametrize("N", sorted(LU_EDGE_SHAPES))
def test_lu_at_the_edges_of_its_panels(oracle_mod, N):
    """a single partial panel (N < 32), N round the panel width 32 and the 64-wide tiles of the trailing GEMM, a multiple of 32, panels of more than 1024 rows"""
    g, H, R = lu_system(oracle_mod, *lu_edge_case(N))
    assert H.shape == (N, N)
    check_lu("edge", g, H, R)


def test_lu_pivot_row_beyond_the_first_stride_of_the_panel_kernel(oracle_mod):
    """the pivot of column 5 of the first panel sits at row 1050: k_lu_panel's 1024 threads reach it in the second trip of their row loops only"""
    g, H, R = lu_system(oracle_mod, *lu_strided_case())
    check_lu("strided", g, H, R)


def test_lu_reports_a_singular_matrix_and_comes_back():
    pkg = load_pkg()
    prob = pr.ConicQP(np.zeros((2, 2)), np.ones(2), np.zeros((0, 2)), np.zeros(0), np.zeros((0, 2)), np.zeros(0), nonnegative_indices=[], second_order_indices=[[]])
    s = pkg.Solver(prob, 2, 0, 0, 0, nonnegative_indices=[], second_order_indices=[[]])
    for name, v in (("central_path", 0.17), ("penalty", 52.0), ("primal_regularization", 0.0), ("dual_regularization", 0.0), ("fraction_to_boundary", 0.99)):
        s.set(name, [v])
    s.set("solution", np.array([0.3, -0.4]))
    s.evaluate(pr.ALL_VARIABLE_FLAGS, 0)
    s.residual()
    assert s.search_direction_nonsymmetric() == 1                      # CALIPSO_WARN_ZERO_PIVOT
    assert s.stats()["fallbacks"] == 1


# ---- 2. one handle, whole Newton step --------------------------------------------------------------------------------------------------------------------------
def place(pkg, s, w):
    """move a handle of test_gpu_group.build() to the point w (what build() itself does after setting its point)"""
    s.set("solution", w)
    fl = pkg.FLAGS
    s.qp_evaluate(fl["objective"] | fl["equality_constraint"] | fl["cone_constraint"], 0)
    s.cone(product=True, target=True)
    s.synchronize()


def handle(pkg, pid, shape, boundary):
    s = build(pkg, pid, shape)
    s.set_option("max_cone_line_search", CONE_SEARCH_LIMIT)          # (helpers.py: the cone search of a fallback step at these points needs more than the default 25 halvings)
    if boundary:
        place(pkg, s, synthetic_step_case(pkg.splitmix_uniform, pid, shape, True)[1])
    return s


def oracle_step(oracle_mod, pkg, pid, shape):
    """(oracle after search_direction! at the boundary point of the case, its step, the cone step sizes of the halving loop on that step)"""
    prob, w, lam = synthetic_step_case(pkg.splitmix_uniform, pid, shape, True)
    o = oracle_newton_state(oracle_mod, prob, w, lam)
    assert o.search_direction() == 2
    return o, np.array(o.buf("step")), [a for a, _ in cone_search_halvings(o, w)]


@pytest.mark.parametrize("shape,pid", SINGLE_HANDLE)
def test_newton_step_whose_refinement_fails_takes_the_oracles_step(oracle_mod, shape, pid):
    pkg = load_pkg()
    s = handle(pkg, pid, shape, True)
    o, so, (a_s, a_t) = oracle_step(oracle_mod, pkg, pid, shape)
    st0 = s.stats()
    info = s.newton_step(advance=False)
    st1 = s.stats()
    assert info["status"] == 2
    assert st1["fallbacks"] == st0["fallbacks"] + 1 and st1["refinement_failures"] == st0["refinement_failures"] + 1
    assert info["refinement_rounds"] == o.stats()["last_refinement_rounds"]
    step = s.data("step").all.copy()
    print("FBP step %s pid=%d err=%.3e" % (shape, pid, rel(step, so)))
    assert rel(step, so) <= 1e-8
    # the step sizes are those of the step the fallback left, not of the discarded one: the cone search's halving loop on the oracle's step; the residual line search
    # then only halves further
    assert info["step_size_cone_slack_dual"] == a_t
    halvings = np.log2(a_s / info["step_size"])
    assert halvings >= 0 and halvings == np.round(halvings)
    R = s.data("residual").all
    assert np.abs(s.jacobian_variables_mul(step) - R).max() <= 1e-8 * max(1.0, np.abs(R).max())
    moved = s.newton_step(advance=True)
    st2 = s.stats()
    assert moved == info
    assert st2["fallbacks"] == st1["fallbacks"] + 1 and st2["refinement_failures"] == st1["refinement_failures"] + 1
    assert same(s.data("step").all, step)


CHILD = r'''
import hashlib, os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
from helpers import SINGLE_HANDLE, load_pkg, synthetic_step_case
from test_gpu_fallback_paths import handle, place
pkg = load_pkg()
out, status = [], []
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
for shape, pid in SINGLE_HANDLE:
    s = handle(pkg, pid, shape, True)
    first = len(status)
    for it in range(4):
        if it == 3:                                   # from the interior point of the case: a step that takes no fallback
            place(pkg, s, synthetic_step_case(pkg.splitmix_uniform, pid, shape, False)[1])
        info = s.newton_step(advance=True)
        assert info["status"] >= 0, info
        status.append(info["status"])
        out += [sha(s.data("step").all), sha(s.solution.all), repr(sorted(info.items()))]
    assert status[first] == 2 and status[-1] == 0, status
    out.append(repr(sorted(s.stats().items())))
print("STATUS " + " ".join(str(v) for v in status))
print("DIGEST " + hashlib.sha256("\n".join(out).encode()).hexdigest())
'''

VARIANTS = [{}, {"CALIPSO_HIP_SPEC_STEP": "0"}, {"CALIPSO_HIP_SPEC_REFINE": "0"}, {"CALIPSO_HIP_SPEC_STEP": "0", "CALIPSO_HIP_SPEC_REFINE": "0"}, {"CALIPSO_HIP_LFAC": "0"}]


def run_variant(env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (env, r.stderr[-2000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("DIGEST ")]
    assert len(lines) == 1, r.stdout[-2000:]
    return lines[0], [l for l in r.stdout.splitlines() if l.startswith("STATUS ")][0]


def test_fallback_steps_do_not_depend_on_the_schedule_of_the_step():
    """By default the cone search, the first candidate and its merit are queued behind the unread refinement report; when the fallback then replaces the step they are
    thrown away and repeated (search_direction_finish: step_changed).  With CALIPSO_HIP_SPEC_STEP=0 / CALIPSO_HIP_SPEC_REFINE=0 nothing is queued ahead.  The switches are
    read once per process: one child each, three steps in a row from a point that falls back and one from a point that does not — steps, iterates, infos and
    counters agree bit for bit."""
    ref, status = run_variant(VARIANTS[0])
    print("FBP schedule default %s" % status)
    for env in VARIANTS[1:]:
        got, st = run_variant(env)
        print("FBP schedule %s equal=%s %s" % (env, got == ref, st))
        assert got == ref and st == status, env


# ---- 3. groups -------------------------------------------------------------------------------------------------------------------------------------------------
def raw_step(s, advance):
    """newton_step that reports a failing member's status instead of raising (a group does the same per member)"""
    import ctypes as C
    info = np.zeros(6)
    rc = s._L.calipso_hip_newton_step(s._h, int(advance), info.ctypes.data_as(C.POINTER(C.c_double)))
    return int(rc), info


def compare_member(single, member):
    for name in ("step", "residual"):
        assert same(single.data(name).all, member.data(name).all), name
    assert same(single.solution.all, member.solution.all)
    assert single.stats() == member.stats()


@pytest.mark.parametrize("case", range(len(MIXED_GROUPS)))
def test_group_members_that_fall_back_next_to_members_that_do_not(oracle_mod, case):
    """the fallback of one member runs on that member's own stream while the others go on refining (group.hip: gb_refinement): every member gets the bits of its
    stand-alone step"""
    pkg = load_pkg()
    shape, members_of = MIXED_GROUPS[case]
    singles = [handle(pkg, pid, shape, b) for pid, b in members_of]
    members = [handle(pkg, pid, shape, b) for pid, b in members_of]
    g = pkg.Group(members)
    for call in range(2):
        ref = [s.newton_step(advance=False) for s in singles]
        got = g.newton_step(advance=False)
        for (pid, falls), r, q, s, m in zip(members_of, ref, got, singles, members):
            assert r == q, (pid, r, q)
            assert r["status"] == (2 if falls else 0)
            compare_member(s, m)
            assert m.stats()["fallbacks"] == ((call + 1) if falls else 0)
    for (pid, falls), m in zip(members_of, members):
        if falls:
            _, so, _ = oracle_step(oracle_mod, pkg, pid, shape)
            print("FBP group %s pid=%d err=%.3e" % (shape, pid, rel(m.data("step").all, so)))
            assert rel(m.data("step").all, so) <= 1e-8
    for it in range(2):
        ref = [s.newton_step(advance=True) for s in singles]
        got = g.newton_step(advance=True)
        for r, q, s, m in zip(ref, got, singles, members):
            assert r == q and r["status"] >= 0, (it, r, q)
            compare_member(s, m)
    g.close()


@pytest.mark.parametrize("shape,seeds", SOLVE_GROUPS)
def test_group_solve_with_members_that_take_fallbacks(shape, seeds):
    """solve! in lockstep through host callbacks, some members taking the fallback along the way and some never: group == alone, bit for bit"""
    pkg = load_pkg()

    def make(seed):
        prob = pr.parametric_conic_qp(*shape, seed=seed)
        s = pkg.Solver(prob, prob.nx, prob.np, prob.ne, prob.nc, parameters=prob.parameters, nonnegative_indices=prob.nonnegative_indices,
                       second_order_indices=prob.second_order_indices)
        pkg.initialize_b(s, np.zeros(prob.nx))
        return s

    singles = [make(k) for k in seeds]
    members = [make(k) for k in seeds]
    ref = [int(pkg.solve_b(s)) for s in singles]
    grp = pkg.Group(members)
    assert grp.solve() == ref and all(ref)
    counts = [s.stats()["fallbacks"] for s in singles]
    assert counts == [f for sh, k, _, f, _ in SOLVES if sh == shape and k in seeds] and min(counts) == 0 and max(counts) >= 1
    for s, m in zip(singles, members):
        assert s.stats() == m.stats()
        assert same(s.solution.all, m.solution.all)
    grp.close()


def test_group_member_with_a_non_finite_refinement_norm_fails_like_the_single_handle():
    """one member of three has a NaN in q: its residual has one, the norm of its refinement residual is reported as +inf, its refinement fails (rounds reported as
    max_iterative_refinement + 1) and it takes the fallback — in the group exactly as alone; the other two members are untouched"""
    pkg = load_pkg()
    shape, ids = NAN_GROUP

    def make(k, pid):
        s = handle(pkg, pid, shape, False)
        if k == 1:
            prob = synthetic_step_case(pkg.splitmix_uniform, pid, shape, False)[0]
            q = prob.q.copy(); q[0] = np.nan
            s.qp_attach(prob.P, q, prob.A, prob.b, prob.G, prob.h, 0.5)
            place(pkg, s, s.get("solution", s.N))
        return s

    singles = [make(k, pid) for k, pid in enumerate(ids)]
    members = [make(k, pid) for k, pid in enumerate(ids)]
    ref = [raw_step(s, False) for s in singles]
    max_rounds = int(singles[1].get("opt.max_iterative_refinement", 1)[0])
    st = singles[1].stats()
    assert st["refinement_failures"] == 1 and st["fallbacks"] == 1 and st["last_refinement_rounds"] == max_rounds + 1
    g = pkg.Group(members)
    got = g.newton_step(advance=False)
    for k, ((rc, info), q, s, m) in enumerate(zip(ref, got, singles, members)):
        assert rc == q["status"], (k, rc, q)
        assert s.stats() == m.stats()
        if rc >= 0:
            mine = [q[n] for n in ("step_size", "step_size_cone_slack_dual", "refinement_rounds", "factorizations", "merit_candidate", "violation_candidate")]
            assert np.array_equal(info, np.array(mine, dtype=np.float64), equal_nan=True), (k, info, q)
        if k != 1:
            assert rc == 0
            compare_member(s, m)
    g.close()


# ---- 4. structured handles -------------------------------------------------------------------------------------------------------------------------------------
def test_structured_handle_takes_the_fallback_through_dense_temporaries(oracle_mod):
    """a structured handle holds the stage blocks only: nonsymmetric_solve unpacks them to dense temporaries (blocks_unpack_dense) — same bits as its dense twin (the
    dense handle with stage blocks on, whose residual has the structured handle's bits: tests/test_gpu_blocks.py); and a search_direction! at a near-boundary point falls
    back on it like the oracle"""
    from test_gpu_blocks import build as build_dense, build_structured
    pkg = load_pkg()
    _, dense = build_dense(pkg, STRUCTURED_ID, *STRUCTURED_SHAPE, blocks=True)
    _, s = build_structured(pkg, STRUCTURED_ID, *STRUCTURED_SHAPE)
    for h in (dense, s):
        h.residual()
    assert same(s.data("residual").all, dense.data("residual").all)              # (the same right-hand side: what differs below is the LU's input matrix alone)
    for h in (dense, s):
        assert h.search_direction_nonsymmetric() == 0
    step, R = s.data("step").all, s.data("residual").all
    assert same(step, dense.data("step").all) and np.isfinite(step).all() and np.abs(step).max() > 0
    assert np.abs(s.jacobian_variables_mul(step) - R).max() <= 1e-9 * max(1.0, np.abs(R).max())
    assert s.stats()["fallbacks"] == 1
    prob, w, lam = staged_step_case(pkg.splitmix_uniform, STRUCTURED_ID, STRUCTURED_SHAPE, True)
    s.set("solution", w)
    fl = pkg.FLAGS
    s.qp_evaluate(fl["objective"] | fl["equality_constraint"] | fl["cone_constraint"] | fl["objective_gradient_variables"] | fl["equality_dual_jacobian_variables"] |
                  fl["cone_dual_jacobian_variables"], 0)
    s.cone(product=True, target=True, barrier=True, barrier_gradient=True)
    s.residual()
    o = oracle_newton_state(oracle_mod, prob, w, lam)
    assert o.search_direction() == 2
    assert s.search_direction() == 2
    st = s.stats()
    assert st["fallbacks"] == 2 and st["refinement_failures"] == 1
    print("FBP structured err=%.3e" % rel(s.data("step").all, o.buf("step")))
    assert rel(s.data("step").all, o.buf("step")) <= 1e-8


# ---- 5. whole solves -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed,iterations,fallbacks,first_row", SOLVES)
def test_cold_solves_take_the_oracles_fallbacks(oracle_mod, shape, seed, iterations, fallbacks, first_row):
    """cold-started solve! of second-order-cone QPs: the same number of iterations and of fallbacks as the oracle, the same iterates up to and including the first step
    that fell back, the same solution"""
    from test_gpu_solve import criteria
    pkg = load_pkg()
    prob = pr.parametric_conic_qp(*shape, seed=seed)
    s = pkg.Solver(prob, prob.nx, prob.np, prob.ne, prob.nc, parameters=prob.parameters, nonnegative_indices=prob.nonnegative_indices,
                   second_order_indices=prob.second_order_indices)
    rows = []
    s.set_callbacks(inner=lambda sv: rows.append(sv.get("solution", sv.N)))
    pkg.initialize_b(s, np.zeros(prob.nx))
    assert pkg.solve_b(s)
    criteria(s)
    o, status = oracle_cold_solve(oracle_mod, prob, np.zeros(prob.nx))
    assert status == 1 and o.stats()["lu_fallbacks"] == fallbacks
    st = s.stats()
    assert st["fallbacks"] == fallbacks and st["total_iterations"] == iterations
    tr = o.trace()
    if fallbacks:
        upto = first_row + 1
        got, want = np.array(rows[:upto]), tr[:upto]
        assert got.shape == want.shape
        err = float((np.abs(got - want) / np.maximum(1.0, np.abs(want).max(axis=1, keepdims=True))).max())
        print("FBP solve %s seed=%d iterates_err=%.3e" % (shape, seed, err))
        assert err <= 1e-8
    sol = o.point()["all"]
    print("FBP solve %s seed=%d solution_err=%.3e" % (shape, seed, rel(s.get("solution", s.N), sol)))
    assert rel(s.get("solution", s.N), sol) <= 1e-6
