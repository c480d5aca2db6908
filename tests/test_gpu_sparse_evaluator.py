"""GPU (run with -m gpu on an MI355X): solve! on the sparse handle for NONLINEAR problems — SparseKKT.set_evaluator / set_parameters / evaluate, the evaluated
instantiation of the solve kernels (csrc/sparse_solve.hip), the sparse route of the generated trajectory evaluators (include/calipso_trajectory.hpp: sparse_eval) and
TrajectoryProblem.sparse_solver — against the host twin TrajectoryProblem.evaluate, against qp_attach on the same handle settings through a hand-written evaluator
(tests/device_eval_sparse), and against the CPU oracle.  Tolerances are the project's own for the same quantities: fields 1e-12 x max(1, |field|max)
(test_gpu_trajectory_codegen.py:63), accepted iterates 1e-8 relative (test_gpu_sparse_solve.py), the final x 1e-6 (test_gpu_trajectory_codegen.py:163), scalars of the
building blocks 1e-12 relative; integers exact."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")      # (one HIP runtime per process: torch first, then the library)

import problems as pr
import sparse_kkt_cases as kc
import sparse_solve_cases as sc
from helpers import ROOT, load_pkg
from test_gpu_trajectory_codegen import tp

pytestmark = pytest.mark.gpu

FULL = (pr.OBJECTIVE | pr.OBJECTIVE_GRADIENT | pr.OBJECTIVE_HESSIAN | pr.EQUALITY | pr.EQUALITY_JACOBIAN | pr.EQUALITY_DUAL_HESSIAN | pr.CONE | pr.CONE_JACOBIAN |
        pr.CONE_DUAL_HESSIAN)          # every variable-side bit the sparse handle asks of its evaluator: the dual gradients it gathers itself
TRACE_ROWS = 64


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()) if np.asarray(b).size else 0.0


def close(a, b, tol):
    return abs(a - b) <= tol * max(1.0, abs(b))


def waits_hold(info):
    return info["host_waits"] == 2 * info["accepted_iterates"] + info["outer_iterations"] + info["line_search_trials"]


# ---- 1. fields on the sparse route -----------------------------------------------------------------------------------------------------------------------------------
def host_fields(TP, w, theta):
    """the host twin at the point: the vectors, and the three matrices as dense arrays"""
    nx, ne, nc = TP.nx, TP.ne, TP.nc
    x, y, z = w[:nx], w[nx + ne + nc:nx + 2 * ne + nc], w[nx + 2 * ne + nc:nx + 2 * ne + 2 * nc]
    sizes = {"objective": 1, "objective_gradient_variables": nx, "equality_constraint": ne, "cone_constraint": nc, "equality_jacobian_variables": ne * nx,
             "cone_jacobian_variables": nc * nx, "objective_jacobian_variables_variables": nx * nx, "equality_dual_jacobian_variables_variables": nx * nx,
             "cone_dual_jacobian_variables_variables": nx * nx}
    out = {}
    TP.evaluate(FULL, x, y, z, theta, lambda name: out.setdefault(name, np.zeros(sizes[name])))
    get = lambda name: out.get(name, np.zeros(sizes[name]))
    H = sum(get(n) for n in ("objective_jacobian_variables_variables", "equality_dual_jacobian_variables_variables", "cone_dual_jacobian_variables_variables"))
    return dict(objective=get("objective"), objective_gradient_variables=get("objective_gradient_variables"), equality_constraint=get("equality_constraint"),
                cone_constraint=get("cone_constraint"), lagrangian_hessian=H.reshape(nx, nx, order="F"),
                equality_jacobian_variables=get("equality_jacobian_variables").reshape(ne, nx, order="F"),
                cone_jacobian_variables=get("cone_jacobian_variables").reshape(nc, nx, order="F"))


@pytest.mark.parametrize("name", ["ragged", "cone_2", "cone_3", "cone_65", "cone_130"])
def test_fields_on_the_sparse_route(name):
    TP, theta = tp().trajectory(name), tp().parameters(name)
    s = TP.sparse_solver(parameters=theta, directory=os.path.join(ROOT, "tests", "device_eval_trajectory"))
    w = np.random.default_rng(2).standard_normal(s.N)
    s.set("solution", w)
    s.evaluate(FULL)
    assert TP.enqueued(s) <= 4
    want = host_fields(TP, w, theta)
    got = {}
    for k, (key, (colptr, rowval)) in enumerate(zip(("lagrangian_hessian", "equality_jacobian_variables", "cone_jacobian_variables"), TP.sparse_patterns())):
        cols = np.repeat(np.arange(TP.nx), np.diff(colptr))
        got[key] = s.get(key)
        assert got[key].shape == (len(rowval),) and np.isfinite(got[key]).all(), key
        dense = want[key]
        if dense.size:
            assert np.abs(got[key] - dense[rowval, cols]).max() <= 1e-12 * max(1.0, np.abs(dense).max()), key
            rest = dense.copy()
            rest[rowval, cols] = 0.0
            assert not rest.any(), key                                      # the stored pattern holds every non-zero of the host twin
    for key in ("objective", "objective_gradient_variables", "equality_constraint", "cone_constraint"):
        a = s.get(key)
        assert a.shape == want[key].shape and np.isfinite(a).all(), key
        if a.size:
            assert np.abs(a - want[key]).max() <= 1e-12 * max(1.0, np.abs(want[key]).max()), key
    # only the equality Jacobian asked for, at another point: the other two arrays keep their bits
    s.set("solution", np.random.default_rng(5).standard_normal(s.N))
    s.evaluate(pr.EQUALITY_JACOBIAN)
    assert TP.enqueued(s) <= 4
    assert np.array_equal(s.get("lagrangian_hessian"), got["lagrangian_hessian"]) and np.array_equal(s.get("cone_jacobian_variables"), got["cone_jacobian_variables"])
    assert not np.array_equal(s.get("equality_jacobian_variables"), got["equality_jacobian_variables"])
    s.close()


# ---- 2. the hand-written evaluator against qp_attach ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def fixture_library():
    L = C.CDLL(os.path.join(ROOT, "tests", "device_eval_sparse", "libqp_sparse_eval.so"))
    pp_i32, pp_dbl = C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_double))
    L.qp_sparse_create.restype = C.c_void_p
    L.qp_sparse_create.argtypes = [C.POINTER(C.c_int32), pp_i32, pp_i32, pp_dbl, pp_dbl] + [C.POINTER(C.c_double)] * 3 + [C.c_double]
    L.qp_sparse_destroy.argtypes = [C.c_void_p]
    L.qp_sparse_fail_with.argtypes = [C.c_void_p, C.c_int32]
    return L


class FixtureEvaluator:
    """the user object of tests/device_eval_sparse/qp_sparse_eval.hip for a problem's sparse inputs"""

    def __init__(self, prob, mats):
        import scipy.sparse as sp
        L = self.L = fixture_library()
        keep = []

        def arrays(ctype, dtype, items):
            items = [np.ascontiguousarray(a, dtype=dtype) for a in items]
            keep.extend(items)
            return (C.POINTER(ctype) * 3)(*[a.ctypes.data_as(C.POINTER(ctype)) for a in items])

        csr = [sp.csr_matrix(A) for A in mats]
        for A in csr:
            A.sort_indices()
        sizes = np.array([prob.nx, prob.ne, prob.nc], dtype=np.int32)
        vec = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        q, b, h = vec(prob.q), vec(prob.b), vec(prob.h)
        pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self.user = L.qp_sparse_create(sizes.ctypes.data_as(C.POINTER(C.c_int32)), arrays(C.c_int32, np.int32, [A.indptr for A in csr]),
                                       arrays(C.c_int32, np.int32, [A.indices for A in csr]), arrays(C.c_double, np.float64, [A.data for A in csr]),
                                       arrays(C.c_double, np.float64, [A.data for A in mats]), pd(q), pd(b), pd(h), 0.0)
        assert self.user
        self.entry = C.cast(L.qp_sparse_eval, C.c_void_p)

    def fail_with(self, code):
        self.L.qp_sparse_fail_with(self.user, code)

    def close(self):
        self.L.qp_sparse_destroy(self.user)


def qp_handles(prob, **kw):
    """the same handle settings twice: the QP attached, and the fixture evaluator set (no set_values: the evaluator writes the matrices)"""
    q, dims = kc.cone_layout(prob)
    mats = kc.sparse_inputs(prob)
    pkg = load_pkg()
    a = pkg.SparseKKT(*mats, n_nonnegative=q, second_order_dims=dims, **kw)
    a.set_values(*mats)
    a.attach_qp(prob.q, prob.b, prob.h)
    b = pkg.SparseKKT(*mats, n_nonnegative=q, second_order_dims=dims, **kw)
    ev = FixtureEvaluator(prob, mats)
    b.set_evaluator(ev.entry, ev.user)
    return a, b, ev


@pytest.mark.parametrize("case", [((2, 3, 1, 1, 0, 3), 0), ((3, 4, 2, 1, 1, 3), 1)], ids=["nonnegative", "second_order"])
def test_hand_written_evaluator_against_qp_attach(oracle_mod, case):
    prob = sc.problem(oracle_mod.splitmix_uniform, *case)
    a, b, ev = qp_handles(prob)
    results = []
    for g in (a, b):
        g.keep_trace(TRACE_ROWS)
        g.initialize(np.zeros(prob.nx))
        status, info = g.solve()
        print("status %d, %r" % (status, info))
        assert status == 1 and waits_hold(info), info
        results.append((status, info, g.trace(), g.get("solution")))
    (_, ia, ta, wa), (_, ib, tb, wb) = results
    assert [ia[k] for k in ("total_iterations", "outer_iterations", "accepted_iterates")] == [ib[k] for k in ("total_iterations", "outer_iterations", "accepted_iterates")]
    assert ia["accepted_iterates"] == sc.SOLVES[case]["accepted"] and ta.shape == tb.shape
    for r in range(ta.shape[0]):
        assert rel(tb[r], ta[r]) <= 1e-8, (r, rel(tb[r], ta[r]))
    assert rel(wb, wa) <= 1e-8
    # the building blocks at a fixed point
    _, pt, lam = pr.staged_conic_qp(oracle_mod.splitmix_uniform, case[1], *case[0])
    w = np.concatenate([pt[k] for k in "xrsyzt"])
    for g in (a, b):
        g.set_values(w=w, penalty=kc.RHO, central_path=kc.KAPPA)
        g.set("dual", lam)
    a.step_prologue()
    step = a.search_direction(a.get("residual"))[0]                         # a real Newton step and its cone step sizes: the candidate stays inside the cones
    a.set("step", step)
    a_s, a_t = a.cone_search()
    got = []
    for g in (a, b):
        p = g.step_prologue()
        g.set("step", step)
        cand = g.candidate(a_s, a_t)
        vectors = {name: g.get(name) for name in ("residual", "merit_gradient", "equality_constraint", "cone_constraint", "objective_gradient_variables", "candidate")}
        got.append((p, cand, g.accept(a_s), vectors, g.get("solution")))
    (pa, ca, va, veca, sa), (pb, cb, vb, vecb, sb) = got
    for key in ("objective", "barrier", "merit", "constraint_violation", "residual_violation", "optimality_error", "slack_violation"):
        print("%s: %r (qp_attach %r)" % (key, pb[key], pa[key]))
        assert close(pb[key], pa[key], 1e-12), key
    assert all(close(x, y, 1e-12) for x, y in zip(cb, ca)), (cb, ca)
    assert all(close(x, y, 1e-12) for x, y in zip(vb, va)), (vb, va)
    for name in veca:
        assert rel(vecb[name], veca[name]) <= 1e-12, name
    assert rel(sb, sa) <= 1e-12
    # a solve through the evaluator repeats bit for bit
    b.initialize(np.zeros(prob.nx))
    status, again = b.solve()
    assert status == 1 and np.array_equal(b.trace(), tb) and np.array_equal(b.get("solution"), wb)
    for g in (a, b):
        g.close()
    ev.close()


# ---- 3. whole nonlinear solves against the oracle -------------------------------------------------------------------------------------------------------------------
HERE_LIBS = os.path.join(ROOT, "tests", "device_eval_trajectory")


def guess(name, TP):
    if name == "pendulum":
        return TP.initialize_actions(TP.initialize_states(np.zeros(TP.nx), TP.linear_interpolation([0.0, 0.0], [np.pi, 0.0], TP.T)), [np.zeros(1)] * (TP.T - 1))
    if name.startswith("cartpole_swingup_"):                  # from rest to upright, as bench/trajectory_codegen.py starts it
        return TP.initialize_actions(TP.initialize_states(np.zeros(TP.nx), TP.linear_interpolation(np.zeros(4), [0.0, np.pi, 0.0, 0.0], TP.T)), [np.full(1, 0.01)] * (TP.T - 1))
    return np.zeros(TP.nx)


def sparse_handle_and_order(name, theta, **kw):
    """sparse_solver() under an explicit elimination order — the nested dissection of its own KKT pattern — so that the oracle can be given the same one"""
    import scipy.sparse as sp
    pkg = load_pkg()
    TP = tp().trajectory(name)
    first = TP.sparse_solver(parameters=theta, directory=HERE_LIBS)
    nz = first.info["nnz_upper"]
    K = sp.csc_matrix((np.ones(nz), first._rowval[:nz] - 1, first._colptr - 1), shape=(first.n, first.n))
    first.close()
    perm = pkg.ordering(K + K.T, "nested_dissection")
    return TP.sparse_solver(parameters=theta, directory=HERE_LIBS, perm=perm, options=dict(krylov_fallback=1, **kw)), perm


@pytest.fixture(scope="module")
def nonlinear_references(oracle_mod):
    """the oracle's whole solves through the host twin, under the handle's elimination order: computed once per problem and left unchanged"""
    cache = {}

    def get(name, perm):
        if name not in cache:
            TP, theta = tp().trajectory(name), tp().parameters(name)
            o = oracle_mod.OracleSolver(TP.nx, TP.np, TP.ne, TP.nc, TP.nonnegative_indices, TP.second_order_indices)
            o.set_perm(perm)
            if TP.np:
                o.buf("parameters")[:] = theta
            o.point()["x"][:] = guess(name, TP)
            status = o.solve(TP)
            ref = dict(status=status, trace=o.trace().copy(), w=o.point()["all"].copy(), x=o.point()["x"].copy(), **o.stats())
            for a in ref.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            cache[name] = ref
        return cache[name]
    return get


@pytest.mark.parametrize("name", ["pendulum", "cone_5", "cartpole_swingup_11"])
def test_whole_nonlinear_solves_against_the_oracle(nonlinear_references, name):
    TP, theta = tp().trajectory(name), tp().parameters(name)
    s, perm = sparse_handle_and_order(name, theta)
    ref = nonlinear_references(name, perm)
    print("oracle: status %d, %d iterations, %d refinement failures" % (ref["status"], ref["total_iterations"], ref["refinement_failures"]))
    assert ref["status"] == 1 and ref["refinement_failures"] == 0                      # the precondition: no `H \ residual` fallback is what is compared
    s.keep_trace(TRACE_ROWS)
    s.initialize(guess(name, TP))
    status, info = s.solve()
    print("status %d, %r" % (status, info))
    assert status == 1 and info["refinement_failures"] == 0
    assert waits_hold(info), info
    assert info["total_iterations"] == ref["total_iterations"] and info["outer_iterations"] == ref["outer"]
    tr = s.trace()
    assert tr.shape == ref["trace"].shape
    worst = max(rel(tr[r], ref["trace"][r]) for r in range(tr.shape[0]))
    print("accepted iterates: %d, worst relative distance from the oracle's %.3e; final x %.3e" % (tr.shape[0], worst, np.abs(s.get("solution")[:TP.nx] - ref["x"]).max()))
    for r in range(tr.shape[0]):
        assert rel(tr[r], ref["trace"][r]) <= 1e-8, (r, rel(tr[r], ref["trace"][r]))
    point = s.get("solution")
    assert np.abs(point[:TP.nx] - ref["x"]).max() <= 1e-6
    if name == "pendulum":
        states, actions = TP.get_trajectory(s)
        assert np.abs(states[0]).max() <= 1e-4 and np.abs(states[-1] - [np.pi, 0.0]).max() <= 1e-4 and len(actions) == TP.T - 1
    # a second solve on the same handle repeats the first bit for bit
    s.initialize(guess(name, TP))
    status, again = s.solve()
    assert status == 1 and np.array_equal(s.trace(), tr) and np.array_equal(s.get("solution"), point)
    assert [again[k] for k in s.SOLVE_INFO[:12]] == [info[k] for k in s.SOLVE_INFO[:12]]
    if name == "cone_5":
        # other parameters move the solution: the goal of every stage at 0.5 instead of 1
        other = theta.copy()
        other[0::2] = 0.5
        s.set_parameters(torch.tensor(other, dtype=torch.float64, device="cuda:0"))
        s.initialize(guess(name, TP))
        status, _ = s.solve()
        moved = s.get("solution")
        assert status == 1 and np.abs(moved[:TP.nx] - point[:TP.nx]).max() > 1e-2
        x, y, z = moved[:TP.nx], moved[TP.nx + TP.ne + TP.nc:TP.nx + 2 * TP.ne + TP.nc], moved[TP.nx + 2 * TP.ne + TP.nc:TP.nx + 2 * TP.ne + 2 * TP.nc]
        g = {}
        TP.evaluate(pr.EQUALITY, x, y, z, other, lambda nm: g.setdefault(nm, np.zeros(TP.ne)))
        assert np.abs(g["equality_constraint"]).max() <= 1e-4                          # ... to a point that is feasible for them (options.equality_tolerance)
    s.close()


# ---- 4. the sparse handle beside today's handle --------------------------------------------------------------------------------------------------------------------
def test_pendulum_on_the_sparse_handle_and_on_the_dense_handle():
    pkg = load_pkg()
    TP = tp().trajectory("pendulum")
    x0 = guess("pendulum", TP)
    dense = tp().solver("pendulum")
    assert dense.structure is None
    pkg.initialize_b(dense, x0)
    assert pkg.solve_b(dense)
    s = TP.sparse_solver(directory=HERE_LIBS, options=dict(krylov_fallback=1))
    s.initialize(x0)
    status, info = s.solve()
    assert status == 1 and info["total_iterations"] == dense.stats()["total_iterations"]
    print("sparse beside dense: %.3e" % rel(s.get("solution"), dense.solution.all))
    assert rel(s.get("solution"), dense.solution.all) <= 1e-8
    s.close()
    dense.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(oracle_mod):
    pkg = load_pkg()
    case = ((2, 3, 1, 1, 0, 3), 0)
    prob = sc.problem(oracle_mod.splitmix_uniform, *case)
    q, dims = kc.cone_layout(prob)
    mats = kc.sparse_inputs(prob)
    g = pkg.SparseKKT(*mats, n_nonnegative=q, second_order_dims=dims)

    def refused(call, code, *texts):
        with pytest.raises(pkg.CalipsoHipError) as e:
            call()
        assert "(%d)" % code in str(e.value) and all(t in str(e.value) for t in texts), str(e.value)

    g.set_values(*mats)
    g.set("solution", np.zeros(g.N))
    refused(g.solve, -4, "calipso_hip_sparse_kkt_solve: no q resident (calipso_hip_sparse_kkt_qp_attach first)")      # neither a QP nor an evaluator
    refused(lambda: g.evaluate(FULL), -4, "no evaluator attached")
    refused(lambda: g.set_parameters(np.zeros(0)), -4, "no evaluator attached")
    ev = FixtureEvaluator(prob, mats)
    g.set_evaluator(ev.entry, ev.user)
    refused(lambda: g.evaluate(FULL | pr.EQUALITY_JACOBIAN_PARAMETERS), -4, "calipso_hip_sparse_kkt_evaluate: flags: parameter-Jacobian bits")
    refused(lambda: g.evaluate(FULL | pr.EQUALITY_DUAL_GRADIENT), -4, "dual-gradient bit")
    refused(lambda: g.evaluate(FULL, which=2), -4, "which")
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.set_parameters(np.zeros(3))
    assert "theta has 3 entries, not 0" in str(e.value)
    ev.fail_with(1)
    refused(lambda: g.evaluate(FULL), -4, "the device evaluator returned 1")
    refused(g.solve, -4, "the device evaluator returned 1")
    ev.fail_with(7)
    refused(g.solve, -5, "the device evaluator returned 7")                  # CALIPSO_ERR_HIP
    ev.fail_with(0)
    # ... and the handle solves afterwards, through the evaluator and, attached again, as a QP
    ref = sc.SOLVES[case]
    g.initialize(np.zeros(prob.nx))
    status, info = g.solve()
    assert status == 1 and info["total_iterations"] == ref["total_iterations"] and waits_hold(info)
    point = g.get("solution")
    g.attach_qp(prob.q, prob.b, prob.h)                       # replaces the evaluator
    refused(lambda: g.evaluate(FULL), -4, "no evaluator attached")
    g.initialize(np.zeros(prob.nx))
    status, info = g.solve()
    assert status == 1 and rel(g.get("solution"), point) <= 1e-8
    g.close()
    ev.close()
