"""GPU (run with -m gpu on an MI355X): differentiate! on the sparse handle with the EVALUATOR's dR/dtheta — SparseKKT.set_parameter_patterns / evaluate_parameters /
differentiate() / vjp(theta=True) (csrc/sparse_solve.hip, csrc/sparse_differentiate.hip), the parameter destinations of the generated trajectory evaluators' sparse route
and a hand-written parametric evaluator (tests/device_eval_sparse_parameters) — against the host twin TrajectoryProblem.evaluate, against the caller-J entry (bit for
bit), against the CPU oracle.

Bounds.  Fields: 1e-12 x max(1, |field|max), the project's field tolerance (test_gpu_sparse_evaluator.py:75).  grad_theta against -J' lambda: the rounding of a
fixed-order sum of m products, entrywise 2 m 2^-53 sum |a| |lambda| (m: the column's non-zeros over the three arrays) — derived, not tuned.  Against S' v: the forward's
entrywise 1e-8 max(1, |S|) carried through the contraction, times ||v||_1 (test_gpu_sparse_differentiate.py).  Sensitivities against the oracle: 1e-8 max(1, |S|)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")      # (one HIP runtime per process: torch first, then the library)

import problems as pr
import sparse_differentiate_cases as dc
import sparse_kkt_cases as kc
from helpers import ROOT, interior_point, load_pkg, make_oracle
from test_c5_cartpole import problem as cartpole
from test_gpu_sparse_evaluator import FULL, HERE_LIBS
from test_gpu_trajectory_codegen import tp
from test_oracle_solve import run as run_oracle

pytestmark = pytest.mark.gpu

SHAPES = ["ragged", "cone_2", "cone_3", "cone_65", "cone_130", "cartpole_mpc"]
PARAMETER_FLAGS = (pr.OBJECTIVE_JACOBIAN_PARAMETERS | pr.EQUALITY_JACOBIAN_PARAMETERS | pr.EQUALITY_DUAL_JACOBIAN_PARAMETERS | pr.CONE_JACOBIAN_PARAMETERS |
                   pr.CONE_DUAL_JACOBIAN_PARAMETERS)
U = 2.0 ** -53


def offsets(s):
    return (0, s.nx + s.ne + s.nc, s.nx + 2 * s.ne + s.nc)                    # the x, y, z rows of the point's layout


def dense_columns(s, patterns, cols):
    """the N x len(cols) block of dR/dtheta built on the host from the three arrays get() returns"""
    J = np.zeros((s.N, len(cols)))
    for (colptr, rowval), name, off in zip(patterns, s.PARAMETER_ARRAYS, offsets(s)):
        v = s.get(name)
        assert v.shape == (len(rowval),)
        for c, j in enumerate(cols):
            at = slice(colptr[j], colptr[j + 1])
            J[off + rowval[at], c] = v[at]
    return J


def twin_arrays(TP, w, theta):
    """the host twin's dense theta-Jacobians at the point: (Lx,theta summed over its three terms, g,theta, h,theta)"""
    nx, ne, nc, npar = TP.nx, TP.ne, TP.nc, TP.np
    x, y, z = w[:nx], w[nx + ne + nc:nx + 2 * ne + nc], w[nx + 2 * ne + nc:nx + 2 * ne + 2 * nc]
    sizes = dict(objective_jacobian_variables_parameters=nx * npar, equality_dual_jacobian_variables_parameters=nx * npar,
                 cone_dual_jacobian_variables_parameters=nx * npar, equality_jacobian_parameters=ne * npar, cone_jacobian_parameters=nc * npar)
    out = {}
    TP.evaluate(PARAMETER_FLAGS, x, y, z, theta, lambda nm: out.setdefault(nm, np.zeros(sizes[nm])))
    get = lambda nm: out.get(nm, np.zeros(sizes[nm]))
    return (sum(get(n) for n in list(sizes)[:3]).reshape(nx, npar, order="F"), get("equality_jacobian_parameters").reshape(ne, npar, order="F"),
            get("cone_jacobian_parameters").reshape(nc, npar, order="F"))


def handle_at_an_interior_point(name, seed=5):
    """sparse_solver() of a built trajectory problem with an interior point, the scalars of test_gpu_sparse_differentiate.py and every matrix resident, (ep, ed) held"""
    TP, theta = tp().trajectory(name), tp().parameters(name)
    s = TP.sparse_solver(parameters=theta, directory=HERE_LIBS)
    pt, lam = interior_point(TP, seed)
    s.set_values(w=np.concatenate([pt[k] for k in "xrsyzt"]), penalty=dc.INTERIOR["rho"], central_path=dc.INTERIOR["kappa"])
    s.set("dual", lam)
    s.evaluate(FULL)
    s.factorize(dc.INTERIOR["ep"], dc.INTERIOR["ed"])
    return TP, theta, s


# ---- 1. fields ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_parameter_fields_against_the_host_twin(name):
    TP, theta = tp().trajectory(name), tp().parameters(name)
    s = TP.sparse_solver(parameters=theta, directory=HERE_LIBS)
    patterns = TP.sparse_parameter_patterns()
    w = np.random.default_rng(2).standard_normal(s.N)
    s.set("solution", w)

    def compare(th):
        s.evaluate_parameters()
        assert TP.enqueued(s) <= 4
        got = [s.get(n) for n in s.PARAMETER_ARRAYS]
        for key, a, D, (colptr, rowval) in zip(s.PARAMETER_ARRAYS, got, twin_arrays(TP, w, th), patterns):
            cols = np.repeat(np.arange(TP.np), np.diff(colptr))
            assert a.shape == (len(rowval),) and np.isfinite(a).all(), key
            if D.size:
                worst = np.abs(a - D[rowval, cols]).max() if a.size else 0.0
                print("%s %s: %d non-zeros, |field| %.3e, distance %.3e" % (name, key, a.size, np.abs(D).max(), worst))
                assert worst <= 1e-12 * max(1.0, np.abs(D).max()), key
        return got

    first = compare(theta)
    w0 = w
    # other parameters AND another point (the cone and ragged problems are bilinear: their arrays move with x, not with theta alone): the arrays are those of the
    # twin there, and differ from the first wherever the twin's do
    other = theta + 0.25 * np.random.default_rng(7).standard_normal(TP.np)
    w = np.random.default_rng(12).standard_normal(s.N)
    s.set_parameters(other)
    s.set("solution", w)
    second = compare(other)
    twin_moved = [not np.array_equal(a, b) for a, b in zip(twin_arrays(TP, w0, theta), twin_arrays(TP, w, other))]
    moved = [not np.array_equal(a, b) for a, b in zip(first, second)]
    print("%s: arrays that moved %r (the twin's %r)" % (name, moved, twin_moved))
    assert moved == twin_moved
    if name in ("cartpole_mpc", "ragged"):                                     # (the cone problems' theta-Jacobians are constants)
        assert moved[0]
    # theta alone: the cart-pole's cost weights enter squared, so Lx,theta depends on theta itself
    if name == "cartpole_mpc":
        s.set_parameters(theta)
        third = compare(theta)
        assert not np.array_equal(third[0], second[0])
    s.close()


# ---- 2. forward: the bits of the caller-J entry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_forward_is_the_caller_j_entry_bit_for_bit(name):
    TP, theta, s = handle_at_an_interior_point(name)
    patterns = TP.sparse_parameter_patterns()
    S = s.differentiate()
    assert S.shape == (s.N, TP.np) and np.isfinite(S).all() and np.abs(S).max() > 0.0
    assert s.differentiate_info()["columns"] == TP.np
    J = dense_columns(s, patterns, range(TP.np))
    assert np.array_equal(S, s.differentiate(J))
    pick = [0, TP.np - 1, 0, TP.np // 2]                                       # a repeated and the last index
    Sp = s.differentiate(columns=pick)
    assert Sp.shape == (s.N, 4) and np.array_equal(Sp, s.differentiate(dense_columns(s, patterns, pick)))
    assert np.array_equal(Sp[:, 0], Sp[:, 2]) and np.abs(Sp - S[:, pick]).max() <= 1e-8 * max(1.0, np.abs(S).max())
    # the device route gives the bits of the host route
    assert np.array_equal(s.differentiate(device=True).cpu().numpy(), S)
    assert np.array_equal(s.differentiate(columns=pick, device=True).cpu().numpy(), Sp)
    s.close()


# ---- 3. reverse --------------------------------------------------------------------------------------------------------------------------------------------------------
def check_gradient(s, patterns, out, V, S):
    """theta against -J' lambda within the rounding of a fixed-order sum, and against S' v within the forward's bound through the contraction"""
    lam, got = out["adjoint"].reshape(s.N, -1), out["theta"].reshape(s.num_parameters, -1)
    V = V.reshape(s.N, -1)
    want = np.zeros(got.shape, dtype=np.longdouble); scale = np.zeros(got.shape); m = np.zeros(s.num_parameters)
    for (colptr, rowval), name, off in zip(patterns, s.PARAMETER_ARRAYS, offsets(s)):
        v = s.get(name)
        for j in range(s.num_parameters):
            at = slice(colptr[j], colptr[j + 1])
            a, l = v[at].astype(np.longdouble)[:, None], lam[off + rowval[at]]
            want[j] -= (a * l.astype(np.longdouble)).sum(axis=0)
            scale[j] += (np.abs(v[at])[:, None] * np.abs(l)).sum(axis=0)
            m[j] += colptr[j + 1] - colptr[j]
    bound = 2.0 * m[:, None] * U * scale
    worst = np.abs(got - want.astype(np.float64))
    print("|theta + J'lambda| %.3e (largest bound %.3e); |theta - S'v| %.3e (bound %.3e)" % (worst.max(), bound.max(), np.abs(got - S.T @ V).max(),
                                                                                              1e-8 * max(1.0, np.abs(S).max()) * np.abs(V).sum(axis=0).max()))
    assert (np.abs(got - want) <= bound).all()
    assert (np.abs(got - S.T @ V) <= 1e-8 * max(1.0, np.abs(S).max()) * np.abs(V).sum(axis=0)[None, :]).all()


@pytest.mark.parametrize("name", SHAPES)
def test_reverse_gradient_with_respect_to_theta(name):
    TP, theta, s = handle_at_an_interior_point(name)
    patterns = TP.sparse_parameter_patterns()
    S = s.differentiate()
    s.evaluate_parameters()
    for k in (1, 3):
        V = np.random.default_rng(9 + k).standard_normal((s.N, k))
        V = V[:, 0] if k == 1 else V
        out = s.vjp(V)                                                         # theta defaults to True on a handle with parameter patterns
        assert set(out) == {"adjoint", "theta"} and out["theta"].shape == ((TP.np,) if k == 1 else (TP.np, k)) and out["adjoint"].shape == V.shape
        check_gradient(s, patterns, out, V, S)
        again = s.vjp(V, theta=True)
        assert np.array_equal(again["theta"], out["theta"]) and np.array_equal(again["adjoint"], out["adjoint"])
        dev = s.vjp(torch.tensor(V, dtype=torch.float64, device="cuda:0"), adjoint=False)
        assert set(dev) == {"theta"} and np.array_equal(dev["theta"].cpu().numpy(), out["theta"])
        assert s.vjp_info()["columns"] == k and s.vjp_times()["gradients"] > 0.0
    assert "theta" not in s.vjp(np.zeros(s.N), theta=False)
    s.close()


# ---- 4. the hand-written parametric evaluator against the oracle ---------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 63, 64, 65, 300)          # the non-zeros of Qt's columns: an empty column, both sides of the wavefront width, both sides of the split length


class AffineParametricQP(pr.ConicQP):
    """ConicQP whose vectors are affine in theta: q = q0 + Qt theta, b = b0 + Bt theta, h = h0 + Ht theta — the host twin of
    tests/device_eval_sparse_parameters/qp_sparse_parameters_eval.hip for the oracle"""

    def __init__(self, base, Qt, Bt, Ht, theta):
        super().__init__(base.P, base.q, base.A, base.b, base.G, base.h, nonnegative_indices=base.nonnegative_indices, second_order_indices=base.second_order_indices,
                         objective_scale=base.c, name="affine_parametric_qp")
        self.Qt, self.Bt, self.Ht = (np.asarray(M.todense()) for M in (Qt, Bt, Ht))
        self.np, self.parameters = len(theta), np.asarray(theta, dtype=np.float64)

    def evaluate(self, flags, x, y, z, theta, out):
        theta = np.asarray(theta, dtype=np.float64)
        q0, b0, h0 = self.q, self.b, self.h
        self.q, self.b, self.h = q0 + self.Qt @ theta, b0 + self.Bt @ theta, h0 + self.Ht @ theta
        try:
            super().evaluate(flags, x, y, z, theta, out)
        finally:
            self.q, self.b, self.h = q0, b0, h0
        put = lambda name, M: pr._put(out, name, M)
        if flags & pr.OBJECTIVE_JACOBIAN_PARAMETERS:
            put("objective_jacobian_variables_parameters", self.Qt)
        if flags & pr.EQUALITY_JACOBIAN_PARAMETERS and self.ne:
            put("equality_jacobian_parameters", -self.Bt)
        if flags & pr.EQUALITY_DUAL_JACOBIAN_PARAMETERS:
            put("equality_dual_jacobian_variables_parameters", np.zeros((self.nx, self.np)))
        if flags & pr.CONE_JACOBIAN_PARAMETERS and self.nc:
            put("cone_jacobian_parameters", self.Ht)
        if flags & pr.CONE_DUAL_JACOBIAN_PARAMETERS:
            put("cone_dual_jacobian_variables_parameters", np.zeros((self.nx, self.np)))


@functools.lru_cache(maxsize=1)
def parametric_library():
    L = C.CDLL(os.path.join(ROOT, "tests", "device_eval_sparse_parameters", "libqp_sparse_parameters_eval.so"))
    pp_i32, pp_dbl = C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_double))
    L.qp_sparse_parameters_create.restype = C.c_void_p
    L.qp_sparse_parameters_create.argtypes = [C.POINTER(C.c_int32), pp_i32, pp_i32, pp_dbl, pp_dbl] + [C.POINTER(C.c_double)] * 3
    L.qp_sparse_parameters_destroy.argtypes = [C.c_void_p]
    return L


def parametric_user(prob, mats):
    """the user object of the fixture for six CSC matrices: Lxx, gx, hx, Qt, Bt, Ht"""
    L, keep = parametric_library(), []

    def arrays(ctype, dtype, items):
        items = [np.ascontiguousarray(a, dtype=dtype) for a in items]
        keep.extend(items)
        return (C.POINTER(ctype) * 6)(*[a.ctypes.data_as(C.POINTER(ctype)) for a in items])

    csr = [sp.csr_matrix(A) for A in mats]
    for A in csr:
        A.sort_indices()
    sizes = np.array([prob.nx, prob.ne, prob.nc, prob.np], dtype=np.int32)
    vec = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (prob.q, prob.b, prob.h)]
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    user = L.qp_sparse_parameters_create(sizes.ctypes.data_as(C.POINTER(C.c_int32)), arrays(C.c_int32, np.int32, [A.indptr for A in csr]),
                                         arrays(C.c_int32, np.int32, [A.indices for A in csr]), arrays(C.c_double, np.float64, [A.data for A in csr]),
                                         arrays(C.c_double, np.float64, [A.data for A in mats]), *[pd(a) for a in vec])
    assert user
    return L, user


@pytest.fixture(scope="module")
def parametric(oracle_mod):
    """the parametric QP (nx = 300), a handle that solved it through the hand-written evaluator, and the oracle differentiated at the handle's own point and scalars
    with its cone Jacobians formed at the handle's differentiate slacks — the method of test_gpu_sparse_differentiate.py's `solved`.  The cones are nonnegative
    rows and the handle runs the correction rounds (differentiate_refinement = 1), as the reference does without a second-order cone: with one (3 nonnegative rows + a
    cone of 3 on the same data) both sides return the UNREFINED solve (quirk B-3), and at N = 326 the two elimination orders were measured 4.5e-07 apart with
    |S| = 0.32, which the 1e-8 of the small cases cannot hold"""
    rng = np.random.default_rng(41)
    base = pr.parametric_conic_qp_dims(300, 4, 6, [], seed=77)
    nx, ne, nc, npar = base.nx, base.ne, base.nc, len(LENGTHS)
    rows = np.concatenate([np.sort(rng.choice(nx, size=n, replace=False)) for n in LENGTHS])
    cols = np.repeat(np.arange(npar), LENGTHS)
    Qt = sp.csc_matrix((0.05 * rng.standard_normal(len(rows)), (rows, cols)), shape=(nx, npar))
    # column 0 is empty in all three arrays; the totals over the three are 0, 5, 4, 63 (a thread's), 64, 66, 302 (a wavefront's)
    Bt = sp.csc_matrix((0.3 * rng.standard_normal(5), ([0, 3, 1, 2, 0], [1, 1, 2, 5, 6])), shape=(ne, npar))
    Ht = sp.csc_matrix((0.3 * rng.standard_normal(4), ([0, 4, 2, 5], [1, 1, 2, 6])), shape=(nc, npar))
    for M in (Qt, Bt, Ht):
        M.sort_indices()
    assert tuple(np.diff(Qt.indptr)) == LENGTHS
    assert tuple(int(v) for v in np.diff(Qt.indptr) + np.diff(Bt.indptr) + np.diff(Ht.indptr)) == (0, 5, 4, 63, 64, 66, 302)
    theta = 0.5 * rng.standard_normal(npar)
    prob = AffineParametricQP(base, Qt, Bt, Ht, theta)
    own = dc.oracle_whole_solve(oracle_mod, prob)
    assert own["status"] == 1 and own["lu_fallbacks"] == 0
    q, dims = kc.cone_layout(base)
    mats = kc.sparse_inputs(base)
    g = load_pkg().SparseKKT(*mats, n_nonnegative=q, second_order_dims=dims)
    g.set_option("differentiate_refinement", 1)
    L, user = parametric_user(prob, list(mats) + [Qt, Bt, Ht])
    g.set_evaluator(C.cast(L.qp_sparse_parameters_eval, C.c_void_p), user, npar)
    patterns = [(M.indptr.astype(np.int64), M.indices.astype(np.int64)) for M in (Qt, -Bt, Ht)]
    g.set_parameter_patterns(Qt, Bt, Ht)
    g.set_parameters(theta)
    g.initialize(np.zeros(nx))
    status, info = g.solve()
    assert status == 1 and info["total_iterations"] == own["total_iterations"]
    w, slacks = g.get("solution"), g.get("differentiate_slacks")
    scalars = dict(kappa=info["central_path"], rho=info["penalty"], ep=own["scalars"]["ep"], ed=own["scalars"]["ed"])
    o = dc.differentiated_oracle(oracle_mod, prob, dc.split(w, nx, ne, nc), g.get("dual"), scalars, slacks=slacks)
    yield dict(g=g, prob=prob, patterns=patterns, S=o.mat("solution_sensitivity", o.N, npar).copy(), J=o.mat("jacobian_parameters", o.N, npar).copy(), mats=(Qt, Bt, Ht))
    g.close()
    L.qp_sparse_parameters_destroy(user)


def test_the_hand_written_parametric_evaluator_against_the_oracle(parametric):
    g, S, patterns = parametric["g"], parametric["S"], parametric["patterns"]
    Qt, Bt, Ht = parametric["mats"]
    g.evaluate_parameters()
    for name, M in zip(g.PARAMETER_ARRAYS, (Qt, -Bt, Ht)):                    # Lx,theta = Qt, g,theta = -Bt, h,theta = Ht: constant, copied to the bit
        assert np.array_equal(g.get(name), sp.csc_matrix(M).data), name
    assert np.array_equal(dense_columns(g, patterns, range(len(LENGTHS))), parametric["J"])
    got = g.differentiate()
    print("parametric QP: N = %d, |S| = %.3e, |S_gpu - S| = %.3e" % (g.N, np.abs(S).max(), np.abs(got - S).max()))
    assert got.shape == S.shape and np.abs(got - S).max() <= 1e-8 * max(1.0, np.abs(S).max())
    assert np.array_equal(got, g.differentiate(parametric["J"]))
    for k in (1, 3):
        V = np.random.default_rng(20 + k).standard_normal((g.N, k))
        V = V[:, 0] if k == 1 else V
        out = g.vjp(V)
        Vc = V.reshape(g.N, -1)
        bound = 1e-8 * max(1.0, np.abs(S).max()) * np.abs(Vc).sum(axis=0)[None, :]
        print("parametric QP, k = %d: |theta - S'v| = %.3e, bound %.3e" % (k, np.abs(out["theta"].reshape(len(LENGTHS), -1) - S.T @ Vc).max(), bound.min()))
        assert (np.abs(out["theta"].reshape(len(LENGTHS), -1) - S.T @ Vc) <= bound).all()
        check_gradient(g, patterns, out, V, got)                                # the empty, the 63 / 64 / 65 and the 300-entry columns: both kernel shapes
        assert np.array_equal(g.vjp(V)["theta"], out["theta"])
    ones = g.vjp(np.ones(g.N))["theta"]
    assert ones[0] == 0.0 and np.all(ones[1:] != 0.0)                            # a parameter with no entry in any array: its gradient is written, as zero


# ---- 4b. the handle's grown buffers: patterns and parameters set again give a fresh handle's bits ---------------------------------------------------------------------------
def parametric_handle(parametric):
    """a fresh handle on the fixture's problem, its sparse inputs, and attach(g, user, mats, count): the hand-written evaluator with that user object and `count`
    parameters, the patterns of the blocks `mats` and the fixture's theta"""
    prob = parametric["prob"]
    q, dims = kc.cone_layout(prob)
    inputs = kc.sparse_inputs(prob)
    g = load_pkg().SparseKKT(*inputs, n_nonnegative=q, second_order_dims=dims)

    def attach(g, user, mats, count=prob.np):
        g.set_evaluator(C.cast(parametric_library().qp_sparse_parameters_eval, C.c_void_p), user, count)
        if count == prob.np:
            g.set_parameter_patterns(*mats)
            g.set_parameters(prob.parameters)
    return g, inputs, attach


def test_parameter_patterns_set_again_give_a_fresh_handles_arrays(parametric):
    prob, full = parametric["prob"], parametric["mats"]

    def thinned(M):                                                            # a strict sub-pattern: every third stored entry dropped
        M = sp.coo_matrix(M)
        keep = np.arange(M.nnz) % 3 != 0
        out = sp.csc_matrix((M.data[keep], (M.row[keep], M.col[keep])), shape=M.shape)
        out.sort_indices()
        return out
    sub = [thinned(M) for M in full]
    assert all(0 < a.nnz < b.nnz for a, b in zip(sub, full))
    g, inputs, attach = parametric_handle(parametric)
    w = np.random.default_rng(6).standard_normal(g.N)
    g.set("solution", w)
    users = []
    for mats in (full, sub, full):
        L, user = parametric_user(prob, list(inputs) + list(mats))
        users.append(user)
        fresh, _, _ = parametric_handle(parametric)
        fresh.set("solution", w)
        got = []
        for h in (g, fresh):
            attach(h, user, mats)
            h.evaluate_parameters()
            got.append([h.get(n) for n in h.PARAMETER_ARRAYS])
        for a, b, M, sign in zip(got[0], got[1], mats, (1.0, -1.0, 1.0)):   # Lx,theta = Qt, g,theta = -Bt, h,theta = Ht on the patterns set last
            assert a.shape == b.shape == (M.nnz,) and np.array_equal(a, b) and np.array_equal(a, sign * M.data)
        fresh.close()
    g.close()
    for user in users:
        L.qp_sparse_parameters_destroy(user)


def test_the_evaluator_set_again_with_another_parameter_count_solves_to_the_same_trace(parametric):
    prob = parametric["prob"]
    g, inputs, attach = parametric_handle(parametric)
    L, user = parametric_user(prob, list(inputs) + list(parametric["mats"]))

    def run():
        g.keep_trace(8)
        g.initialize(np.zeros(prob.nx))
        status, info = g.solve()
        return status, info["total_iterations"], g.trace(), info["accepted_iterates"]
    attach(g, user, parametric["mats"])
    before = run()
    attach(g, user, None, prob.np + 3)                                         # more parameters: theta grows
    attach(g, user, parametric["mats"])                                        # ... and back: theta is set again
    after = run()
    assert before[0] == after[0] == 1 and before[1] == after[1] and before[3] > 0
    assert before[2].shape == (min(8, before[3]), g.N) and np.array_equal(before[2], after[2])
    g.close()
    L.qp_sparse_parameters_destroy(user)


# ---- 5. a nonlinear whole solve ----------------------------------------------------------------------------------------------------------------------------------------
def test_cartpole_mpc_solved_then_differentiated_against_the_oracle_at_the_handles_own_state(oracle_mod):
    """the method of test_gpu_trajectory_codegen.py:220-243 with its 1e-8: the oracle differentiated at the handle's point, scalars, Hessian, Jacobian and slacks"""
    prob = cartpole()
    TP = tp().trajectory("cartpole_mpc")
    own, st = run_oracle(oracle_mod, prob)
    assert st == 1
    s = TP.sparse_solver(parameters=prob.parameters, directory=HERE_LIBS, options=dict(krylov_fallback=1))
    s.initialize(prob.x0)
    status, info = s.solve()
    assert status == 1 and info["total_iterations"] == own.stats()["total_iterations"]
    w = s.get("solution")
    scalars = dict(kappa=info["central_path"], rho=info["penalty"], ep=float(own.buf("primal_regularization")[0]), ed=float(own.buf("dual_regularization")[0]))
    o = make_oracle(oracle_mod, prob, dc.split(w, prob.nx, prob.ne, prob.nc), s.get("dual"), **scalars)
    o.buf("parameters")[:] = prob.parameters
    dense = lambda key, pattern, rows: np.asarray(sp.csc_matrix((s.get(key), pattern[1], pattern[0]), shape=(rows, prob.nx)).todense()).reshape(-1, order="F")
    pats = TP.sparse_patterns()
    o.buf("objective_jacobian_variables_variables")[:] = dense("lagrangian_hessian", pats[0], prob.nx)
    o.buf("equality_dual_jacobian_variables_variables")[:] = 0.0
    o.buf("cone_dual_jacobian_variables_variables")[:] = 0.0
    o.buf("equality_jacobian_variables")[:] = dense("equality_jacobian_variables", pats[1], prob.ne)
    assert prob.nc == 0                                                       # no cone: no slacks to keep, no cone Jacobian to hand over
    o.cone(product=True, jacobian=True, target=True)
    assert o.differentiate(prob) >= 0
    S_cpu = o.mat("solution_sensitivity", o.N, prob.np)
    S = s.differentiate()
    print("cartpole_mpc on the sparse handle: |S| = %.3e, |S_gpu - S| = %.3e" % (np.abs(S_cpu).max(), np.abs(S - S_cpu).max()))
    assert S.shape == S_cpu.shape and np.abs(S - S_cpu).max() <= 1e-8 * max(1.0, np.abs(S_cpu).max())
    v = np.random.default_rng(3).standard_normal(s.N)
    grad = s.vjp(v, theta=True)["theta"]                                       # dLoss/dtheta with no host evaluation
    assert np.abs(grad - S_cpu.T @ v).max() <= 1e-8 * max(1.0, np.abs(S_cpu).max()) * np.abs(v).sum()
    s.close()


def test_the_layers_backward_is_the_handles_vjp_on_host_and_on_device_tensors():
    load_pkg()
    from calipso_jl_amd.torch_layer import SparseTrajectoryLayer
    TP, theta = tp().trajectory("cone_3"), tp().parameters("cone_3")
    s = TP.sparse_solver(parameters=np.zeros(TP.np), directory=HERE_LIBS)
    weights = np.random.default_rng(4).standard_normal(s.N)
    for device in ("cpu", "cuda:0"):
        th = torch.tensor(theta, dtype=torch.float64, device=device, requires_grad=True)
        w = SparseTrajectoryLayer.apply(s, th, torch.zeros(TP.nx, dtype=torch.float64, device=device))
        assert w.device.type == device[:4] and w.shape == (s.N,) and s.solve_info["status"] == 1
        assert np.array_equal(w.detach().cpu().numpy(), s.get("solution"))
        (w * torch.tensor(weights, device=device)).sum().backward()
        want = s.vjp(weights, adjoint=False, theta=True)["theta"]                # the handle still holds the layer's solve
        assert th.grad.device.type == device[:4] and np.abs(want).max() > 0.0 and np.array_equal(th.grad.cpu().numpy(), want)
    s.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_the_handle_solves_afterwards():
    pkg = load_pkg()
    TP, theta = tp().trajectory("cone_3"), tp().parameters("cone_3")
    s = TP.sparse_solver(parameters=theta, directory=HERE_LIBS)
    L = s._L

    def refused(call, *texts):
        with pytest.raises(pkg.CalipsoHipError) as e:
            call()
        assert "(-4)" in str(e.value) and all(t in str(e.value) for t in texts), str(e.value)

    s.initialize(np.zeros(TP.nx))
    status, first = s.solve()
    assert status == 1
    point = s.get("solution")
    refused(lambda: s.differentiate(columns=[0, TP.np]), "calipso_hip_sparse_kkt_differentiate_parameters", "columns[1] = %d" % (TP.np + 1))
    refused(lambda: s.differentiate(columns=[-1]), "columns[0] = 0")
    refused(lambda: s.differentiate(columns=[]), "k: at least one column")
    out, cols = np.zeros(s.N * (TP.np - 1)), None
    refused(lambda: s._check(L.calipso_hip_sparse_kkt_differentiate_parameters(s._h, TP.np - 1, cols, out.ctypes.data_as(C.POINTER(C.c_double))), "differentiate_parameters"),
            "k: columns = NULL selects all %d parameters" % TP.np)
    refused(lambda: s._check(L.calipso_hip_sparse_kkt_differentiate_parameters(s._h, TP.np, None, None), "differentiate_parameters"), "sensitivity is NULL")
    v = np.ones(s.N)
    refused(lambda: s._check(L.calipso_hip_sparse_kkt_differentiate_adjoint_parameters(s._h, 1, v.ctypes.data_as(C.POINTER(C.c_double)), None, None), "adjoint_parameters"),
            "grad_theta is NULL")
    refused(lambda: s._check(L.calipso_hip_sparse_kkt_differentiate_adjoint_parameters(s._h, 0, v.ctypes.data_as(C.POINTER(C.c_double)), None, None), "adjoint_parameters"), "k:")
    refused(lambda: s.evaluate(pr.EQUALITY_JACOBIAN_PARAMETERS), "calipso_hip_sparse_kkt_evaluate: flags: parameter-Jacobian bits")      # evaluate keeps refusing them
    Lp, gp, hp = TP.sparse_parameter_patterns()
    bad = (hp[0], hp[1].copy())
    bad[1][-1] = TP.nc                                                         # a row past the last row
    refused(lambda: s.set_parameter_patterns(Lp, gp, bad), "hp_rowval")
    assert s._has_parameter_patterns() and np.array_equal(s.differentiate(columns=[1]), s.differentiate(columns=[1]))      # a refused call leaves the patterns there were
    s.set_evaluator(C.cast(getattr(s._library, TP.name + "_sparse_eval"), C.c_void_p), s._user, TP.np)                   # the evaluator set again: no patterns
    s.set_parameters(theta)
    assert not s._has_parameter_patterns()
    refused(lambda: s.differentiate(), "no parameter patterns set")
    refused(lambda: s.vjp(v, theta=True), "no parameter patterns set")
    refused(lambda: s.evaluate_parameters(), "no parameter patterns set")
    refused(lambda: s.get("equality_jacobian_parameters"), "no parameter patterns set")
    # a handle without patterns behaves as before: vjp has no "theta"
    assert set(s.vjp(v)) == {"adjoint"}
    s.set_parameter_patterns(Lp, gp, hp)
    S = s.differentiate()
    assert S.shape == (s.N, TP.np)
    s.initialize(np.zeros(TP.nx))
    status, again = s.solve()
    assert status == 1 and np.array_equal(s.get("solution"), point) and again["total_iterations"] == first["total_iterations"]
    s.set_evaluator(None)                                                      # drops the patterns with the evaluator
    assert not s._has_parameter_patterns()
    s.close()
