"""GPU (run with -m gpu on an MI355X): differentiate! on sparse problem data — SparseKKT.solve_columns / differentiate / vjp (csrc/sparse_differentiate.hip) and
torch_layer.SparseQPLayer — against the CPU oracle and closed forms, never the code under test.  The inputs are those of tests/sparse_differentiate_cases.py, which
tests/test_sparse_differentiate_inputs_cpu.py pins with the oracle alone.

Bounds.  1e-8 relative to max(1, |M|) is the project's step tolerance against the oracle (a wrong term of a map gives errors of order one).  For the gradients that
are S' v, the forward's entrywise bound 1e-8 max(1, |S|) carried through the contraction with the cotangent: times ||v||_1 (test_gpu_differentiate_adjoint.py).  The
matrix gradients against their closed forms: 8 eps times the scale of their products (closed_forms of that file)."""
import types
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")      # (one HIP runtime per process: torch first, then the library)

import problems as pr
import sparse_differentiate_cases as dc
import sparse_kkt_cases as kc
import sparse_solve_cases as sc
from helpers import load_pkg
from test_gpu_differentiate_adjoint import DirectionalQP, closed_forms

pytestmark = pytest.mark.gpu

MULTIFRONTAL, COLUMNS = "nested_dissection", "minimum_degree"
EPS = np.finfo(np.float64).eps


def block_handle(prob, w, method=MULTIFRONTAL, extra=None):
    """SparseKKT of a building-block case with its values, point and scalars resident, factored at the fixed regularisation"""
    q, dims = kc.cone_layout(prob)
    Lxx, gx, hx = kc.sparse_inputs(prob, extra)
    g = load_pkg().SparseKKT(Lxx, gx, hx, n_nonnegative=q, second_order_dims=dims, method=method)
    g.set_values(Lxx, gx, hx, w, kc.RHO, central_path=kc.KAPPA)
    g.factorize(kc.EP, kc.ED)
    return g


def conic_handle(prob, pt=None, scalars=None, **kw):
    """SparseConicQP of a problem (the stored patterns: the non-zeros of P, A, G); with a point: that point and the scalars resident, (ep, ed) held"""
    q, dims = kc.cone_layout(prob)
    mats = [sp.csc_matrix(M) for M in (prob.P, prob.A, prob.G)]
    g = load_pkg().SparseConicQP(mats[0], prob.q, mats[1], prob.b, mats[2], prob.h, n_nonnegative=q, second_order_dims=dims, objective_scale=prob.c, **kw)
    if pt is not None:
        g.set_values(w=np.concatenate([pt[k] for k in "xrsyzt"]), penalty=scalars["rho"], central_path=scalars["kappa"])
        g.factorize(scalars["ep"], scalars["ed"])      # (the regularisation the handle holds is that of its last assemble)
    return g, mats


@pytest.fixture(scope="module")
def block_references(oracle_mod):
    """per building-block case, computed once and left unchanged: the problem, the point, the oracle's map M and its H"""
    cache = {}

    def get(name):
        if name not in cache:
            prob, w, o = dc.block_oracle(oracle_mod, name)
            ref = dict(prob=prob, w=w, H=o.H_dense().copy(), M=dc.map_matrix(o), tolerance=float(o.buf("opt.iterative_refinement_tolerance")[0]))
            for a in ref.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            cache[name] = ref
        return cache[name]
    return get


# ---- 1. the maps ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [MULTIFRONTAL, COLUMNS])
@pytest.mark.parametrize("name", kc.BLOCK_CASES)
def test_the_maps_against_the_oracles_forward_map(block_references, name, method):
    ref = block_references(name)
    M, N = ref["M"], ref["M"].shape[0]
    g = block_handle(ref["prob"], ref["w"], method)
    bound = 1e-8 * max(1.0, np.abs(M).max())
    I = np.eye(N)
    fwd, rev = g.solve_columns(I), g.solve_columns(I, transposed=True)      # k = N: more than 64 columns everywhere but on the smallest case
    print("%s %s: N = %d, |M| = %.2e, |X - M| = %.2e, |Lambda - M'| = %.2e" % (name, method, N, np.abs(M).max(), np.abs(fwd - M).max(), np.abs(rev - M.T).max()))
    assert fwd.shape == rev.shape == (N, N)
    assert np.abs(fwd - M).max() <= bound and np.abs(rev - M.T).max() <= bound
    for transposed, want in ((False, M), (True, M.T)):
        three = g.solve_columns(I[:, :3], transposed=transposed)
        one = g.solve_columns(I[:, 0], transposed=transposed)
        assert three.shape == (N, 3) and one.shape == (N,)
        assert np.abs(three - want[:, :3]).max() <= bound and np.abs(one - want[:, 0]).max() <= bound
        assert np.abs(one - three[:, 0]).max() <= bound


# ---- 2. differentiate! in both directions against the oracle's -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def differentiate_references(oracle_mod):
    cache = {}

    def get(case):
        if case not in cache:
            prob, pt, lam = dc.differentiate_case(case)
            o = dc.differentiated_oracle(oracle_mod, prob, pt, lam, dc.INTERIOR)
            ref = dict(prob=prob, pt=pt, J=o.mat("jacobian_parameters", o.N, prob.np).copy(), S=o.mat("solution_sensitivity", o.N, prob.np).copy())
            ref["J"].setflags(write=False); ref["S"].setflags(write=False)
            cache[case] = ref
        return cache[case]
    return get


def point_of(g):
    w = g.get("solution")
    oy, oz = g.nx + g.ne + g.nc, g.nx + 2 * g.ne + g.nc
    return types.SimpleNamespace(variables=w[:g.nx], equality_dual=w[oy:oy + g.ne], cone_dual=w[oz:oz + g.nc])


def check_closed_forms(g, mats, c, out, v_columns):
    """every gradient of `out` (one column) against the closed forms from its adjoint and the resident point, on the stored patterns"""
    want = closed_forms(c, point_of(g), out["adjoint"])
    for name, M in zip("PAG", mats):
        rows, cols = M.indices, np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
        arr, scale = want[name]
        assert out[name].shape == (M.nnz,), name
        assert np.abs(out[name] - arr[rows, cols]).max() <= 8 * EPS * scale if M.nnz else True, (name, np.abs(out[name] - arr[rows, cols]).max(), scale)
    for name in "qbh":
        arr, scale = want[name]
        assert out[name].shape == arr.shape and (np.abs(out[name] - arr).max() <= 8 * EPS * scale if arr.size else True), name


@pytest.mark.parametrize("case", dc.DIFFERENTIATE, ids=dc.DIFFERENTIATE_IDS)
def test_differentiate_in_both_directions_against_the_oracle(differentiate_references, case):
    ref = differentiate_references(case)
    prob, S = ref["prob"], ref["S"]
    g, mats = conic_handle(prob, ref["pt"], dc.INTERIOR)
    got = g.differentiate(ref["J"])
    print("%s: N = %d, columns %d, |S| = %.2e, |S_gpu - S| = %.2e" % (case, g.N, prob.np, np.abs(S).max(), np.abs(got - S).max()))
    assert got.shape == S.shape and np.abs(got - S).max() <= 1e-8 * max(1.0, np.abs(S).max())
    assert g.differentiate_info() == dict(columns=prob.np, rounds=0, failed_columns=0, final_norm=0.0)
    v = np.random.default_rng(9).standard_normal(g.N)
    out = g.vjp(v, qp="PqAbGh")
    stacked = np.concatenate([out["q"], out["b"], out["h"]])      # theta = [dq; db; dh] moves q, b, h themselves
    bound = 1e-8 * max(1.0, np.abs(S).max()) * np.abs(v).sum()
    print("%s: |[q; b; h] - S'v| = %.2e, bound %.2e" % (case, np.abs(stacked - S.T @ v).max(), bound))
    assert np.abs(stacked - S.T @ v).max() <= bound
    assert g.vjp_info() == dict(columns=1, rounds=0, failed_columns=0, final_norm=0.0)
    check_closed_forms(g, mats, prob.c, out, 1)
    # the handle's own letters: Lxx, gx, hx on their patterns
    own = g.vjp(v, adjoint=False, qp="LgH")
    x, lam = point_of(g), out["adjoint"]
    Lxx = sp.csc_matrix(prob.c * (mats[0] + mats[0].T)); Lxx.sort_indices()
    rows, cols = Lxx.indices, np.repeat(np.arange(g.nx), np.diff(Lxx.indptr))
    want_L = -lam[:g.nx][rows] * x.variables[cols]
    assert own["L"].shape == (Lxx.nnz,) and np.abs(own["L"] - want_L).max() <= 8 * EPS * np.abs(lam[:g.nx]).max() * np.abs(x.variables).max()
    assert np.array_equal(own["g"], out["A"]) and np.array_equal(own["H"], -out["G"])
    # grad_P is symmetric to the bit wherever P's pattern is
    dense = np.zeros((g.nx, g.nx)); dense[mats[0].indices, np.repeat(np.arange(g.nx), np.diff(mats[0].indptr))] = out["P"]
    assert np.array_equal(dense, dense.T)
    # a k axis: columns 0 and 1 of two cotangents are the single calls'
    V = np.stack([v, np.random.default_rng(10).standard_normal(g.N)], axis=1)
    two = g.vjp(V, qp="qA")
    assert two["adjoint"].shape == (g.N, 2) and two["q"].shape == (g.nx, 2) and two["A"].shape == (mats[1].nnz, 2)
    assert np.abs(two["adjoint"][:, 0] - out["adjoint"]).max() <= 1e-8 * max(1.0, np.abs(out["adjoint"]).max())


def test_matrix_gradients_against_a_problem_whose_parameters_move_them(oracle_mod):
    base, pt, lam = pr.staged_conic_qp(oracle_mod.splitmix_uniform, 0, *dc.DIRECTIONAL)
    D_P, D_A, D_G = dc.pattern_directions(base, 12)
    o = dc.differentiated_oracle(oracle_mod, DirectionalQP(base, D_P, D_A, D_G), pt, lam, dc.INTERIOR)
    S = o.mat("solution_sensitivity", o.N, 3)
    g, mats = conic_handle(base, pt, dc.INTERIOR)
    v = np.random.default_rng(13).standard_normal(g.N)
    want = S.T @ v
    bound = 1e-8 * max(1.0, np.abs(S).max()) * np.abs(v).sum()
    on_pattern = lambda M, D: D[M.indices, np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))]
    out = g.vjp(v, adjoint=False, qp="PAGLgH")
    got = np.array([(out["P"] * on_pattern(mats[0], D_P)).sum(), (out["A"] * on_pattern(mats[1], D_A)).sum(), (out["G"] * on_pattern(mats[2], D_G)).sum()])
    Lxx = sp.csc_matrix(base.c * (mats[0] + mats[0].T)); Lxx.sort_indices()
    # Lxx = c (P + P') moves along c (D_P + D_P'), gx = A along D_A, hx = -G along -D_G
    own = np.array([(out["L"] * on_pattern(Lxx, base.c * (D_P + D_P.T))).sum(), (out["g"] * on_pattern(mats[1], D_A)).sum(), (out["H"] * on_pattern(mats[2], -D_G)).sum()])
    print("<grad, D> for P, A, G: %s; for Lxx, gx, hx: %s; oracle %s, bound %.2e" % (got, own, want, bound))
    assert np.abs(want).min() > 1e3 * bound            # (the three derivatives are far from zero: a dropped term or a wrong sign cannot pass)
    assert np.abs(got - want).max() <= bound and np.abs(own - want).max() <= bound


def test_a_superset_pattern_with_stored_zeros_gives_the_same_gradients(block_references):
    ref = block_references(dc.INERT)
    prob, w = ref["prob"], ref["w"]
    exact, wide = kc.sparse_inputs(prob), kc.sparse_inputs(prob, extra=np.random.default_rng(1))
    assert all(a.nnz > b.nnz for a, b in zip(wide, exact))
    outs = []
    for inputs, extra in ((exact, None), (wide, np.random.default_rng(1))):
        g = block_handle(prob, w, extra=extra)
        g.attach_qp(prob.q, prob.b, prob.h)
        outs.append(g.vjp(np.random.default_rng(3).standard_normal(g.N), qp="LqgbHh"))
    assert np.abs(outs[0]["adjoint"] - outs[1]["adjoint"]).max() <= 1e-8 * max(1.0, np.abs(outs[0]["adjoint"]).max())
    for name, a, b in zip("LgH", exact, wide):
        dense = lambda M, vals: sp.csc_matrix((vals, M.indices, M.indptr), shape=M.shape).toarray()
        shared = a.toarray() != 0.0
        ga, gb = dense(a, outs[0][name]), dense(b, outs[1][name])
        assert shared.sum() == a.nnz and np.abs(ga[shared]).max() > 0.0
        assert np.abs(ga[shared] - gb[shared]).max() <= 1e-8 * max(1.0, np.abs(ga).max()), name
    for name in "qbh":
        assert np.abs(outs[0][name] - outs[1][name]).max() <= 1e-8 * max(1.0, np.abs(outs[0][name]).max())


# ---- 3. the correction rounds ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.REFINEMENT)
def test_the_rounds_against_the_oracles_H(block_references, name):
    ref = block_references(name)
    prob, H, M = ref["prob"], ref["H"], ref["M"]
    g = block_handle(prob, ref["w"])
    g.attach_qp(prob.q, prob.b, prob.h)
    V = dc.refinement_cotangents(g.N)
    defect = lambda out: np.abs(H.T @ out["adjoint"] - V).max(axis=0)
    off = g.vjp(V, qp="qbh")
    assert g.vjp_info() == dict(columns=3, rounds=0, failed_columns=0, final_norm=0.0)
    g.set_option("differentiate_refinement", 1)
    on = g.vjp(V, qp="qbh")
    info = g.vjp_info()
    d_off, d_on = defect(off), defect(on)
    print("%s: |H' lam - v| off %s, on %s, %s" % (name, ["%.1e" % v for v in d_off], ["%.1e" % v for v in d_on], info))
    assert info["columns"] == 3 and info["rounds"] >= 1 and info["failed_columns"] == 0
    for j in range(3):
        assert d_on[j] <= ref["tolerance"] and d_on[j] <= d_off[j], (j, d_on, d_off)
    bound = 1e-8 * max(1.0, np.abs(M).max())
    for out in (off, on):      # the adjoint against the oracle's map, and the vector gradients, which are its parts
        assert np.abs(out["adjoint"] - M.T @ V).max() <= bound
        lam = out["adjoint"]
        oy, oz = g.nx + g.ne + g.nc, g.nx + 2 * g.ne + g.nc
        assert np.array_equal(out["q"], -lam[:g.nx]) and np.array_equal(out["b"], lam[oy:oy + g.ne]) and np.array_equal(out["h"], -lam[oz:oz + g.nc])
    # forward: the rounds against H
    J = np.random.default_rng(18).standard_normal((g.N, 2))
    S = g.differentiate(J)
    finfo = g.differentiate_info()
    assert finfo["columns"] == 2 and finfo["rounds"] >= 1 and finfo["failed_columns"] == 0
    assert np.abs(H @ S + J).max() <= ref["tolerance"]
    assert np.abs(S + M @ J).max() <= bound
    g.set_option("differentiate_refinement", 0)
    pkg = load_pkg()
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.set_option("differentiate_refinement", 2)
    assert "differentiate_refinement is 0 or 1" in str(e.value)


def test_a_second_order_cone_leaves_the_option_inert(block_references):
    ref = block_references(dc.INERT)
    g = block_handle(ref["prob"], ref["w"])
    V = dc.refinement_cotangents(g.N)
    off, S_off = g.vjp(V)["adjoint"], g.differentiate(V)
    g.set_option("differentiate_refinement", 1)
    on, S_on = g.vjp(V)["adjoint"], g.differentiate(V)
    assert np.array_equal(on, off) and np.array_equal(S_on, S_off) and np.abs(off).max() > 0.0
    assert g.vjp_info()["rounds"] == 0 and g.differentiate_info()["rounds"] == 0


# ---- 4. a whole solve, and the layer -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solved(oracle_mod):
    """the whole-solve problem, a handle that solved it, and the oracle differentiated at the handle's own point and scalars with its cone Jacobians formed at the
    handle's differentiate slacks (the regularisation: the handle has no getter for (ep, ed); they are the oracle's own, where its solve of the same problem ends —
    the walk the two share is pinned by test_gpu_sparse_kkt.py)"""
    shape, pid = dc.WHOLE_SOLVE
    base = sc.problem(oracle_mod.splitmix_uniform, shape, pid)
    prob = dc.parametric(base)
    own = dc.oracle_whole_solve(oracle_mod, prob)
    assert own["status"] == 1 and own["lu_fallbacks"] == 0
    g, mats = conic_handle(base)
    g.initialize(np.zeros(base.nx))
    status, info = g.solve()
    assert status == 1
    w, slacks = g.get("solution"), g.get("differentiate_slacks")
    scalars = dict(kappa=info["central_path"], rho=info["penalty"], ep=own["scalars"]["ep"], ed=own["scalars"]["ed"])
    pt = dc.split(w, base.nx, base.ne, base.nc)
    o = dc.differentiated_oracle(oracle_mod, prob, pt, g.get("dual"), scalars, slacks=slacks)
    D = dc.pattern_directions(base, 12)
    od = dc.differentiated_oracle(oracle_mod, DirectionalQP(base, *D), pt, g.get("dual"), scalars, slacks=slacks)
    return dict(base=base, g=g, mats=mats, info=info, w=w, slacks=slacks, S=o.mat("solution_sensitivity", o.N, prob.np).copy(), D=D,
                S_directional=od.mat("solution_sensitivity", od.N, 3).copy(), own=own)


def test_a_whole_solve_then_vjp_against_the_oracle(solved):
    base, g, mats, S = solved["base"], solved["g"], solved["mats"], solved["S"]
    nc = base.nc
    # the slacks are those of the iterate before the last accepted one, not the solution's own
    s_own, t_own = solved["w"][g.nx + g.ne:g.nx + g.ne + nc], solved["w"][-nc:]
    assert solved["slacks"].shape == (2 * nc,) and not np.array_equal(solved["slacks"], np.concatenate([s_own, t_own]))
    assert np.abs(solved["slacks"] - solved["own"]["slacks"]).max() <= 1e-8 * max(1.0, np.abs(solved["own"]["slacks"]).max())
    v = np.random.default_rng(9).standard_normal(g.N)
    out = g.vjp(v, qp="PqAbGh")
    bound = 1e-8 * max(1.0, np.abs(S).max()) * np.abs(v).sum()
    stacked = np.concatenate([out["q"], out["b"], out["h"]])
    print("whole solve: |[q; b; h] - S'v| = %.2e, bound %.2e, |S| = %.2e" % (np.abs(stacked - S.T @ v).max(), bound, np.abs(S).max()))
    assert np.abs(stacked - S.T @ v).max() <= bound
    check_closed_forms(g, mats, base.c, out, 1)
    on_pattern = lambda M, D: D[M.indices, np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))]
    got = np.array([(out[n] * on_pattern(M, D)).sum() for n, M, D in zip("PAG", mats, solved["D"])])
    Sd = solved["S_directional"]
    want, bound_d = Sd.T @ v, 1e-8 * max(1.0, np.abs(Sd).max()) * np.abs(v).sum()
    print("whole solve: <grad, D> %s, oracle %s, bound %.2e" % (got, want, bound_d))
    assert np.abs(got - want).max() <= bound_d
    dense = np.zeros((g.nx, g.nx)); dense[mats[0].indices, np.repeat(np.arange(g.nx), np.diff(mats[0].indptr))] = out["P"]
    assert np.array_equal(dense, dense.T) and np.abs(dense).max() > 0.0
    # after set("solution") the slacks are the resident point's own
    g.set("solution", solved["w"])
    assert np.array_equal(g.get("differentiate_slacks"), np.concatenate([s_own, t_own]))


def test_repetition_and_the_solve_is_left_alone(solved):
    base = solved["base"]
    g, _ = conic_handle(base)
    g.initialize(np.zeros(base.nx))
    status, info = g.solve()
    first_solution = g.get("solution")
    v = np.random.default_rng(21).standard_normal((g.N, 5))
    a = g.vjp(v, qp="PqAbGh")
    held = g.differentiate_bytes()
    b = g.vjp(v, qp="PqAbGh")
    assert g.differentiate_bytes() == held > 0                           # the second call allocates nothing
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert g.vjp_info() == dict(columns=5, rounds=0, failed_columns=0, final_norm=0.0) and g.vjp_times()["device"] > 0.0
    g.initialize(np.zeros(base.nx))
    again, info2 = g.solve()
    assert (again, info2["host_waits"], info2["total_iterations"]) == (status, info["host_waits"], info["total_iterations"]) and status == 1
    assert np.array_equal(g.get("solution"), first_solution)
    assert np.array_equal(first_solution, solved["w"]) and info["host_waits"] == solved["info"]["host_waits"]


def test_buffers_that_grow_give_a_fresh_handles_bits(block_references, solved):
    """the column workspace and the trace are grown on demand and kept: what comes out of a buffer that grew is what a fresh handle gives"""
    ref = block_references(dc.INERT)                                     # nx 12
    B = np.random.default_rng(5).standard_normal((ref["M"].shape[0], 5))
    g, held = block_handle(ref["prob"], ref["w"]), []
    for k in (1, 5, 2):
        got = g.solve_columns(B[:, :k])
        held.append(g.differentiate_bytes())
    assert np.array_equal(got, block_handle(ref["prob"], ref["w"]).solve_columns(B[:, :2]))
    assert 0 < held[0] < held[1] == held[2]                              # grew once, did not shrink
    base = solved["base"]

    def traced(*rows):
        h, _ = conic_handle(base)
        for r in rows:
            h.keep_trace(r)
        h.initialize(np.zeros(base.nx))
        status, info = h.solve()
        assert status == 1 and info["accepted_iterates"] > 5
        return h.trace()
    grown, want = traced(2, 5), traced(5)
    assert grown.shape == want.shape == (5, solved["w"].size) and np.array_equal(grown, want) and np.abs(want[4]).max() > 0.0


def test_sparse_qp_layer_gradients_against_the_oracle(solved):
    from calipso_jl_amd.torch_layer import SparseQPLayer
    base, mats, S = solved["base"], solved["mats"], solved["S"]
    c = np.random.default_rng(31).standard_normal(base.nx)
    values = [mats[0].data, base.q, mats[1].data, base.b, mats[2].data, base.h]
    grads = {}
    for where in ("cpu", "cuda:0"):
        g, _ = conic_handle(base)
        T = [torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, device=where, requires_grad=True) for a in values]
        with warnings.catch_warnings():
            warnings.simplefilter("error")                               # the solve converges: no warning, no NaN
            x = SparseQPLayer.apply(g, *T)
            (torch.tensor(c, dtype=torch.float64, device=where) * x).sum().backward()
        assert x.shape == (base.nx,) and x.device.type == where[:4]
        assert all(t.grad is not None and t.grad.shape == t.shape and t.grad.device == t.device for t in T)
        assert np.array_equal(x.detach().cpu().numpy(), solved["w"][:base.nx])
        grads[where] = [t.grad.cpu().numpy() for t in T]
    assert all(np.array_equal(a, b) for a, b in zip(grads["cpu"], grads["cuda:0"]))      # the device route has the host route's bits
    v = np.zeros(S.shape[0]); v[:base.nx] = c
    want, bound = S.T @ v, 1e-8 * max(1.0, np.abs(S).max()) * np.abs(v).sum()
    got = np.concatenate([grads["cpu"][i] for i in (1, 3, 5)])
    print("SparseQPLayer: |[grad q; b; h] - S'v| = %.2e, bound %.2e" % (np.abs(got - want).max(), bound))
    assert np.abs(got - want).max() <= bound
    on_pattern = lambda M, D: D[M.indices, np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))]
    Sd = solved["S_directional"]
    got_d = np.array([(grads["cpu"][i] * on_pattern(M, D)).sum() for i, M, D in zip((0, 2, 4), mats, solved["D"])])
    assert np.abs(got_d - Sd.T @ v).max() <= 1e-8 * max(1.0, np.abs(Sd).max()) * np.abs(v).sum()


def test_a_solve_that_does_not_converge_gives_nan_gradients(solved):
    from calipso_jl_amd.torch_layer import SparseQPLayer
    base, mats = solved["base"], solved["mats"]
    g, _ = conic_handle(base, options=dict(max_outer_iterations=1, max_residual_iterations=1))
    T = [torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=True) for a in (mats[0].data, base.q, mats[1].data, base.b, mats[2].data, base.h)]
    x = SparseQPLayer.apply(g, *T)
    with pytest.warns(UserWarning, match="did not converge"):
        x.sum().backward()
    assert all(torch.isnan(t.grad).all() for t in T)


# ---- 5. the device route and the refusals ----------------------------------------------------------------------------------------------------------------------------
def test_the_device_route_gives_the_bits_of_the_host_route(block_references):
    ref = block_references(dc.INERT)
    prob = ref["prob"]
    g = block_handle(prob, ref["w"])
    g.attach_qp(prob.q, prob.b, prob.h)
    V = dc.refinement_cotangents(g.N)
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0")
    for host, device in ((g.solve_columns(V), g.solve_columns(dev(V))), (g.solve_columns(V[:, 0], transposed=True), g.solve_columns(dev(V[:, 0]), transposed=True)),
                         (g.differentiate(V), g.differentiate(dev(V)))):
        assert device.is_cuda and device.shape == host.shape and np.array_equal(device.cpu().numpy(), host)
    g.factorize(kc.EP, kc.ED)
    host, device = g.vjp(V, qp="LqgbHh"), g.vjp(dev(V), qp="LqgbHh")
    assert sorted(host) == sorted(device)
    for k in host:
        assert device[k].is_cuda and device[k].shape == host[k].shape and np.array_equal(device[k].cpu().numpy(), host[k]), k
    pkg = load_pkg()
    with pytest.raises(pkg.CalipsoHipError) as e:                        # a host pointer in a device entry: refused, naming the argument
        g._check(g._L.calipso_hip_sparse_kkt_differentiate_adjoint_device(g._h, 1, torch.zeros(g.N, dtype=torch.float64).data_ptr(), None, None), "adjoint_device")
    assert "calipso_hip_sparse_kkt_differentiate_adjoint_device: cotangent is not device memory" in str(e.value)
    assert np.array_equal(g.vjp(V, qp="q")["q"], host["q"])              # ... and the handle is as it was


def test_refusals_name_the_argument_and_leave_the_handle_usable(block_references):
    import ctypes as C
    pkg = load_pkg()
    ref = block_references("staged_2_3_1_1_0_3")
    prob = ref["prob"]
    q, dims = kc.cone_layout(prob)
    Lxx, gx, hx = kc.sparse_inputs(prob)
    g = pkg.SparseKKT(Lxx, gx, hx, n_nonnegative=q, second_order_dims=dims)
    v = np.ones(g.N)
    L, pd = g._L, lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out = np.zeros(g.N)
    raw = lambda rc: g._check(rc, "entry")
    cases = [
        (lambda: g.vjp(v), "no Lxx resident"),                                                                   # no values resident
        (lambda: g.differentiate(v), "no Lxx resident"),
        (lambda: g.solve_columns(v), "factorize first"),
    ]
    for call, word in cases:
        with pytest.raises(pkg.CalipsoHipError) as e:
            call()
        assert "(-4)" in str(e.value) and word in str(e.value), (word, str(e.value))
    g.set_values(Lxx, gx, hx, ref["w"], kc.RHO, central_path=kc.KAPPA)
    g.factorize(kc.EP, kc.ED)
    grad = (C.POINTER(C.c_double) * 6)(None, pd(np.zeros(g.nx)), None, None, None, None)
    cases = [
        (lambda: raw(L.calipso_hip_sparse_kkt_solve_columns(g._h, 0, 0, pd(v), pd(out))), "k: at least one column"),
        (lambda: raw(L.calipso_hip_sparse_kkt_differentiate(g._h, -1, pd(v), pd(out))), "k: at least one column"),
        (lambda: raw(L.calipso_hip_sparse_kkt_differentiate_adjoint(g._h, 65536, pd(v), pd(out), None)), "k: at most 65535 columns"),
        (lambda: raw(L.calipso_hip_sparse_kkt_solve_columns(g._h, 1, 0, None, pd(out))), "B is NULL"),
        (lambda: raw(L.calipso_hip_sparse_kkt_solve_columns(g._h, 1, 0, pd(v), None)), "X is NULL"),
        (lambda: raw(L.calipso_hip_sparse_kkt_differentiate(g._h, 1, None, pd(out))), "jacobian_parameters is NULL"),
        (lambda: raw(L.calipso_hip_sparse_kkt_differentiate(g._h, 1, pd(v), None)), "sensitivity is NULL"),
        (lambda: raw(L.calipso_hip_sparse_kkt_differentiate_adjoint(g._h, 1, None, pd(out), None)), "cotangent is NULL"),
        (lambda: raw(L.calipso_hip_sparse_kkt_differentiate_adjoint(g._h, 1, pd(v), pd(out), grad)), "grad: no QP attached"),
        (lambda: g.vjp(v, qp="P"), None),
    ]
    for call, word in cases:
        with pytest.raises((pkg.CalipsoHipError, ValueError)) as e:
            call()
        if word:
            assert "(-4)" in str(e.value) and word in str(e.value), (word, str(e.value))
    lam = g.vjp(v)["adjoint"]                                            # a refused call leaves the handle usable
    assert np.abs(lam - ref["M"].T @ v).max() <= 1e-8 * max(1.0, np.abs(ref["M"]).max())
    # grad without a resident point: a handle with the QP attached and values, but no w
    h = pkg.SparseKKT(Lxx, gx, hx, n_nonnegative=q, second_order_dims=dims)
    h.set_values(Lxx, gx, hx, penalty=kc.RHO)
    h.attach_qp(prob.q, prob.b, prob.h)
    with pytest.raises(pkg.CalipsoHipError) as e:
        h.vjp(np.ones(h.N), qp="q")
    assert "(-4)" in str(e.value) and ("no w resident" in str(e.value) or "grad: no point resident" in str(e.value))
