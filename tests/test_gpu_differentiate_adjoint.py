"""differentiate! in reverse mode on a Solver handle (calipso_hip_differentiate_adjoint, csrc/api.hip + csrc/columns.hip + csrc/adjoint.hip + the wide-cone kernels of csrc/soc_wide.hip):
Solver.vjp against the ORACLE's forward maps — search_direction_symmetric! column by column at interior points (the transposed map itself, every cone branch), the
sensitivities of differentiate! at solutions (grad_theta = S' v, with and without the correction rounds against H'), the multifrontal factor, the QP data gradients
(closed forms, signs against a parametric handle, P / A / G against a problem whose parameters move them) and torch_layer.SolverQPLayer.

Bounds.  1e-8 relative to max(1, |M|) is the project's step tolerance against the oracle (a wrong term of the transposed map gives errors of order one).  For
grad_theta the forward's entrywise bound |S_gpu - S_cpu| <= 1e-8 max(1, |S_cpu|) carried through the contraction with a cotangent v: |S' v| moves by at most that
times ||v||_1."""
import warnings

import numpy as np
import pytest

import problems as pr
from helpers import interior_point, load_pkg, make_oracle, make_pair
from test_gpu_differentiate_refined import CASES, SCALARS, handle_point, pair_at_solution, rel

pytestmark = pytest.mark.gpu

INTERIOR = dict(kappa=0.17, rho=52.0, ep=0.05, ed=0.03)      # the scalars of test_smallnewton_adjoint_cpu
# (nx, ne, n_nn, n_soc, soc_dim): nonnegative only; no cones; no equalities; dimension 3 and 4 (the register branch, 4 its last); 5 (the first wide cone); 70 (two elements per lane)
LAYOUTS = [(10, 4, 6, 0, 0), (12, 5, 0, 0, 0), (9, 0, 2, 2, 3), (12, 5, 3, 2, 3), (16, 5, 0, 3, 4), (14, 6, 4, 1, 5), (20, 4, 2, 1, 70)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_transposed_map_against_the_oracles_forward_map(oracle_mod, layout):
    nx, ne, nnn, nsoc, sdim = layout
    prob = pr.parametric_conic_qp(nx, ne, nnn, nsoc, sdim, seed=900 + nx)
    pt, lam = interior_point(prob, seed=5, tail=0.05 if sdim > 16 else 0.3)
    o, g = make_pair(oracle_mod, prob, pt, lam, **INTERIOR)
    o.cone(product=True, jacobian=True, target=True)
    g.cone(product=True, jacobian=True, target=True)
    o.residual_jacobian_variables(); o.residual_jacobian_variables_symmetric()
    N = o.N
    M = np.zeros((N, N))
    for j in range(N):                                       # M column by column, factored once
        o.buf("residual")[:] = 0.0
        o.buf("residual")[j] = 1.0
        o.search_direction_symmetric(0, fact=(j == 0))
        M[:, j] = o.buf("step")
    Lam = g.vjp(np.eye(N), theta=False)["adjoint"]          # ONE call, k = N unit cotangents: column j = M' e_j
    err = np.abs(Lam - M.T).max()
    print("%s: N = %d, |M| = %.2e, |Lambda - M'| = %.2e" % (layout, N, np.abs(M).max(), err))
    assert err <= 1e-8 * max(1.0, np.abs(M).max())
    assert g.vjp_info() == dict(columns=N, rounds=0, failed_columns=0, final_norm=0.0)


def dense_H(g):
    E = np.eye(g.N)
    return np.stack([g.jacobian_variables_mul(E[:, j]) for j in range(g.N)], axis=1)


def check_grad_theta_against_oracle(prob, o, g, name, single_column=False):
    """(every case here has a symmetric Lagrangian Hessian — QPs, the cart-pole's —, so Lxx' X_x in the rounds' residual, the transposed dense GEMM and the transposed
    block product k_bgemm_l<true>, cannot be told from Lxx X_x by these tests: of H' only the swapped (s, t) rows of k_refine_rows_multi<true> are pinned, by the
    |H' lambda - v| <= tolerance assertion below)"""
    S_cpu = o.mat("solution_sensitivity", o.N, prob.np)
    V = np.random.default_rng(17).standard_normal((o.N, 3))
    want = S_cpu.T @ V
    bound = lambda j: 1e-8 * max(1.0, np.abs(S_cpu).max()) * np.abs(V[:, j]).sum()
    off = g.vjp(V)
    assert g.vjp_info() == dict(columns=3, rounds=0, failed_columns=0, final_norm=0.0)
    H = dense_H(g)
    defect = lambda out: np.abs(H.T @ out["adjoint"] - V).max(axis=0)
    g.set_option("differentiate_refinement", 1)
    on = g.vjp(V)
    info = g.vjp_info()
    d_off, d_on = defect(off), defect(on)
    print("%s: N = %d, p = %d, |S| = %.2e; option off: errors %s, |H' lam - v| %s; on: errors %s, |H' lam - v| %s, %s" % (
        name, o.N, prob.np, np.abs(S_cpu).max(), ["%.1e" % np.abs(off["theta"][:, j] - want[:, j]).max() for j in range(3)], ["%.1e" % v for v in d_off],
        ["%.1e" % np.abs(on["theta"][:, j] - want[:, j]).max() for j in range(3)], ["%.1e" % v for v in d_on], info))
    for out in (off, on):
        assert out["theta"].shape == (prob.np, 3) and out["adjoint"].shape == (o.N, 3)
        for j in range(3):
            assert np.abs(out["theta"][:, j] - want[:, j]).max() <= bound(j), (j, np.abs(out["theta"][:, j] - want[:, j]).max(), bound(j))
    assert info["columns"] == 3 and info["rounds"] >= 1 and info["failed_columns"] == 0
    tol = g.scalar("opt.iterative_refinement_tolerance")
    for j in range(3):
        assert d_on[j] <= tol, (j, d_on, tol)
        assert d_on[j] <= d_off[j], (j, d_on, d_off)
    if single_column:
        # one cotangent takes the triangular solve and the mat-vecs of a Newton step instead of the GEMM forms: the same map, so column 0 again, to the project's step
        # tolerance (the two paths sum in different orders), with the option off and on
        for opt, ref in ((0, off), (1, on)):
            g.set_option("differentiate_refinement", opt)
            one = g.vjp(V[:, 0])
            assert one["adjoint"].shape == (o.N,) and one["theta"].shape == (prob.np,)
            err = np.abs(one["adjoint"] - ref["adjoint"][:, 0]).max()
            print("%s: k = 1 against column 0 of k = 3, option %d: |lambda| = %.2e, difference %.2e" % (name, opt, np.abs(ref["adjoint"][:, 0]).max(), err))
            assert err <= 1e-8 * max(1.0, np.abs(ref["adjoint"][:, 0]).max())
            assert np.abs(one["theta"] - want[:, 0]).max() <= bound(0)
            assert g.vjp_info()["columns"] == 1 and g.vjp_info()["failed_columns"] == 0


@pytest.mark.parametrize("name", [k for k in CASES if "stage_parallel" not in k])
def test_grad_theta_against_the_oracles_sensitivities(oracle_mod, name):
    prob, o, g = pair_at_solution(oracle_mod, name)
    check_grad_theta_against_oracle(prob, o, g, name)


def test_stage_parallel_factor_takes_the_cotangents(oracle_mod):
    name = "qp70_20_6_stage_parallel"
    prob, o, g = pair_at_solution(oracle_mod, name)
    g.analyze_structure()
    g.set_stage_parallel(True)
    check_grad_theta_against_oracle(prob, o, g, name, single_column=True)


def test_second_order_cones_leave_the_option_inert(oracle_mod):
    prob = pr.parametric_conic_qp(20, 8, 4, 2, 3, seed=20)
    pt, lam = interior_point(prob, 3)
    o, g = make_pair(oracle_mod, prob, pt, lam, ep=1e-5, ed=1e-5)
    g.cone(product=True, jacobian=True, target=True)
    V = np.random.default_rng(4).standard_normal((g.N, 3))
    off = g.vjp(V)
    g.set_option("differentiate_refinement", 1)
    on = g.vjp(V)
    assert np.array_equal(on["adjoint"], off["adjoint"]) and np.array_equal(on["theta"], off["theta"])
    assert np.abs(off["adjoint"]).max() > 0.0
    assert g.vjp_info()["rounds"] == 0


# ---- QP data gradients ---------------------------------------------------------------------------------------------------------------------------
QP_SHAPE = (12, 5, 6, 0, 0)


def qp_handle(pkg, prob, pt, lam, sc):
    """a qp_attach'ed handle holding prob's QP at the point pt with the scalars sc, evaluated, cone Jacobians formed"""
    h = pkg.Solver(prob, prob.nx, 0, prob.ne, prob.nc, nonnegative_indices=prob.nonnegative_indices, second_order_indices=prob.second_order_indices)
    for field, kw in SCALARS:
        h.set(field, [sc[kw]])
    h.set("solution", np.concatenate([pt[k] for k in "xrsyzt"]))
    if prob.ne:
        h.set("dual", lam)
    h.qp_attach(prob.P, prob.q, prob.A, prob.b, prob.G, prob.h, prob.c)
    h.qp_evaluate(pr.ALL_VARIABLE_FLAGS, 0)
    h.cone(product=True, jacobian=True, target=True)
    return h


def closed_forms(c, w, lam):
    """the closed forms of the data gradients from lambda (N,) and the point w (a _Point): dict name -> (array, scale of its products)"""
    x, y, z = w.variables, w.equality_dual, w.cone_dual
    nx, ne, nc = x.size, y.size, z.size
    lx, ly, lz = lam[:nx], lam[nx + ne + nc:nx + 2 * ne + nc], lam[nx + 2 * ne + nc:nx + 2 * ne + 2 * nc]
    mx = lambda a: np.abs(a).max() if a.size else 0.0
    return dict(P=(-c * (np.outer(lx, x) + np.outer(x, lx)), 2 * c * mx(lx) * mx(x)), q=(-lx, mx(lx)),
                A=(-(np.outer(ly, x) + np.outer(y, lx)), mx(ly) * mx(x) + mx(y) * mx(lx)), b=(ly, mx(ly)),
                G=(np.outer(lz, x) + np.outer(z, lx), mx(lz) * mx(x) + mx(z) * mx(lx)), h=(-lz, mx(lz)))


def interior_state(seed=300):
    prob = pr.parametric_conic_qp(*QP_SHAPE, seed=seed)
    pt, lam = interior_point(prob, seed=5)
    return prob, pt, lam, dict(kappa=0.17, rho=52.0, ep=0.05, ed=0.03, tau=0.99)


def test_qp_data_gradients_are_the_closed_forms():
    pkg = load_pkg()
    prob, pt, lam, sc = interior_state()
    h = qp_handle(pkg, prob, pt, lam, sc)
    eps = np.finfo(np.float64).eps
    rng = np.random.default_rng(8)
    for V in (rng.standard_normal(h.N), rng.standard_normal((h.N, 2))):      # one column (the mat-vec / triangular-solve path) and a k axis
        out = h.vjp(V, theta=False, qp=True)
        cols = [(out, V)] if V.ndim == 1 else [({k: a[..., j] for k, a in out.items()}, V[:, j]) for j in range(V.shape[1])]
        for o_j, _ in cols:
            want = closed_forms(prob.c, h.solution, o_j["adjoint"])
            for name in "PqAbGh":
                arr, scale = want[name]
                assert o_j[name].shape == arr.shape, name
                assert np.abs(o_j[name] - arr).max() <= 8 * eps * scale, (name, np.abs(o_j[name] - arr).max(), scale)
            assert np.array_equal(o_j["P"], o_j["P"].T)
    some = h.vjp(V, adjoint=False, theta=False, qp="hA")                      # a subset, in any order
    assert sorted(some) == ["A", "h"] and np.array_equal(some["A"], out["A"]) and np.array_equal(some["h"], out["h"])


def test_qp_vector_gradients_have_the_signs_of_a_parametric_handle(oracle_mod):
    """ParametricConicQP.evaluate moves the data with theta = [dq; db; dh] as q + dq, b + db, h + dh (the data THEMSELVES, whatever sign they enter the residual
    with), so d Loss / d theta = [grad_q; grad_b; grad_h], all three with a plus sign"""
    pkg = load_pkg()
    prob, pt, lam, sc = interior_state()
    h = qp_handle(pkg, prob, pt, lam, sc)
    o, g = make_pair(oracle_mod, prob, pt, lam, **sc)
    o.buf("parameters")[:] = prob.parameters
    o.cone(product=True, jacobian=True, target=True)
    g.cone(product=True, jacobian=True, target=True)
    assert o.differentiate(prob) >= 0
    S_cpu = o.mat("solution_sensitivity", o.N, prob.np)
    v = np.random.default_rng(9).standard_normal(h.N)
    bound = 1e-8 * max(1.0, np.abs(S_cpu).max()) * np.abs(v).sum()
    gth = g.vjp(v)["theta"]
    out = h.vjp(v, theta=False, qp="qbh")
    stacked = np.concatenate([out["q"], out["b"], out["h"]])
    print("signs: |theta - S'v| = %.2e, |[q; b; h] - S'v| = %.2e, bound %.2e" % (np.abs(gth - S_cpu.T @ v).max(), np.abs(stacked - S_cpu.T @ v).max(), bound))
    assert np.abs(gth - S_cpu.T @ v).max() <= bound
    assert np.abs(stacked - S_cpu.T @ v).max() <= bound
    assert np.abs(stacked - gth).max() <= 1e-8 * max(1.0, np.abs(gth).max())


class DirectionalQP(pr.ConicQP):
    """ConicQP whose matrices move with three parameters along fixed directions: P + th0 D_P (D_P symmetric), A + th1 D_A, G + th2 D_G"""

    def __init__(self, base, D_P, D_A, D_G):
        super().__init__(base.P, base.q, base.A, base.b, base.G, base.h, nonnegative_indices=base.nonnegative_indices, second_order_indices=base.second_order_indices,
                         objective_scale=base.c, name="directional_qp")
        self.D_P, self.D_A, self.D_G = D_P, D_A, D_G
        self.np = 3
        self.parameters = np.zeros(3)

    def evaluate(self, flags, x, y, z, theta, out):
        th = np.asarray(theta, dtype=np.float64)
        x = np.asarray(x); y = np.asarray(y); z = np.asarray(z)
        keep = self.P, self.A, self.G, self.Psym
        self.P, self.A, self.G = keep[0] + th[0] * self.D_P, keep[1] + th[1] * self.D_A, keep[2] + th[2] * self.D_G
        self.Psym = self.c * (self.P + self.P.T)
        try:
            super().evaluate(flags, x, y, z, theta, out)
        finally:
            self.P, self.A, self.G, self.Psym = keep
        col = lambda rows, j, v: np.stack([v if k == j else np.zeros(rows) for k in range(3)], axis=1)
        if flags & pr.OBJECTIVE_JACOBIAN_PARAMETERS:
            pr._put(out, "objective_jacobian_variables_parameters", col(self.nx, 0, self.c * (self.D_P + self.D_P.T) @ x))
        if flags & pr.EQUALITY_JACOBIAN_PARAMETERS and self.ne:
            pr._put(out, "equality_jacobian_parameters", col(self.ne, 1, self.D_A @ x))
        if flags & pr.EQUALITY_DUAL_JACOBIAN_PARAMETERS:
            pr._put(out, "equality_dual_jacobian_variables_parameters", col(self.nx, 1, self.D_A.T @ y))
        if flags & pr.CONE_JACOBIAN_PARAMETERS and self.nc:
            pr._put(out, "cone_jacobian_parameters", col(self.nc, 2, -self.D_G @ x))
        if flags & pr.CONE_DUAL_JACOBIAN_PARAMETERS:
            pr._put(out, "cone_dual_jacobian_variables_parameters", col(self.nx, 2, -self.D_G.T @ z))


def evaluated(prob, flags, x, y, z, theta):
    store = {}
    sizes = dict(objective_gradient_variables=prob.nx, equality_constraint=prob.ne, equality_dual_jacobian_variables=prob.nx, cone_constraint=prob.nc,
                 cone_dual_jacobian_variables=prob.nx, objective_jacobian_variables_parameters=prob.nx * 3, equality_jacobian_parameters=prob.ne * 3,
                 equality_dual_jacobian_variables_parameters=prob.nx * 3, cone_jacobian_parameters=prob.nc * 3, cone_dual_jacobian_variables_parameters=prob.nx * 3)
    prob.evaluate(flags, x, y, z, theta, lambda name: store.setdefault(name, np.zeros(sizes.get(name, 1))))
    return store


def test_qp_matrix_gradients_against_a_problem_whose_parameters_move_them(oracle_mod):
    pkg = load_pkg()
    base, pt, lam, sc = interior_state()
    rng = np.random.default_rng(12)
    D = rng.standard_normal((base.nx, base.nx))
    D_P, D_A, D_G = 0.5 * (D + D.T), rng.standard_normal(base.A.shape), rng.standard_normal(base.G.shape)
    prob = DirectionalQP(base, D_P, D_A, D_G)
    # its parameter Jacobians against central differences of its own evaluate (everything is linear in theta: exact up to rounding)
    x, y, z = pt["x"], pt["y"], pt["z"]
    par = (pr.OBJECTIVE_JACOBIAN_PARAMETERS | pr.EQUALITY_JACOBIAN_PARAMETERS | pr.EQUALITY_DUAL_JACOBIAN_PARAMETERS | pr.CONE_JACOBIAN_PARAMETERS |
           pr.CONE_DUAL_JACOBIAN_PARAMETERS)
    var = pr.OBJECTIVE_GRADIENT | pr.EQUALITY | pr.EQUALITY_DUAL_GRADIENT | pr.CONE | pr.CONE_DUAL_GRADIENT
    J = evaluated(prob, par, x, y, z, np.zeros(3))
    pairs = (("objective_jacobian_variables_parameters", "objective_gradient_variables"), ("equality_jacobian_parameters", "equality_constraint"),
             ("equality_dual_jacobian_variables_parameters", "equality_dual_jacobian_variables"), ("cone_jacobian_parameters", "cone_constraint"),
             ("cone_dual_jacobian_variables_parameters", "cone_dual_jacobian_variables"))
    for k in range(3):
        e = np.zeros(3); e[k] = 0.5
        up, dn = evaluated(prob, var, x, y, z, e), evaluated(prob, var, x, y, z, -e)
        for jac, val in pairs:
            fd = up[val] - dn[val]
            rows = fd.size
            assert np.abs(J[jac][k * rows:(k + 1) * rows] - fd).max() <= 1e-12 * max(1.0, np.abs(fd).max()), (jac, k)
    o, g = make_pair(oracle_mod, prob, pt, lam, **sc)
    o.buf("parameters")[:] = prob.parameters
    o.cone(product=True, jacobian=True, target=True)
    assert o.differentiate(prob) >= 0
    S_cpu = o.mat("solution_sensitivity", o.N, 3)
    h = qp_handle(pkg, base, pt, lam, sc)
    v = np.random.default_rng(13).standard_normal(h.N)
    out = h.vjp(v, adjoint=False, theta=False, qp="PAG")
    got = np.array([(out["P"] * D_P).sum(), (out["A"] * D_A).sum(), (out["G"] * D_G).sum()])
    want = S_cpu.T @ v
    bound = 1e-8 * max(1.0, np.abs(S_cpu).max()) * np.abs(v).sum()
    print("<grad, D> for P, A, G: %s, oracle %s, bound %.2e" % (got, want, bound))
    assert np.abs(got - want).max() <= bound
    assert np.abs(want).min() > 1e3 * bound            # (the three derivatives are far from zero: a dropped term or a wrong sign cannot pass)


# ---- workspace, refusals, the layer --------------------------------------------------------------------------------------------------------------
def test_repetition_same_bits_and_the_forward_workspace_is_left_alone(oracle_mod):
    prob, o, g = pair_at_solution(oracle_mod, "qp24_9_11")
    g.differentiate()
    S = g.data("solution_sensitivity")
    V = np.random.default_rng(21).standard_normal((g.N, prob.np + 5))      # more columns than the forward's workspace was sized for
    first = g.vjp(V)
    info1, bytes1 = g.vjp_info(), g.device_bytes()
    second = g.vjp(V)
    assert np.array_equal(first["adjoint"], second["adjoint"]) and np.array_equal(first["theta"], second["theta"])
    assert g.device_bytes() == bytes1 and g.vjp_info() == info1
    g.differentiate()
    assert np.array_equal(g.data("solution_sensitivity"), S)


def test_refusals_name_the_argument(oracle_mod):
    pkg = load_pkg()
    prob, pt, lam, sc = interior_state()
    h = qp_handle(pkg, prob, pt, lam, sc)                   # np = 0, QP attached
    o, g = make_pair(oracle_mod, prob, pt, lam, **sc)       # parameters, no QP
    g.cone(product=True, jacobian=True, target=True)
    v = np.ones(h.N)
    for call, word in ((lambda: g.vjp(np.zeros((g.N, 0))), "k must be"), (lambda: g.vjp(None), "cotangent"), (lambda: h.vjp(v, theta=True), "grad_theta"),
                       (lambda: g.vjp(v, qp=True), "grad_qp")):
        with pytest.raises(pkg.CalipsoHipError) as e:
            call()
        assert word in str(e.value), (word, str(e.value))
    assert g.vjp(v)["theta"].shape == (prob.np,)           # a refused call leaves the handle usable


def test_solver_qp_layer_gradients_against_the_oracle(oracle_mod):
    import torch
    pkg = load_pkg()
    from calipso_jl_amd.torch_layer import SolverQPLayer
    prob = pr.parametric_conic_qp(*QP_SHAPE, seed=300)
    h = pkg.Solver(prob, prob.nx, 0, prob.ne, prob.nc, nonnegative_indices=prob.nonnegative_indices, second_order_indices=prob.second_order_indices)
    T = {k: torch.tensor(np.asarray(getattr(prob, k)), dtype=torch.float64, requires_grad=True) for k in "PqAbGh"}
    c = np.random.default_rng(31).standard_normal(prob.nx)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # the solve converges: no warning, no NaN
        x = SolverQPLayer.apply(h, T["P"], T["q"], T["A"], T["b"], T["G"], T["h"], False, prob.c)
        (torch.from_numpy(c) * x).sum().backward()
    assert x.shape == (prob.nx,) and all(T[k].grad is not None and T[k].grad.shape == T[k].shape for k in "PqAbGh")
    # the oracle differentiated at the handle's own point and fields (the procedure of test_c5_whole_solve_dense_and_structured)
    pt, lam, sc = handle_point(h)
    o = make_oracle(oracle_mod, prob, pt, lam, **sc)
    o.buf("parameters")[:] = prob.parameters
    o.buf("objective_jacobian_variables_variables")[:] = h.get("lagrangian_hessian", prob.nx * prob.nx)
    o.buf("equality_dual_jacobian_variables_variables")[:] = 0.0
    o.buf("cone_dual_jacobian_variables_variables")[:] = 0.0
    o.buf("equality_jacobian_variables")[:] = h.get("equality_jacobian_variables", prob.ne * prob.nx)
    o.cone(product=True, jacobian=True, target=True)
    assert o.differentiate(prob) >= 0
    S_cpu = o.mat("solution_sensitivity", o.N, prob.np)
    v = np.zeros(o.N); v[:prob.nx] = c
    want = S_cpu.T @ v                                      # theta = [dq; db; dh] moves q, b, h themselves
    bound = 1e-8 * max(1.0, np.abs(S_cpu).max()) * np.abs(v).sum()
    got = np.concatenate([T[k].grad.numpy() for k in "qbh"])
    print("SolverQPLayer: |[grad q; b; h] - S'v| = %.2e, bound %.2e, |S| = %.2e" % (np.abs(got - want).max(), bound, np.abs(S_cpu).max()))
    assert np.abs(got - want).max() <= bound
    gP = T["P"].grad.numpy()
    assert np.array_equal(gP, gP.T)
    lam_v = h.vjp(v, theta=False)["adjoint"]                # the same state, the same bits as the backward pass saw
    arr, scale = closed_forms(prob.c, h.solution, lam_v)["P"]
    assert np.abs(gP - arr).max() <= 8 * np.finfo(np.float64).eps * scale
