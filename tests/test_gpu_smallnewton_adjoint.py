"""GPU (-m gpu): differentiate! in reverse mode for a batch in one launch (calipso_hip_smallnewton_differentiate_adjoint, SmallNewtonBatch.vjp, torch_layer.QPLayer).
lambda = M' v for the map M of the forward differentiate!, contracted with dR/dtheta in the kernel: held to the forward mode on the same handle (the transposed map
of the same factorisation), to the ORACLE's solution_sensitivity, to closed-form dR/dtheta columns of every QP data entry, to the analytic KKT-inverse gradients of an
equality-only QP, and for the device evaluators of tests/device_eval_small to the oracle; the refusals; the PyTorch layer against vjp and gradcheck."""
import ctypes
import functools
import os
import warnings

import numpy as np
import pytest

import problems as pr
from helpers import load_pkg
from test_oracle_solve import run as run_oracle

pytestmark = pytest.mark.gpu

THREADS = [0, 64, 128, 256]
TIGHT = dict(residual_tolerance=1e-6, optimality_tolerance=1e-6, equality_tolerance=1e-6, complementarity_tolerance=1e-6, slack_tolerance=1e-6)
C5 = dict(residual_tolerance=1e-3, optimality_tolerance=1e-3, equality_tolerance=1e-3, complementarity_tolerance=1e-3, slack_tolerance=1e-3)
LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_eval_small", "libsmall_evaluators.so")


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())


@functools.lru_cache(maxsize=1)
def evlib():
    return ctypes.CDLL(LIB)


def qp_batch(pkg, layout, n, seed, threads=0, **opts):
    nx, ne, nnn, nsoc, sdim = layout
    probs = [pr.parametric_conic_qp(nx, ne, nnn, nsoc, sdim, seed=seed + k) for k in range(n)]
    sn = pkg.SmallNewtonBatch(nx, ne, probs[0].nc, n, options=dict(threads=threads, **opts))
    if nsoc:
        sn.set_cones(nnn, [sdim] * nsoc)
    st = lambda name: np.stack([np.asarray(getattr(p, name), dtype=np.float64) for p in probs])
    sn.set_qp(st("P"), st("q"), st("A"), st("b"), st("G"), st("h"), objective_scale=probs[0].c, shared=False)
    sn.initialize(np.stack([p.x0 for p in probs]))
    return sn, probs


def contract(J, lam):
    """-R_theta' lambda per instance: J (batch, N, p), lam (batch, N, k) -> (batch, p, k)"""
    return -np.einsum("bnp,bnk->bpk", J, lam)


# R+ shapes of test_gpu_smallnewton.py (C5's among them) and mixed R+ / second-order-cone layouts: (nx, ne, nonnegative, cones, cone dimension)
RPLUS = [(12, 5, 6, 0, 0), (49, 40, 0, 0, 0), (24, 9, 11, 0, 0)]
MIXED = [(12, 4, 4, 2, 3), (16, 5, 6, 1, 5), (20, 8, 4, 2, 3)]


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("layout", RPLUS + MIXED)
def test_adjoint_is_the_transpose_of_forward_mode_on_the_same_handle(layout, threads):
    """-J' adjoint equals S' v for the S = differentiate(J) of the same handle, k = 1 and k = 3.  Without second-order cones, after solve: the forward columns refine
    against H and the adjoint against H', both stop within the refinement tolerance of H^-1 and H'^-1, 1e-9.  With second-order cones neither side refines (quirk B-3):
    the same unrefined map transposed, 1e-10 — at INTERIOR points, as test_gpu_smallnewton.py's forward cone test (cold-started cone problems mostly end in the
    reference's fallback, and at what they reach the condensed matrix is so ill-conditioned that any two summation orders of the same map differ by up to 1e-3)"""
    pkg = load_pkg()
    sn, probs = qp_batch(pkg, layout, 5, 300, threads, **TIGHT)
    sn.solve()
    N, soc = sn.N, layout[3] > 0
    if soc:
        from helpers import interior_point
        pts = [interior_point(p, seed=40 + k) for k, p in enumerate(probs)]
        W = np.stack([np.concatenate([pt[f] for f in "xrsyzt"]) for pt, _ in pts])
        sn.set_state(w=W, dual=np.stack([lam for _, lam in pts]) if sn.ne else None, scalars=np.tile([0.17, 0.99, 52.0], (5, 1)))
        _, stp, _ = sn.steps(1, advance=False)                 # the cone Jacobians of a search direction at these points (quirk B-12)
        assert (stp == 0).all(), stp
    rng = np.random.default_rng(7)
    J = rng.standard_normal((5, N, 20))
    S, st, _ = sn.differentiate(J)
    for k in (1, 3):
        v = rng.standard_normal((5, N, k))
        out = sn.vjp(v, theta=False, qp=False)
        assert out["adjoint"].shape == (5, N, k) and np.array_equal(out["status"], st)
        g, ref = contract(J, out["adjoint"]), np.einsum("bnp,bnk->bpk", S, v)
        for b in range(5):
            if st[b] != 0:
                continue
            assert rel(g[b], ref[b]) <= (1e-10 if soc else 1e-9), (b, k, rel(g[b], ref[b]))
    # the short form: (batch, N) without a k axis
    v1 = rng.standard_normal((5, N))
    a1 = sn.vjp(v1, qp=False)["adjoint"]
    a3 = sn.vjp(v1[:, :, None], qp=False)["adjoint"]
    assert a1.shape == (5, N) and np.array_equal(a1, a3[:, :, 0])
    sn.close()


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("layout", [(12, 5, 6, 0, 0), (49, 40, 0, 0, 0)])
def test_adjoint_against_the_oracle(oracle_mod, layout, threads):
    """at the ORACLE's solution: -J' adjoint = solution_sensitivity' v of the oracle's differentiate!, 1e-8 (the tolerance of the forward tests)"""
    pkg = load_pkg()
    sn, probs = qp_batch(pkg, layout, 4, 300, threads, **TIGHT)
    res, _ = sn.solve()
    nx, ne, nc = sn.nx, sn.ne, sn.nc
    N, npar = sn.N, nx + ne + nc
    oy, oz = nx + ne + nc, nx + 2 * ne + nc
    J = np.zeros((4, N, npar))
    J[:, :nx, :nx] = np.eye(nx)
    J[:, oy:oy + ne, nx:nx + ne] = -np.eye(ne)
    J[:, oz:oz + nc, nx + ne:] = np.eye(nc)
    W = sn.get_state()["solution"].copy()
    So = {}
    for k, prob in enumerate(probs):
        o, status = run_oracle(oracle_mod, prob, differentiate=1, **TIGHT)
        assert status == 1 and res[k] == 1
        W[k] = o.point()["all"]
        So[k] = o.mat("solution_sensitivity", o.N, prob.np).copy()
    sn.set_state(w=W)
    v = np.random.default_rng(3).standard_normal((4, N, 2))
    out = sn.vjp(v, qp=False)
    assert (out["status"] == 0).all()
    g = contract(J, out["adjoint"])
    for k in range(4):
        ref = So[k].T @ v[k]
        assert rel(g[k], ref) <= 1e-8, (k, rel(g[k], ref))
    sn.close()


def qp_theta_columns(nx, ne, nc, c, w):
    """dR/dtheta columns, at the point w, of every entry of P (symmetric pairs), q, A, b, G, h; and how each maps onto grad_qp's entries"""
    oy, oz = nx + ne + nc, nx + 2 * ne + nc
    N = nx + 2 * ne + 3 * nc
    x, y, z = w[:nx], w[oy:oy + ne], w[oz:oz + nc]
    cols, picks = [], []
    for k in range(nx):
        for l in range(k, nx):
            col = np.zeros(N)
            col[k] += 2 * c * x[l]
            if l != k:
                col[l] += 2 * c * x[k]
            cols.append(col); picks.append([("P", (k, l))] + ([("P", (l, k))] if l != k else []))
    for i in range(nx):
        col = np.zeros(N); col[i] = 1.0
        cols.append(col); picks.append([("q", (i,))])
    for k in range(ne):
        for l in range(nx):
            col = np.zeros(N); col[l] += y[k]; col[oy + k] += x[l]
            cols.append(col); picks.append([("A", (k, l))])
    for k in range(ne):
        col = np.zeros(N); col[oy + k] = -1.0
        cols.append(col); picks.append([("b", (k,))])
    for k in range(nc):
        for l in range(nx):
            col = np.zeros(N); col[l] -= z[k]; col[oz + k] -= x[l]
            cols.append(col); picks.append([("G", (k, l))])
    for k in range(nc):
        col = np.zeros(N); col[oz + k] = 1.0
        cols.append(col); picks.append([("h", (k,))])
    return np.stack(cols, axis=1), picks


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("layout", [(6, 2, 4, 0, 0), (8, 2, 3, 1, 3)])
def test_qp_data_gradients_match_forward_mode_columns(layout, threads):
    """grad_qp against forward differentiate! fed the closed-form dR/dtheta column of every data entry (P by symmetric pairs), contracted with v: 1e-9 — after solve
    for R+, at interior points with a second-order cone (at its cold-started solution the two agree to 4e-9 only: the conditioning of the test above)"""
    pkg = load_pkg()
    sn, probs = qp_batch(pkg, layout, 3, 40, threads, **TIGHT)
    sn.solve()
    if layout[3]:
        from helpers import interior_point
        pts = [interior_point(p, seed=50 + k) for k, p in enumerate(probs)]
        sn.set_state(w=np.stack([np.concatenate([pt[f] for f in "xrsyzt"]) for pt, _ in pts]), dual=np.stack([lam for _, lam in pts]),
                     scalars=np.tile([0.17, 0.99, 52.0], (3, 1)))
        assert (sn.steps(1, advance=False)[1] == 0).all()
    w = sn.get_state()["solution"]
    nx, ne, nc, N = sn.nx, sn.ne, sn.nc, sn.N
    Js, picks = zip(*[qp_theta_columns(nx, ne, nc, probs[0].c, w[b]) for b in range(3)])
    J = np.stack(Js)
    S, st, _ = sn.differentiate(J)
    v = np.random.default_rng(5).standard_normal((3, N, 2))
    out = sn.vjp(v, adjoint=False)
    assert out["P"].shape == (3, nx, nx, 2) and out["G"].shape == (3, nc, nx, 2) and out["h"].shape == (3, nc, 2)
    fwd = np.einsum("bnp,bnk->bpk", S, v)
    for b in range(3):
        assert st[b] == 0
        got = np.stack([sum(out[name][b][idx] for name, idx in pk) for pk in picks[b]])
        assert rel(got, fwd[b]) <= 1e-9, (b, rel(got, fwd[b]))
        assert rel(out["P"][b], np.swapaxes(out["P"][b], 0, 1)) <= 1e-15       # (symmetric up to the contraction of a multiply-add)
    sn.close()


@pytest.mark.parametrize("threads", THREADS)
def test_equality_only_qp_gradients_against_the_kkt_inverse(threads):
    """nc = 0: x* solves [2cP A'; A 0] [x; y] = [-q; b]; mu = K'^-1 [v; 0] gives dq = -mu_x, db = mu_y, dA = -(mu_y x' + y mu_x'), dP = -c(mu_x x' + x mu_x').
    2e-6 (reached: 1.2e-6, in dA, whose x and y come from the solve; dq and db hold 1e-6): the penalty and regularisation the solve leaves sit at O(1e-7) of the KKT matrix (the solve starts at penalty 1e8: with the default it ends at a penalty
    of a few thousand, and the map it differentiates carries -1/penalty in the y block — 4e-4 from the KKT inverse)"""
    pkg = load_pkg()
    nx, ne, B = 7, 3, 4
    rng = np.random.default_rng(12)
    probs = [pr.parametric_conic_qp(nx, ne, 0, 0, 0, seed=60 + k) for k in range(B)]
    tol = dict(residual_tolerance=1e-10, optimality_tolerance=1e-10, equality_tolerance=1e-10, complementarity_tolerance=1e-10, slack_tolerance=1e-10)
    sn = pkg.SmallNewtonBatch(nx, ne, 0, B, options=dict(threads=threads, penalty_initial=1e8, **tol))
    st = lambda name: np.stack([np.asarray(getattr(p, name), dtype=np.float64) for p in probs])
    c = probs[0].c
    sn.set_qp(st("P"), st("q"), st("A").reshape(B, ne, nx), st("b"), np.zeros((B, 0, nx)), np.zeros((B, 0)), objective_scale=c, shared=False)
    sn.initialize(np.zeros((B, nx)))
    res, _ = sn.solve()
    assert (res == 1).all()
    v = rng.standard_normal((B, nx))
    out = sn.vjp(v)
    for b, p in enumerate(probs):
        P, A = np.asarray(p.P), np.asarray(p.A).reshape(ne, nx)
        K = np.block([[2 * c * P, A.T], [A, np.zeros((ne, ne))]])
        xy = np.linalg.solve(K, np.concatenate([-np.asarray(p.q), np.asarray(p.b)]))
        x, y = xy[:nx], xy[nx:]
        mu = np.linalg.solve(K.T, np.concatenate([v[b], np.zeros(ne)]))
        mx, my = mu[:nx], mu[nx:]
        for name, ref in (("q", -mx), ("b", my), ("A", -(np.outer(my, x) + np.outer(y, mx))), ("P", -c * (np.outer(mx, x) + np.outer(x, mx)))):
            assert rel(out[name][b], ref) <= (1e-6 if name in "qb" else 2e-6), (b, name, rel(out[name][b], ref))
    sn.close()


# ---- device evaluators ------------------------------------------------------------------------------------------------------------------------
def ev_handle(pkg, prob, symbol, thetas, cones=None, **opts):
    sn = pkg.SmallNewtonBatch(prob.nx, prob.ne, prob.nc, len(thetas), options=opts)
    if cones is not None:
        sn.set_cones(*cones)
    sn.set_evaluator(evlib(), symbol, prob.np)
    sn.set_parameters(thetas)
    sn.initialize(np.repeat(prob.x0[None], len(thetas), axis=0))
    return sn


def oracle_points(oracle_mod, prob, thetas, idx, **opts):
    W, So, ok = {}, {}, []
    for k in idx:
        prob.parameters = thetas[k].copy()
        o, status = run_oracle(oracle_mod, prob, differentiate=1, **opts)
        if status != 1 or o.stats()["lu_fallbacks"] > 0:
            continue
        W[k] = o.point()["all"].copy(); So[k] = o.mat("solution_sensitivity", o.N, prob.np).copy(); ok.append(k)
    return W, So, ok


@pytest.mark.parametrize("threads", THREADS)
def test_cartpole_gradients_and_the_autotuning_row(oracle_mod, threads):
    """C5 cart-pole, 256 instances with their own theta: grad_theta against the oracle's solution_sensitivity' v (1e-8), and the autotuning loop's question —
    cotangent e_{u_1} — against row actions[1] of the forward sensitivity"""
    import test_gpu_smallnewton_evaluator as te
    pkg = load_pkg()
    prob = te.cartpole()
    B = 256
    th = te.cartpole_thetas(B)
    sn = ev_handle(pkg, prob, "cartpole_mpc_kernels", th, threads=threads, **C5)
    res, _ = sn.solve()
    assert (res == 1).all()
    idx = list(range(0, B, B // 6))[:5] + [B - 1]
    Wo, So, ok = oracle_points(oracle_mod, prob, th, idx, **C5)
    assert len(ok) == len(idx)
    W = sn.get_state()["solution"].copy()
    for k in ok:
        W[k] = Wo[k]
    sn.set_state(w=W)
    N = sn.N
    v = np.random.default_rng(9).standard_normal((B, N, 2))
    out = sn.vjp(v)
    assert out["theta"].shape == (B, prob.np, 2) and (out["status"] == 0).all() and "P" not in out
    for k in ok:
        ref = So[k].T @ v[k]
        assert rel(out["theta"][k], ref) <= 1e-8, (k, rel(out["theta"][k], ref))
    u1 = 4                                                          # actions[1]: the first action, after the 4 states of stage 1
    e = np.zeros((B, N)); e[:, u1] = 1.0
    row = sn.vjp(e, adjoint=False)["theta"]
    S, _, _ = sn.differentiate()
    for k in range(B):
        assert rel(row[k], S[k][u1]) <= 1e-8, (k, rel(row[k], S[k][u1]))
    for k in ok:
        assert rel(row[k], So[k][u1]) <= 1e-8
    sn.close()


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("which", ["nonlinear_cone", "friction_cone"])
def test_evaluator_gradients_against_the_oracle(oracle_mod, which, threads):
    import test_gpu_smallnewton_evaluator as te
    pkg = load_pkg()
    if which == "nonlinear_cone":
        prob, th, cones = te.nonlinear_cone(), te.nonlinear_thetas(12), None
    else:
        prob, th, cones = te.friction_cone(), te.friction_thetas(12), (0, [3])
    sn = ev_handle(pkg, prob, which + "_kernels", th, cones=cones, threads=threads)
    sn.solve()
    Wo, So, ok = oracle_points(oracle_mod, prob, th, range(len(th)))
    assert len(ok) >= 1
    W = sn.get_state()["solution"].copy()
    for k in ok:
        W[k] = Wo[k]
    sn.set_state(w=W)
    v = np.random.default_rng(4).standard_normal((len(th), sn.N, 2))
    out = sn.vjp(v)
    for k in ok:
        assert out["status"][k] == 0
        ref = So[k].T @ v[k]
        assert rel(out["theta"][k], ref) <= 1e-8, (k, rel(out["theta"][k], ref))
    sn.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
class _Launch(ctypes.Structure):
    _fields_ = [("op", ctypes.c_int32), ("abi", ctypes.c_int32), ("out", ctypes.POINTER(ctypes.c_int64))]


def test_refusals():
    pkg = load_pkg()
    L = pkg.SmallNewtonBatch(3, 1, 2, 2)
    fn, last = L._L.calipso_hip_smallnewton_differentiate_adjoint, lambda h: h._L.calipso_hip_smallnewton_last_error(h._h).decode()
    v = np.zeros(2 * L.N)
    pd = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert fn(L._h, 1, pd(v), pd(np.zeros(2 * L.N)), None, None, None, None) == -4 and "no problem data" in last(L)
    qps = [pr.random_qp(3, 1, 2, seed=40 + k, nonnegative_indices=[1, 2]) for k in range(2)]
    stk = lambda name: np.stack([np.asarray(getattr(p, name), dtype=np.float64) for p in qps])
    L.set_qp(stk("P"), stk("q"), stk("A"), stk("b"), stk("G"), stk("h"), objective_scale=qps[0].c, shared=False)
    L.initialize(np.zeros((2, 3)))
    assert (L.solve()[0] == 1).all()
    assert fn(L._h, 0, pd(v), None, None, None, None, None) == -4 and "k >= 1" in last(L)
    assert fn(L._h, 1, None, None, None, None, None, None) == -4 and "cotangent" in last(L)
    with pytest.raises(pkg.CalipsoHipError, match="grad_theta"):
        L.vjp(np.zeros((2, L.N)), theta=True)
    L.close()
    import test_gpu_smallnewton_evaluator as te
    prob = te.nonlinear_cone()
    th = te.nonlinear_thetas(2)
    E = ev_handle(pkg, prob, "nonlinear_cone_kernels", th)
    with pytest.raises(pkg.CalipsoHipError, match="grad_qp"):
        E.vjp(np.zeros((2, E.N)), qp=True)
    E.close()
    E0 = pkg.SmallNewtonBatch(prob.nx, prob.ne, prob.nc, 2)
    E0.set_evaluator(evlib(), "nonlinear_cone_kernels", 0)            # (no parameters: grad_theta is refused before any launch)
    with pytest.raises(pkg.CalipsoHipError, match="grad_theta"):
        E0.vjp(np.zeros((2, E0.N)), theta=True)
    E0.close()
    # an entry built before the reverse mode: its QUERY answers four slots (a stand-in that forwards every other request to a current entry)
    real = evlib().nonlinear_cone_kernels
    real.restype, real.argtypes = ctypes.c_int32, [ctypes.c_void_p]
    FN = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p)

    def old_entry(p):
        req = ctypes.cast(p, ctypes.POINTER(_Launch)).contents
        if req.op == 0:
            buf = (ctypes.c_int64 * 5)()
            scratch = _Launch(0, req.abi, ctypes.cast(buf, ctypes.POINTER(ctypes.c_int64)))
            rc = real(ctypes.addressof(scratch))
            for i in range(4):
                req.out[i] = buf[i]
            return rc
        return real(p)

    cb = FN(old_entry)
    O = pkg.SmallNewtonBatch(prob.nx, prob.ne, prob.nc, 2)
    assert O._L.calipso_hip_smallnewton_set_evaluator(O._h, ctypes.cast(cb, ctypes.c_void_p), 3) == 0
    O.n_parameters, O._evaluator = 3, True
    O.set_parameters(th)
    O.initialize(np.zeros((2, prob.nx)))
    assert (O.solve()[0] == 1).all()                                   # (the old entry still solves)
    rc = fn(O._h, 1, pd(np.zeros(2 * O.N)), pd(np.zeros(2 * O.N)), None, None, None, None)
    assert rc == -4 and "rebuild it against the current include/calipso_smallnewton.hpp" in last(O)
    O.close()


# ---- the PyTorch layer ------------------------------------------------------------------------------------------------------------------------
def _torch_data(torch, probs, shared):
    st = lambda name: torch.tensor(np.stack([np.asarray(getattr(p, name), dtype=np.float64) for p in probs]), requires_grad=True)
    one = lambda name: torch.tensor(np.asarray(getattr(probs[0], name), dtype=np.float64), requires_grad=True)
    return [(one if name in shared else st)(name) for name in "PqAbGh"]


@pytest.mark.parametrize("shared", ["", "PqAbGh", "PAG"])
def test_torch_layer_backward_equals_vjp(shared):
    torch = pytest.importorskip("torch")
    from calipso_jl_amd.torch_layer import QPLayer
    pkg = load_pkg()
    probs = [pr.parametric_conic_qp(6, 2, 4, 0, 0, seed=20 + k) for k in range(4)]
    if shared == "PqAbGh":
        probs = [probs[0]] * 4
    sn = pkg.SmallNewtonBatch(6, 2, 4, 4, options=TIGHT)
    data = _torch_data(torch, probs, shared)
    x, y, z = QPLayer.apply(sn, *data, True, probs[0].c)
    wx = torch.tensor(np.random.default_rng(1).standard_normal((4, 6)))
    wz = torch.tensor(np.random.default_rng(2).standard_normal((4, 4)))
    ((x * wx).sum() + (z * wz).sum()).backward()
    # the same through vjp on the resident solution
    v = np.zeros((4, sn.N))
    v[:, :6] = wx.numpy()
    oz = 6 + 2 * 2 + 4
    v[:, oz:oz + 4] = wz.numpy()
    ref = sn.vjp(v, adjoint=False)
    for name, t in zip("PqAbGh", data):
        r = ref[name].sum(axis=0) if name in shared else ref[name]
        assert np.array_equal(t.grad.numpy(), r), name
    sn.close()


def test_torch_layer_gradcheck_and_non_converged_instances():
    """gradcheck (float64) on a small equality-only QP: finite differences of whole solves, eps 1e-6, atol 1e-5, rtol 1e-3 (the solves stop at 1e-10 tolerances
    and start at penalty 1e8: the penalty and regularisation they leave are O(1e-7) of the KKT matrix)"""
    torch = pytest.importorskip("torch")
    from calipso_jl_amd.torch_layer import QPLayer
    pkg = load_pkg()
    nx, ne = 4, 2
    p = pr.parametric_conic_qp(nx, ne, 0, 0, 0, seed=77)
    tol = dict(residual_tolerance=1e-10, optimality_tolerance=1e-10, equality_tolerance=1e-10, complementarity_tolerance=1e-10, slack_tolerance=1e-10, penalty_initial=1e8)
    sn = pkg.SmallNewtonBatch(nx, ne, 0, 2, options=tol)
    P = torch.tensor(np.asarray(p.P), requires_grad=False)
    q = torch.tensor(np.stack([np.asarray(p.q), np.asarray(p.q) + 0.5]), requires_grad=True)
    A = torch.tensor(np.asarray(p.A).reshape(ne, nx), requires_grad=True)
    b = torch.tensor(np.asarray(p.b), requires_grad=True)
    G, h = torch.zeros((0, nx), dtype=torch.float64), torch.zeros(0, dtype=torch.float64)
    f = lambda q_, A_, b_: QPLayer.apply(sn, P, q_, A_, b_, G, h, False, p.c)
    assert torch.autograd.gradcheck(f, (q, A, b), eps=1e-6, atol=1e-5, rtol=1e-3)
    sn.close()
    # an instance that does not converge: NaN gradients and a warning
    sn = pkg.SmallNewtonBatch(nx, ne, 0, 2, options=dict(max_outer_iterations=1, max_residual_iterations=1))
    x = QPLayer.apply(sn, P, q, A, b, G, h, False, p.c)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        x.sum().backward()
    assert any("did not converge" in str(r.message) for r in rec)
    assert torch.isnan(q.grad).all()
    sn.close()
