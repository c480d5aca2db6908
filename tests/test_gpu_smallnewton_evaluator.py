"""GPU (-m gpu): the batched small-problem kernel (csrc/smallnewton.hip) with DEVICE EVALUATORS (include/calipso_smallnewton.hpp) compiled into a user library
(tests/device_eval_small/): the cart-pole MPC problem of BASELINE config C5 with per-instance parameters, a nonconvex problem with nonlinear f and h over nonnegative
cones and a second-order-cone problem.  Every instance compared is held to the ORACLE's solve! of the same problem and theta: status, counters and every accepted
iterate (1e-8), as tests/test_gpu_smallnewton.py does for QPs; differentiate! with dR/dtheta from the evaluator against the oracle's solution_sensitivity."""
import ctypes
import functools
import os

import numpy as np
import pytest

import problems as pr
from helpers import load_pkg
from test_oracle_solve import run as run_oracle

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_eval_small", "libsmall_evaluators.so")
THREADS = [0, 64, 128, 256]
# the C5 options of tests/test_c5_cartpole.py (the batch takes no "differentiate" option: it always can)
C5 = dict(residual_tolerance=1e-3, optimality_tolerance=1e-3, equality_tolerance=1e-3, complementarity_tolerance=1e-3, slack_tolerance=1e-3)


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())


@functools.lru_cache(maxsize=1)
def evlib():
    return ctypes.CDLL(LIB)


@functools.lru_cache(maxsize=1)
def cartpole():
    return pr.cartpole_mpc()


@functools.lru_cache(maxsize=1)
def nonlinear_cone():
    """twin of tests/device_eval_small/nonlinear_cone.hip"""
    return pr.SymbolicProblem(3, lambda x, th: (1 - x[0]) ** 2 + 10 * (x[1] - x[0] ** 2) ** 2 + 0.5 * x[2] ** 2,
                              lambda x, th: [x[0] + x[1] + x[2] - th[0]],
                              lambda x, th: [th[1] - x[0] ** 2 - x[1] ** 2, x[2] + th[2] - x[0] * x[1]],
                              np_=3, parameters=np.array([1.0, 2.0, 0.5]), name="nonlinear_cone")


@functools.lru_cache(maxsize=1)
def friction_cone():
    """twin of tests/device_eval_small/friction_cone.hip: theta = [v (3); mu; gamma]"""
    return pr.SymbolicProblem(3, lambda x, th: 0.5 * ((x[0] - th[0]) ** 2 + (x[1] - th[1]) ** 2 + (x[2] - th[2]) ** 2) + 0.25 * th[4] * x[0] ** 4,
                              None, lambda x, th: [th[3] * (x[0] + 1), x[1], x[2]],
                              np_=5, nonnegative_indices=[], second_order_indices=[[1, 2, 3]], parameters=np.array([0.3, 1.0, -0.5, 0.8, 1.0]), name="friction_cone")


def cartpole_thetas(B, seed=0):
    """per instance: the initial state and the stage weights moved from the C5 parameters by a few per cent (modest moves: every instance stays in the regime of the
    C5 problem, whose oracle solve converges in a few iterations with clear line-search and regularisation decisions — no knife-edge test decides an iterate)"""
    base = cartpole().parameters
    rng = np.random.default_rng(seed)
    th = np.repeat(base[None], B, axis=0)
    th[:, 10:14] += 0.05 * rng.uniform(-1, 1, (B, 4))                   # x_init
    offs = [0] + [14 + 10 * t for t in range(9)]
    for t in range(9):
        th[:, offs[t] + 5:offs[t] + 10] *= 1.0 + 0.1 * rng.uniform(-1, 1, (B, 5))   # w_Q, w_R
    th[:, 98:102] *= 1.0 + 0.1 * rng.uniform(-1, 1, (B, 4))                        # terminal w_Q
    return th


def nonlinear_thetas(B, seed=1):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.5, 1.5, B), rng.uniform(1.5, 3.0, B), rng.uniform(0.3, 1.0, B)], axis=1)


def friction_thetas(B, seed=2):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(0.5, 1.5, B), rng.uniform(0.5, 2.0, B)], axis=1)


def make(pkg, prob, symbol, thetas, cones=None, **opts):
    sn = pkg.SmallNewtonBatch(prob.nx, prob.ne, prob.nc, len(thetas), options=opts)
    if cones is not None:
        sn.set_cones(*cones)
    sn.set_evaluator(evlib(), symbol, prob.np)
    sn.set_parameters(thetas)
    sn.initialize(np.repeat(prob.x0[None], len(thetas), axis=0))
    return sn


def compare_with_oracle(oracle_mod, sn, prob, thetas, res, idx, rows, lu=False, **opts):
    """status, counters and every accepted iterate of the instances idx against the oracle's solve! with the same theta; returns how many were compared"""
    st = sn.get_state()
    tr = sn.trace()
    compared = 0
    for k in idx:
        prob.parameters = thetas[k].copy()
        o, status = run_oracle(oracle_mod, prob, **opts)
        os_ = o.stats()
        if not lu and os_["lu_fallbacks"] > 0:                  # the reference fell back to H \ residual: without lu_fallback this path stops there and says so
            assert res[k] == -102, (k, res[k])
            continue
        assert status == int(res[k]), (k, status, res[k])
        assert st["counters"]["total_iterations"][k] == os_["total_iterations"], (k, st["counters"]["total_iterations"][k], os_["total_iterations"])
        assert st["counters"]["outer"][k] == os_["outer"]
        assert st["counters"]["max_refinement_rounds"][k] == os_["max_refinement_rounds"]
        ot = o.trace()
        n = int(st["counters"]["accepted_iterates"][k])
        assert n == ot.shape[0]
        for r in range(min(n, rows)):
            assert rel(tr[k, r], ot[r]) <= 1e-8, (k, r, rel(tr[k, r], ot[r]))
        assert rel(st["solution"][k], o.point()["all"]) <= 1e-8
        compared += 1
    return compared


def test_cartpole_batch_of_1024_with_per_instance_parameters(oracle_mod):
    """C5 (nx 49, ne 40, np 102) for 1024 different (x_init, weights) in one launch: every instance converges; 16 instances spread over the batch match the oracle's
    counters and accepted iterates; differentiate! with the evaluator's dR/dtheta matches the oracle's solution_sensitivity, and so does the caller-given-dR/dtheta
    entry fed the oracle's jacobian_parameters"""
    pkg = load_pkg()
    prob = cartpole()
    B = 1024
    th = cartpole_thetas(B)
    sn = make(pkg, prob, "cartpole_mpc_kernels", th, **C5)
    sn.keep_trace(32)
    res, ms = sn.solve()
    assert (res == 1).all(), np.unique(res, return_counts=True)
    idx = list(range(0, B, B // 16))[:15] + [B - 1]
    assert compare_with_oracle(oracle_mod, sn, prob, th, res, idx, 32, **C5) == 16
    # sensitivities at the oracle's solution (the same point to rounding; differentiate! runs at the resident point)
    W = sn.get_state()["solution"].copy()
    So, Jo = {}, {}
    for k in idx:
        prob.parameters = th[k].copy()
        o, status = run_oracle(oracle_mod, prob, differentiate=1, **C5)
        W[k] = o.point()["all"]
        So[k] = o.mat("solution_sensitivity", o.N, prob.np).copy()
        Jo[k] = o.mat("jacobian_parameters", o.N, prob.np).copy()
    sn.set_state(w=W)
    S, st, _ = sn.differentiate()
    assert S.shape == (B, prob.nx + 2 * prob.ne, prob.np) and (st == 0).all()
    J = np.zeros((B, prob.nx + 2 * prob.ne, prob.np))
    for k in idx:
        assert rel(S[k], So[k]) <= 1e-8, (k, rel(S[k], So[k]))
        J[k] = Jo[k]
    S2, st2, _ = sn.differentiate(J)
    for k in idx:
        assert rel(S2[k], So[k]) <= 1e-8, (k, rel(S2[k], So[k]))
    sn.close()


@pytest.mark.parametrize("threads", THREADS)
def test_nonlinear_cone_problem_matches_the_oracle(oracle_mod, threads):
    """nonlinear f and h, nonnegative cones, theta in the constraint offsets: per accepted iterate against the oracle at every workgroup size"""
    pkg = load_pkg()
    prob = nonlinear_cone()
    th = nonlinear_thetas(24)
    sn = make(pkg, prob, "nonlinear_cone_kernels", th, threads=threads)
    sn.keep_trace(64)
    res, _ = sn.solve()
    assert compare_with_oracle(oracle_mod, sn, prob, th, res, range(len(th)), 64) >= 20
    sn.close()


@pytest.mark.parametrize("lu", [0, 1])
@pytest.mark.parametrize("threads", THREADS)
def test_second_order_cone_problem_matches_the_oracle(oracle_mod, threads, lu):
    """the SOC = true builds with an evaluator; with lu_fallback = 1 also through the reference's H \\ residual steps"""
    pkg = load_pkg()
    prob = friction_cone()
    th = friction_thetas(24)
    sn = make(pkg, prob, "friction_cone_kernels", th, cones=(0, [3]), threads=threads, lu_fallback=lu)
    sn.keep_trace(64)
    res, _ = sn.solve()
    compared = compare_with_oracle(oracle_mod, sn, prob, th, res, range(len(th)), 64, lu=bool(lu))
    assert compared >= (len(th) if lu else 1), compared
    sn.close()


def test_steps_without_advancing_leave_an_evaluator_handle_untouched():
    pkg = load_pkg()
    prob = nonlinear_cone()
    th = nonlinear_thetas(9)
    sn = make(pkg, prob, "nonlinear_cone_kernels", th)
    res, _ = sn.solve()
    assert (res == 1).all(), res
    w = sn.get_state()["solution"].copy()
    nx, ne, nc = prob.nx, prob.ne, prob.nc
    w[:, nx + ne:nx + ne + nc] += 0.5; w[:, -nc:] += 0.5
    sn.set_state(w=w, scalars=np.tile([1e-3, 0.99, 52.0], (len(th), 1)))      # (a small central path: the moved slacks are far from it, every instance steps)
    before = sn.get_state()
    info1, st1, _ = sn.steps(1, advance=False)
    info3, st3, _ = sn.steps(3, advance=False)
    after = sn.get_state()
    assert (st1 == 0).all() and (st3 == 0).all() and (info1[:, 6] == 0).all()
    assert np.array_equal(info1, info3)
    assert np.array_equal(before["solution"], after["solution"]) and np.array_equal(before["scalars"][:, :3], after["scalars"][:, :3])
    info_a, _, _ = sn.steps(1, advance=True)
    assert np.array_equal(info_a[:, :6], info1[:, :6]) and not np.array_equal(sn.get_state()["solution"], before["solution"])
    sn.close()


def test_refusals_and_switching_back_to_a_qp():
    pkg = load_pkg()
    prob = nonlinear_cone()
    th = nonlinear_thetas(4)
    sn = pkg.SmallNewtonBatch(prob.nx, prob.ne, prob.nc, len(th))
    with pytest.raises(pkg.CalipsoHipError, match="another calipso_smallnewton.hpp"):
        sn.set_evaluator(evlib(), "mismatched_abi_kernels", 3)
    with pytest.raises(pkg.CalipsoHipError, match="no problem data"):
        sn.solve()
    sn.set_evaluator(evlib(), "nonlinear_cone_kernels", 3)
    sn.initialize(np.zeros((len(th), prob.nx)))
    with pytest.raises(pkg.CalipsoHipError, match="parameters"):
        sn.solve()
    sn.set_parameters(th)
    res, _ = sn.solve()
    assert (res == 1).all()
    info = np.zeros(4)
    assert sn._L.calipso_hip_debug_smallnewton_describe(sn._h, info.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0 and info[2] >= 1
    # back to a QP: the same results as a fresh handle
    qps = [pr.random_qp(3, 1, 2, seed=40 + k, nonnegative_indices=[1, 2]) for k in range(len(th))]
    stk = lambda name: np.stack([np.asarray(getattr(p, name), dtype=np.float64) for p in qps])
    fresh = pkg.SmallNewtonBatch(3, 1, 2, len(th))
    for h in (sn, fresh):
        h.set_qp(stk("P"), stk("q"), stk("A"), stk("b"), stk("G"), stk("h"), objective_scale=qps[0].c, shared=False)
        h.initialize(np.stack([p.x0 for p in qps]))
    ra, _ = sn.solve(); rb, _ = fresh.solve()
    a, b = sn.get_state(), fresh.get_state()
    assert np.array_equal(ra, rb) and np.array_equal(a["solution"], b["solution"])
    assert all(np.array_equal(a["counters"][n], b["counters"][n]) for n in a["counters"])
    sn.close(); fresh.close()
