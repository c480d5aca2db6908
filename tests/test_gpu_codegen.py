"""GPU (-m gpu): the evaluators calipso.jl_amd/codegen.py GENERATES from the functions of tests/device_eval_generated/problems.py (compiled by build(): no test here
runs hipcc) in the one-launch batch kernel, held to what tests/test_gpu_smallnewton_evaluator.py holds the hand-written fixtures to — status, counters and every
accepted iterate of the oracle's solve! (1e-8), differentiate! with the evaluator's dR/dtheta against the oracle's solution_sensitivity (1e-8) and its reverse mode
against S'v (1e-8) — and, for the cart-pole problem, to the hand-written evaluator on the same batch."""
import functools
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

import test_gpu_smallnewton_evaluator as te
from helpers import ROOT, load_pkg
from test_oracle_solve import run as run_oracle

pytestmark = pytest.mark.gpu

GEN = os.path.join(ROOT, "tests", "device_eval_generated")
rel = te.rel
# second-order-cone instances fall back to the reference's H \ residual now and then (tests/test_gpu_smallnewton_evaluator.py compares what it can): friction_cone
# runs with lu_fallback = 1, and with the seed of te.friction_thetas at which the ORACLE converges on all 64 instances and takes no fallback on the 8 compared ones
# (5 of the others take one).  With the generator's default seed the oracle itself returns status 0 on instances 35 and 49.
FRICTION_SEED = 27


@functools.lru_cache(maxsize=1)
def gp():
    spec = importlib.util.spec_from_file_location("generated_problems", os.path.join(GEN, "problems.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["generated_problems"] = m
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def generated(name):
    """(codegen.Problem, Compiled) of a fixture build() compiled"""
    load_pkg()
    P = gp().generated(name)
    assert os.path.exists(P.library_path(directory=GEN)), "%s: not built — python __graft_entry__.py build" % P.library_path(directory=GEN)
    return P, P.compile(directory=GEN)


@functools.lru_cache(maxsize=None)
def twin(name):
    """the oracle's problem from the same callables (cartpole_mpc: tests/problems.py's own, which carries the C5 parameters and the initial guess)"""
    return te.cartpole() if name == "cartpole_mpc" else gp().symbolic(name)


def batch(name, thetas, **opts):
    """Problem.batch() on the library build() compiled — for cartpole_mpc what it does, by hand from build()'s manifest: deriving that problem again takes sympy
    ten seconds, and tests/test_codegen_cpu.py already holds its generated text to sympy's derivatives"""
    if name == "cartpole_mpc":
        with open(os.path.join(GEN, "built.json")) as fh:
            info = json.load(fh)[name]
        nx, ne, nc, npar = info["dims"]
        sn = load_pkg().SmallNewtonBatch(nx, ne, nc, len(thetas), options=opts)
        sn.set_cones(info["n_nonnegative"], info["second_order_dims"])
        sn.set_evaluator(os.path.join(GEN, info["library"]), info["symbol"], npar)
        sn.set_parameters(thetas)
        sn.initialize(np.repeat(twin(name).x0[None], len(thetas), axis=0))
        return sn
    P, built = generated(name)
    sn = P.batch(len(thetas), options=opts, directory=GEN)
    if P.np:
        sn.set_parameters(thetas)
    sn.initialize(np.repeat(twin(name).x0[None], len(thetas), axis=0))
    return sn


def spread(B, n):
    return list(range(0, B, B // n))[:n - 1] + [B - 1]


def against_the_oracle(oracle_mod, sn, prob, th, idx, res, rows, lu=False, **opts):
    """the instances idx: compare_with_oracle; then differentiate() and vjp(k = 3) at the oracle's points against its solution_sensitivity"""
    assert te.compare_with_oracle(oracle_mod, sn, prob, th, res, idx, rows, lu=lu, **opts) == len(idx)
    W = sn.get_state()["solution"].copy()
    So = {}
    for k in idx:
        prob.parameters = th[k].copy()
        o, status = run_oracle(oracle_mod, prob, differentiate=1, **opts)
        assert status == 1
        W[k] = o.point()["all"]
        So[k] = o.mat("solution_sensitivity", o.N, prob.np).copy()
    sn.set_state(w=W)
    S, st, _ = sn.differentiate()
    assert S.shape == (len(th), sn.N, prob.np)
    v = np.random.default_rng(11).standard_normal((len(th), sn.N, 3))
    out = sn.vjp(v, theta=True)
    assert out["theta"].shape == (len(th), prob.np, 3)
    for k in idx:
        assert st[k] == 0 and out["status"][k] == 0
        assert rel(S[k], So[k]) <= 1e-8, (k, rel(S[k], So[k]))
        assert rel(out["theta"][k], So[k].T @ v[k]) <= 1e-8, (k, rel(out["theta"][k], So[k].T @ v[k]))
    return S


@pytest.mark.parametrize("threads", te.THREADS)
@pytest.mark.parametrize("name", ["nonlinear_cone", "friction_cone"])
def test_generated_small_problems_match_the_oracle(oracle_mod, name, threads):
    B = 64
    prob = twin(name)
    th = te.nonlinear_thetas(B) if name == "nonlinear_cone" else te.friction_thetas(B, seed=FRICTION_SEED)
    lu = name == "friction_cone"
    sn = batch(name, th, threads=threads, lu_fallback=int(lu))
    sn.keep_trace(64)
    res, _ = sn.solve()
    assert (res == 1).all(), np.unique(res, return_counts=True)
    against_the_oracle(oracle_mod, sn, prob, th, spread(B, 8), res, 64, lu=lu)
    sn.close()


@pytest.mark.parametrize("threads", [0, 64])
def test_generated_cartpole_matches_the_oracle_and_the_hand_written_evaluator(oracle_mod, threads):
    pkg = load_pkg()
    B = 64
    prob = twin("cartpole_mpc")
    th = te.cartpole_thetas(B)
    sn = batch("cartpole_mpc", th, threads=threads, **te.C5)
    sn.keep_trace(32)
    res, _ = sn.solve()
    assert (res == 1).all(), np.unique(res, return_counts=True)
    hand = te.make(pkg, prob, "cartpole_mpc_kernels", th, threads=threads, **te.C5)
    res_h, _ = hand.solve()
    a, b = sn.get_state(), hand.get_state()
    assert np.array_equal(res, res_h)
    for n in ("total_iterations", "outer", "factorizations", "newton_steps", "accepted_iterates"):
        assert np.array_equal(a["counters"][n], b["counters"][n]), n
    for k in range(B):
        assert rel(a["solution"][k], b["solution"][k]) <= 1e-8, (k, rel(a["solution"][k], b["solution"][k]))
    Sg, stg, _ = sn.differentiate()
    Sh, sth, _ = hand.differentiate()
    assert (stg == 0).all() and (sth == 0).all()
    for k in range(B):
        assert rel(Sg[k], Sh[k]) <= 1e-8, (k, rel(Sg[k], Sh[k]))
    against_the_oracle(oracle_mod, sn, prob, th, spread(B, 4), res, 32, **te.C5)
    sn.close(); hand.close()


def test_batch_takes_a_caller_given_jacobian_beside_the_evaluators_own():
    """Problem.batch() hands back a working handle; differentiate(J) with the caller's dR/dtheta (here the problem's, which is constant, and twice its first column)"""
    B = 8
    P, built = generated("nonlinear_cone")
    assert built.symbol == "generated_nonlinear_cone_kernels" and os.path.dirname(built.path) == GEN
    sn = batch("nonlinear_cone", te.nonlinear_thetas(B))
    assert (sn.nx, sn.ne, sn.nc, sn.n_parameters) == (3, 1, 2, 3)
    res, _ = sn.solve()
    assert (res == 1).all()
    S, st, _ = sn.differentiate()
    assert (st == 0).all() and np.abs(S).max() > 0
    J = np.zeros((sn.N, 3))
    oy, oz = P.nx + P.ne + P.nc, P.nx + 2 * P.ne + P.nc
    J[oy, 0], J[oz, 1], J[oz + 1, 2] = -1.0, 1.0, 1.0
    S2, st2, _ = sn.differentiate(J)
    S3, st3, _ = sn.differentiate(np.repeat(2.0 * J[None, :, :1], B, axis=0))
    assert (st2 == 0).all() and (st3 == 0).all() and S3.shape == (B, sn.N, 1)
    for k in range(B):
        assert rel(S2[k], S[k]) <= 1e-8 and rel(S3[k], 2.0 * S[k][:, :1]) <= 1e-8
    sn.close()


def test_a_problem_without_parameters_solves_and_refuses_differentiate(oracle_mod):
    pkg = load_pkg()
    B = 5
    prob = twin("no_parameters")
    sn = batch("no_parameters", np.zeros((B, 0)))
    sn.keep_trace(64)
    res, _ = sn.solve()
    assert (res == 1).all(), res
    assert te.compare_with_oracle(oracle_mod, sn, prob, np.zeros((B, 0)), res, range(B), 64) == B
    with pytest.raises(pkg.CalipsoHipError, match="needs an evaluator that provides dR/dtheta and has parameters"):
        sn.differentiate()
    sn.close()
