"""What tests/test_gpu_sparse_differentiate.py assumes about its inputs (tests/sparse_differentiate_cases.py), pinned with the oracle alone: no GPU, no code under test."""
import numpy as np
import pytest

import problems as pr
import sparse_differentiate_cases as dc
import sparse_kkt_cases as kc
import sparse_solve_cases as sc


@pytest.mark.parametrize("name", kc.BLOCK_CASES)
def test_the_inertia_at_the_fixed_regularisation(oracle_mod, name):
    prob, w, o = dc.block_oracle(oracle_mod, name)
    o.factorize(update=False)
    assert o.compute_inertia() == (prob.nx, prob.ne + prob.nc, 0)


@pytest.mark.parametrize("case", dc.DIFFERENTIATE, ids=dc.DIFFERENTIATE_IDS)
def test_the_inertia_at_the_differentiate_cases(oracle_mod, case):
    prob, pt, lam = dc.differentiate_case(case)
    assert prob.nonnegative_indices == list(range(1, case[2] + 1))      # laid out as the handle takes them
    o = dc.differentiated_oracle(oracle_mod, prob, pt, lam, dc.INTERIOR)
    o.residual_jacobian_variables(); o.residual_jacobian_variables_symmetric()
    o.factorize(update=False)
    assert o.compute_inertia() == (prob.nx, prob.ne + prob.nc, 0)
    S = o.mat("solution_sensitivity", o.N, prob.np)
    assert np.isfinite(S).all() and np.abs(S).max() > 1e-3


@pytest.mark.parametrize("name", dc.REFINEMENT)
def test_the_rounds_meet_the_tolerance_in_a_numpy_replay(oracle_mod, name):
    prob, w, o = dc.block_oracle(oracle_mod, name)
    assert not any(c for c in prob.second_order_indices)
    H = o.H_dense().copy()
    M = dc.map_matrix(o)
    tolerance, max_rounds = float(o.buf("opt.iterative_refinement_tolerance")[0]), o.get_int("max_iterative_refinement")
    rounds = dc.replay_rounds(M, H, dc.refinement_cotangents(o.N), tolerance, max_rounds)
    print("%s: tolerance %.1e, rounds per column %s of at most %d" % (name, tolerance, rounds, max_rounds))
    assert all(r is not None for r in rounds)


def test_the_inert_shape_has_a_second_order_cone(oracle_mod):
    prob, _, _ = kc.block_case(oracle_mod.splitmix_uniform, dc.INERT)
    assert any(c for c in prob.second_order_indices)


def test_the_slacks_reconstruction_reproduces_the_oracles_own_sensitivities(oracle_mod):
    """the oracle's solve! + differentiate! against the oracle set at the final point and scalars with the cone Jacobians formed at the slacks of the iterate before:
    the same solution_sensitivity bit for bit — and NOT with the cone Jacobians formed at the final point's own slacks"""
    shape, pid = dc.WHOLE_SOLVE
    assert (shape, pid) in sc.SOLVES
    prob = dc.parametric(sc.problem(oracle_mod.splitmix_uniform, shape, pid))
    own = dc.oracle_whole_solve(oracle_mod, prob)
    assert own["status"] == 1 and own["lu_fallbacks"] == 0
    pt = dc.split(own["w"], prob.nx, prob.ne, prob.nc)
    rebuilt = dc.differentiated_oracle(oracle_mod, prob, pt, own["dual"], own["scalars"], slacks=own["slacks"])
    assert np.array_equal(rebuilt.mat("solution_sensitivity", rebuilt.N, prob.np), own["S"])
    at_the_point = dc.differentiated_oracle(oracle_mod, prob, pt, own["dual"], own["scalars"])
    assert not np.array_equal(at_the_point.mat("solution_sensitivity", at_the_point.N, prob.np), own["S"])


def test_the_directional_problem_has_derivatives_far_from_zero(oracle_mod):
    """the matrix-gradient test contracts the gradients with directions on the patterns: the oracle's three derivatives are far above the test's bound"""
    from test_gpu_differentiate_adjoint import DirectionalQP
    base, pt, lam = pr.staged_conic_qp(oracle_mod.splitmix_uniform, 0, *dc.DIRECTIONAL)
    prob = DirectionalQP(base, *dc.pattern_directions(base, 12))
    o = dc.differentiated_oracle(oracle_mod, prob, pt, lam, dc.INTERIOR)
    S = o.mat("solution_sensitivity", o.N, 3)
    v = np.random.default_rng(13).standard_normal(o.N)
    bound = 1e-8 * max(1.0, np.abs(S).max()) * np.abs(v).sum()
    assert np.abs(S.T @ v).min() > 1e3 * bound
