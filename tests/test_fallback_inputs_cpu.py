"""CPU: the inputs of tests/test_gpu_fallback_paths.py, pinned with the oracle alone.  Those tests hold the device's `H \\ residual` fallback
(csrc/fallback.hip) and the decisions round it (api.hip, group.hip) against the oracle, so every input has to be one on which the oracle decides
CLEARLY: a fallback case falls back — and keeps falling back, with the same counts, when its point is perturbed by +-1e-9 relative and +1e-9
absolute (far more than the rounding differences between the device and the oracle) —, a no-fallback member of a mixed group never does, and the
systems the LU is measured on are well conditioned and really pivot.  A case that fails here is replaced, not loosened."""
import numpy as np
import pytest

import helpers as fc
import problems as pr
from helpers import (LU_EDGE_SHAPES, lapack_row_interchanges, lu_edge_case, lu_strided_case, make_oracle, oracle_cold_solve, oracle_newton_state,
                     perturbations, refined_solve)


def oracle_system(oracle_mod, prob, pt, lam):
    o = make_oracle(oracle_mod, prob, pt, lam, ep=0.0, ed=0.0)
    o.cone(product=True, jacobian=True, target=True, barrier=True, barrier_gradient=True)
    o.residual()
    o.residual_jacobian_variables()
    return o.H_dense(), np.array(o.buf("residual"))


@pytest.mark.parametrize("N", sorted(LU_EDGE_SHAPES))
def test_lu_edge_systems_are_well_conditioned_and_pivot(oracle_mod, N):
    prob, pt, lam = lu_edge_case(N)
    H, R = oracle_system(oracle_mod, prob, pt, lam)
    assert H.shape == (N, N)
    assert np.linalg.cond(H) <= 1e4
    # at least N / 8 real row interchanges (a 1 x 1 system has none to make)
    assert N == 1 or lapack_row_interchanges(H)[1] >= N / 8.0
    x, x_lapack = refined_solve(H, R)
    assert np.abs(x_lapack - x).max() <= 1e-13 * max(1.0, np.abs(x).max())      # (the reference the device is held against is itself settled)


def test_lu_strided_system_takes_a_first_panel_pivot_from_beyond_row_1024(oracle_mod):
    prob, pt, lam = lu_strided_case()
    H, R = oracle_system(oracle_mod, prob, pt, lam)
    N = H.shape[0]
    oy = prob.nx + prob.ne + prob.nc
    assert 1400 <= N <= 1700 and oy < 1024 < oy + prob.ne + prob.nc
    assert np.linalg.cond(H) <= 1e4
    piv, count = lapack_row_interchanges(H)
    assert count >= N / 8.0
    assert (piv[:32] >= 1024).any()
    assert piv[fc.LU_STRIDED_COLUMN] == oy + fc.LU_STRIDED_EQUALITY >= 1024
    # every other candidate of that column is at least 2^28 times smaller: a search that misses the row is not a matter of rounding
    col = np.abs(H[:, fc.LU_STRIDED_COLUMN]).copy()
    col[oy + fc.LU_STRIDED_EQUALITY] = 0.0
    assert col.max() <= 2.0 ** -28


def verdicts(oracle_mod, prob, w, lam, cone_search=False):
    out = []
    for v in [w] + perturbations(w):
        o = oracle_newton_state(oracle_mod, prob, v, lam)
        out.append((o.search_direction(), o.stats()["last_refinement_rounds"], o.stats()["lu_fallbacks"]))
        if cone_search:                                # the Newton-step tests go on to the cone search: it must end well inside the limit they set
            assert max(k for _, k in fc.cone_search_halvings(o, v)) <= fc.CONE_SEARCH_PINNED
    return out


@pytest.mark.parametrize("shape,pid", fc.STEP_FALLBACK)
def test_step_cases_that_fall_back(oracle_mod, shape, pid):
    prob, w, lam = fc.synthetic_step_case(oracle_mod.splitmix_uniform, pid, shape, True)
    v = verdicts(oracle_mod, prob, w, lam, cone_search=True)
    assert v[0][0] == 2 and v[0][2] == 1 and len(set(v)) == 1, v


def test_structured_case_falls_back(oracle_mod):
    prob, w, lam = fc.staged_step_case(oracle_mod.splitmix_uniform, fc.STRUCTURED_ID, fc.STRUCTURED_SHAPE, True)
    v = verdicts(oracle_mod, prob, w, lam)
    assert v[0][0] == 2 and v[0][2] == 1 and len(set(v)) == 1, v


@pytest.mark.parametrize("shape,pid", fc.STEP_NO_FALLBACK)
def test_step_cases_that_do_not_fall_back(oracle_mod, shape, pid):
    prob, w, lam = fc.synthetic_step_case(oracle_mod.splitmix_uniform, pid, shape, False)
    v = verdicts(oracle_mod, prob, w, lam)
    assert v[0][0] == 0 and v[0][2] == 0 and len(set(v)) == 1, v
    assert v[0][1] <= 6                                # settled after a few rounds, nowhere near the round limit


def test_cases_of_every_gpu_test_are_pinned_here():
    """the group / schedule / structured tests name their members from these lists only"""
    for shape, members in fc.MIXED_GROUPS:
        for pid, boundary in members:
            assert ((shape, pid) in fc.STEP_FALLBACK) if boundary else ((shape, pid) in fc.STEP_NO_FALLBACK), (shape, pid, boundary)
        falls = [b for _, b in members]
        assert 4 <= len(members) <= 6 and any(falls) and not all(falls)
    assert any(m[0][1] for _, m in fc.MIXED_GROUPS) and any(not m[0][1] and any(b for _, b in m[1:]) for _, m in fc.MIXED_GROUPS)   # the base handle falls back / a later member does
    for case in fc.SINGLE_HANDLE:
        assert case in fc.STEP_FALLBACK and case in fc.STEP_NO_FALLBACK     # (the schedule children step from the interior point too)
    for pid in fc.NAN_GROUP[1]:
        assert (fc.NAN_GROUP[0], pid) in fc.STEP_NO_FALLBACK
    for shape, seeds in fc.SOLVE_GROUPS:
        counts = [f for s, k, _, f, _ in fc.SOLVES if s == shape and k in seeds]
        assert len(counts) == len(seeds) and min(counts) == 0 and max(counts) >= 1


@pytest.mark.parametrize("shape,seed,iterations,fallbacks,first_row", fc.SOLVES)
def test_cold_solves_take_the_listed_fallbacks(oracle_mod, shape, seed, iterations, fallbacks, first_row):
    prob = pr.parametric_conic_qp(*shape, seed=seed)
    x0 = np.zeros(prob.nx)
    for v in [x0] + perturbations(x0):
        o, status = oracle_cold_solve(oracle_mod, prob, v)
        st = o.stats()
        assert status == 1
        assert (st["total_iterations"], st["lu_fallbacks"], st["first_lu_fallback_row"]) == (iterations, fallbacks, first_row)
