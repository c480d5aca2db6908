"""CPU: the inputs of tests/test_gpu_sparse_fallback.py (tests/sparse_fallback_cases.py), pinned with the oracle alone.  The GPU tests hold whole solves WITH
`H \\ residual` fallbacks against the oracle's — counts, fallbacks, every accepted iterate — while the handle eliminates in another order and solves H step = R by
GMRES where the oracle factorises H.  So every row has to be one on which the oracle itself does not care about the order (status, counts and fallbacks stay under
two other elimination orders, the traces agree far below the 1e-8 the GPU tests allow), and whose first fallback point is a well-conditioned system: there a
residual of 1e-10 pins the step, whoever computes it.  A case that fails here is replaced, not loosened."""
import numpy as np
import pytest

import sparse_fallback_cases as fc
import sparse_solve_cases as sc

ORDER_AGREEMENT = 1e-10


def rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max()) if b.size else 0.0


@pytest.fixture(scope="module")
def solves(oracle_mod):
    cache = {}

    def get(case):
        if case not in cache:
            prob = sc.problem(oracle_mod.splitmix_uniform, *case)
            cache[case] = (prob, sc.oracle_solve(oracle_mod, prob))
        return cache[case]
    return get


@pytest.mark.parametrize("case", list(fc.CASES), ids=fc.CASE_IDS)
def test_every_row_behaves_as_listed(oracle_mod, solves, case):
    want = fc.CASES[case]
    prob, ref = solves(case)
    n = prob.nx + prob.ne + prob.nc
    assert ref["o"].N == want["N"]
    runs = [ref] + ([sc.oracle_solve(oracle_mod, prob, perm=p) for p in sc.orders(n, case[1])] if want["N"] <= fc.ORDERS_UP_TO else [])
    for r in runs:
        got = dict(N=want["N"], total_iterations=r["total_iterations"], outer=r["outer"], accepted=r["accepted"], fallbacks=r["lu_fallbacks"],
                   first_row=r["first_lu_fallback_row"])
        assert r["status"] == 1 and got == want, (r["status"], got)
        assert r["trace"].shape == ref["trace"].shape and rel(r["trace"], ref["trace"]) <= ORDER_AGREEMENT
        assert rel(r["w"], ref["w"]) <= ORDER_AGREEMENT


@pytest.mark.parametrize("case", list(fc.CASES), ids=fc.CASE_IDS)
def test_the_first_fallback_point_is_a_well_conditioned_system_the_refinement_fails_on(oracle_mod, solves, case):
    prob, ref = solves(case)
    o, w, lam, R = fc.fixed_point(oracle_mod, prob, ref, fc.CASES[case]["first_row"])
    assert o.search_direction() == 2                        # the refinement fails: the oracle went on to `H \ residual`
    step = o.buf("step").copy()
    H = o.H_dense()
    want = np.linalg.solve(H, R)
    cond = np.linalg.cond(H)
    print("N %d: cond(H) %.3e, |oracle step - numpy| %.3e, |R - H step|_inf %.3e" % (o.N, cond, rel(step, want), np.abs(R - H @ step).max()))
    assert rel(step, want) <= 1e-12
    assert cond <= fc.CONDITION_BOUND
