"""CPU: the inputs of tests/test_gpu_sparse_kkt.py (tests/sparse_kkt_cases.py), pinned with the oracle alone.  The GPU tests hold SparseKKT's search_direction
against the oracle's — the regularisation walk bit for bit, the factorisation count, the refinement round count — so every input has to be one on which the
oracle does what the table says, and keeps doing it when the point is perturbed by +-1e-9 relative and +1e-9 absolute (far more than the rounding differences
between the device and the oracle).  A failure on the GPU can then not be blamed on the inputs.  A case that fails here is replaced, not loosened."""
import numpy as np
import pytest

import helpers
import sparse_kkt_cases as kc


def verdicts(oracle_mod, prob, w, lam):
    return [kc.oracle_search_direction(oracle_mod, prob, v, lam)[1] for v in [w] + helpers.perturbations(w)]


@pytest.mark.parametrize("name", sorted(kc.WHOLE))
def test_whole_cases_behave_as_stated(oracle_mod, name):
    shape, pid, kind, want = kc.WHOLE[name]
    prob, w, lam = kc.whole_case(oracle_mod.splitmix_uniform, shape, pid, kind)
    got = verdicts(oracle_mod, prob, w, lam)
    for g in got:                                                # the regularisation walk and the verdict: the same on every copy
        assert (g["status"], g["factorizations"], g["ep"], g["fallbacks"]) == (want["status"], want["factorizations"], want["ep"], want["fallbacks"]), got
        assert g["ep_last"] == (g["ep"] if g["factorizations"] > 1 else 0.0) and g["ed"] == 1.0e-7, got
    assert got[0]["rounds"] == want["rounds"], got
    assert (len(set(g["rounds"] for g in got)) == 1) == want["rounds_stable"], got      # where this holds the GPU test asserts the round count too


def test_the_failure_case_fails_at_the_boundary_and_not_inside(oracle_mod):
    prob, w, lam = helpers.staged_step_case(oracle_mod.splitmix_uniform, kc.FAILURE_ID, kc.FAILURE_SHAPE, True)
    got = verdicts(oracle_mod, prob, w, lam)
    assert all((g["status"], g["fallbacks"], g["factorizations"]) == (2, 1, got[0]["factorizations"]) and g["ep"] == got[0]["ep"] for g in got), got
    assert got[0]["factorizations"] > 1                          # (an ep walk to compare)
    prob, w, lam = helpers.staged_step_case(oracle_mod.splitmix_uniform, kc.FAILURE_ID, kc.FAILURE_SHAPE, False)
    got = verdicts(oracle_mod, prob, w, lam)
    assert all((g["status"], g["fallbacks"], g["factorizations"]) == (0, 0, 1) for g in got), got


@pytest.mark.parametrize("name", kc.BLOCK_CASES)
def test_block_cases_are_quasidefinite_at_the_fixed_regularisation(oracle_mod, name):
    prob, pt, lam = kc.block_case(oracle_mod.splitmix_uniform, name)
    o = helpers.make_oracle(oracle_mod, prob, pt, lam, ep=kc.EP, ed=kc.ED)
    o.cone(product=True, jacobian=True, target=True)
    o.residual(); o.residual_jacobian_variables(); o.residual_jacobian_variables_symmetric()
    o.factorize()
    assert o.compute_inertia() == (prob.nx, prob.ne + prob.nc, 0)
    q, dims = kc.cone_layout(prob)
    assert q + sum(dims) == prob.nc
    # the sparse inputs carry the dense data exactly, and the superset stores more
    for dense, A, B in zip((prob.Psym, prob.A, -prob.G), kc.sparse_inputs(prob), kc.sparse_inputs(prob, np.random.default_rng(1))):
        assert np.array_equal(A.toarray(), np.asarray(dense).reshape(A.shape)) and np.array_equal(B.toarray(), A.toarray())
        assert A.has_sorted_indices and B.has_sorted_indices and B.nnz >= A.nnz and A.nnz == np.count_nonzero(dense)
