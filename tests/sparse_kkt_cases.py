"""Inputs shared by tests/test_sparse_kkt_inputs_cpu.py (which pins, with the oracle alone, that each behaves as stated here) and tests/test_gpu_sparse_kkt.py
(which holds calipso.jl_amd.SparseKKT against the oracle on them).  Shapes are the arguments of problems.staged_conic_qp after (uniform, pid):
(T, nv, nd, n_nn_stage, n_soc_stage, soc_dim)."""
import numpy as np
import scipy.sparse as sp

import helpers
import problems as pr

EP, ED = 0.12, 0.21                     # the fixed regularisation of the building-block cases (helpers.make_oracle's defaults)
KAPPA, RHO = 0.17, 52.0                 # the scalars helpers.make_oracle and helpers.oracle_newton_state set

# ---- building blocks at a fixed regularisation -----------------------------------------------------------------------------------------------------------
BLOCK_SHAPES = [(2, 3, 1, 1, 0, 3),     # nx 6, ne 1, nc 2: nonnegative only
                (3, 4, 2, 1, 1, 3),     # nx 12, ne 4, nc 12: nonnegative rows and cones of dimension 3
                (5, 7, 3, 0, 1, 5),     # cones of dimension 5 only
                (4, 6, 6, 2, 0, 3),     # no second-order cone
                (40, 6, 3, 1, 1, 3)]    # n = 517: several tree levels
# dense-pattern cases of tests/test_gpu_parity.py, with its tails
DENSE_CASES = {
    "qp_noeq_7_0_4": (lambda: pr.random_qp(7, 0, 4, seed=6), 0.3),
    "qp_nocone_9_4_0": (lambda: pr.random_qp(9, 4, 0, seed=7), 0.3),
    "qp_soc64_70_5_66": (lambda: pr.random_qp(70, 5, 66, seed=12, nonnegative_indices=[1, 2], second_order_indices=[list(range(3, 67))]), 0.05),
}
BLOCK_CASES = ["staged_%d_%d_%d_%d_%d_%d" % s for s in BLOCK_SHAPES] + sorted(DENSE_CASES)


def block_case(uniform, name):
    """(problem, point dict, lam) of a building-block case"""
    if name in DENSE_CASES:
        make, tail = DENSE_CASES[name]
        prob = make()
        pt, lam = helpers.interior_point(prob, seed=1, tail=tail)
        return prob, pt, lam
    return pr.staged_conic_qp(uniform, 0, *[int(v) for v in name.split("_")[1:]])


# ---- whole search_direction from regularization = (0, 0, 0) -----------------------------------------------------------------------------------------------
# name -> (shape, pid, kind, what the oracle does: status, factorisations, ep at exit, refinement rounds, `H \ residual` fallbacks, whether the round count is the
# same under helpers.perturbations of the point).  kind: "interior" (the problem's own point), "indefinite" (the same with P - 6 I: the inertia correction walks
# ep up), "boundary" (helpers.push_cones_to_the_boundary with default_rng(pid))
SMALL, CONES5, TREE = (3, 4, 2, 1, 1, 3), (5, 7, 3, 0, 1, 5), (40, 6, 3, 1, 1, 3)
WHOLE = {
    "interior_small": (SMALL, 0, "interior", dict(status=0, factorizations=1, ep=1.0e-7, rounds=5, fallbacks=0, rounds_stable=True)),
    "interior_tree": (TREE, 0, "interior", dict(status=0, factorizations=1, ep=1.0e-7, rounds=5, fallbacks=0, rounds_stable=True)),
    "indefinite_small": (SMALL, 0, "indefinite", dict(status=0, factorizations=13, ep=99.99999999999999, rounds=2, fallbacks=0, rounds_stable=True)),
    "indefinite_tree": (TREE, 0, "indefinite", dict(status=0, factorizations=13, ep=99.99999999999999, rounds=2, fallbacks=0, rounds_stable=True)),
    "boundary_small": (SMALL, 0, "boundary", dict(status=0, factorizations=14, ep=9999.999999999998, rounds=5, fallbacks=0, rounds_stable=True)),
    "boundary_cones5": (CONES5, 0, "boundary", dict(status=0, factorizations=15, ep=999999.9999999998, rounds=11, fallbacks=0, rounds_stable=True)),
}
# refinement failure: the oracle returns 2 with one LU fallback; the same problem at its interior point then solves with status 0
FAILURE_SHAPE, FAILURE_ID = helpers.STRUCTURED_SHAPE, helpers.STRUCTURED_ID


def whole_case(uniform, shape, pid, kind):
    """(problem, w, lam)"""
    prob, pt, lam = pr.staged_conic_qp(uniform, pid, *shape)
    if kind == "indefinite":
        prob.P = prob.P - 6.0 * np.eye(prob.nx)
        prob.Psym = prob.c * (prob.P + prob.P.T)
    if kind == "boundary":
        helpers.push_cones_to_the_boundary(prob, pt, np.random.default_rng(pid))
    return prob, np.concatenate([pt[k] for k in "xrsyzt"]), lam


def oracle_search_direction(oracle_mod, prob, w, lam):
    """the oracle's search_direction! at w from ep_last = 0: (oracle, dict(status, factorizations, ep, ep_last, ed, rounds, fallbacks))"""
    o = helpers.oracle_newton_state(oracle_mod, prob, w, lam, kappa=KAPPA, rho=RHO)
    status = o.search_direction()
    st = o.stats()
    return o, dict(status=status, factorizations=st["factorizations"], ep=float(o.buf("primal_regularization")[0]), ep_last=float(o.buf("primal_regularization_last")[0]),
                   ed=float(o.buf("dual_regularization")[0]), rounds=st["last_refinement_rounds"], fallbacks=st["lu_fallbacks"])


# ---- the sparse inputs of a problem ------------------------------------------------------------------------------------------------------------------------
def cone_layout(prob):
    """(n_nonnegative, second-order dimensions) of a problem whose cones are laid out as the handle takes them"""
    dims = [len(c) for c in prob.second_order_indices if c]
    assert prob.nonnegative_indices == list(range(1, len(prob.nonnegative_indices) + 1))
    return len(prob.nonnegative_indices), dims


def sparse_inputs(prob, extra=None):
    """(Lxx, gx, hx) as scipy CSC with the non-zero pattern of the dense prob.Psym, prob.A, -prob.G — what prob.evaluate writes into the oracle's lagrangian_hessian,
    equality_jacobian_variables and cone_jacobian_variables.  extra: a random generator; then about a fifth of the zeros are stored too (a strict superset)"""
    out = []
    for dense in (prob.Psym, prob.A, -prob.G):
        dense = np.asarray(dense, dtype=np.float64).reshape(dense.shape[0], prob.nx)
        mask = dense != 0.0
        if extra is not None and dense.size:
            more = extra.random(dense.shape) < 0.2
            if not (more & ~mask).any() and (~mask).any():
                more[tuple(np.argwhere(~mask)[0])] = True
            mask = mask | more
        rows, cols = np.nonzero(mask)
        out.append(sp.csc_matrix((dense[rows, cols], (rows, cols)), shape=dense.shape))
    return out
