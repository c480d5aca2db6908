"""Inputs shared by tests/test_sparse_differentiate_inputs_cpu.py (which pins, with the oracle alone, that each behaves as stated here) and
tests/test_gpu_sparse_differentiate.py (which holds SparseKKT.solve_columns / differentiate / vjp and torch_layer.SparseQPLayer against the oracle on them).  The
building-block cases are sparse_kkt_cases.BLOCK_CASES at kc.EP, kc.ED, kc.KAPPA, kc.RHO; the whole solve is one of sparse_solve_cases.SOLVES."""
import numpy as np

import helpers
import problems as pr
import sparse_kkt_cases as kc

# differentiate! on problems whose parameters move q, b, h (pr.parametric_conic_qp_dims: nonnegative rows first, then the cones, as the handle takes them):
# (nx, ne, n_nn, dims, tail of helpers.interior_point) — nonnegative only; no cone; no equality; cones of dimension 3 and 5 beside nonnegative rows; a cone of 70
DIFFERENTIATE = [(10, 4, 6, (), 0.3), (12, 5, 0, (), 0.3), (9, 0, 2, (3, 3), 0.3), (12, 5, 3, (3, 5), 0.3), (20, 4, 2, (70,), 0.05)]
DIFFERENTIATE_IDS = ["%d_%d_%d_%s" % (c[0], c[1], c[2], "x".join(str(d) for d in c[3]) or "none") for c in DIFFERENTIATE]
INTERIOR = dict(kappa=0.17, rho=52.0, ep=0.05, ed=0.03)      # the scalars of test_gpu_differentiate_adjoint.py

# the correction rounds: the two staged shapes without a second-order cone; the shape on which the option must be inert
REFINEMENT = ["staged_2_3_1_1_0_3", "staged_4_6_6_2_0_3"]
INERT = "staged_3_4_2_1_1_3"
REFINEMENT_COLUMNS = 3

# the whole solve: mixed cones, N = 56; the oracle solves it with status 1 and no `H \\ residual` fallback
WHOLE_SOLVE = ((3, 4, 2, 1, 1, 3), 1)
# the staged shape of the matrix-gradient test (directions supported on the patterns)
DIRECTIONAL = (3, 4, 2, 1, 1, 3)


def split(w, nx, ne, nc):
    return dict(zip("xrsyzt", np.split(np.asarray(w, dtype=np.float64), np.cumsum([nx, ne, nc, ne, nc]))))


def block_oracle(oracle_mod, name):
    """(problem, w, oracle) of a building-block case at the fixed regularisation, cone Jacobians and both residual Jacobians formed"""
    prob, pt, lam = kc.block_case(oracle_mod.splitmix_uniform, name)
    o = helpers.make_oracle(oracle_mod, prob, pt, lam, kappa=kc.KAPPA, rho=kc.RHO, ep=kc.EP, ed=kc.ED)
    o.cone(product=True, jacobian=True, target=True)
    o.residual()
    o.residual_jacobian_variables(); o.residual_jacobian_variables_symmetric()
    return prob, np.concatenate([pt[k] for k in "xrsyzt"]), o


def map_matrix(o):
    """M column by column from the oracle's search_direction_symmetric! on unit residuals, factored once (test_transposed_map_against_the_oracles_forward_map)"""
    N = o.N
    M = np.zeros((N, N))
    for j in range(N):
        o.buf("residual")[:] = 0.0
        o.buf("residual")[j] = 1.0
        o.search_direction_symmetric(0, fact=(j == 0))
        M[:, j] = o.buf("step")
    return M


def refinement_cotangents(N):
    return np.random.default_rng(17).standard_normal((N, REFINEMENT_COLUMNS))


def replay_rounds(M, H, V, tolerance, max_rounds):
    """the rounds of iterative_refinement.jl:14-44 on the reverse columns in numpy: Lambda = M' V, then E = V - H' Lambda, Lambda += M' E.  Per column: the rounds
    until |E|_inf <= tolerance (None: not within max_rounds)"""
    out = []
    for j in range(V.shape[1]):
        lam, rounds = M.T @ V[:, j], None
        for it in range(max_rounds + 1):
            E = V[:, j] - H.T @ lam
            if np.abs(E).max() <= tolerance:
                rounds = it
                break
            lam = lam + M.T @ E
        out.append(rounds)
    return out


def differentiate_case(case):
    """(problem, point dict, lam) of a DIFFERENTIATE case"""
    nx, ne, n_nn, dims, tail = case
    prob = pr.parametric_conic_qp_dims(nx, ne, n_nn, list(dims), seed=900 + nx)
    pt, lam = helpers.interior_point(prob, seed=5, tail=tail)
    return prob, pt, lam


def differentiated_oracle(oracle_mod, prob, pt, lam, scalars, slacks=None):
    """the oracle at the point with its own differentiate! run: jacobian_parameters and solution_sensitivity are its.  slacks (s, then t): the cone product
    Jacobians are formed THERE (differentiate! calls no cone!: it works on them where the last search direction left them, quirk B-12) and the point written back"""
    o = helpers.make_oracle(oracle_mod, prob, pt, lam, **scalars)
    o.buf("parameters")[:] = prob.parameters
    op = o.point()
    if slacks is not None:
        nc = prob.nc
        op["s"][:] = slacks[:nc]; op["t"][:] = slacks[nc:]
    o.cone(product=True, jacobian=True, target=True)
    if slacks is not None:
        op["s"][:] = pt["s"]; op["t"][:] = pt["t"]
    assert o.differentiate(prob) >= 0
    return o


def parametric(prob):
    """the same QP with theta = [dq; db; dh] moving q, b, h"""
    return pr.ParametricConicQP(prob.P, prob.q, prob.A, prob.b, prob.G, prob.h, nonnegative_indices=prob.nonnegative_indices,
                                second_order_indices=prob.second_order_indices, objective_scale=prob.c, name="parametric_staged_qp")


def pattern_directions(prob, seed):
    """directions supported on the patterns of P (symmetric), A, G"""
    rng = np.random.default_rng(seed)
    D = rng.standard_normal(prob.P.shape) * ((prob.P != 0.0) | (prob.P.T != 0.0))
    return 0.5 * (D + D.T), rng.standard_normal(prob.A.shape) * (prob.A != 0.0), rng.standard_normal(prob.G.shape) * (prob.G != 0.0)


def oracle_whole_solve(oracle_mod, prob):
    """the oracle's own solve! from x0 = 0 of a problem with parameters, then its own differentiate!: dict(o, status, w, dual, scalars, S, slacks = the s, t of the
    iterate its last search direction was assembled at)"""
    o, status = helpers.oracle_cold_solve(oracle_mod, prob, np.zeros(prob.nx))
    trace = o.trace().copy()
    assert trace.shape[0] >= 2
    before = split(trace[-2], prob.nx, prob.ne, prob.nc)
    assert o.differentiate(prob) >= 0
    scalars = dict(kappa=float(o.buf("central_path")[0]), rho=float(o.buf("penalty")[0]), ep=float(o.buf("primal_regularization")[0]),
                   ed=float(o.buf("dual_regularization")[0]))
    return dict(o=o, status=status, w=o.point()["all"].copy(), dual=o.buf("dual").copy(), scalars=scalars, S=o.mat("solution_sensitivity", o.N, prob.np).copy(),
                slacks=np.concatenate([before["s"], before["t"]]), **o.stats())
