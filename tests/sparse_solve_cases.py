"""Inputs shared by tests/test_sparse_solve_inputs_cpu.py (which pins, with the oracle alone, that each behaves as stated here) and tests/test_gpu_sparse_solve.py
(which holds SparseKKT.solve and its building blocks against the oracle on them).  Problems are problems.staged_conic_qp(uniform, pid, *shape) with shape =
(T, nv, nd, n_nn_stage, n_soc_stage, soc_dim), cold-started from x0 = 0; the sparse inputs are sparse_kkt_cases.sparse_inputs."""
import numpy as np

import problems as pr
import sparse_kkt_cases as kc

# whole solves without an `H \ residual` fallback anywhere; the oracle returns 1.  (shape, pid): N, total_iterations, outer iterations, accepted iterates, the most
# refinement rounds of a step
SOLVES = {
    ((2, 3, 1, 1, 0, 3), 0): dict(N=14, total_iterations=5, outer=6, accepted=4, max_rounds=1),        # smallest; nonnegative only
    ((3, 5, 2, 0, 0, 3), 0): dict(N=23, total_iterations=5, outer=5, accepted=4, max_rounds=1),        # nc = 0
    ((1, 6, 0, 2, 1, 3), 1): dict(N=21, total_iterations=6, outer=6, accepted=5, max_rounds=4),        # ne = 0
    ((3, 4, 2, 1, 1, 3), 1): dict(N=56, total_iterations=7, outer=6, accepted=6, max_rounds=5),        # mixed cones
    ((3, 4, 2, 1, 1, 3), 2): dict(N=56, total_iterations=7, outer=6, accepted=6, max_rounds=4),
    ((5, 7, 3, 0, 1, 5), 0): dict(N=134, total_iterations=7, outer=6, accepted=6, max_rounds=8),       # cones of 5 only
    ((3, 24, 4, 1, 1, 20), 2): dict(N=277, total_iterations=7, outer=6, accepted=6, max_rounds=8),     # cone dimension 20: a wavefront's
    ((6, 20, 10, 2, 2, 3), 3): dict(N=364, total_iterations=7, outer=6, accepted=6, max_rounds=7),
    ((40, 6, 3, 2, 0, 3), 0): dict(N=714, total_iterations=7, outer=6, accepted=6, max_rounds=1),      # several tree levels
    ((40, 6, 3, 4, 1, 3), 1): dict(N=1314, total_iterations=8, outer=6, accepted=7, max_rounds=8),     # nc = 280 > 256: cone rows span workgroups
}
SOLVE_IDS = ["%s-%d" % ("_".join(str(v) for v in s), p) for s, p in SOLVES]
ROUNDS_PINNED_UP_TO = 8                  # where the table's count is at most this, the handle's count is asserted equal

# refinement failures: the oracle falls back to `H \ residual`.  fallbacks, accepted iterates before the first one, accepted iterates in all (None: not pinned)
FAILURES = {
    ((3, 4, 2, 1, 1, 3), 0): dict(fallbacks=1, first_row=3, rows=5),
    ((40, 6, 3, 1, 1, 3), 3): dict(fallbacks=2, first_row=2, rows=None),
}
WARM_START = ((3, 4, 2, 1, 1, 3), 1)

# building blocks at a fixed point: the shapes of sparse_kkt_cases.BLOCK_SHAPES, cones that start at cone row 164 so that one straddles row 256, a cone of
# dimension 20 (a wavefront's) and one wider than a wavefront
BLOCK_SHAPES = kc.BLOCK_SHAPES + [(41, 6, 3, 4, 1, 3), (3, 24, 4, 1, 1, 20), (2, 80, 4, 1, 1, 70)]


def problem(uniform, shape, pid):
    return pr.staged_conic_qp(uniform, pid, *shape)[0]


def orders(n, pid):
    """two elimination orders besides the oracle's default, 1-based: the natural one and a seeded shuffle"""
    return [np.arange(1, n + 1), np.random.default_rng(100 + pid).permutation(n) + 1]


def oracle_solve(oracle_mod, prob, perm=None, start=None, options=None):
    """the oracle's solve! from x0 = 0 (or, start = (w, ...) given, warm-started from that point): dict(o, status, trace, the counters of o.stats(), accepted)"""
    o = oracle_mod.OracleSolver(prob.nx, prob.np, prob.ne, prob.nc, prob.nonnegative_indices, prob.second_order_indices)
    if perm is not None:
        o.set_perm(perm)
    for k, v in (options or {}).items():
        o.set_opt(k, v)
    if start is not None:
        o.point()["all"][:] = start
        o.set_int("warmstart", 1)
    else:
        o.point()["x"][:] = 0.0
    status = o.solve(prob)
    trace = o.trace().copy()
    return dict(o=o, status=status, trace=trace, accepted=trace.shape[0], w=o.point()["all"].copy(), dual=o.buf("dual").copy(),
                kappa=float(o.buf("central_path")[0]), rho=float(o.buf("penalty")[0]), **o.stats())
