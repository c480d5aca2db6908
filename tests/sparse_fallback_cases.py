"""Inputs shared by tests/test_sparse_fallback_inputs_cpu.py (which pins, with the oracle alone, that each behaves as stated here) and
tests/test_gpu_sparse_fallback.py (which holds SparseKKT's `H \\ residual` fallback by preconditioned GMRES against the oracle on them).  Problems are
sparse_solve_cases.problem(uniform, shape, pid), cold-started from x0 = 0; on every one the oracle's refinement fails and it goes on to `H \\ residual`."""
import numpy as np

import helpers
import sparse_solve_cases as sc

# (shape, pid): N, the oracle's total_iterations / outer iterations / accepted iterates, its `H \ residual` fallbacks, the accepted iterates before the first one
CASES = {
    ((1, 6, 0, 2, 1, 3), 3): dict(N=21, total_iterations=7, outer=6, accepted=6, fallbacks=2, first_row=3),        # ne = 0, N below one workgroup
    ((3, 4, 2, 1, 1, 3), 0): dict(N=56, total_iterations=6, outer=6, accepted=5, fallbacks=1, first_row=3),
    ((5, 7, 3, 0, 1, 5), 4): dict(N=134, total_iterations=7, outer=6, accepted=6, fallbacks=1, first_row=3),       # cones of 5 only
    ((3, 24, 4, 1, 1, 20), 4): dict(N=277, total_iterations=9, outer=7, accepted=8, fallbacks=4, first_row=2),     # cone dimension 20: a wavefront's
    ((6, 20, 10, 2, 2, 3), 1): dict(N=364, total_iterations=7, outer=6, accepted=6, fallbacks=2, first_row=1),
    ((2, 80, 4, 1, 1, 70), 3): dict(N=594, total_iterations=9, outer=6, accepted=8, fallbacks=4, first_row=1),     # a cone wider than a wavefront
    ((40, 6, 3, 1, 1, 3), 3): dict(N=954, total_iterations=8, outer=6, accepted=7, fallbacks=2, first_row=2),      # several workgroups, several tree levels
    ((40, 6, 3, 4, 1, 3), 4): dict(N=1314, total_iterations=8, outer=6, accepted=7, fallbacks=2, first_row=5),
}
CASE_IDS = ["%s-%d" % ("_".join(str(v) for v in s), p) for s, p in CASES]
ROW_4 = ((3, 24, 4, 1, 1, 20), 4)          # the row the restart tests run on
ROW_2 = ((3, 4, 2, 1, 1, 3), 0)            # the row that guards the default (-102 without the option)
ORDERS_UP_TO = 600                         # the counts are pinned under two more elimination orders where N is at most this

KAPPA, RHO = 1.0, 1.0                      # central_path and penalty at the first fallback point: the initial ones
TOLERANCE = 1e-10                          # |R - H step|_inf a fallback has to reach
CONDITION_BOUND = 1e4                      # cond(H) at every fixed point is at most this: a residual of 1e-10 then pins the step to 1e-9 relative
STEP_AGREEMENT = 1e-9                      # ... which is the tolerance of test_gpu_fallback.py


def fixed_point(oracle_mod, prob, ref, first_row):
    """the oracle in the state in which solve! met its first fallback: the accepted iterate before it, a zero dual, the initial central_path and penalty.
    Returns (o, w, lam, R): the oracle with cones and residual evaluated, the point, the dual, the residual"""
    w = np.array(ref["trace"][first_row - 1])
    lam = np.zeros(prob.ne)
    o = helpers.oracle_newton_state(oracle_mod, prob, w, lam, kappa=KAPPA, rho=RHO)
    return o, w, lam, o.buf("residual").copy()
