"""Inputs shared by tests/test_sparse_kkt_group_host_cpu.py (which records, with the oracle alone, what every member's search_direction! does and replays the
lockstep bookkeeping on it) and tests/test_gpu_sparse_kkt_group.py (which holds calipso.jl_amd.SparseKKTGroup against the oracle and against single SparseKKT
handles).  Members are (pid, kind) of tests/sparse_kkt_cases.py: one shape, so one pattern — sparse_inputs() of a shape is the same for every pid and kind."""
import numpy as np

import helpers
import sparse_kkt_cases as kc

# the group of mixed walks on SMALL = (3, 4, 2, 1, 1, 3), N = 56: (pid, kind) -> factorisations, refinement rounds, status of the oracle, the same under all three
# helpers.perturbations of the point ((1, "boundary") is left out: its round count moves under perturbation)
MIXED = [((0, "interior"), (1, 5, 0)), ((0, "indefinite"), (13, 2, 0)), ((0, "boundary"), (14, 5, 0)),
         ((1, "interior"), (1, 3, 0)), ((2, "boundary"), (14, 8, 0)), ((3, "boundary"), (14, 11, 2))]
MIXED_FACTOR_ROUNDS, MIXED_REFINE_ROUNDS = 14, 11                     # the maxima over the members: what a lockstep call runs
SLOWEST = (3, "boundary")                                              # the member that alone takes as many rounds of both kinds
# three members of TREE = (40, 6, 3, 1, 1, 3), N = 954, several tree levels, all pid 0: kind -> factorisations, rounds
TREE_GROUP = [((0, "interior"), (1, 5)), ((0, "indefinite"), (13, 2)), ((0, "boundary"), (15, 11))]
# with max_regularization = 1e3 the boundary members of MIXED walk to ep ~ 1e4 and fail, the indefinite one stops at ep ~ 100 and passes
FAILING_MAX_REGULARIZATION = 1.0e3
FAILING_STATUSES = [0, 0, -1, 0, -1, -1]
LIMIT_SHAPE = (2, 3, 1, 1, 0, 3)                                       # the group of 128: pids cycling over 0 .. 3

# the defaults of include/calipso_options.hpp the recording below walks with (options.jl:6-59)
IC = dict(primal_regularization_initial=1.0e-7, dual_regularization_initial=1.0e-7, min_regularization=1.0e-20, max_regularization=1.0e40, dual_regularization=1.0e-8,
          dual_regularization_exponent=0.25, scaling_regularization_initial=100.0, scaling_regularization=8.0, scaling_regularization_last=1.0 / 3.0)


def member(uniform, shape, pid, kind):
    """(problem, w, lam) of a member"""
    return kc.whole_case(uniform, shape, pid, kind)


def record(oracle_mod, prob, w, lam, max_regularization=None):
    """what the oracle's search_direction! reads on its way at the point w from ep_last = 0, step by step through the oracle's building blocks: dict(inertias: one
    triple per factorisation of inertia_correction! (inertia.jl:30-80), norms: |R - H step|_inf before the first and after every refinement round
    (iterative_refinement.jl:1-52), want: the oracle's own search_direction! on the same state: status, factorisations, rounds, regularisation).  The walk below only
    decides WHERE the next factorisation is taken (IC-2 .. IC-6); that it took the oracle's walk is asserted against the oracle's own counts and regularisation"""
    opt = dict(IC)
    if max_regularization is not None:
        opt["max_regularization"] = max_regularization
    whole = helpers.oracle_newton_state(oracle_mod, prob, w, lam, kappa=kc.KAPPA, rho=kc.RHO)
    if max_regularization is not None:
        whole.set_opt("max_regularization", max_regularization)
    status = whole.search_direction()
    st = whole.stats()
    want = dict(status=status, factorizations=st["factorizations"], rounds=st["last_refinement_rounds"], ep=float(whole.buf("primal_regularization")[0]),
                ep_last=float(whole.buf("primal_regularization_last")[0]), ed=float(whole.buf("dual_regularization")[0]))
    o = helpers.oracle_newton_state(oracle_mod, prob, w, lam, kappa=kc.KAPPA, rho=kc.RHO)
    R = o.buf("residual").copy()
    good = (prob.nx, prob.ne + prob.nc, 0)

    def factorize(ep, ed):
        o.buf("primal_regularization")[0] = ep; o.buf("dual_regularization")[0] = ed
        o.residual_jacobian_variables(); o.residual_jacobian_variables_symmetric()
        o.factorize(update=False)
        return o.compute_inertia()

    ep, ed, ep_last, failed = opt["primal_regularization_initial"], opt["dual_regularization_initial"], 0.0, False
    inertias = [factorize(ep, ed)]
    if inertias[-1] != good:
        if inertias[-1][2] != 0:
            ed = opt["dual_regularization"] * kc.KAPPA ** opt["dual_regularization_exponent"]
        ep = max(opt["min_regularization"], opt["scaling_regularization_last"] * ep_last)
        while True:
            inertias.append(factorize(ep, ed))
            if inertias[-1] == good:
                break
            ep = (opt["scaling_regularization_initial"] if ep_last == 0.0 else opt["scaling_regularization"]) * ep
            if ep > opt["max_regularization"]:
                failed = True
                break
    assert failed == (status == -1) and len(inertias) == want["factorizations"], (len(inertias), want)
    assert failed or ep == want["ep"], (ep, want)
    norms = []
    if not failed:
        o.search_direction_symmetric(0, fact=False)
        step = o.buf("step").copy()
        for k in range(want["rounds"] + 1):
            err = R - o.H_mul(step)
            norms.append(float(np.abs(err).max()))
            if k < want["rounds"]:
                o.buf("residual")[:] = err
                o.search_direction_symmetric(0, fact=False)
                step = step + o.buf("step")
    return dict(inertias=inertias, norms=norms, want=want)
