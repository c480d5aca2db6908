"""Inputs shared by tests/test_sparse_solve_group_inputs_cpu.py (which pins, with the oracle alone, that each member behaves as stated here),
tests/test_sparse_solve_group_host_cpu.py (which replays the lockstep of csrc/sparse_solve_group.hpp on what the oracle does on them) and
tests/test_gpu_sparse_solve_group.py (which holds SparseKKTGroup.solve against single SparseKKT handles, bit for bit, and against the oracle).  Members are
problems.staged_conic_qp(uniform, pid, *shape), cold-started from x0 = 0 with the default options unless stated: one shape, so one pattern."""
import numpy as np

import problems as pr
import sparse_solve_cases as sc

SMALL, LIMIT, TREE, WIDE = (3, 4, 2, 1, 1, 3), (2, 3, 1, 1, 0, 3), (40, 6, 3, 4, 1, 3), (3, 24, 4, 1, 1, 20)
SIZES = {SMALL: 56, LIMIT: 14, TREE: 1314, WIDE: 277}                # N

# members the oracle solves without an `H \ residual` fallback: pid -> accepted iterates
SOLVED = {
    SMALL: {1: 6, 2: 6, 3: 5, 4: 5, 5: 6, 6: 6, 7: 6},
    LIMIT: {0: 4, 1: 5, 2: 5, 3: 5, 4: 5, 5: 4, 6: 5, 7: 5},
    TREE: {0: 6, 1: 7, 2: 9, 7: 7},
    WIDE: {2: 6},
}
TREE_OUTER = {0: 6, 1: 6, 2: 7, 7: 6}                                 # outer iterations: the members leave at different ticks
TREE_ROUNDS_AT_MOST = {0: 9, 1: 8, 2: 11, 7: 11}                      # the most refinement rounds of a step
# members that meet a refinement failure (WIDE: all but pid 2): pid -> accepted iterates before the first one (None: not pinned, only that there is one)
FAILING = {SMALL: {0: 3}, WIDE: {0: 3, 1: None, 3: None, 4: None, 5: None, 6: None, 7: None}, TREE: {3: None, 4: None, 5: None, 6: None}}

# the groups of the GPU tests: (shape, pids)
GROUP_SMALL_SOLVED = (SMALL, [1, 2, 3, 4, 5, 6, 7])
GROUP_SMALL_WITH_FAILURE = (SMALL, [0, 1, 2, 3])
GROUP_TREE = (TREE, [0, 1, 2, 7])
GROUP_WIDE = (WIDE, [2, 0])
GROUP_LIMIT = (LIMIT, [k % 8 for k in range(128)])
PLACES_PID = 2                                                        # SMALL: alone, member 0 of 3, member 2 of 3, 8 identical members

# Line-search trials.  With the oracle, cold from x0 = 0, NO member (pids 0 .. 7) of the four shapes takes a trial in any step, under the default
# scaling_line_search and under 0.9 and 0.25 (the first two pinned by the CPU test for SMALL and LIMIT); nor did warm starts from other members' solved points or
# from perturbed duals and slacks.  The one member found with the oracle: SMALL pid 7 warm-started from its solved point with x perturbed (line_search_start) runs its
# seventh step's line search to the cap of 25 trials — but only after the oracle's `H \ residual` fallback (first after 4 accepted iterates), which a group does not
# have, so a device solve does not walk that path.  The group the GPU test uses is therefore one in which the DEVICE route takes trials: SMALL pids 1, 0, 2 cold
# with continue_after_refinement_failure = 1, where member pid 0 goes on past its refinement failure and runs line searches while pids 1 and 2 take no trial in
# any step (their oracle solves, pinned, are fallback-free and trial-free).  It is held against single handles with the same option, bit for bit.
LINE_SEARCH_GROUP = (SMALL, [1, 0, 2], 0, dict(continue_after_refinement_failure=1))
LINE_SEARCH_ORACLE = dict(shape=SMALL, pid=7, scale=4.0, seed=7000, trials=[0, 0, 0, 0, 0, 0, 25, 0], first_fallback_row=4)


def line_search_start(oracle_mod, case=LINE_SEARCH_ORACLE):
    """the point the oracle's member with line-search trials is warm-started from: its solved point with x perturbed"""
    prob = sc.problem(oracle_mod.splitmix_uniform, case["shape"], case["pid"])
    w = sc.oracle_solve(oracle_mod, prob)["w"].copy()
    w[:prob.nx] += case["scale"] * np.random.default_rng(case["seed"]).standard_normal(prob.nx)
    return w


CANDIDATE_FLAGS =pr.OBJECTIVE | pr.EQUALITY | pr.CONE                # what solve! evaluates at a candidate (solve.jl:231-250, 278-297)


class CountingProblem:
    """a problem that records the flags of every evaluate! the oracle asks for: the oracle's stats() do not count line-search trials, its callbacks show them"""

    def __init__(self, prob):
        self._prob, self.flags = prob, []

    def __getattr__(self, name):
        return getattr(self._prob, name)

    def evaluate(self, flags, x, y, z, theta, out):
        self.flags.append(int(flags))
        return self._prob.evaluate(flags, x, y, z, theta, out)


def candidates_per_step(flags):
    """the candidates each accepted step of a solve evaluated, from the flags of its callbacks: 1 + its line-search trials (a run of candidate evaluations is a step's)"""
    out, run = [], 0
    for f in list(flags) + [0]:
        if f == CANDIDATE_FLAGS:
            run += 1
        elif run:
            out.append(run)
            run = 0
    return out


def oracle_solve_counting(oracle_mod, shape, pid, options=None, start=None):
    """(problem, the oracle's solve as sparse_solve_cases.oracle_solve gives it, line-search trials per accepted step)"""
    prob = sc.problem(oracle_mod.splitmix_uniform, shape, pid)
    counting = CountingProblem(prob)
    ref = sc.oracle_solve(oracle_mod, counting, options=options, start=start)
    return prob, ref, [c - 1 for c in candidates_per_step(counting.flags)]


# ---- what the oracle reads step by step on a member's cold solve: the recording that tests/sparse_solve_group_host replays ------------------------------------------
OPT = dict(residual_tolerance=1.0e-4, slack_tolerance=1.0e-4, equality_tolerance=1.0e-4, complementarity_tolerance=1.0e-4, optimality_tolerance=1.0e-4,
           central_path_update_tolerance=10.0, central_path_scaling=0.2, central_path_exponent=1.5, penalty_scaling=10.0, max_penalty=1.0e8, scaling_line_search=0.5,
           max_residual_line_search=25, max_cone_line_search=25, max_outer_iterations=10, max_residual_iterations=100, violation_tolerance=1.0e-5, merit_tolerance=1.0e-5,
           violation_exponent=1.1, merit_exponent=2.3, armijo_tolerance=1.0e-4, machine_tolerance=1.0e-16, max_iterative_refinement=10,
           primal_regularization_initial=1.0e-7, dual_regularization_initial=1.0e-7, min_regularization=1.0e-20, max_regularization=1.0e40, dual_regularization=1.0e-8,
           dual_regularization_exponent=0.25, scaling_regularization_initial=100.0, scaling_regularization=8.0, scaling_regularization_last=1.0 / 3.0)
MASK_WORDS = 26                                                       # step_decisions.hpp: CONE_MASK_WORDS


def record_solve(oracle_mod, shape, pid):
    """The cold solve of a member walked through the ORACLE's building blocks, solve.jl:8-377 line by line, recording in the order a lockstep consumes them:
    ("P" | "A", published block of 16, |g|_inf, |s o t|_inf) a prologue at the start / after an outer update, or behind an accepted iterate; ("S", inertias, norms)
    what search_direction! reads (one inertia triple per factorisation of inertia_correction!, |R - H step|_inf before the first and after every refinement round);
    ("C", slack masks, dual masks, a_s, a_t, merit, violation, dd) the cone search and first candidate; ("T", merit, violation) a line-search trial.  The walk only
    decides what is evaluated next; that it is the oracle's walk is asserted against the oracle's own solve!: every accepted iterate against its trace, the counts,
    the central path and the penalty.  A member whose refinement fails stops there (the oracle goes on through `H \\ residual`, a group does not).  Returns
    (records, want) with want = the oracle's status (-102 for that member), counts, kappa, rho and primal_regularization_last"""
    import helpers
    o_ = OPT
    prob = sc.problem(oracle_mod.splitmix_uniform, shape, pid)
    ref = sc.oracle_solve(oracle_mod, prob)
    nx, ne, nc = prob.nx, prob.ne, prob.nc
    N = nx + 2 * ne + 3 * nc
    off = np.cumsum([0, nx, ne, nc, ne, nc, nc])                       # x, r, s, y, z, t
    w = np.zeros(N)
    if ne:
        w[off[1]:off[2]] = np.asarray(prob.A).reshape(ne, nx) @ w[:nx] - np.asarray(prob.b).reshape(-1)
    interior = np.zeros(nc)
    interior[np.asarray(prob.nonnegative_indices, dtype=int) - 1] = 1.0
    for cone in prob.second_order_indices:
        if cone:
            interior[np.asarray(cone, dtype=int) - 1] = 0.1
            interior[cone[0] - 1] = 1.0
    w[off[2]:off[3]] = interior; w[off[5]:off[6]] = interior
    kappa, rho, lam, ep_last = 1.0, 1.0, np.zeros(ne), 0.0
    tau = max(0.99, 1.0 - kappa)
    inf = lambda v: float(np.abs(v).max()) if v.size else 0.0

    def state():
        o = helpers.oracle_newton_state(oracle_mod, prob, w, lam, kappa=kappa, rho=rho, tau=tau)
        o.merit_gradient()
        return o

    def block(o):
        R, p = o.buf("residual"), o.point()
        f, barrier = float(o.buf("objective")[0]), float(o.buf("barrier")[0])
        M = o.merit(f, p["r"], barrier)
        theta = o.constraint_violation(o.buf("equality_constraint"), p["r"], o.buf("cone_constraint"), p["s"])
        return [f, barrier, float(np.dot(lam, p["r"])), float(np.dot(p["r"], p["r"])), M, theta, 0.0, 0.0, float(np.abs(R).sum()), inf(R[:off[3]]), inf(R[off[3]:off[4]]),
                inf(R[off[4]:off[5]]), inf(R[off[5]:]), float(np.abs(p["y"]).sum()), float(np.abs(p["z"]).sum()), float(np.abs(p["t"]).sum())]

    def exit_kind(b, eqv, cpv, o):
        sd = max(100.0, (b[13] + b[14]) / (ne + nc)) / 100.0 if ne + nc else 1.0
        scn = max(100.0, b[15] / nc) / 100.0 if nc else 1.0
        optimality = max(b[9] / sd, b[10], b[11], b[12] / scn)
        assert abs(optimality - o.optimality_error()) <= 1e-12 * max(1.0, optimality)          # the norms above are the oracle's optimality_error
        if b[8] / N < o_["residual_tolerance"] and max(b[10], b[11]) < o_["slack_tolerance"] and eqv <= o_["equality_tolerance"] and cpv <= o_["complementarity_tolerance"]:
            return 1
        return 2 if optimality <= max(o_["central_path_update_tolerance"] * kappa, o_["optimality_tolerance"]) else 0

    def search_direction():
        whole = state()
        whole.buf("primal_regularization_last")[0] = ep_last
        status = whole.search_direction()
        st = whole.stats()
        got = dict(status=status, factorizations=st["factorizations"], rounds=st["last_refinement_rounds"], ep=float(whole.buf("primal_regularization")[0]),
                   ep_last=float(whole.buf("primal_regularization_last")[0]), ed=float(whole.buf("dual_regularization")[0]))
        o = state()
        R = o.buf("residual").copy()
        good = (nx, ne + nc, 0)

        def factorize(ep, ed):
            o.buf("primal_regularization")[0] = ep; o.buf("dual_regularization")[0] = ed
            o.residual_jacobian_variables(); o.residual_jacobian_variables_symmetric()
            o.factorize(update=False)
            return o.compute_inertia()
        ep, ed, first, inertias = o_["primal_regularization_initial"], o_["dual_regularization_initial"], True, []
        while True:                                                   # step_decisions.hpp: ic_after
            inertias.append(factorize(ep, ed))
            if inertias[-1] == good:
                break
            if first:
                if inertias[-1][2] != 0:
                    ed = o_["dual_regularization"] * kappa ** o_["dual_regularization_exponent"]
                ep, first = max(o_["min_regularization"], o_["scaling_regularization_last"] * ep_last), False
                continue
            ep = (o_["scaling_regularization_initial"] if ep_last == 0.0 else o_["scaling_regularization"]) * ep
            assert ep <= o_["max_regularization"]
        assert len(inertias) == got["factorizations"] and ep == got["ep"] and status in (0, 2), (inertias, got)
        o.search_direction_symmetric(0, fact=False)
        step, norms = o.buf("step").copy(), []
        for k in range(got["rounds"] + 1):
            err = R - o.H_mul(step)
            norms.append(inf(err))
            if k < got["rounds"]:
                o.buf("residual")[:] = err
                o.search_direction_symmetric(0, fact=False)
                step = step + o.buf("step")
        return whole, got, inertias, norms

    def candidate(o, step, a_s, a_t, first):
        cand, pt = o.point("candidate"), o.point()
        parts = dict(zip("xrsyzt", np.split(step, off[1:6])))
        for name in "xrs":
            cand[name][:] = pt[name] - a_s * parts[name]
        if first:
            cand["t"][:] = pt["t"] - a_t * parts["t"]
        prob.evaluate(CANDIDATE_FLAGS, cand["x"], pt["y"], pt["z"], np.zeros(0), o.buf)
        o.cone(which=1, barrier=True, barrier_gradient=True)
        Mh = o.merit(float(o.buf("objective")[0]), cand["r"], float(o.buf("barrier")[0]))
        return Mh, o.constraint_violation(o.buf("equality_constraint"), cand["r"], o.buf("cone_constraint"), cand["s"])

    def switching_and_armijo(theta, M, Mh, dd, a):
        switching = dd < 0.0 and a * (-dd) ** o_["merit_exponent"] > theta ** o_["violation_exponent"]
        return switching and Mh - M - 10.0 * o_["machine_tolerance"] * abs(M) <= o_["armijo_tolerance"] * a * dd

    def accepts(filt, theta, M, thetah, Mh, dd, a):                   # step_decisions.hpp: line_search_accepts with the filter's verdict
        if not all(thetah < ft or Mh < fm for ft, fm in filt):
            return False
        if theta <= o_["slack_tolerance"] and switching_and_armijo(theta, M, Mh, dd, a):
            return True
        mach = o_["machine_tolerance"]
        return thetah - 10.0 * mach * abs(theta) <= (1.0 - o_["violation_tolerance"]) * theta or Mh - 10.0 * mach * abs(M) <= M - o_["merit_tolerance"] * theta

    records, filt = [], []
    o = state()
    b, eqv, cpv = block(o), inf(o.buf("equality_constraint")[:ne]), 0.0          # solve.jl:85-86: the cone product as it lies before it is first formed
    records.append(("P", b, eqv, cpv))
    outer, inner, accepted, status, factorizations, max_rounds = 1, 1, 0, None, 0, 0
    while status is None:
        kind = 2 if inner > o_["max_residual_iterations"] else exit_kind(b, eqv, cpv, o)
        if kind == 1:
            status = 1
            break
        if kind == 2:                                                 # solve.jl:356-368
            kappa = max(o_["residual_tolerance"] / 10.0, min(o_["central_path_scaling"] * kappa, kappa ** o_["central_path_exponent"]))
            tau = max(0.99, 1.0 - kappa)
            lam = lam + rho * w[off[1]:off[2]]
            rho = min(max(o_["penalty_scaling"] * rho, 1.0 / kappa), o_["max_penalty"])
            filt = []
            if outer >= o_["max_outer_iterations"]:
                status = 0
                break
            o = state()
            b = block(o)
            records.append(("P", b, eqv, cpv))
            outer, inner = outer + 1, 1
            continue
        whole, got, inertias, norms = search_direction()
        records.append(("S", inertias, norms))
        factorizations, max_rounds, ep_last = factorizations + got["factorizations"], max(max_rounds, got["rounds"]), got["ep_last"]
        if got["status"] == 2:
            status = -102
            break
        step = whole.buf("step").copy()
        dd = float(np.dot(whole.buf("merit_gradient"), step[:nx + ne + nc]))
        masks, sizes = [], []
        for name in ("cone_slack", "cone_slack_dual"):
            idx, words, a, size = whole.index(name) - 1, [0] * MASK_WORDS, 1.0, None
            for k in range(o_["max_cone_line_search"] + 1):
                if whole.cone_violation(w[idx] - a * step[idx], w[idx], tau):
                    words[k >> 5] |= 1 << (k & 31)
                elif size is None:
                    size = a
                a = o_["scaling_line_search"] * a
            assert size is not None
            masks.append(words); sizes.append(size)
        a, a_t = sizes
        M, theta = b[4], b[5]
        Mh, thetah = candidate(whole, step, a, a_t, True)
        records.append(("C", masks[0], masks[1], a, a_t, Mh, thetah, dd))
        trials = 0
        while trials < o_["max_residual_line_search"] and not accepts(filt, theta, M, thetah, Mh, dd, a):
            a = o_["scaling_line_search"] * a
            Mh, thetah = candidate(whole, step, a, a_t, False)
            records.append(("T", Mh, thetah))
            trials += 1
        if not switching_and_armijo(theta, M, Mh, dd, a):            # filter.jl:52-89 (the pairs that the new one dominates leave)
            pair = ((1.0 - o_["violation_tolerance"]) * theta, M - o_["merit_tolerance"] * theta)
            if not filt or all(pair[0] < ft or pair[1] < fm for ft, fm in filt):
                filt = [pair] + [(ft, fm) for ft, fm in filt if not (ft >= pair[0] and fm >= pair[1])]
        parts = dict(zip("xrsyzt", np.split(step, off[1:6])))
        new = np.concatenate([w[off[0]:off[3]] - a * step[off[0]:off[3]], w[off[3]:off[5]] - a * step[off[3]:off[5]], w[off[5]:] - a_t * parts["t"]])
        row = ref["trace"][accepted]
        assert np.abs(new - row).max() <= 1e-9 * max(1.0, np.abs(row).max()), (pid, accepted, np.abs(new - row).max())      # the oracle's own accepted iterate
        w = row.copy()
        accepted, inner = accepted + 1, inner + 1
        o = state()
        b, eqv, cpv = block(o), inf(o.buf("equality_constraint")[:ne]), inf(o.buf("cone_product")[:nc])
        records.append(("A", b, eqv, cpv))
    want = dict(status=status, total_iterations=accepted + 1, outer=outer, accepted=accepted, factorizations=factorizations, max_rounds=max_rounds, kappa=kappa, rho=rho,
                ep_last=ep_last, sizes=(N, ne, nc, nx))
    if status == 1:                                                   # the walk was the oracle's: its counts, its scalars, its last regularisation
        assert (ref["status"], ref["total_iterations"], ref["outer"], ref["accepted"]) == (1, want["total_iterations"], outer, accepted), (want, ref["outer"])
        assert abs(kappa - ref["kappa"]) <= 1e-15 and abs(rho - ref["rho"]) <= 1e-9 * max(1.0, ref["rho"])
        assert ep_last == float(ref["o"].buf("primal_regularization_last")[0])
    else:
        assert status == -102 and accepted == ref["first_lu_fallback_row"]
    return records, want


def recording_text(recordings, continue_after_refinement_failure=False):
    """the recordings of a group's members (record_solve, in member order) as the text tests/sparse_solve_group_host/main.cpp replays (`main recorded`); floats by
    repr, which round-trips"""
    N, ne, nc, nx = recordings[0][1]["sizes"]
    lines = ["%d %d %d %d %d %d" % (N, ne, nc, nx, len(recordings), int(continue_after_refinement_failure))]
    for records, _ in recordings:
        lines.append(str(len(records)))
        for r in records:
            if r[0] in "PA":
                lines.append(" ".join([r[0]] + [repr(float(v)) for v in list(r[1]) + [r[2], r[3]]]))
            elif r[0] == "S":
                lines.append(" ".join(["S", str(len(r[1])), str(len(r[2]))] + [str(int(v)) for t in r[1] for v in t] + [repr(float(v)) for v in r[2]]))
            elif r[0] == "C":
                lines.append(" ".join(["C"] + [str(int(v)) for v in list(r[1]) + list(r[2])] + [repr(float(v)) for v in r[3:]]))
            else:
                lines.append(" ".join(["T", repr(float(r[1])), repr(float(r[2]))]))
    return "\n".join(lines) + "\n"
