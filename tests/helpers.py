"""shared test helpers: package loader (the package directory is named `calipso.jl_amd`, not importable by name) and
construction of an (oracle, HIP) solver pair in identical states."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_pkg():
    if "calipso_jl_amd" in sys.modules:
        return sys.modules["calipso_jl_amd"]
    path = os.path.join(ROOT, "calipso.jl_amd")
    spec = importlib.util.spec_from_file_location("calipso_jl_amd", os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    m = importlib.util.module_from_spec(spec)
    sys.modules["calipso_jl_amd"] = m
    spec.loader.exec_module(m)
    return m


def interior_point(prob, seed, tail=0.3):
    """tail: scale of the second-order cone tails (head = 1 + |tail|): wide cones need a smaller one to stay as far inside the cone, relatively,
    as the small ones (the upper-triangle symmetrisation of the reference, quirk B-3, is the coarser the closer to the boundary)"""
    rng = np.random.default_rng(seed)
    pt = dict(x=rng.standard_normal(prob.nx), r=rng.random(prob.ne), s=0.5 + rng.random(prob.nc), y=rng.standard_normal(prob.ne),
              z=rng.standard_normal(prob.nc), t=0.5 + rng.random(prob.nc))
    for c in prob.second_order_indices:
        if c:
            i = np.array(c) - 1
            pt["s"][i[1:]] = tail * rng.standard_normal(len(i) - 1)
            pt["t"][i[1:]] = tail * rng.standard_normal(len(i) - 1)
            pt["s"][i[0]] = 1.0 + np.linalg.norm(pt["s"][i[1:]])
            pt["t"][i[0]] = 1.0 + np.linalg.norm(pt["t"][i[1:]])
    lam = rng.standard_normal(prob.ne)
    return pt, lam


def make_oracle(oracle_mod, prob, pt, lam, kappa=0.17, rho=52.0, ep=0.12, ed=0.21, tau=0.99):
    """oracle solver holding the problem data, the iterate and the scalars"""
    import problems as pr
    o = oracle_mod.OracleSolver(prob.nx, prob.np, prob.ne, prob.nc, prob.nonnegative_indices, prob.second_order_indices)
    op = o.point()
    for k in "xrsyzt":
        op[k][:] = pt[k]
    o.buf("dual")[:] = lam
    for name, v in (("central_path", kappa), ("penalty", rho), ("primal_regularization", ep), ("dual_regularization", ed), ("fraction_to_boundary", tau)):
        o.buf(name)[0] = v
    prob.evaluate(pr.ALL_VARIABLE_FLAGS, op["x"], op["y"], op["z"], prob.parameters, o.buf)
    return o


def make_pair(oracle_mod, prob, pt, lam, kappa=0.17, rho=52.0, ep=0.12, ed=0.21, tau=0.99):
    """oracle solver and HIP solver holding the same problem data, iterate and scalars"""
    import problems as pr
    pkg = load_pkg()
    o = make_oracle(oracle_mod, prob, pt, lam, kappa, rho, ep, ed, tau)
    g = pkg.Solver(prob, prob.nx, prob.np, prob.ne, prob.nc, parameters=prob.parameters,
                   nonnegative_indices=prob.nonnegative_indices, second_order_indices=prob.second_order_indices)
    for name, v in (("central_path", kappa), ("penalty", rho), ("primal_regularization", ep), ("dual_regularization", ed), ("fraction_to_boundary", tau)):
        g.set(name, [v])
    g.set("solution", o.point()["all"].copy())
    if prob.ne:
        g.set("dual", lam)
    g.evaluate(pr.ALL_VARIABLE_FLAGS, 0)
    return o, g


def near_boundary_point(prob, seed):
    """interior point whose second-order cone slacks / duals sit close to the cone boundary with unrelated directions: the
    upper-triangle symmetrisation of the condensed SOC blocks is then so coarse that iterative refinement diverges and
    search_direction! takes its `H \\ residual` fallback (search_direction.jl:22)"""
    rng = np.random.default_rng(seed)
    pt, lam = interior_point(prob, seed)
    push_cones_to_the_boundary(prob, pt, rng)
    return pt, lam


def push_cones_to_the_boundary(prob, pt, rng):
    """the cone part of near_boundary_point on any point dict: new second-order slacks / duals, 1e-6 .. 1e-2 (relative) inside their cones"""
    for c in prob.second_order_indices:
        if c:
            i = np.array(c) - 1
            u = rng.standard_normal(len(i) - 1); v = rng.standard_normal(len(i) - 1)
            pt["s"][i[1:]] = u; pt["s"][i[0]] = (1 + 10 ** rng.uniform(-6, -2)) * np.linalg.norm(u)
            pt["t"][i[1:]] = v; pt["t"][i[0]] = (1 + 10 ** rng.uniform(-6, -2)) * np.linalg.norm(v)


# ---- inputs of the `H \ residual` fallback tests --------------------------------------------------------------------------------
# Shared by tests/test_fallback_inputs_cpu.py, which pins with the oracle alone that every input below decides clearly (falls back / does
# not, also under perturbations of 1e-9; the LU systems are well conditioned and really pivot), and by tests/test_gpu_fallback_paths.py.

# N = nx + 2 ne + 3 nc of the unreduced system -> (nx, ne, nonnegative rows, second-order cones, cone dimension): a single partial panel of the
# LU (N < 32), N around its panel width 32 and the 64-wide tiles of the trailing GEMM, an exact multiple of 32 (96), and panels of more than
# 1024 rows (the stride of k_lu_panel's loops over rows)
LU_EDGE_SHAPES = {1: (1, 0, 0, 0, 3), 7: (2, 1, 1, 0, 3), 31: (10, 3, 2, 1, 3), 32: (11, 3, 2, 1, 3), 33: (12, 3, 2, 1, 3),
                  63: (24, 6, 3, 2, 3), 64: (25, 6, 3, 2, 3), 65: (26, 6, 3, 2, 3), 96: (28, 10, 4, 3, 4),
                  1023: (553, 100, 30, 20, 3), 1024: (554, 100, 30, 20, 3), 1025: (555, 100, 30, 20, 3), 2049: (1109, 200, 60, 40, 3)}
LU_STRIDED_SHAPE = (500, 200, 80, 40, 3)          # oy = 900 < 1024 < ot = 1300, N = 1500
LU_STRIDED_COLUMN, LU_STRIDED_EQUALITY = 5, 150   # the pivot of column 5 is the y-row of equality 150: row 900 + 150 = 1050


def lu_edge_case(N):
    """(problem, point, lam) of the LU edge case with an N x N unreduced system, for ep = ed = 0 (zero diagonal in the s-, y- and z-rows)"""
    import problems as pr
    prob = pr.parametric_conic_qp(*LU_EDGE_SHAPES[N], seed=N)
    pt, lam = interior_point(prob, 5)
    return prob, pt, lam


def lu_strided_case():
    """the case built for the strided row loops of k_lu_panel: variable x_c (c = LU_STRIDED_COLUMN < 32) scaled down by 2^-30 everywhere but in one
    equality, whose y-row sits at index 1050 >= 1024: that row is the partial pivot of column c of the FIRST panel (its 1500 rows take two strides of
    the 1024 threads); a search that misses it divides by an entry 2^-30 times smaller instead"""
    import problems as pr
    prob = pr.parametric_conic_qp(*LU_STRIDED_SHAPE, seed=77)
    c, k, sigma = LU_STRIDED_COLUMN, LU_STRIDED_EQUALITY, 2.0 ** -30
    prob.P[c, :] *= sigma; prob.P[:, c] *= sigma
    prob.A[:, c] *= sigma; prob.G[:, c] *= sigma
    prob.A[k, c] = 1.0
    prob.Psym = prob.c * (prob.P + prob.P.T)
    pt, lam = interior_point(prob, 5)
    return prob, pt, lam


def refined_solve(H, R):
    """(x, x_lapack): x_lapack = LAPACK's partially pivoted LU solve of H x = R, x = the same refined with residuals in numpy.longdouble until the
    correction is below 1e-18 relative"""
    import scipy.linalg as sla
    lu = sla.lu_factor(H)
    x0 = sla.lu_solve(lu, R)
    Hl, Rl, x = H.astype(np.longdouble), R.astype(np.longdouble), x0.astype(np.longdouble)
    for _ in range(10):
        d = sla.lu_solve(lu, (Rl - Hl @ x).astype(np.float64))
        x = x + d
        if np.abs(d).max() <= 1e-18 * np.abs(x).max():
            return x, x0
    raise AssertionError("refinement of the reference did not settle")


def lapack_row_interchanges(H):
    """(pivot rows of LAPACK's LU, 0-based: row piv[k] was swapped into position k; number of real interchanges)"""
    import scipy.linalg as sla
    piv = sla.lu_factor(H)[1]
    return piv, int((piv != np.arange(H.shape[0])).sum())


def perturbations(w):
    """the three copies every fallback / no-fallback input must decide the same on: +-1e-9 relative, +1e-9 absolute"""
    w = np.asarray(w, dtype=np.float64)
    return [w * (1.0 + 1e-9), w * (1.0 - 1e-9), w + 1e-9]


# Newton-step cases on the synthetic conic QPs of tests/test_gpu_group.py's build(): (shape, problem id).  With the cone parts of the point pushed to the boundary
# the ids of STEP_FALLBACK take the fallback (and only they are used that way); at build()'s own interior point the ids of STEP_NO_FALLBACK settle in 3 to 5 rounds
SHAPE_S, SHAPE_M, SHAPE_L = (60, 20, 8, 6, 3), (300, 140, 40, 20, 3), (1100, 60, 10, 10, 3)      # SHAPE_L: nx pads to NP = 1536 = 1024 + 512: the left-looking plan and the W-form
# of the solves are live, and with the W-form the queue-ahead schedules of the step (api.hip: spec_refinement_ok)
STEP_FALLBACK = [(SHAPE_S, 5), (SHAPE_S, 8), (SHAPE_M, 8), (SHAPE_M, 9), (SHAPE_L, 8)]
STEP_NO_FALLBACK = [(SHAPE_S, 3), (SHAPE_S, 4), (SHAPE_S, 5), (SHAPE_S, 6), (SHAPE_M, 0), (SHAPE_M, 1), (SHAPE_L, 8)]
# The step the fallback leaves at such a point is cut back hard by the cone search: its halving loop (solve.jl:190-221) needs up to 33 halvings on these cases, more
# than the default max_cone_line_search = 25 admits (the reference raises "cone search failure" there).  The Newton-step tests therefore run their handles with
# max_cone_line_search = CONE_SEARCH_LIMIT; test_fallback_inputs_cpu.py pins that the oracle's step needs at most CONE_SEARCH_PINNED halvings
CONE_SEARCH_LIMIT, CONE_SEARCH_PINNED = 60, 40
SINGLE_HANDLE = [(SHAPE_S, 5), (SHAPE_L, 8)]                                      # one handle, whole Newton step, every schedule
# (shape, [(problem id, pushed to the boundary = falls back)]): the base handle (member 0) falls back / only later members do
MIXED_GROUPS = [(SHAPE_S, [(5, True), (3, False), (8, True), (4, False)]),
                (SHAPE_S, [(3, False), (5, True), (4, False), (8, True), (6, False)]),
                (SHAPE_M, [(0, False), (8, True), (1, False), (9, True)])]
NAN_GROUP = (SHAPE_S, [3, 4, 6])                                                  # interior members; the middle one gets a NaN in q
STRUCTURED_SHAPE, STRUCTURED_ID = (6, 20, 10, 2, 2, 3), 4                         # staged_conic_qp: N = 364; falls back at the boundary
# cold-started solve! of parametric_conic_qp from x0 = 0: (shape, seed, total_iterations, lu_fallbacks, accepted iterates before the first fallback) of the oracle
SOLVES = [((12, 5, 4, 2, 3), 0, 12, 1, 1), ((12, 5, 4, 2, 3), 1, 15, 1, 7), ((12, 5, 4, 2, 3), 2, 8, 0, -1), ((12, 5, 4, 2, 3), 3, 9, 1, 4),
          ((30, 8, 4, 6, 3), 0, 15, 0, -1), ((30, 8, 4, 6, 3), 1, 9, 0, -1), ((30, 8, 4, 6, 3), 2, 13, 2, 7), ((30, 8, 4, 6, 3), 3, 10, 0, -1),
          ((20, 6, 3, 3, 4), 0, 9, 0, -1), ((20, 6, 3, 3, 4), 1, 10, 0, -1), ((20, 6, 3, 3, 4), 2, 10, 1, 6), ((20, 6, 3, 3, 4), 3, 13, 6, 2)]
SOLVE_GROUPS = [((12, 5, 4, 2, 3), [0, 1, 2, 3]), ((20, 6, 3, 3, 4), [0, 1, 2, 3])]      # Group.solve(): members with and without fallbacks


def synthetic_step_case(uniform, pid, shape, boundary):
    """(problem, w, lam): the synthetic conic QP `pid` of tests/test_gpu_group.py's build() at its own interior point, or (boundary) with the cone
    parts of that point overwritten as near_boundary_point does (generator seeded with pid)"""
    import problems as pr
    prob, pt, lam = pr.synthetic_conic_qp(uniform, pid, *shape)
    if boundary:
        push_cones_to_the_boundary(prob, pt, np.random.default_rng(pid))
    return prob, np.concatenate([pt[k] for k in "xrsyzt"]), lam


def staged_step_case(uniform, pid, shape, boundary):
    """the same for the stage-structured QP of tests/test_gpu_blocks.py's build_structured()"""
    import problems as pr
    prob, pt, lam = pr.staged_conic_qp(uniform, pid, *shape)
    if boundary:
        push_cones_to_the_boundary(prob, pt, np.random.default_rng(pid))
    return prob, np.concatenate([pt[k] for k in "xrsyzt"]), lam


def oracle_newton_state(oracle_mod, prob, w, lam, kappa=0.17, rho=52.0, tau=0.99):
    """the oracle in the state in which a Newton step (calipso_hip_newton_step on a handle of test_gpu_group.build) calls search_direction! at the
    point w: cones and residual evaluated, the regularisation left to inertia_correction! (it starts from the options' initial values)"""
    import problems as pr
    o = oracle_mod.OracleSolver(prob.nx, 0, prob.ne, prob.nc, prob.nonnegative_indices, prob.second_order_indices)
    o.point()["all"][:] = w
    o.buf("dual")[:] = lam
    o.buf("central_path")[0] = kappa; o.buf("penalty")[0] = rho; o.buf("fraction_to_boundary")[0] = tau
    o.set_int("linear_solve_refactor", 0)
    op = o.point()
    prob.evaluate(pr.ALL_VARIABLE_FLAGS, op["x"], op["y"], op["z"], np.zeros(0), o.buf)
    o.cone(product=True, jacobian=True, target=True, barrier=True, barrier_gradient=True)
    o.residual()
    return o


def cone_search_halvings(o, w):
    """the halving loops of the cone search (solve.jl:190-221) on the oracle's step at the point w: (step size, halvings) for the cone slacks and for their duals"""
    so, out = np.array(o.buf("step")), []
    for name in ("cone_slack", "cone_slack_dual"):
        idx = o.index(name) - 1
        a, k = 1.0, 0
        while o.cone_violation(w[idx] - a * so[idx], w[idx], o.buf("fraction_to_boundary")[0]) and k < 1000:
            a *= 0.5; k += 1
        out.append((a, k))
    return out


def oracle_cold_solve(oracle_mod, prob, x0):
    """solve! of the oracle from initialize!(solver, x0): (oracle, status)"""
    o = oracle_mod.OracleSolver(prob.nx, prob.np, prob.ne, prob.nc, prob.nonnegative_indices, prob.second_order_indices)
    o.buf("parameters")[:] = prob.parameters
    o.point()["x"][:] = x0
    return o, o.solve(prob)
