"""differentiate! on a Solver handle with set_option("differentiate_refinement", 1): the correction rounds of iterative_refinement.jl:14-44 on all parameter columns
together (calipso_hip_differentiate, csrc/columns.hip: differentiate_columns), against the oracle's differentiate! (QDLDL on the (nx + ne + nc) symmetric matrix, unrefined)
at solution-like points — penalty 1e7, central path 1e-7 — where the constraint-first condensed solve of the default path loses digits.

The 1e-8 bound: at these points the oracle's sensitivities are within 7e-10 (relative to max(1, |S|)) of an extended-precision solve of the dense H
(helpers.refined_solve), so 1e-8 leaves more than 10x headroom over the reference's own error.

Measured on an MI355X (unrefined = option off, against the oracle, relative to max(1, |S|); rounds = the largest over the columns; final norm = the largest
||dR/dtheta(:, j) - H X(:, j)||_inf):
  problem                     unrefined   refined    rounds  final norm
  cartpole (C5, p = 102)      1.97e-09    5.21e-10   1       1.5e-14
  (12,5,6,0,0) seed 300       1.42e-09    3.00e-10   1       1.5e-15
  (12,5,6,0,0) seed 301       4.78e-10    3.17e-10   1       7.2e-16
  (24,9,11,0,0)               8.36e-10    3.49e-10   1       7.1e-16
  (40,12,9,0,0)               1.08e-09    6.77e-10   1       7.2e-16
  (12,0,6,0,0) no equalities  3.33e-16    5.55e-16   1       2.2e-16
  (12,5,0,0,0) no cones       6.03e-13    2.09e-13   1       7.8e-16
  (70,20,6,0,3) stage-par.    9.37e-10    8.27e-10   1       1.0e-15
The unrefined columns of this path are thus already below 1e-8 at these points (the 1e-5 of the batch kernel's comment is not what the general path loses): what the
rounds change is the defining equation, |H S + dR/dtheta| from 1e-10 .. 1e-9 to 1e-16; against the oracle both sit at the oracle's own error.
"""
import numpy as np
import pytest

import problems as pr
from helpers import interior_point, load_pkg, make_oracle, make_pair
from test_c5_cartpole import OPTS, problem as cartpole      # (C5 is built once for both modules)
from test_oracle_solve import run as run_oracle

pytestmark = pytest.mark.gpu

TOL6 = dict(residual_tolerance=1e-6, optimality_tolerance=1e-6, equality_tolerance=1e-6, complementarity_tolerance=1e-6, slack_tolerance=1e-6)
SCALARS = (("central_path", "kappa"), ("penalty", "rho"), ("primal_regularization", "ep"), ("dual_regularization", "ed"), ("fraction_to_boundary", "tau"))
CASES = {"cartpole": None, "qp12_5_6_s300": ((12, 5, 6, 0, 0), 300), "qp12_5_6_s301": ((12, 5, 6, 0, 0), 301), "qp24_9_11": ((24, 9, 11, 0, 0), 300),
         "qp40_12_9": ((40, 12, 9, 0, 0), 300), "qp12_0_6_no_equalities": ((12, 0, 6, 0, 0), 300), "qp12_5_0_no_cones": ((12, 5, 0, 0, 0), 300),
         "qp70_20_6_stage_parallel": ((70, 20, 6, 0, 3), 300)}


def rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def problem(name):
    return cartpole() if CASES[name] is None else pr.parametric_conic_qp(*CASES[name][0], seed=CASES[name][1])


_solved = {}


def solved_point(oracle_mod, name):
    """(problem, status, point, dual, scalars) where the oracle's solve! with the five tolerances at 1e-6 ends; computed once per problem and not modified"""
    if name not in _solved:
        prob = problem(name)
        o, st = run_oracle(oracle_mod, prob, **TOL6)
        pt = {k: o.point()[k].copy() for k in "xrsyzt"}
        _solved[name] = (prob, st, pt, o.buf("dual").copy(), {kw: float(o.buf(field)[0]) for field, kw in SCALARS})
    return _solved[name]


def pair_at_solution(oracle_mod, name):
    """the oracle and a handle at that point, cone Jacobians formed (differentiate! uses those of the last cone! call), the oracle differentiated"""
    prob, st, pt, lam, sc = solved_point(oracle_mod, name)
    assert st == 1
    o, g = make_pair(oracle_mod, prob, pt, lam, **sc)
    o.buf("parameters")[:] = prob.parameters      # (make_oracle evaluates AT prob.parameters but leaves the oracle's own copy zero: its differentiate! forms dR/dtheta from that copy)
    o.cone(product=True, jacobian=True, target=True)
    g.cone(product=True, jacobian=True, target=True)
    assert o.differentiate(prob) >= 0
    return prob, o, g


def check_refined_against_oracle(prob, o, g, name):
    S_cpu = o.mat("solution_sensitivity", o.N, prob.np)
    g.differentiate()
    S_plain = g.data("solution_sensitivity")
    g.set_option("differentiate_refinement", 1)
    g.differentiate()
    S_ref = g.data("solution_sensitivity")
    info = g.differentiate_info()
    J = g.data("jacobian_parameters")
    assert np.abs(J - o.mat("jacobian_parameters", o.N, prob.np)).max() <= 1e-9      # both differentiate the same dR/dtheta
    cols = sorted({0, prob.np // 2, prob.np - 1})
    defect = lambda S: [np.abs(g.jacobian_variables_mul(S[:, j]) + J[:, j]).max() for j in cols]
    d_plain, d_ref = defect(S_plain), defect(S_ref)
    print("%s: N = %d, p = %d, max|S| = %.2e: unrefined error %.2e, refined error %.2e, rounds %d, failed columns %d, final norm %.2e, |H S + J| %s -> %s" % (
        name, o.N, prob.np, np.abs(S_cpu).max(), rel(S_plain, S_cpu), rel(S_ref, S_cpu), info["rounds"], info["failed_columns"], info["final_norm"],
        ["%.1e" % v for v in d_plain], ["%.1e" % v for v in d_ref]))
    assert np.abs(S_ref - S_cpu).max() <= 1e-8 * max(1.0, np.abs(S_cpu).max()), (np.abs(S_ref - S_cpu).max(), np.abs(S_cpu).max())
    assert info["columns"] == prob.np and info["failed_columns"] == 0 and info["rounds"] >= 1
    assert info["final_norm"] <= g.scalar("opt.iterative_refinement_tolerance"), info
    for a, b in zip(d_ref, d_plain):                 # the defining equation H S = -dR/dtheta holds no worse with the option than without
        assert a <= b, (d_ref, d_plain)


@pytest.mark.parametrize("name", [k for k in CASES if "stage_parallel" not in k])
def test_refined_columns_match_oracle_at_a_solution(oracle_mod, name):
    prob, o, g = pair_at_solution(oracle_mod, name)
    check_refined_against_oracle(prob, o, g, name)


def handle_point(h):
    w = h.solution
    pt = dict(x=w.variables, r=w.equality_slack, s=w.cone_slack, y=w.equality_dual, z=w.cone_dual, t=w.cone_slack_dual)
    return pt, h.get("dual", h.ne), {kw: h.scalar(field) for field, kw in SCALARS}


def test_c5_whole_solve_dense_and_structured(oracle_mod):
    """solve! of C5 with differentiate = 1: the sensitivities it leaves, against the oracle differentiated at the handle's own point and scalars"""
    prob = cartpole()
    pkg = load_pkg()
    st = pr.structure_from_pattern(prob)
    make = lambda opts, **kw: pkg.Solver(prob, prob.nx, prob.np, prob.ne, prob.nc, parameters=prob.parameters, options=opts, **kw)
    on = dict(OPTS, differentiate_refinement=1)
    dense, struct = make(on), make(on, structure=st)
    never, dense_off, struct_never, struct_off = make(OPTS), make(on), make(OPTS, structure=st), make(on, structure=st)
    for h in (dense_off, struct_off):
        h.set_option("differentiate_refinement", 0)
    for h in (dense, struct, never, dense_off, struct_never, struct_off):
        pkg.initialize_b(h, prob.x0)
        assert pkg.solve_b(h)
    S = {}
    for name, h in (("dense", dense), ("structured", struct)):
        pt, lam, sc = handle_point(h)
        o = make_oracle(oracle_mod, prob, pt, lam, **sc)
        o.buf("parameters")[:] = prob.parameters
        # solve! leaves the Lagrangian Hessian and the Jacobians where its last search direction left them, one iterate before the point it returns (as the reference's
        # fields, next to quirk B-12), and differentiate! works on those: the handle's own state is its point AND these fields, so they go into the oracle as well
        o.buf("objective_jacobian_variables_variables")[:] = h.get("lagrangian_hessian", prob.nx * prob.nx)
        o.buf("equality_dual_jacobian_variables_variables")[:] = 0.0
        o.buf("cone_dual_jacobian_variables_variables")[:] = 0.0
        o.buf("equality_jacobian_variables")[:] = h.get("equality_jacobian_variables", prob.ne * prob.nx)
        o.cone(product=True, jacobian=True, target=True)
        assert o.differentiate(prob) >= 0
        S_cpu = o.mat("solution_sensitivity", o.N, prob.np)
        S[name] = h.data("solution_sensitivity")
        info = h.differentiate_info()
        off = (never if name == "dense" else struct_never).data("solution_sensitivity")
        print("C5 solve!, %s handle: unrefined error %.2e, refined error %.2e, %s" % (name, rel(off, S_cpu), rel(S[name], S_cpu), info))
        assert np.abs(S[name] - S_cpu).max() <= 1e-8 * max(1.0, np.abs(S_cpu).max())
        assert info["columns"] == prob.np and info["rounds"] >= 1
    assert np.abs(S["dense"] - S["structured"]).max() <= 1e-8 * max(1.0, np.abs(S["dense"]).max())
    # option off: bitwise the sensitivities of a handle that never heard of the option, and nothing to report
    assert np.array_equal(dense_off.data("solution_sensitivity"), never.data("solution_sensitivity"))
    assert np.array_equal(struct_off.data("solution_sensitivity"), struct_never.data("solution_sensitivity"))
    assert dense_off.differentiate_info() == dict(columns=prob.np, rounds=0, failed_columns=0, final_norm=0.0)


def test_second_order_cones_leave_the_option_inert(oracle_mod):
    prob = pr.parametric_conic_qp(20, 8, 4, 2, 3, seed=20)
    pt, lam = interior_point(prob, 3)
    o, g = make_pair(oracle_mod, prob, pt, lam, ep=1e-5, ed=1e-5)
    g.cone(product=True, jacobian=True, target=True)
    g.differentiate()
    S_off = g.data("solution_sensitivity")
    g.set_option("differentiate_refinement", 1)
    g.differentiate()
    assert np.array_equal(g.data("solution_sensitivity"), S_off)
    assert g.differentiate_info() == dict(columns=prob.np, rounds=0, failed_columns=0, final_norm=0.0)


def test_refinement_options_are_honoured(oracle_mod):
    prob, o, g = pair_at_solution(oracle_mod, "qp12_5_6_s300")
    pkg = load_pkg()
    g.differentiate()
    S_off = g.data("solution_sensitivity")
    g.set_option("differentiate_refinement", 1)
    g.set_option("iterative_refinement", 0)                  # no rounds, as in the batch kernel
    g.differentiate()
    assert np.array_equal(g.data("solution_sensitivity"), S_off)
    assert g.differentiate_info()["rounds"] == 0
    g.set_option("iterative_refinement", 1)
    g.set_option("max_iterative_refinement", 1)
    g.set_option("iterative_refinement_tolerance", 0.0)      # never met: the reference's loop runs it = 0, 1
    g.differentiate()
    assert g.differentiate_info()["rounds"] == 2
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.set_option("differentiate_refinement", 2)
    assert "differentiate_refinement must be 0 or 1" in str(e.value)
    assert g.scalar("opt.differentiate_refinement") == 1.0   # the refused value changed nothing


def test_stage_parallel_factor_takes_the_corrections(oracle_mod):
    """the factor in the fronts of the multifrontal LDL^T (calipso_hip_set_stage_parallel): the correction's right-hand sides go through the tree as well"""
    name = "qp70_20_6_stage_parallel"
    prob, o, g = pair_at_solution(oracle_mod, name)
    g.analyze_structure()
    g.set_stage_parallel(True)
    check_refined_against_oracle(prob, o, g, name)


def test_repetition_same_bits_no_new_memory(oracle_mod):
    prob, o, g = pair_at_solution(oracle_mod, "qp24_9_11")
    g.set_option("differentiate_refinement", 1)
    g.differentiate()
    S1, info1, bytes1 = g.data("solution_sensitivity"), g.differentiate_info(), g.device_bytes()
    g.differentiate()
    assert np.array_equal(g.data("solution_sensitivity"), S1)
    assert g.differentiate_info() == info1
    assert g.device_bytes() == bytes1
