"""GPU (-m gpu): the device evaluators calipso.jl_amd/trajectory.py generates from per-stage functions (tests/device_eval_trajectory, built by __graft_entry__.build()):
every ProblemData field on the dense route and on the block route against the host-callback handle, tails and several workgroups, whole solves without a host
evaluation, sensitivities, groups, and the number of operations one call enqueues."""
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest

import problems as pr
from helpers import ROOT, load_pkg
from test_c5_cartpole import problem as cartpole      # (C5 is built once for the modules that use it, and not modified)
from test_oracle_solve import run as run_oracle

pytestmark = pytest.mark.gpu

FIELDS = lambda p: (("objective", 1), ("objective_gradient_variables", p.nx), ("equality_constraint", p.ne), ("cone_constraint", p.nc),
                    ("equality_dual_jacobian_variables", p.nx), ("cone_dual_jacobian_variables", p.nx), ("lagrangian_hessian", p.nx ** 2),
                    ("equality_jacobian_variables", p.ne * p.nx), ("cone_jacobian_variables", p.nc * p.nx))      # tests/test_gpu_device_eval.py:83-85


@functools.lru_cache(maxsize=1)
def tp():
    if "trajectory_problems" in sys.modules:
        return sys.modules["trajectory_problems"]
    spec = importlib.util.spec_from_file_location("trajectory_problems", os.path.join(ROOT, "tests", "device_eval_trajectory", "problems.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["trajectory_problems"] = m
    spec.loader.exec_module(m)
    return m


class Counting:
    """wraps a problem and counts host evaluations"""

    def __init__(self, prob):
        self.prob, self.calls = prob, 0

    def evaluate(self, *a):
        self.calls += 1
        return self.prob.evaluate(*a)


def host_handle(TP, prob, theta, structure=None, options=None):
    return load_pkg().Solver(prob, TP.nx, TP.np, TP.ne, TP.nc, parameters=theta, nonnegative_indices=TP.nonnegative_indices, second_order_indices=TP.second_order_indices,
                             structure=structure, options=options)


def compare_fields(dev, host, TP, seed=0):
    """both handles at one random point: every field to 1e-12 x max(1, |field|max); returns the device route's fields"""
    w = np.random.default_rng(seed).standard_normal(dev.N)
    for s in (dev, host):
        s.set("solution", w)
    dev.device_evaluate(pr.ALL_VARIABLE_FLAGS, 0)
    host.evaluate(pr.ALL_VARIABLE_FLAGS, 0)
    got = {}
    for name, ln in FIELDS(TP):
        a, b = dev.get(name, ln), host.get(name, ln)
        assert a.shape == b.shape and np.isfinite(a).all(), name
        if ln:
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), name
        got[name] = a
    return got


def test_fields_on_the_dense_route_pendulum():
    TP = tp().trajectory("pendulum")
    counted = Counting(pr.pendulum())
    dev = tp().solver("pendulum", methods=counted)
    assert dev.structure is None
    host = host_handle(TP, pr.pendulum(), np.zeros(0))
    first = compare_fields(dev, host, TP)
    # the last-writer entries are there: the Hessian differs from the exact one
    exact = host_handle(TP, pr.pendulum(hessian_mode="sum"), np.zeros(0))
    exact.set("solution", dev.get("solution", dev.N))
    exact.evaluate(pr.ALL_VARIABLE_FLAGS, 0)
    assert np.abs(first["lagrangian_hessian"] - exact.get("lagrangian_hessian", TP.nx ** 2)).max() > 1e-3
    dev.device_evaluate(pr.ALL_VARIABLE_FLAGS, 0)
    for name, ln in FIELDS(TP):
        assert np.array_equal(dev.get(name, ln), first[name]), name              # the same bits from run to run
    assert counted.calls == 0
    for s in (dev, host, exact):
        s.close()


def test_fields_on_the_block_route_cartpole_mpc():
    TP = tp().trajectory("cartpole_mpc")
    prob = cartpole()
    counted = Counting(prob)
    dev = tp().solver("cartpole_mpc", parameters=prob.parameters, methods=counted)
    assert dev.structure is not None
    host = host_handle(TP, prob, prob.parameters, structure=TP.structure())
    before = dev.device_bytes()
    got = compare_fields(dev, host, TP)
    assert dev.device_bytes() == before                                          # no dense scratch (tests/test_gpu_device_eval.py:196)
    # only the equality Jacobian asked for, at another point: the Hessian blocks keep their values
    w2 = np.random.default_rng(5).standard_normal(dev.N)
    for s in (dev, host):
        s.set("solution", w2)
    dev.device_evaluate(pr.EQUALITY_JACOBIAN, 0)
    host.evaluate(pr.EQUALITY_JACOBIAN, 0)
    assert np.array_equal(dev.get("lagrangian_hessian", TP.nx ** 2), got["lagrangian_hessian"])
    a, b = dev.get("equality_jacobian_variables", TP.ne * TP.nx), host.get("equality_jacobian_variables", TP.ne * TP.nx)
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()) and not np.array_equal(a, got["equality_jacobian_variables"])
    assert counted.calls == 0
    for s in (dev, host):
        s.close()


def test_one_jacobian_asked_for_leaves_the_cone_blocks():
    TP = tp().trajectory("cone_5")
    theta = tp().parameters("cone_5")
    dev, host = tp().solver("cone_5", parameters=theta), host_handle(TP, TP, theta, structure=TP.structure())
    got = compare_fields(dev, host, TP)
    dev.set("solution", np.random.default_rng(8).standard_normal(dev.N))
    dev.device_evaluate(pr.EQUALITY_JACOBIAN, 0)
    assert np.array_equal(dev.get("cone_jacobian_variables", TP.nc * TP.nx), got["cone_jacobian_variables"])
    assert np.array_equal(dev.get("lagrangian_hessian", TP.nx ** 2), got["lagrangian_hessian"])
    assert not np.array_equal(dev.get("equality_jacobian_variables", TP.ne * TP.nx), got["equality_jacobian_variables"])
    for s in (dev, host):
        s.close()


@pytest.mark.parametrize("name", ["ragged", "cone_2", "cone_3", "cone_65", "cone_130"])
def test_lanes_and_tails(name):
    """a single dynamics stage, fewer stages than a wavefront, a tail lane in the second wavefront, more than one workgroup — on both routes where structure() allows"""
    TP = tp().trajectory(name)
    theta = tp().parameters(name)
    routes = [False] + ([True] if TP.structure() is not None else [])
    assert routes == ([False] if name == "ragged" else [False, True])
    for structured in routes:
        dev = tp().solver(name, parameters=theta, structured=structured)
        host = host_handle(TP, TP, theta, structure=TP.structure() if structured else None)
        assert (dev.structure is not None) == structured
        compare_fields(dev, host, TP, seed=2)
        assert TP.enqueued(dev) <= 4
        for s in (dev, host):
            s.close()


def solve_three_ways(oracle_mod, name, prob, theta, x0, options=None):
    """the generated route (its host callback counted), the host-callback route on the same kind of handle, the oracle: (device handle, host handle, oracle)"""
    pkg = load_pkg()
    TP = tp().trajectory(name)
    counted = Counting(prob)
    dev = tp().solver(name, parameters=theta, methods=counted, options=options)
    host = host_handle(TP, prob, theta, structure=TP.structure(), options=options)
    for s in (dev, host):
        pkg.initialize_b(s, x0)
    assert pkg.solve_b(dev) and pkg.solve_b(host)
    assert counted.calls == 0
    o = oracle_mod.OracleSolver(TP.nx, TP.np, TP.ne, TP.nc, TP.nonnegative_indices, TP.second_order_indices)
    for k, v in (options or {}).items():
        o.set_opt(k, v) if isinstance(v, float) else o.set_int(k, v)
    if TP.np:
        o.buf("parameters")[:] = theta
    o.point()["x"][:] = x0
    assert o.solve(prob) == 1
    assert dev.stats()["total_iterations"] == host.stats()["total_iterations"] == o.stats()["total_iterations"]
    assert np.abs(dev.solution.all - host.solution.all).max() <= 1e-8 * max(1.0, np.abs(host.solution.all).max())       # tests/test_gpu_device_eval.py:95-100
    assert np.abs(dev.solution.variables - o.point()["x"]).max() <= 1e-6
    return dev, host, o


def test_pendulum_solved_without_a_host_evaluation(oracle_mod):
    TP = tp().trajectory("pendulum")
    x0 = TP.initialize_actions(TP.initialize_states(np.zeros(TP.nx), TP.linear_interpolation([0.0, 0.0], [np.pi, 0.0], TP.T)), [np.zeros(1)] * (TP.T - 1))
    dev, host, o = solve_three_ways(oracle_mod, "pendulum", pr.pendulum(action_guess=np.zeros(10)), np.zeros(0), x0)
    states, actions = TP.get_trajectory(dev)
    assert np.abs(states[0]).max() <= 1e-4 and np.abs(states[-1] - [np.pi, 0.0]).max() <= 1e-4 and len(actions) == 10      # options.equality_tolerance
    for s in (dev, host):
        s.close()


def test_cartpole_mpc_solved_on_the_structured_handle(oracle_mod):
    prob = cartpole()
    dev, host, o = solve_three_ways(oracle_mod, "cartpole_mpc", prob, prob.parameters, prob.x0)
    assert dev.structure is not None
    for s in (dev, host):
        s.close()


def test_cone_problem_solved(oracle_mod):
    TP = tp().trajectory("cone_5")
    dev, host, o = solve_three_ways(oracle_mod, "cone_5", TP, tp().parameters("cone_5"), np.zeros(TP.nx))
    assert dev.structure is not None and dev.stats()["refinement_failures"] == 0
    for s in (dev, host):
        s.close()


def test_sensitivities_of_cartpole_mpc_on_the_generated_route(oracle_mod):
    """differentiate! after the solve, evaluated by the generated kernels (the parameter flags): the tolerances of tests/test_c5_cartpole.py, with and without
    differentiate_refinement.  The oracle, like the reference, differentiates at the Hessian and the Jacobians of its last search direction, one iterate before the
    point it returns (tests/test_gpu_differentiate_refined.py:126-127): a handle with a user's device evaluator must leave them there too, so its step does not
    evaluate them ahead of the exit tests (csrc/api.hip: inner_iteration)."""
    from test_c5_cartpole import OPTS
    pkg = load_pkg()
    prob = cartpole()
    counted = Counting(prob)
    s = tp().solver("cartpole_mpc", parameters=prob.parameters, methods=counted, options=OPTS)
    pkg.initialize_b(s, prob.x0)
    assert pkg.solve_b(s)
    o, st = run_oracle(oracle_mod, prob, **OPTS)
    assert st == 1 and s.stats()["total_iterations"] == o.stats()["total_iterations"]
    assert np.abs(s.solution.all - o.point()["all"]).max() <= 1e-6 * max(1.0, np.abs(o.point()["all"]).max())
    S_cpu = o.mat("solution_sensitivity", o.N, prob.np)
    for refinement in (0, 1):
        s.set_option("differentiate_refinement", refinement)
        s.differentiate()
        assert counted.calls == 0
        assert np.abs(s.data("jacobian_parameters") - o.mat("jacobian_parameters", o.N, prob.np)).max() <= 1e-9, refinement
        S_gpu = s.data("solution_sensitivity")
        print("differentiate_refinement = %d: sensitivities %.3e from the oracle's" % (refinement, np.abs(S_gpu - S_cpu).max() / max(1.0, np.abs(S_cpu).max())))
        assert np.abs(S_gpu - S_cpu).max() <= 1e-6 * max(1.0, np.abs(S_cpu).max()), refinement
    s.close()


def test_sensitivities_against_the_oracle_at_the_handles_own_matrices(oracle_mod):
    """what differentiate! computes on the generated route is right for the state the handle holds, whatever that state is: the oracle differentiated at the handle's point and scalars AND its
    Lagrangian Hessian and Jacobian (as tests/test_gpu_differentiate_refined.py:122-139 does for the host-callback route, with that file's 1e-8: the oracle's own
    error at such points is 7e-10)"""
    from helpers import make_oracle
    from test_c5_cartpole import OPTS
    from test_gpu_differentiate_refined import handle_point
    pkg = load_pkg()
    prob = cartpole()
    counted = Counting(prob)
    s = tp().solver("cartpole_mpc", parameters=prob.parameters, methods=counted, options=dict(OPTS, differentiate_refinement=1))
    pkg.initialize_b(s, prob.x0)
    assert pkg.solve_b(s) and counted.calls == 0
    pt, lam, sc = handle_point(s)
    o = make_oracle(oracle_mod, prob, pt, lam, **sc)
    o.buf("parameters")[:] = prob.parameters
    o.buf("objective_jacobian_variables_variables")[:] = s.get("lagrangian_hessian", prob.nx * prob.nx)
    o.buf("equality_dual_jacobian_variables_variables")[:] = 0.0
    o.buf("cone_dual_jacobian_variables_variables")[:] = 0.0
    o.buf("equality_jacobian_variables")[:] = s.get("equality_jacobian_variables", prob.ne * prob.nx)
    o.cone(product=True, jacobian=True, target=True)
    assert o.differentiate(prob) >= 0
    S_cpu = o.mat("solution_sensitivity", o.N, prob.np)
    assert np.abs(s.data("solution_sensitivity") - S_cpu).max() <= 1e-8 * max(1.0, np.abs(S_cpu).max())
    s.close()


def test_group_of_three_pendulum_handles():
    """as tests/test_gpu_device_eval.py:104-125: each member bit-identical to the same handle solved alone"""
    pkg = load_pkg()
    TP = tp().trajectory("pendulum")
    states = TP.linear_interpolation([0.0, 0.0], [np.pi, 0.0], TP.T)
    guesses = [[np.full(1, a)] * (TP.T - 1) for a in (0.0, 0.5, -0.7)]

    def make(k):
        s = tp().solver("pendulum", methods=Counting(pr.pendulum()))
        pkg.initialize_b(s, TP.initialize_actions(TP.initialize_states(np.zeros(TP.nx), states), guesses[k]))
        return s

    singles = [make(k) for k in range(3)]
    for s in singles:
        assert pkg.solve_b(s)
    members = [make(k) for k in range(3)]
    g = pkg.Group(members)
    assert g.solve() == [1, 1, 1]
    for s, m in zip(singles, members):
        assert m.methods.calls == 0
        assert m.stats()["total_iterations"] == s.stats()["total_iterations"]
        assert np.array_equal(m.solution.all, s.solution.all)
    g.close()
    for s in singles + members:
        s.close()


@pytest.mark.parametrize("name", ["cone_3", "cone_130"])
def test_one_call_enqueues_at_most_four_operations(name):
    """counted by the generated host code: the table upload of the first call, the fill, the evaluation kernel, the finishing pass — whatever the horizon"""
    TP = tp().trajectory(name)
    for structured in (False, True):
        dev = tp().solver(name, parameters=tp().parameters(name), structured=structured)
        dev.set("solution", np.random.default_rng(1).standard_normal(dev.N))
        counts = []
        for flags in (pr.ALL_VARIABLE_FLAGS, pr.ALL_VARIABLE_FLAGS, (1 << 16) - 1, pr.OBJECTIVE | pr.EQUALITY | pr.CONE, pr.EQUALITY_JACOBIAN):
            dev.device_evaluate(flags, 0)
            counts.append(TP.enqueued(dev))
        assert counts == [4, 3, 3, 2, 2], counts
        dev.close()
