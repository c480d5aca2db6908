"""The trajectory problems whose device evaluators calipso.jl_amd/trajectory.py generates for the tests, as lists of per-stage functions written ONCE: the generator
(trajectory(name)) and the flat twins the CPU tests compare it with take the same callables.

  pendulum       T = 11, test/examples/pendulum.jl:3-59: implicit midpoint dynamics (the Hessian couples x_t with x_t+1: a dense handle, quirk B-11)
  cartpole_mpc   tests/problems.py: cartpole_mpc (BASELINE config C5): explicit dynamics, 102 per-stage parameters in that problem's order, a structured handle
  ragged         num_states [2, 3, 2], num_actions [1, 2], polynomial-plus-sin stage functions, stage equalities at t = 1 and 3, two nonnegative rows at t = 2, one
                 3-dimensional second-order cone at t = 3, num_parameters [2, 0, 1]: never solved, only evaluated
  cone_T         a point mass under a bounded force: per stage two nonnegative rows (|position| <= 5), on every stage but the last ||u|| <= u_max as a 3-dimensional
                 second-order cone, theta_t = [goal; u_max] (the last stage: [goal]); explicit dynamics with a sin term: a structured handle.  cone_2, cone_3, cone_5,
                 cone_65, cone_130 are built
  cartpole_swingup_T   the cart-pole of cartpole_mpc without parameters, from rest to upright (bench/trajectory_codegen.py; one library for every horizon)

build.py compiles BUILT into this directory; `python __graft_entry__.py build` runs it.  The text of a library does not depend on the horizon: the cone_T share one."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
BUILT = ("pendulum", "cartpole_mpc", "ragged", "cone_2", "cone_3", "cone_5", "cone_65", "cone_130", "cartpole_swingup_11")


def _cartpole_discrete(h=0.05):
    import sympy as sp
    mc, mp_, l, g = 1.0, 0.2, 0.5, 9.81

    def fcont(x, u):
        s_, c_ = sp.sin(x[1]), sp.cos(x[1])
        H11, H12, H22 = mc + mp_, mp_ * l * c_, mp_ * l ** 2
        det = H11 * H22 - H12 * H12
        r0 = -mp_ * x[3] * l * s_ * x[3] + 0 - u[0]
        r1 = 0 + mp_ * g * l * s_ - 0
        return [x[2], x[3], -(H22 * r0 - H12 * r1) / det, -(-H12 * r0 + H11 * r1) / det]

    def fdisc(x, u):
        k1 = fcont(x, u)
        k2 = fcont([x[i] + 0.5 * h * k1[i] for i in range(4)], u)
        return [x[i] + h * k2[i] for i in range(4)]

    return lambda y, x, u: [y[i] - fd for i, fd in enumerate(fdisc(x, u))]


def functions(name):
    """the arguments of codegen.TrajectoryProblem for the problem `name` (without hessian= and name=)"""
    import sympy as sp
    if name == "pendulum":
        T, h = 11, 0.05

        def pendulum_continuous(x, u):
            mass, length_com, gravity, damping = 1.0, 0.5, 9.81, 0.1
            return [x[1], u[0] / (mass * length_com * length_com) - gravity * sp.sin(x[0]) / length_com - damping * x[1] / (mass * length_com * length_com)]

        def pendulum_discrete(y, x, u):
            f = pendulum_continuous([0.5 * (x[i] + y[i]) for i in range(2)], u)
            return [y[i] - (x[i] + h * f[i]) for i in range(2)]

        stage = lambda x, u: 0.1 * (x[0] ** 2 + x[1] ** 2) + 0.1 * u[0] ** 2
        final = lambda x, u: 0.1 * (x[0] ** 2 + x[1] ** 2)
        initial, goal = [0.0, 0.0], [sp.pi, 0.0]
        return dict(objective=[stage] * (T - 1) + [final], dynamics=[pendulum_discrete] * (T - 1), num_states=[2] * T, num_actions=[1] * (T - 1),
                    equality=[lambda x, u: [x[i] - initial[i] for i in range(2)]] + [None] * (T - 2) + [lambda x, u: [x[i] - goal[i] for i in range(2)]])
    if name == "cartpole_mpc":
        T = 10
        dyn = _cartpole_discrete()
        # theta_t = [xbar(4); ubar(1); w_Q(4); w_R(1); x_init(4) if t = 1], theta_T = [xbar(4); w_Q(4)]
        stage = lambda x, u, w: sum(0.5 * w[5 + i] ** 2 * (x[i] - w[i]) ** 2 for i in range(4)) + 0.5 * w[9] ** 2 * (u[0] - w[4]) ** 2
        final = lambda x, u, w: sum(0.5 * w[4 + i] ** 2 * (x[i] - w[i]) ** 2 for i in range(4))
        return dict(objective=[stage] * (T - 1) + [final], dynamics=[dyn] * (T - 1), num_states=[4] * T, num_actions=[1] * (T - 1),
                    equality=[lambda x, u, w: [x[i] - w[10 + i] for i in range(4)]] + [None] * (T - 1), num_parameters=[14] + [10] * (T - 2) + [8])
    if name == "ragged":
        return dict(
            num_states=[2, 3, 2], num_actions=[1, 2], num_parameters=[2, 0, 1],
            objective=[lambda x, u, w: w[0] * x[0] ** 2 + sp.sin(x[1]) * u[0] + 0.5 * u[0] ** 2 + w[1] * x[1],
                       lambda x, u: x[0] * x[1] * x[2] + 0.3 * u[0] ** 2 * u[1] + sp.sin(u[1]) + 0.5 * x[2] ** 2,
                       lambda x, u, w: (x[0] - w[0]) ** 2 + 0.25 * x[1] ** 4],
            dynamics=[lambda y, x, u, w: [y[0] - x[0] * x[1] - w[0] * u[0], y[1] - sp.sin(x[0] + y[1]) - u[0] ** 2, y[2] - x[1] * y[0] - w[1]],
                      lambda y, x, u: [y[0] - x[0] * u[0] - sp.sin(x[2] * y[0]), y[1] * y[0] - x[1] ** 2 - u[1]]],
            equality=[lambda x, u, w: [x[0] * u[0] - w[1], sp.sin(x[1]) - 0.1], None, lambda x, u, w: [x[0] ** 2 + x[1] - w[0]]],
            nonnegative=[None, lambda x, u: [1.0 + x[0] - u[0] ** 2, 2.0 - x[1] * x[2] + sp.sin(u[1])], None],
            second_order=[None, None, [lambda x, u, w: [2.0 + x[0] ** 2 + w[0], x[0] * x[1], sp.sin(x[1])]]])
    if name.startswith("cone_"):
        T, h = int(name[5:]), 0.1
        dyn = lambda y, x, u: [y[0] - (x[0] + h * x[1]), y[1] - (x[1] + h * (u[0] + u[1] - 0.5 * sp.sin(x[0])))]
        stage = lambda x, u, w: 0.5 * (x[0] - w[0]) ** 2 + 0.05 * x[1] ** 2 + 0.05 * (u[0] ** 2 + u[1] ** 2)
        final = lambda x, u, w: 5.0 * (x[0] - w[0]) ** 2 + 0.5 * x[1] ** 2
        box = lambda x, u: [5.0 + x[0], 5.0 - x[0]]
        force = lambda x, u, w: [w[1], u[0], u[1]]
        return dict(objective=[stage] * (T - 1) + [final], dynamics=[dyn] * (T - 1), num_states=[2] * T, num_actions=[2] * (T - 1),
                    equality=[lambda x, u: [x[0] + 1.0, x[1]]] + [None] * (T - 1), nonnegative=[box] * T, second_order=[[force]] * (T - 1) + [None],
                    num_parameters=[2] * (T - 1) + [1])
    if name.startswith("cartpole_swingup_"):
        T = int(name[len("cartpole_swingup_"):])
        dyn = _cartpole_discrete()
        stage = lambda x, u: 0.05 * (x[0] ** 2 + (x[1] - sp.pi) ** 2 + x[2] ** 2 + x[3] ** 2) + 0.05 * u[0] ** 2
        final = lambda x, u: 5.0 * (x[0] ** 2 + (x[1] - sp.pi) ** 2 + x[2] ** 2 + x[3] ** 2)
        return dict(objective=[stage] * (T - 1) + [final], dynamics=[dyn] * (T - 1), num_states=[4] * T, num_actions=[1] * (T - 1),
                    equality=[lambda x, u: [x[i] for i in range(4)]] + [None] * (T - 1))
    raise KeyError(name)


def parameters(name):
    """theta for the solves of the tests"""
    if name.startswith("cone_"):
        T = int(name[5:])
        return np.array([v for t in range(T - 1) for v in (1.0, 2.0)] + [1.0])
    if name == "cartpole_mpc":
        sys.path.insert(0, os.path.join(ROOT, "tests")) if os.path.join(ROOT, "tests") not in sys.path else None
        import problems as pr
        return pr.cartpole_mpc().parameters
    if name == "ragged":
        return np.array([0.7, -0.4, 1.3])
    return np.zeros(0)


def library_name(name):
    """the cone problems of every horizon share one library (and one name in it)"""
    return "trajectory_" + ("cone" if name.startswith("cone_") else "cartpole_swingup" if name.startswith("cartpole_swingup_") else name)


def load_codegen():
    """calipso.jl_amd/codegen.py as calipso_jl_amd.codegen (the package directory's name is not importable)"""
    import importlib.util
    if "calipso_jl_amd" not in sys.modules:
        path = os.path.join(ROOT, "calipso.jl_amd")
        spec = importlib.util.spec_from_file_location("calipso_jl_amd", os.path.join(path, "__init__.py"), submodule_search_locations=[path])
        m = importlib.util.module_from_spec(spec)
        sys.modules["calipso_jl_amd"] = m
        spec.loader.exec_module(m)
    import calipso_jl_amd.codegen as codegen
    return codegen


_made = {}


def trajectory(name, hessian="reference"):
    """codegen.TrajectoryProblem of `name` (cached: deriving the cart-pole takes seconds)"""
    if (name, hessian) not in _made:
        _made[(name, hessian)] = load_codegen().TrajectoryProblem(name=library_name(name), hessian=hessian, **functions(name))
    return _made[(name, hessian)]


def solver(name, **kw):
    """TP.solver() on the library build.py left in this directory"""
    return trajectory(name).solver(directory=HERE, **kw)
