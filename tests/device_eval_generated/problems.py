"""The functions of the problems whose device evaluators calipso.jl_amd/codegen.py generates for the tests, written ONCE: the generator (generated(name)) and the
oracle's host callbacks (symbolic(name): tests/problems.py: SymbolicProblem) take the same callables.

  nonlinear_cone  (nx, ne, nc, np) = (3, 1, 2, 3)      tests/device_eval_small/nonlinear_cone.hip, tests/test_gpu_smallnewton_evaluator.py: nonlinear_cone
  friction_cone   (3, 0, 3, 5), one second-order cone  tests/device_eval_small/friction_cone.hip, ...: friction_cone
  cartpole_mpc    (49, 40, 0, 102)                     tests/device_eval_small/cartpole_mpc.hip, tests/problems.py: cartpole_mpc (BASELINE config C5)
  chain           (80, 78, 0, 78)                      only evaluated, never solved: g_j = x_j x_{j+1} x_{j+2} - theta_j, f = sum_i 1/2 (x_i - 1)^2 + 0.1 x_i^4;
                                                        its Jacobian's three diagonals have 78 members each, more than one wavefront
  no_parameters   (2, 1, 2, 0)                         f(x) alone: an evaluator without theta and without dR/dtheta

build.py compiles BUILT into this directory; `python __graft_entry__.py build` runs it."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
BUILT = ("nonlinear_cone", "friction_cone", "cartpole_mpc", "no_parameters")
NAMES = BUILT + ("chain",)


def _cartpole(horizon=10, h=0.05):
    """the functions of tests/problems.py: cartpole_mpc (examples/autotuning/cartpole.jl:85-146, models/cartpole.jl:2-33)"""
    import sympy as sp
    ns, na, T = 4, 1, horizon
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

    xs = lambda z, t: z[t * (ns + na): t * (ns + na) + ns]
    us = lambda z, t: z[t * (ns + na) + ns: t * (ns + na) + ns + na]
    offs = [0]
    for t in range(T - 1):
        offs.append(offs[-1] + (14 if t == 0 else 10))

    def objective(z, th):
        J = 0
        for t in range(T - 1):
            w = th[offs[t]:]
            X, U = xs(z, t), us(z, t)
            J += sum(0.5 * w[5 + i] ** 2 * (X[i] - w[i]) ** 2 for i in range(4)) + 0.5 * w[9] ** 2 * (U[0] - w[4]) ** 2
        w = th[offs[T - 1]:]
        XT = xs(z, T - 1)
        return J + sum(0.5 * w[4 + i] ** 2 * (XT[i] - w[i]) ** 2 for i in range(4))

    def equality(z, th):
        e = []
        for t in range(T - 1):
            X, U, Y = xs(z, t), us(z, t), xs(z, t + 1)
            fd = fdisc(X, U)
            e += [Y[i] - fd[i] for i in range(4)]
        return e + [xs(z, 0)[i] - th[10 + i] for i in range(4)]

    return dict(num_variables=ns * T + na * (T - 1), objective=objective, equality=equality, cone=None, num_parameters=offs[-1] + 8)


def functions(name):
    """the arguments of codegen.Problem for the problem `name`"""
    if name == "nonlinear_cone":
        return dict(num_variables=3, num_parameters=3,
                    objective=lambda x, th: (1 - x[0]) ** 2 + 10 * (x[1] - x[0] ** 2) ** 2 + 0.5 * x[2] ** 2,
                    equality=lambda x, th: [x[0] + x[1] + x[2] - th[0]],
                    cone=lambda x, th: [th[1] - x[0] ** 2 - x[1] ** 2, x[2] + th[2] - x[0] * x[1]])
    if name == "friction_cone":
        return dict(num_variables=3, num_parameters=5,
                    objective=lambda x, th: 0.5 * ((x[0] - th[0]) ** 2 + (x[1] - th[1]) ** 2 + (x[2] - th[2]) ** 2) + 0.25 * th[4] * x[0] ** 4,
                    equality=None, cone=lambda x, th: [th[3] * (x[0] + 1), x[1], x[2]], nonnegative_indices=[], second_order_indices=[[1, 2, 3]])
    if name == "cartpole_mpc":
        return _cartpole()
    if name == "chain":
        n = 80
        return dict(num_variables=n, num_parameters=n - 2,
                    objective=lambda x, th: sum(0.5 * (x[i] - 1) ** 2 + 0.1 * x[i] ** 4 for i in range(n)),
                    equality=lambda x, th: [x[j] * x[j + 1] * x[j + 2] - th[j] for j in range(n - 2)], cone=None)
    if name == "no_parameters":
        return dict(num_variables=2, num_parameters=0, objective=lambda x: (x[0] - 1) ** 2 + (x[1] + 0.5) ** 2 + 0.1 * x[0] ** 4,
                    equality=lambda x: [x[0] + x[1] - 0.2], cone=lambda x: [x[0], 1 - x[1] ** 2])
    raise KeyError(name)


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


def generated(name):
    """codegen.Problem of `name`; its entry is generated_<name>_kernels (the hand-written fixtures keep <name>_kernels)"""
    return load_codegen().Problem(name="generated_" + name, **functions(name))


def symbolic(name, **kw):
    """the oracle's twin of `name` from the same callables (parameters / x0 as the caller sets them)"""
    if os.path.join(ROOT, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
    import problems as pr
    a = functions(name)
    return pr.SymbolicProblem(a["num_variables"], a["objective"], a.get("equality"), a.get("cone"), np_=a["num_parameters"],
                              nonnegative_indices=a.get("nonnegative_indices"), second_order_indices=a.get("second_order_indices"), name=name, **kw)
