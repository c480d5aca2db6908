"""Shared by tests/test_differentiate_wide_cones_cpu.py and tests/test_gpu_differentiate_wide_cones.py (test infrastructure): the layouts at which the one-wavefront-per-
cone kernels of csrc/soc_wide.hip change branch, the interior points and scalars, and the references — test_smallnewton_adjoint_cpu's Condensed (the condensed map and
its transpose in numpy, for any list of cone dimensions) and the oracle.  Every reference is computed once per process and handed out read-only."""
import numpy as np

import problems as pr
from helpers import interior_point, make_oracle
from test_smallnewton_adjoint_cpu import Condensed

# (nx, ne, n_nn, dims); E = elements per lane of the wide kernels, chosen from the handle's widest cone (soc_wide.hip: wide_E)
LAYOUTS = {
    "A": (12, 3, 2, [64]),            # E = 1, the wavefront exactly full
    "B": (12, 3, 2, [65]),            # first E = 2, one element in the second slot
    "C": (14, 4, 3, [128, 5]),        # last E = 2, last block in LDS; a 5-cone under E = 2 (every lane of its second slot outside the cone)
    "D": (14, 4, 3, [129, 3, 70]),    # first E = 4, first block in the cone scratch; a register cone and an E = 2-sized cone beside it
    "E": (12, 3, 2, [257]),           # first E = 8
    "F": (12, 3, 0, [513]),           # first E = 16, no nonnegative rows
    "G": (10, 0, 0, [5, 6]),          # no equalities, two adjacent wide cones of different dimension, the first wide size
}
INTERIOR = dict(kappa=0.17, rho=52.0, ep=0.05, ed=0.03)      # the scalars of the adjoint tests
ORACLE_DIFFERENTIATES = "ABCDEG"      # (the oracle's column loop takes about 15 s on F's 528 columns: there Condensed is the reference, pinned by the CPU test)
WHOLE_MAP = "ABCDG"                   # N <= 640: M' as a matrix


def frozen(a):
    a = np.array(a, dtype=np.float64)
    a.setflags(write=False)
    return a


def parameter_jacobian(prob, pt):
    """dR/dtheta (N x np) as residual_jacobian_parameters.jl:1-40 assembles it from the problem's own parameter Jacobians at the point"""
    nx, ne, nc, npar = prob.nx, prob.ne, prob.nc, prob.np
    sizes = dict(objective_jacobian_variables_parameters=nx * npar, equality_jacobian_parameters=ne * npar, equality_dual_jacobian_variables_parameters=nx * npar,
                 cone_jacobian_parameters=nc * npar, cone_dual_jacobian_variables_parameters=nx * npar)
    store = {}
    flags = (pr.OBJECTIVE_JACOBIAN_PARAMETERS | pr.EQUALITY_JACOBIAN_PARAMETERS | pr.EQUALITY_DUAL_JACOBIAN_PARAMETERS | pr.CONE_JACOBIAN_PARAMETERS |
             pr.CONE_DUAL_JACOBIAN_PARAMETERS)
    prob.evaluate(flags, pt["x"], pt["y"], pt["z"], prob.parameters, lambda name: store.setdefault(name, np.zeros(sizes[name])))
    part = lambda name, rows: store.get(name, np.zeros(rows * npar)).reshape(npar, rows).T      # column-major
    J = np.zeros((nx + 2 * ne + 3 * nc, npar))
    J[:nx] = (part("objective_jacobian_variables_parameters", nx) + part("equality_dual_jacobian_variables_parameters", nx) +
              part("cone_dual_jacobian_variables_parameters", nx))
    J[nx + ne + nc:nx + 2 * ne + nc] = part("equality_jacobian_parameters", ne)
    J[nx + 2 * ne + nc:nx + 2 * ne + 2 * nc] = part("cone_jacobian_parameters", nc)
    return J


class Case:
    """one layout at its interior point: the problem, the point, the scalars, Condensed and dR/dtheta; sensitivities and M' on first use"""

    def __init__(self, key, member=0, one_parameter=False, scalars=None):
        nx, ne, n_nn, dims = LAYOUTS[key]
        build = pr.one_parameter_conic_qp_dims if one_parameter else pr.parametric_conic_qp_dims
        self.key, self.member, self.dims, self.n_nn = key, member, list(dims), n_nn
        self.prob = build(nx, ne, n_nn, dims, seed=900 + nx + 17 * member)
        self.pt, self.lam = interior_point(self.prob, seed=5 + member, tail=0.05)
        self.sc = dict(INTERIOR if scalars is None else scalars)
        p = self.prob
        self.w = frozen(np.concatenate([self.pt[k] for k in "xrsyzt"]))
        self.cm = Condensed(2.0 * p.c * np.asarray(p.P), np.asarray(p.A).reshape(ne, nx), np.asarray(p.G).reshape(p.nc, nx), self.w, n_nn, self.dims,
                            self.sc["rho"], self.sc["ep"], self.sc["ed"])
        self.N = self.cm.N
        self.J = frozen(parameter_jacobian(p, self.pt))
        self._S = self._MT = None

    def sensitivities(self):
        """-M dR/dtheta column by column through Condensed.forward (differentiate.jl:54-56)"""
        if self._S is None:
            self._S = frozen(np.stack([-self.cm.forward(self.J[:, j]) for j in range(self.J.shape[1])], axis=1))
        return self._S

    def transposed_map(self):
        """M' column by column through Condensed.transposed"""
        if self._MT is None:
            self._MT = frozen(np.stack([self.cm.transposed(e) for e in np.eye(self.N)], axis=1))
        return self._MT

    def transposed_columns(self, V):
        return np.stack([self.cm.transposed(V[:, j]) for j in range(V.shape[1])], axis=1)

    def wide_cone_rows(self):
        """[(label, rows)]: the z, s and t rows of every cone of dimension > 4, so that a failure names the cone"""
        p, out, at = self.prob, [], self.n_nn
        oz, os_, ot = p.nx + 2 * p.ne + p.nc, p.nx + p.ne, p.nx + 2 * p.ne + 2 * p.nc
        for j, dm in enumerate(self.dims):
            if dm > 4:
                local = np.arange(at, at + dm)
                out.append(("cone %d (dimension %d)" % (j, dm), np.concatenate([oz + local, os_ + local, ot + local])))
            at += dm
        return out

    def oracle(self, oracle_mod):
        """a fresh oracle at the point: evaluated, cones and both Jacobians formed, its own copy of the parameters set"""
        o = make_oracle(oracle_mod, self.prob, self.pt, self.lam, **self.sc)
        o.buf("parameters")[:] = self.prob.parameters
        o.cone(product=True, jacobian=True, target=True)
        o.residual_jacobian_variables(); o.residual_jacobian_variables_symmetric()
        return o


_cases, _oracle_results = {}, {}


def case(key, member=0, one_parameter=False, scalars=None):
    """member i of a group: problem seed 900 + nx + 17 i, point seed 5 + i, the caller's scalars (INTERIOR when none are given)"""
    k = (key, member, one_parameter, tuple(sorted((scalars or INTERIOR).items())))
    if k not in _cases:
        _cases[k] = Case(key, member, one_parameter, scalars)
    return _cases[k]


def oracle_step(o, r, fact):
    """the oracle's search_direction_symmetric! on the residual r"""
    o.buf("residual")[:] = r
    o.search_direction_symmetric(0, fact=fact)
    return o.buf("step").copy()


def oracle_differentiate(oracle_mod, c):
    """(solution_sensitivity, jacobian_parameters) of the oracle's differentiate! at the case's point"""
    k = ("differentiate", c.key, c.member, c.prob.np)
    if k not in _oracle_results:
        o = c.oracle(oracle_mod)
        assert o.differentiate(c.prob) >= 0
        _oracle_results[k] = (frozen(o.mat("solution_sensitivity", o.N, c.prob.np)), frozen(o.mat("jacobian_parameters", o.N, c.prob.np)))
    return _oracle_results[k]


def oracle_map(oracle_mod, c):
    """the oracle's M column by column, factored once (as test_gpu_differentiate_adjoint.py builds it)"""
    k = ("map", c.key, c.member)
    if k not in _oracle_results:
        o = c.oracle(oracle_mod)
        _oracle_results[k] = frozen(np.stack([oracle_step(o, e, j == 0) for j, e in enumerate(np.eye(c.N))], axis=1))
    return _oracle_results[k]


def rel(a, ref):
    return np.abs(a - ref).max() / max(1.0, np.abs(ref).max())
