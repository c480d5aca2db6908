"""CPU (no GPU): the reverse mode of differentiate! on Solver handles (calipso_hip_differentiate_adjoint) — the entries are exported and refuse a NULL handle, and the
transposed map that csrc/adjoint.hip and the wide-cone kernels of csrc/soc_wide.hip implement (test_smallnewton_adjoint_cpu's Condensed, the numpy statement of it)
holds for WIDE second-order cones as well: dimension 20 (one element per lane on the device) and 70 (two), pinned to the oracle's search_direction_symmetric! before
any device run."""
import ctypes as C

import numpy as np
import pytest

import problems as pr
from helpers import interior_point, load_pkg
from test_smallnewton_adjoint_cpu import Condensed


def test_entries_are_exported_and_refuse_a_null_handle():
    load_pkg()
    from calipso_jl_amd._lib import SYMBOLS, lib
    L = lib()
    for name in ("calipso_hip_differentiate_adjoint", "calipso_hip_differentiate_adjoint_info", "calipso_hip_differentiate_adjoint_times"):
        assert name in SYMBOLS and hasattr(L, name)
    ERR_ARGUMENT = -4      # CALIPSO_ERR_ARGUMENT (include/calipso_hip.h)
    v = np.zeros(4)
    pd = v.ctypes.data_as(C.POINTER(C.c_double))
    from calipso_jl_amd._lib import EVAL_FN
    assert L.calipso_hip_differentiate_adjoint(None, EVAL_FN(), None, 1, pd, pd, None, None) == ERR_ARGUMENT
    assert L.calipso_hip_differentiate_adjoint_info(None, pd) == ERR_ARGUMENT
    assert L.calipso_hip_differentiate_adjoint_times(None, pd) == ERR_ARGUMENT


@pytest.mark.parametrize("layout", [(14, 4, 3, 1, 20), (20, 4, 2, 1, 70)])
def test_transposed_map_with_wide_cones(oracle_mod, layout):
    nx, ne, nnn, nsoc, sdim = layout
    prob = pr.parametric_conic_qp(nx, ne, nnn, nsoc, sdim, seed=900 + nx)
    kappa, tau, rho, ep, ed = 0.17, 0.99, 52.0, 0.05, 0.03
    pt, lam = interior_point(prob, seed=5, tail=0.05)
    o = oracle_mod.OracleSolver(prob.nx, prob.np, prob.ne, prob.nc, prob.nonnegative_indices, prob.second_order_indices)
    op = o.point()
    for f in "xrsyzt":
        op[f][:] = pt[f]
    o.buf("dual")[:] = lam
    for name, val in (("central_path", kappa), ("penalty", rho), ("primal_regularization", ep), ("dual_regularization", ed), ("fraction_to_boundary", tau)):
        o.buf(name)[0] = val
    prob.evaluate(pr.ALL_VARIABLE_FLAGS, op["x"], op["y"], op["z"], prob.parameters, o.buf)
    o.cone(product=True, jacobian=True, target=True)
    o.residual_jacobian_variables(); o.residual_jacobian_variables_symmetric()
    cm = Condensed(2.0 * prob.c * np.asarray(prob.P), np.asarray(prob.A).reshape(ne, nx), np.asarray(prob.G).reshape(prob.nc, nx), op["all"].copy(), nnn,
                   [sdim] * nsoc, rho, ep, ed)
    rng = np.random.default_rng(11)
    for j in range(3):
        r = rng.standard_normal(cm.N)
        o.buf("residual")[:] = r
        o.search_direction_symmetric(0, fact=(j == 0))
        Mr = o.buf("step").copy()
        assert np.abs(cm.forward(r) - Mr).max() <= 1e-10 * max(1.0, np.abs(Mr).max())
    M = np.stack([cm.forward(e) for e in np.eye(cm.N)], axis=1)
    MT = np.stack([cm.transposed(e) for e in np.eye(cm.N)], axis=1)
    assert np.abs(MT - M.T).max() <= 1e-12 * np.abs(M).max()
