"""CPU-side checks (no GPU needed) of the batch kernel's device-resident entries: the header declares them, the library exports them, the ctypes table carries them,
and the Python *_device methods of SmallNewtonBatch refuse what they must — CPU tensors, wrong dtypes, wrong shapes, non-contiguous tensors — with ValueError before
any C call (the handle here is a stand-in that fails the test if it is ever called)."""
import os
import re

import pytest

from helpers import ROOT, load_pkg

ENTRIES = ["calipso_hip_smallnewton_set_stream", "calipso_hip_smallnewton_set_qp_device", "calipso_hip_smallnewton_initialize_device",
           "calipso_hip_smallnewton_set_state_device", "calipso_hip_smallnewton_set_parameters_device", "calipso_hip_smallnewton_solve_device",
           "calipso_hip_smallnewton_get_solution_device", "calipso_hip_smallnewton_differentiate_adjoint_device"]


def test_header_declares_and_library_exports_the_device_entries():
    load_pkg()
    from calipso_jl_amd._lib import SYMBOLS, lib
    txt = open(os.path.join(ROOT, "include", "calipso_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = lib()
    for name in ENTRIES:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, code), "not declared: " + name
        assert name in SYMBOLS, "not in the ctypes table: " + name
        assert hasattr(L, name), "not exported: " + name
    assert hasattr(L, "calipso_hip_debug_smallnewton_buffers")
    assert re.search(r"#define\s+CALIPSO_SMALLNEWTON_ABI\s+1\b", txt)


class _NoCalls:
    """stands where the loaded library would: any C call fails the test"""

    def __getattr__(self, name):
        raise AssertionError("a C entry was reached: " + name)


def stand_in(pkg, nx=4, ne=2, nc=3, batch=5, n_parameters=None):
    sn = object.__new__(pkg.SmallNewtonBatch)
    sn._L, sn._h = _NoCalls(), None
    sn.nx, sn.ne, sn.nc, sn.batch, sn.device = nx, ne, nc, batch, 0
    sn.N = nx + 2 * ne + 3 * nc
    if n_parameters is not None:
        sn.n_parameters, sn._evaluator = n_parameters, True
    return sn


def qp_tensors(torch, sn, dtype=None):
    z = lambda *s: torch.zeros(s, dtype=dtype or torch.float64)
    B, nx, ne, nc = sn.batch, sn.nx, sn.ne, sn.nc
    return [z(B, nx, nx), z(B, nx), z(ne, nx), z(ne), z(B, nc, nx), z(nc)]


def test_device_methods_refuse_bad_tensors_before_any_c_call():
    torch = pytest.importorskip("torch")
    pkg = load_pkg()
    sn = stand_in(pkg)
    B, nx, ne, nc, N = sn.batch, sn.nx, sn.ne, sn.nc, sn.N
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)
    # CPU tensors of the right dtype, shape and layout: refused as not CUDA
    with pytest.raises(ValueError, match="CUDA"):
        sn.set_qp_device(*qp_tensors(torch, sn))
    with pytest.raises(ValueError, match="CUDA"):
        sn.initialize_device(f64(B, nx))
    with pytest.raises(ValueError, match="CUDA"):
        sn.set_state_device(w=f64(B, N))
    with pytest.raises(ValueError, match="CUDA"):
        sn.set_state_device(dual=f64(B, ne))
    with pytest.raises(ValueError, match="CUDA"):
        sn.set_state_device(scalars=f64(B, 3))
    with pytest.raises(ValueError, match="CUDA"):
        sn.solution_device(out=dict(x=f64(B, nx)))
    with pytest.raises(ValueError, match="CUDA"):
        sn.solution_device(out=dict(status=torch.zeros(B, dtype=torch.int32)))
    with pytest.raises(ValueError, match="CUDA"):
        sn.vjp_device(cotangent=f64(B, N))
    with pytest.raises(ValueError, match="CUDA"):
        sn.vjp_device(x=f64(B, nx, 3))
    # not a tensor
    import numpy as np
    with pytest.raises(ValueError, match="torch tensor"):
        sn.initialize_device(np.zeros((B, nx)))
    # wrong dtype
    with pytest.raises(ValueError, match="float64"):
        sn.set_qp_device(*qp_tensors(torch, sn, torch.float32))
    with pytest.raises(ValueError, match="float64"):
        sn.initialize_device(torch.zeros((B, nx), dtype=torch.float32))
    with pytest.raises(ValueError, match="int32"):
        sn.solution_device(out=dict(status=torch.zeros(B, dtype=torch.int64)))
    with pytest.raises(ValueError, match="float64"):
        sn.vjp_device(cotangent=torch.zeros((B, N), dtype=torch.float32))
    # wrong shape
    bad = qp_tensors(torch, sn)
    bad[2] = f64(ne + 1, nx)
    with pytest.raises(ValueError, match="A must have shape"):
        sn.set_qp_device(*bad)
    bad = qp_tensors(torch, sn)
    bad[0] = f64(B + 1, nx, nx)
    with pytest.raises(ValueError, match="P must have shape"):
        sn.set_qp_device(*bad)
    with pytest.raises(ValueError, match="shape"):
        sn.initialize_device(f64(nx))
    with pytest.raises(ValueError, match="shape"):
        sn.set_state_device(w=f64(B, N + 1))
    with pytest.raises(ValueError, match="shape"):
        sn.set_state_device(scalars=f64(B, 6))
    with pytest.raises(ValueError, match="shape"):
        sn.solution_device(out=dict(z=f64(B, nc + 1)))
    with pytest.raises(ValueError, match="shape"):
        sn.vjp_device(cotangent=f64(B, N - 1))
    with pytest.raises(ValueError, match="shape"):
        sn.vjp_device(x=f64(B, nx), y=f64(B, ne + 1))
    with pytest.raises(ValueError):
        sn.vjp_device()                                       # no cotangent
    with pytest.raises(ValueError):
        sn.vjp_device(cotangent=f64(B, N), x=f64(B, nx))      # both forms
    with pytest.raises(ValueError, match="k >= 1"):
        sn.vjp_device(cotangent=f64(B, N, 0))
    with pytest.raises(ValueError, match="reduce"):
        sn.vjp_device(cotangent=f64(B, N), reduce="Q")
    with pytest.raises(ValueError, match="unknown output"):
        sn.solution_device(out=dict(t=f64(B, nc)))
    # non-contiguous
    with pytest.raises(ValueError, match="contiguous"):
        sn.initialize_device(f64(nx, B).t())
    nc_P = qp_tensors(torch, sn)
    nc_P[0] = torch.arange(B * nx * nx, dtype=torch.float64).reshape(B, nx, nx).transpose(1, 2)
    with pytest.raises(ValueError, match="contiguous"):
        sn.set_qp_device(*nc_P)
    with pytest.raises(ValueError, match="contiguous"):
        sn.vjp_device(cotangent=f64(N, B).t())
    # the evaluator's parameters
    ev = stand_in(pkg, n_parameters=6)
    with pytest.raises(ValueError, match="CUDA"):
        ev.set_parameters_device(f64(B, 6))
    with pytest.raises(ValueError, match="shape"):
        ev.set_parameters_device(f64(B, 5))
    with pytest.raises(ValueError, match="float64"):
        ev.set_parameters_device(torch.zeros(6, dtype=torch.float32))


def test_layers_are_exported_and_the_qp_layer_keeps_its_host_path_for_cpu_tensors():
    torch = pytest.importorskip("torch")
    load_pkg()
    from calipso_jl_amd import torch_layer
    assert issubclass(torch_layer.QPLayer, torch.autograd.Function) and issubclass(torch_layer.ParametricLayer, torch.autograd.Function)
    with pytest.raises(ValueError, match="CUDA"):
        torch_layer.ParametricLayer.apply(object(), torch.zeros(3, dtype=torch.float64))
