"""The shared pieces of differentiate! on the sparse handle (calipso.jl_amd/csrc/sparse_differentiate.hpp: the per-row and per-cone arithmetic of the condensed solve's
four maps, the workspace layout, the argument checks) on the CPU: tests/sparse_differentiate_host/main.cpp includes only that header and sparse_kkt.hpp, is built
with the plain host compiler under the address and undefined-behaviour sanitizers, and run as a child process.  Also here: the new entries resolve in the built
library and refuse a NULL handle."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT, load_pkg

ENTRIES = ["solve_columns", "solve_columns_device", "differentiate", "differentiate_device", "differentiate_adjoint", "differentiate_adjoint_device", "differentiate_info",
           "differentiate_adjoint_info", "differentiate_adjoint_times"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("sparse_differentiate") / "sparse_differentiate")
    # (gcc links the sanitizer runtimes dynamically unless told otherwise; clang links them statically by itself and does not know gcc's two flags)
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtimes = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"] +
                           static_runtimes + [os.path.join(ROOT, "tests", "sparse_differentiate_host", "main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def run(program, *args):
    r = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_each_transposed_map_is_the_transpose_of_its_forward_map(program):
    """an equality row, a nonnegative row, cones of dimension 2, 3, 5 and 70 at ep = 0.12, ed = 0.21, rho = 52: within 64 eps (largest entry), asserted by the program"""
    lines = run(program, "maps").splitlines()
    print("\n".join(lines))
    assert [l.split()[:2] for l in lines[:-1]] == [["equality", "1"], ["nonnegative", "1"]] + [["second_order", str(d)] for d in (2, 3, 5, 70)]
    assert all(l.endswith(" ok") for l in lines[:-1]) and lines[-1] == "maps ok"
    for l in lines[2:-1]:                                   # (the cones' maps are not the identity: the deviations are measured, not zero by construction)
        assert max(float(v) for v in l.split()[3:8:2]) > 0.0


def test_the_workspace_layout_has_no_overlap_and_stays_in_bounds(program):
    assert run(program, "layout") == "layout ok cases=324\n"


def test_the_argument_checks(program):
    assert run(program, "checks").splitlines() == [
        "ok", "ok", "differentiate: k: at least one column, not 0", "differentiate: k: at least one column, not -3",
        "differentiate: k: at most 65535 columns in one call (the multi-column solve's grid limit), not 65536", "ok", "solve_columns: B is NULL", "ok", "ok",
        "differentiate_adjoint: grad: no QP attached (calipso_hip_sparse_kkt_qp_attach first)",
        "differentiate_adjoint: grad: no point resident (calipso_hip_sparse_kkt_initialize, or set_values with w, first)", "option 1 1 0 0 0"]


def test_the_new_entries_resolve_and_refuse_a_null_handle():
    load_pkg()
    from calipso_jl_amd._lib import SYMBOLS, lib
    L = lib()
    for n in ENTRIES:
        assert "calipso_hip_sparse_kkt_" + n in SYMBOLS
        getattr(L, "calipso_hip_sparse_kkt_" + n)
    ERR_ARGUMENT = -4
    assert L.calipso_hip_sparse_kkt_solve_columns(None, 1, 0, None, None) == ERR_ARGUMENT
    assert L.calipso_hip_sparse_kkt_solve_columns_device(None, 1, 0, None, None) == ERR_ARGUMENT
    assert L.calipso_hip_sparse_kkt_differentiate(None, 1, None, None) == ERR_ARGUMENT
    assert L.calipso_hip_sparse_kkt_differentiate_device(None, 1, None, None) == ERR_ARGUMENT
    assert L.calipso_hip_sparse_kkt_differentiate_adjoint(None, 1, None, None, None) == ERR_ARGUMENT
    assert L.calipso_hip_sparse_kkt_differentiate_adjoint_device(None, 1, None, None, None) == ERR_ARGUMENT
    for n in ENTRIES[6:]:
        assert getattr(L, "calipso_hip_sparse_kkt_" + n)(None, None) == ERR_ARGUMENT
    assert L.calipso_hip_sparse_kkt_differentiate_bytes(None, None) == ERR_ARGUMENT


def test_the_layer_and_the_methods_are_exported():
    pkg = load_pkg()
    from calipso_jl_amd import torch_layer
    assert "SparseQPLayer" in torch_layer.__all__
    for name in ("solve_columns", "differentiate", "vjp", "differentiate_info", "vjp_info", "vjp_times"):
        assert callable(getattr(pkg.SparseKKT, name))
