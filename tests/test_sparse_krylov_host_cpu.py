"""The host half of the sparse handle's `H \\ residual` fallback (calipso.jl_amd/csrc/sparse_krylov.hpp: the Givens/Hessenberg cycle of restarted GMRES, the verdicts
between cycles, the option checks, the workspace layout) on the CPU: tests/sparse_krylov_host/main.cpp includes only that header, is built with the plain host
compiler under the address and undefined-behaviour sanitizers, and run as a child process.  Also here: the new entries resolve in the built library and refuse a
NULL handle."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT, load_pkg

ENTRIES = ["solve_nonsymmetric", "solve_nonsymmetric_device", "fallback_info"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("sparse_krylov") / "sparse_krylov")
    # (gcc links the sanitizer runtimes dynamically unless told otherwise; clang links them statically by itself and does not know gcc's two flags)
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtimes = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"] +
                           static_runtimes + [os.path.join(ROOT, "tests", "sparse_krylov_host", "main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def run(program, *args):
    r = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_the_cycle_reproduces_known_answers_and_its_estimate_is_the_true_residual(program):
    """systems of 1, 2, 5, 12 and 30 unknowns with a solution known by construction; an exact preconditioner (one iteration), a perturbed one, restarts of two
    columns, a capped run: the solution to 1e-9, the estimate |g| within 64 eps (scaled by |b| + |A| |x|, the rounding of forming b - A x) of the true 2-norm
    residual at EVERY column — asserted by the program; printed: iterations / cycles, and that gap in units of the bound"""
    lines = run(program, "gmres").splitlines()
    print("\n".join(lines))
    assert [l.split()[:2] for l in lines[:-1]] == [["n", str(n)] for n in (1, 2, 5, 12, 30)]
    assert all(l.endswith(" ok") for l in lines[:-1]) and lines[-1] == "gmres ok"
    for l in lines[:-1]:
        w = l.split()
        assert w[3] == "1/1"                                                     # exact preconditioner
        assert max(float(v) for v in w[-4:-1]) <= 1.0


def test_breakdown_restart_caps_and_non_finite_input(program):
    assert run(program, "edges") == "edges ok\n"


def test_the_workspace_layout_has_no_overlap_and_stays_in_bounds(program):
    assert run(program, "layout") == "layout ok cases=320\n"


def test_the_option_checks(program):
    out = run(program, "options").splitlines()
    print("\n".join(out))
    assert out[0] == "defaults 0 16 4"
    got = [(l.split(" -> ")[0], int(l.split(" -> ")[1].split()[0]), l.split("[")[1].split("]")[0]) for l in out[1:]]
    assert got == [
        ("krylov_fallback 1", 1, "1 16 4"), ("krylov_fallback 0", 1, "0 16 4"), ("krylov_fallback 2", -1, "0 16 4"), ("krylov_fallback -1", -1, "0 16 4"),
        ("krylov_fallback 0.5", -1, "0 16 4"), ("krylov_fallback nan", -1, "0 16 4"),
        ("krylov_restart 1", 1, "0 1 4"), ("krylov_restart 32", 1, "0 32 4"), ("krylov_restart 0", -1, "0 32 4"), ("krylov_restart 33", -1, "0 32 4"),
        ("krylov_restart 2.5", -1, "0 32 4"),
        ("krylov_max_cycles 1", 1, "0 32 1"), ("krylov_max_cycles 16", 1, "0 32 16"), ("krylov_max_cycles 0", -1, "0 32 16"), ("krylov_max_cycles 17", -1, "0 32 16"),
        ("krylov_max_cycles nan", -1, "0 32 16"),
        ("krylov_tolerance 1", 0, "0 32 16"), ("iterative_refinement_tolerance 1e-08", 0, "0 32 16")]
    refusals = [l for l in out[1:] if " -> -1 " in l]
    assert all("an integer in" in l for l in refusals) and "krylov_restart: an integer in 1 .. 32" in out[9]


def test_the_new_entries_resolve_and_refuse_a_null_handle():
    load_pkg()
    from calipso_jl_amd._lib import SYMBOLS, lib
    L = lib()
    for n in ENTRIES:
        assert "calipso_hip_sparse_kkt_" + n in SYMBOLS
        getattr(L, "calipso_hip_sparse_kkt_" + n)
    ERR_ARGUMENT = -4
    assert L.calipso_hip_sparse_kkt_solve_nonsymmetric(None, None, None) == ERR_ARGUMENT
    assert L.calipso_hip_sparse_kkt_solve_nonsymmetric_device(None, None, None) == ERR_ARGUMENT
    assert L.calipso_hip_sparse_kkt_fallback_info(None, None) == ERR_ARGUMENT


def test_the_methods_are_exported():
    pkg = load_pkg()
    for name in ("solve_nonsymmetric", "fallback_info"):
        assert callable(getattr(pkg.SparseKKT, name))
    assert len(pkg.SparseKKT.FALLBACK_INFO) == 12
