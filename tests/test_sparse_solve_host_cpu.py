"""The host pieces of solve! on the sparse handle (calipso.jl_amd/csrc/sparse_solve.hpp: the filter, the layout of the reduction workspace, the argument checks) on
the CPU: tests/sparse_solve_host/main.cpp includes only that header and step_decisions.hpp, is built with the plain host compiler under the address and
undefined-behaviour sanitizers, and run as a child process.  The filter is held against the oracle's (filter.jl:1-89) on the same sequences.  Also here: the new
entries resolve in the built library, and without a HIP device SparseConicQP fails loudly, like every other handle type."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import ROOT, load_pkg


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("sparse_solve") / "sparse_solve")
    # (gcc links the sanitizer runtimes dynamically unless told otherwise; clang links them statically by itself and does not know gcc's two flags)
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtimes = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"] +
                           static_runtimes + [os.path.join(ROOT, "tests", "sparse_solve_host", "main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def run(program, *args):
    r = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def oracle_replay(oracle_mod, ops):
    """the same operations through the oracle's filter: (the checks' verdicts, the kept pairs)"""
    o = oracle_mod.OracleSolver(2, 0, 1, 1)
    checks = []
    for op in ops:
        if op[0] == "r":
            o._L.oracle_filter_reset(o._h)
        elif op[0] == "a":
            o._L.oracle_augment_filter(o._h, op[1], op[2])
        else:
            checks.append(int(o._L.oracle_check_filter(o._h, op[1], op[2])))
    out = np.zeros(2 * 1000)                                  # (max_filter pairs: options.jl:57)
    n = int(o._L.oracle_filter_pairs(o._h, out.ctypes.data_as(oracle_mod.C.POINTER(oracle_mod.C.c_double))))
    return checks, [(out[2 * i], out[2 * i + 1]) for i in range(n)]


def sequences():
    rng = np.random.default_rng(7)
    random = []
    for _ in range(60):
        u = rng.random()
        th, m = float(rng.random()), float(rng.standard_normal())
        random.append(("r",) if u < 0.05 else (("c", th, m) if u < 0.4 else ("a", th, m)))
    # twelve pairs none of which dominates another: the filter keeps them all, four more than the capacity the program starts with
    chain = [("a", 1.0 - 0.05 * k, -1.0 + 0.1 * k) for k in range(12)] + [("c", 0.7, 0.0), ("c", 0.2, -2.0), ("c", 0.3, -0.95), ("c", 0.31, -0.9)]
    # ties and repeats: the comparisons of filter.jl:43-50 and :68 are strict on one side only
    ties = [("a", 0.5, 0.5), ("a", 0.5, 0.5), ("c", 0.5, 0.5), ("a", 0.5, 0.4), ("a", 0.4, 0.5), ("c", 0.4, 0.4), ("a", 0.4, 0.4), ("r",), ("c", 2.0, 2.0), ("a", 1e9, 1e9)]
    return dict(random=random, chain=chain, ties=ties)


@pytest.mark.parametrize("name", ["random", "chain", "ties"])
@pytest.mark.parametrize("capacity", [8, 1000])
def test_the_filter_keeps_the_oracles_pairs(oracle_mod, program, tmp_path, name, capacity):
    ops = sequences()[name]
    path = tmp_path / "ops.txt"
    path.write_text("".join(" ".join([op[0]] + [repr(float(v)) for v in op[1:]]) + "\n" for op in ops))
    lines = run(program, "filter", capacity, path).splitlines()
    checks = [int(l.split()[1]) for l in lines if l.startswith("check")]
    pairs = [tuple(float(v) for v in l.split()[1:]) for l in lines if l.startswith("pair")]
    index, cap = [int(v) for v in [l for l in lines if l.startswith("index")][0].split()[1::2]]
    want_checks, want_pairs = oracle_replay(oracle_mod, ops)
    assert checks == want_checks and pairs == want_pairs and index == len(want_pairs)       # bit for bit: the values are only compared and copied
    if name == "chain":
        assert index == 12 and cap == (16 if capacity == 8 else 1000)                        # grown once, where the reference would write past the end


def test_the_workspace_layout_has_no_overlap_and_stays_in_bounds(program):
    out = run(program, "layout")
    assert out.startswith("layout ok cases=3888 capped="), out
    assert int(out.split("capped=")[1]) > 0                                                 # (the sweep reached the grid cap)


def test_the_argument_checks(program):
    lines = run(program, "checks").splitlines()
    assert lines[:15] == ["ok", "get: len: solution has 56 entries, not 55", "get: name: no resident vector called no_such_vector", "get: the array is NULL", "ok",
                          "set: name: only solution, dual and step can be set, not residual", "ok",
                          "calipso_hip_sparse_kkt_keep_trace: rows: 1 .. 1048576 rows can be kept, not 0", "ok",
                          "calipso_hip_sparse_kkt_keep_trace: rows: 1 .. 1048576 rows can be kept, not 1048577", "calipso_hip_sparse_kkt_trace: out is NULL with cap_rows > 0", "ok",
                          "ok", "candidate: a_s: a step size lies in (0, 1]", "candidate: a_t: a step size lies in (0, 1]"]
    pkg = load_pkg()
    assert dict((l.split()[0], int(l.split()[1])) for l in lines[15:]) == dict(
        (name, dict(N=56, n=28, nx=12, ne=4, nc=12)[kind]) for name, kind in pkg.SparseKKT.VECTORS.items())


def test_the_new_entries_resolve_in_the_built_library():
    load_pkg()
    from calipso_jl_amd._lib import SYMBOLS, lib
    names = ["qp_attach", "qp_attach_device", "initialize", "initialize_device", "solve", "step_prologue", "cone_search", "candidate", "accept", "outer_update", "get", "set",
             "solution_device", "keep_trace", "trace"]
    for n in names:
        assert "calipso_hip_sparse_kkt_" + n in SYMBOLS
        getattr(lib(), "calipso_hip_sparse_kkt_" + n)


def test_no_cpu_fallback():
    """without a HIP device SparseConicQP fails loudly: there is no CPU path behind the C ABI"""
    pkg = load_pkg()
    from calipso_jl_amd._lib import lib
    if lib().calipso_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.CalipsoHipError) as e:
        pkg.SparseConicQP(sp.identity(4, format="csc"), np.ones(4), sp.csc_matrix(np.ones((1, 4))), np.ones(1), sp.csc_matrix(np.ones((2, 4))), np.ones(2))
    assert "(-5)" in str(e.value) and "no HIP device" in str(e.value)
