"""The analysis of the sparse search_direction! handle (calipso.jl_amd/csrc/sparse_kkt.hpp: the pattern of triu(K), the slot of every written entry, the row
views) on the CPU: tests/sparse_kkt_host/main.cpp includes only that header, is built with the plain host compiler (no HIP include path) under the address and
undefined-behaviour sanitizers, and run as a child process, one case per run.  The program rebuilds the pattern of K by brute force from dense 0/1 masks,
round-trips every map and prints "sparse kkt ok", or the refusal.  Also here: without a HIP device SparseKKT fails loudly, like every other handle type."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import ROOT, load_pkg

ARGUMENT = -4


@pytest.fixture(scope="module")
def analyser(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("sparse_kkt") / "sparse_kkt")
    # (gcc links the sanitizer runtimes dynamically unless told otherwise; clang links them statically by itself and does not know gcc's two flags)
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtimes = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"] +
                           static_runtimes + [os.path.join(ROOT, "tests", "sparse_kkt_host", "main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def pattern1(A):
    """(colptr, rowval), 1-based, of a scipy matrix or of an explicit (colptr, rowval) pair"""
    if isinstance(A, tuple):
        return A
    A = sp.csc_matrix(A)
    A.sort_indices()
    return list(A.indptr + 1), list(A.indices + 1)


def analyse(analyser, tmp_path, nx, ne, nc, nonnegative, dims, Lxx, gx, hx):
    """writes the case, runs the program; returns (the sizes it printed or the refusal, its whole output)"""
    line = lambda key, v: "%s %d %s\n" % (key, len(v), " ".join(str(int(x)) for x in v))
    text = "nx %d\nne %d\nnc %d\nnonnegative %d\n" % (nx, ne, nc, nonnegative) + line("dims", dims)
    for name, A in (("Lxx", Lxx), ("gx", gx), ("hx", hx)):
        colptr, rowval = pattern1(A)
        text += line(name + "_colptr", colptr) + line(name + "_rowval", rowval)
    case = tmp_path / "case.txt"
    case.write_text(text)
    run = subprocess.run([analyser, str(case)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    if run.stdout.startswith("refused"):
        status, message = re.match(r"refused (-?\d+) (.*)\n", run.stdout).groups()
        return dict(refused=int(status), message=message), run.stdout
    assert run.stdout.endswith("sparse kkt ok\n"), run.stdout
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", run.stdout)}, run.stdout


def random_patterns(rng, nx, ne, nc, density, diagonal=True):
    L = rng.random((nx, nx)) < density
    L = L | L.T
    if diagonal:
        L = L | np.eye(nx, dtype=bool)
    else:
        L[::2, ::2] &= ~np.eye(nx, dtype=bool)[::2, ::2]      # every other diagonal entry missing from the pattern
    return L.astype(float), (rng.random((ne, nx)) < density).astype(float), (rng.random((nc, nx)) < density).astype(float)


@pytest.mark.parametrize("nx, ne, nc, nonnegative, dims, density, diagonal", [
    (6, 1, 2, 2, [], 0.5, True),                 # nonnegative only
    (12, 4, 12, 3, [3, 3, 3], 0.3, True),        # nonnegative rows and cones
    (9, 0, 10, 0, [5, 5], 0.4, False),           # no equality, cones only, diagonal entries missing from the pattern of Lxx
    (7, 5, 0, 0, [], 0.4, False),                # no cone
    (10, 3, 9, 2, [2, 4], 0.2, True),            # a cone row in no cone (2 + 2 + 4 < 9), a cone of dimension 2
    (5, 2, 70, 2, [64, 4], 1.0, True),           # a wide cone, dense patterns
    (8, 3, 4, 4, [], 0.0, False),                # empty patterns: the diagonals alone
])
def test_tables_against_brute_force(analyser, tmp_path, nx, ne, nc, nonnegative, dims, density, diagonal):
    rng = np.random.default_rng(nx * 100 + nc)
    L, g, h = random_patterns(rng, nx, ne, nc, density, diagonal)
    r, out = analyse(analyser, tmp_path, nx, ne, nc, nonnegative, dims, L, g, h)
    assert r["n"] == nx + ne + nc and r["N"] == nx + 2 * ne + 3 * nc and r["cone_columns"] == sum(dims) and r["max_dim"] == max(dims + [0]), out
    want = np.count_nonzero(np.triu(L) + np.eye(nx)) + np.count_nonzero(g) + np.count_nonzero(h) + ne + nc + sum(d * (d - 1) // 2 for d in dims)
    assert r["nnzK"] == want, out


def test_refusals_keep_their_status_and_text(analyser, tmp_path):
    eye = (list(range(1, 5)), [1, 2, 3])                        # a 3 x 3 identity pattern
    none3 = ([1, 1, 1, 1], [])
    ok = dict(nx=3, ne=2, nc=4, nonnegative=1, dims=[3], Lxx=eye, gx=([1, 2, 3, 3], [1, 2]), hx=([1, 2, 3, 5], [1, 2, 3, 4]))
    r, out = analyse(analyser, tmp_path, **ok)
    assert r["nnzK"] == 3 + 2 + 4 + 2 + 1 + 6, out
    cases = [(dict(Lxx=([1, 3, 4, 5], [2, 1, 2, 3])), "Lxx: row indices must ascend within a column"),
             (dict(Lxx=([1, 3, 4, 5], [1, 1, 2, 3])), "Lxx: duplicate entry in the CSC pattern"),
             (dict(gx=([1, 3, 3, 3], [2, 2])), "gx: duplicate entry in the CSC pattern"),
             (dict(hx=([1, 3, 3, 3], [4, 1])), "hx: row indices must ascend within a column"),
             (dict(Lxx=([1, 2, 3, 4], [1, 2, 4])), "Lxx: row index out of range"),
             (dict(gx=([1, 2, 2, 2], [0])), "gx: row index out of range"),
             (dict(hx=([1, 2, 2, 2], [5])), "hx: row index out of range"),
             (dict(Lxx=([0, 1, 2, 3], [1, 2, 3])), "Lxx: colptr must be 1-based (Julia SparseMatrixCSC)"),
             (dict(gx=([1, 3, 2, 3], [1, 2])), "gx: colptr must be non-decreasing"),
             (dict(dims=[1], nonnegative=3), "a second-order cone has dimension >= 2 (cone 1 has 1)"),
             (dict(dims=[3, 2]), "the cone dimensions exceed nc = 4"),
             (dict(dims=[4]), "the cone dimensions exceed nc = 4"),
             (dict(nonnegative=5, dims=[]), "the cone layout: 0 <= n_nonnegative <= nc, n_soc >= 0 with its dimensions")]
    for change, text in cases:
        r, out = analyse(analyser, tmp_path, **dict(ok, **change))
        assert r == dict(refused=ARGUMENT, message=text), out
    r, out = analyse(analyser, tmp_path, **dict(ok, hx=none3, gx=none3))       # (empty Jacobian patterns are fine)
    assert r["nnzK"] == 3 + 2 + 1 + 6, out


def test_no_cpu_fallback():
    """without a HIP device SparseKKT fails loudly: there is no CPU path behind the C ABI"""
    pkg = load_pkg()
    from calipso_jl_amd._lib import lib
    if lib().calipso_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.CalipsoHipError) as e:
        pkg.SparseKKT(sp.identity(4, format="csc"), sp.csc_matrix((1, 4)), sp.csc_matrix(np.ones((2, 4))))
    assert "no HIP device" in str(e.value)
    # a refused pattern is refused before any device is looked for
    bad = sp.csc_matrix((np.ones(2), np.array([1, 0]), np.array([0, 2, 2, 2, 2])), shape=(4, 4))
    with pytest.raises(pkg.CalipsoHipError) as e:
        pkg.SparseKKT(bad, sp.csc_matrix((0, 4)), sp.csc_matrix((0, 4)))
    assert "row indices must ascend" in str(e.value)
