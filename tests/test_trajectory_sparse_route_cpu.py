"""The sparse route of the trajectory evaluators without a GPU: include/calipso_trajectory_tables.hpp (SparseLayout, sparse_route) through
tests/trajectory_host/sparse_route_main.cpp — a stand-alone program built with the host compiler under the address and undefined-behaviour sanitizers and run as a
child process, as tests/test_trajectory_codegen_cpu.py builds tables_main.cpp — against scipy's CSC of TrajectoryProblem.sparse_patterns(); its refusals;
sparse_patterns() against _patterns(), and its memory on a long horizon; the argument checks of the evaluator's entries on the sparse handle
(csrc/sparse_solve.hpp through tests/sparse_solve_host/evaluator_main.cpp, built the same way)."""
import os
import shutil
import subprocess
import sys
import time
import tracemalloc

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import ROOT
from test_trajectory_codegen_cpu import covered, tp


def build(tmp_path_factory, source, name):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp(name) / name)
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtimes = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    made = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"] + static_runtimes +
                          ["-I" + os.path.join(ROOT, "include"), source, "-o", exe], capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    return exe


@pytest.fixture(scope="module")
def route_host(tmp_path_factory):
    return build(tmp_path_factory, os.path.join(ROOT, "tests", "trajectory_host", "sparse_route_main.cpp"), "sparse_route")


def route(exe, tmp_path, TP, patterns, blob=None, sizes=None):
    """(return code, {(table, template or category): words}) of the sparse route for TP's shape, `blob` (default TP.tables()) and the 0-based (colptr, rowval)
    patterns; (None, {}) when the program refuses the blob"""
    kinds = sys.modules[type(TP).__module__].KINDS
    blob = TP.tables() if blob is None else blob
    shape = [[kinds.index(t.kind) for t in TP.templates]] + [[getattr(t, a) for t in TP.templates] for a in ("nv", "m", "nth", "nd", "nq")]
    lines = [str(len(TP.templates))] + [" ".join(str(v) for v in vals) for vals in shape] + [str(blob.size), " ".join(str(int(v)) for v in blob)]
    lines.append(" ".join(str(v) for v in (sizes or (TP.nx, TP.np, TP.ne, TP.nc))))
    for colptr, rowval in patterns:
        lines += [str(len(rowval)), " ".join(str(int(v) + 1) for v in colptr), " ".join(str(int(v) + 1) for v in rowval)]
    (tmp_path / "route.txt").write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(tmp_path / "route.txt")], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.endswith("done\n"), run.stdout[-2000:] + run.stderr[-4000:]
    out = run.stdout.splitlines()[:-1]
    if out == ["refused"]:
        return None, {}
    got = {(f[0], int(f[1])): np.array([int(v) for v in f[2:]], dtype=np.int64) for f in (line.split() for line in out[1:])}
    return int(out[0].split()[1]), got


def positions(pattern, rows, nx):
    """(row, column) -> the position of that non-zero in the nzval array, by scipy's CSC of the pattern; -1 where there is none"""
    colptr, rowval = pattern
    A = sp.csc_matrix((np.arange(1, len(rowval) + 1, dtype=np.float64), rowval, colptr), shape=(rows, nx))
    assert A.has_sorted_indices
    return lambda i, j: np.asarray(A[i, j]).reshape(-1).astype(np.int64) - 1


@pytest.mark.parametrize("name", ["ragged", "cone_3"])
def test_every_address_of_the_sparse_route_is_the_position_in_the_stored_pattern(route_host, tmp_path, name):
    TP = tp().trajectory(name)
    tr = sys.modules[type(TP).__module__]
    pats = TP.sparse_patterns()
    rc, got = route(route_host, tmp_path, TP, pats)
    assert rc == 0
    where = {tr.D_LXX: positions(pats[0], TP.nx, TP.nx), tr.D_GX: positions(pats[1], TP.ne, TP.nx), tr.D_HX: positions(pats[2], TP.nc, TP.nx)}
    for k, t in enumerate(TP.templates):
        want = np.zeros((t.nd, t.n), dtype=np.int64)
        for e, f in enumerate(t.d_field):
            want[e] = where[int(f)](t.d_i[e], t.d_j[e]) if int(f) in where else 0          # (dg/dtheta, dh/dtheta: no destination on this route)
        assert (want >= 0).all() and np.array_equal(got[("ad", k)], want.reshape(-1)), (k, t.kind)
        for key, table in (("vi", t.vi), ("ri", t.ri), ("pi", t.pi)):
            assert np.array_equal(got[(key, k)], table.reshape(-1)), (key, k)
    want = np.where(np.isin(TP.g_field, (tr.D_GYX, tr.D_HZX)), TP.g_i, 0)
    H = TP.g_field == tr.D_LXX
    assert H.any()
    want[H] = where[tr.D_LXX](TP.g_i[H], TP.g_j[H])
    assert (want >= 0).all() and np.array_equal(got[("g_addr", 0)], want)
    assert np.array_equal(np.sort(want[H]), np.arange(len(pats[0][1])))                    # every stored non-zero of the Hessian has exactly one writer
    # the fill: each nzval array exactly once, nothing for the parameter destinations
    for c, pattern in ((0, pats[1]), (1, pats[2]), (2, pats[0])):
        assert np.array_equal(covered(got[("fill", c)]), np.arange(len(pattern[1]))), c
    for c in (3, 4, 5):
        assert got[("fill", c)].size == 0


def test_refusals_of_the_sparse_route(route_host, tmp_path):
    TP = tp().trajectory("ragged")
    pats = [(c.copy(), r.copy()) for c, r in TP.sparse_patterns()]
    assert route(route_host, tmp_path, TP, pats)[0] == 0

    def without(pattern, at):
        colptr, rowval = pattern
        col = int(np.searchsorted(colptr, at, side="right") - 1)
        colptr = colptr.copy()
        colptr[col + 1:] -= 1
        return colptr, np.delete(rowval, at)

    for k in range(3):                                          # a pattern missing one needed non-zero: code 4, whichever matrix and wherever
        for at in (0, len(pats[k][1]) - 1):
            assert route(route_host, tmp_path, TP, [without(p, at) if i == k else p for i, p in enumerate(pats)])[0] == 4, (k, at)
    colptr, rowval = pats[1]
    col = int(np.argmax(np.diff(colptr) >= 2))
    assert colptr[col + 1] - colptr[col] >= 2
    swapped = rowval.copy()
    swapped[[colptr[col], colptr[col] + 1]] = swapped[[colptr[col] + 1, colptr[col]]]
    assert route(route_host, tmp_path, TP, [pats[0], (colptr, swapped), pats[2]])[0] == 1         # rows not ascending within a column
    doubled = rowval.copy()
    doubled[colptr[col] + 1] = doubled[colptr[col]]
    assert route(route_host, tmp_path, TP, [pats[0], (colptr, doubled), pats[2]])[0] == 1         # a duplicate
    beyond = rowval.copy()
    beyond[-1] = TP.ne
    assert route(route_host, tmp_path, TP, [pats[0], (colptr, beyond), pats[2]])[0] == 1          # a row index past the last row
    short = colptr.copy()
    short[-1] -= 1
    assert route(route_host, tmp_path, TP, [pats[0], (short, rowval[:-1]), pats[2]])[0] == 4      # (a consistent shorter pattern: the non-zero is missing)
    assert route(route_host, tmp_path, TP, [pats[0], (short, rowval), pats[2]])[0] == 1           # column pointers that do not end at nnz + 1
    assert route(route_host, tmp_path, TP, pats, sizes=(TP.nx, TP.np, TP.ne + 1, TP.nc))[0] == 1  # a handle of other sizes
    # a blob for another shape is refused before any route is built
    other = tp().trajectory("cone_3")
    assert route(route_host, tmp_path, TP, pats, blob=other.tables())[0] is None


@pytest.mark.parametrize("name", list(tp().BUILT))
def test_sparse_patterns_are_the_dense_patterns_in_csc(name):
    TP = tp().trajectory(name)
    Zp, Hp = TP._patterns()
    for (colptr, rowval), dense in zip(TP.sparse_patterns(), (Hp, Zp[:TP.ne], Zp[TP.ne:])):
        A = sp.csc_matrix(dense)
        A.sort_indices()
        assert colptr.dtype == rowval.dtype == np.int64
        assert np.array_equal(colptr, A.indptr) and np.array_equal(rowval, A.indices)


def test_sparse_patterns_of_a_long_horizon_allocate_nothing_dense():
    """2001 stages of the cart-pole (nx = 10 004): within seconds and far below an nx x nx boolean array, which _patterns() and structure() would build"""
    codegen = tp().load_codegen()
    TP = codegen.TrajectoryProblem(name="trajectory_cartpole_swingup", **tp().functions("cartpole_swingup_2001"))      # (derived like every horizon; nothing is compiled)
    assert TP.nx == 5 * 2001 - 1 and TP.ne == 4 * 2000 + 4
    tracemalloc.start()
    t0 = time.perf_counter()
    pats = TP.sparse_patterns()
    seconds = time.perf_counter() - t0
    _, peak = tracemalloc.get_traced_memory()
    tracemalloc.stop()
    print("sparse_patterns: %.3f s, peak %d bytes (nx^2 / 8 = %d)" % (seconds, peak, TP.nx ** 2 // 8))
    assert seconds < 10.0 and peak < TP.nx ** 2 // 8
    # the stage structure: the counts grow by the same amount per stage as from 11 to 12 stages
    count = lambda name: [len(r) for _, r in codegen.TrajectoryProblem(name="trajectory_cartpole_swingup", **tp().functions(name)).sparse_patterns()]
    at11, at12 = [len(r) for _, r in tp().trajectory("cartpole_swingup_11").sparse_patterns()], count("cartpole_swingup_12")
    for (colptr, rowval), a, b, rows in zip(pats, at11, at12, (TP.nx, TP.ne, TP.nc)):
        assert colptr[-1] == len(rowval) == a + (b - a) * (2001 - 11)
        A = sp.csc_matrix((np.ones(len(rowval)), rowval, colptr), shape=(rows, TP.nx))
        assert A.has_sorted_indices and (len(rowval) == 0 or rowval.max() < rows)


@pytest.fixture(scope="module")
def checks_host(tmp_path_factory):
    return build(tmp_path_factory, os.path.join(ROOT, "tests", "sparse_solve_host", "evaluator_main.cpp"), "evaluator_checks")


def test_argument_checks_of_the_evaluator_entries(checks_host):
    run = subprocess.run([checks_host], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.endswith("done\n"), run.stdout + run.stderr
    out = run.stdout.splitlines()
    assert out[0] == "ok" and out[1] == "ok"
    assert "which: 0 the solution, 1 the candidate, not 2" in out[2] and "nothing asked for" in out[3]
    for k, bit in enumerate(range(11, 16)):
        assert "calipso_hip_sparse_kkt_evaluate: flags: parameter-Jacobian bits %d" % (1 << bit) in out[4 + k]
    assert "dual-gradient bit" in out[9] and "dual-gradient bit" in out[10] and "bits beyond" in out[11]
    assert out[12] == "ok" and "np: -1 parameters" in out[13]
    assert out[14] == "ok" and out[15] == "ok" and "theta is NULL, the evaluator takes 3 parameters" in out[16] and "no evaluator attached" in out[17]
    assert out[18:22] == ["objective 1 1", "lagrangian_hessian 40 -1", "equality_jacobian_variables 30 -1", "cone_jacobian_variables 20 -1"]
    assert out[22] == "ok" and "lagrangian_hessian has 40 entries, not 41" in out[23] and "only solution, dual and step can be set" in out[24]
    every = sum(1 << b for b in (0, 1, 2, 3, 4, 6, 7, 8, 10))
    assert out[25] == "flags %d %d" % (every, (1 << 0) | (1 << 3) | (1 << 7))
