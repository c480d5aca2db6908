"""The analyse phase of the sparse LDL^T (calipso.jl_amd/csrc/sparse_plan.hpp: P A P', elimination tree, pattern of L, row view, column levels and the whole
multifrontal plan) on the CPU: tests/sparse_plan_host/main.cpp includes only that header and ordering.hpp, is built with the plain host compiler (no HIP include
path) under the address and undefined-behaviour sanitizers, and run as a child process, one case per run.  The program checks every table by brute force (a dense
symbolic elimination, a round trip of every address table to global indices) and prints the route the plan took; the cases below assert that route."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import ROOT
from test_oracle_qdldl import quasidefinite
from test_ordering_symbolic import csc1, staged_kkt

NATURAL, RCM, MINIMUM_DEGREE, PERM, NESTED_DISSECTION = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("sparse_plan") / "sparse_plan")
    # (gcc links the sanitizer runtimes dynamically unless told otherwise; clang links them statically by itself and does not know gcc's two flags)
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtimes = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"] +
                           static_runtimes + [os.path.join(ROOT, "tests", "sparse_plan_host", "main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def plan(planner, tmp_path, pattern, method, perm=None, pieces=None, **limits):
    """writes the case, runs the program; returns (the fields of its route line or the refusal, its whole output)"""
    if isinstance(pattern, tuple):
        n, colptr, rowval = pattern
    else:
        colptr, rowval, _ = csc1(sp.triu(sp.csc_matrix(pattern)))
        n = pattern.shape[0]
    line = lambda key, v: "%s %d %s\n" % (key, len(v), " ".join(str(int(x)) for x in v))
    text = "n %d\nmethod %d\n" % (n, method) + line("colptr", colptr) + line("rowval", rowval)
    if perm is not None:
        text += line("perm", perm)
    if pieces is not None:
        text += line("pieces", [x for fc in pieces for x in fc])
    text += "".join("limit %s %d\n" % kv for kv in limits.items())
    case = tmp_path / "case.txt"
    case.write_text(text)
    run = subprocess.run([planner, str(case)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    if run.stdout.startswith("refused"):
        status, message = re.match(r"refused (-?\d+) (.*)\n", run.stdout).groups()
        return dict(refused=int(status), message=message), run.stdout
    assert run.stdout.endswith("sparse plan ok\n"), run.stdout
    kind = re.match(r"route (\w+)", run.stdout).group(1)
    return dict(route=kind, **{k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", run.stdout)}), run.stdout


def stage_chain():
    """the stage-chained KKT pattern of the GPU sparse tests (test_ordering_symbolic.staged_kkt), 12 stages of 3 states and 1 control: n = 87, more than one leaf piece"""
    return staged_kkt(12, 3, 1, np.random.default_rng(3))


def block_star(leaves=6, w=3, root=8):
    """`leaves` dense blocks of w columns, each coupled densely to one dense root block at the end, in natural order with its pieces: every leaf front has w + root
    rows, the root front `root` rows and `leaves` children.  All pieces are narrower than 16 columns, so every chunk width gives the same fronts."""
    n = leaves * w + root
    K = np.zeros((n, n))
    for b in range(leaves):
        K[b * w:(b + 1) * w, b * w:(b + 1) * w] = 1
        K[b * w:(b + 1) * w, leaves * w:] = 1
    K[leaves * w:, leaves * w:] = 1
    K = K + K.T
    return K, [(b * w, w) for b in range(leaves)] + [(leaves * w, root)]


def two_stages_in_one_piece():
    """two dense stage blocks of 40 columns in ONE piece of 80, chained by one entry (row 40, column 39), each coupled to its own 10 of the last 20 (dense) columns.
    A chunk that straddles the two stages (widths 64, 56, 48) carries both stages' neighbours: its front has 64 + 16 + 20 = 56 + 24 + 20 = 48 + 32 + 20 = 100 rows;
    of the chunks of 40 columns the first has 40 + 1 + 10 rows and the second, which inherits the first's neighbours as fill, 40 + 20."""
    K = np.zeros((100, 100))
    K[0:40, 0:40] = 1; K[40:80, 40:80] = 1; K[80:, 80:] = 1
    K[0:40, 80:90] = 1; K[40:80, 90:100] = 1
    K[39, 40] = 1
    K = K + K.T
    return K, [(0, 80), (80, 20)]


def test_first_width_on_a_stage_chained_kkt_pattern(planner, tmp_path):
    r, out = plan(planner, tmp_path, stage_chain(), NESTED_DISSECTION)
    assert r["route"] == "multifrontal" and r["width"] == 64 and r["last_resort"] == 0 and r["nodes"] > 2, out
    assert r["global_levels"] == 0 and r["wide_levels"] == 0 and r["item_nodes"] == r["nodes"] and r["items"] > 1 and r["pool"] == 0, out


def test_a_narrower_width_when_the_first_attempts_largest_front_is_just_over_the_limit(planner, tmp_path):
    K, pieces = two_stages_in_one_piece()
    first, out = plan(planner, tmp_path, K, NATURAL, pieces=pieces)
    assert first["route"] == "multifrontal" and first["width"] == 64 and first["max_front"] == 100 and first["last_resort"] == 0, out
    r, out = plan(planner, tmp_path, K, NATURAL, pieces=pieces, max_front=first["max_front"] - 1)
    assert r["route"] == "multifrontal" and r["width"] == 40 and r["last_resort"] == 0 and r["max_front"] == 60 and r["global_levels"] == 0, out


@pytest.mark.parametrize("max_front, lds_levels, global_levels", [(9, 1, 1), (7, 0, 2)])
def test_last_resort_with_one_workgroup_per_global_front(planner, tmp_path, max_front, lds_levels, global_levels):
    # leaf fronts of 11 rows exceed the limit at every width: the last resort, the leaves' level (and, at 7, the root's of 8 rows) in global memory, no wide tables
    K, pieces = block_star()
    r, out = plan(planner, tmp_path, K, NATURAL, pieces=pieces, max_front=max_front, wide_fronts=0)
    assert r["route"] == "multifrontal" and r["last_resort"] == 1 and r["width"] == 64 and r["max_front"] == 11, out
    assert r["lds_levels"] == lds_levels and r["global_levels"] == global_levels and r["wide_levels"] == 0 and r["pool"] == 6 * 66, out
    assert r["item_nodes"] == (1 if lds_levels else 0), out


@pytest.mark.parametrize("limits, by_m, by_nch, wide_blocks", [(dict(), 0, 1, 1),                                           # the root's six children exceed four
                                                                (dict(wide_solve_m=10, wide_solve_nch=100), 1, 0, 2)])       # the leaves' 11 rows exceed ten; r = 8: two row blocks of 4
def test_last_resort_with_wide_fronts_and_both_conditions_of_the_wide_sweeps(planner, tmp_path, limits, by_m, by_nch, wide_blocks):
    K, pieces = block_star()
    r, out = plan(planner, tmp_path, K, NATURAL, pieces=pieces, max_front=7, wide_fronts=1, wf_solve_rows=4, **limits)
    assert r["route"] == "multifrontal" and r["last_resort"] == 1 and r["global_levels"] == 2 and r["wide_levels"] == 2 and r["item_nodes"] == 0, out
    assert r["solve_by_m"] == by_m and r["solve_by_nch"] == by_nch and r["wide_blocks"] == wide_blocks, out
    # a wide level below an LDS level: the root fits, its children's rows come from the pool
    r, out = plan(planner, tmp_path, K, NATURAL, pieces=pieces, max_front=9, wide_fronts=1, **limits)
    assert r["last_resort"] == 1 and r["lds_levels"] == 1 and r["wide_levels"] == 1 and r["item_nodes"] == 1, out


def test_no_multifrontal_plan(planner, tmp_path):
    K = stage_chain()
    for method in (NATURAL, RCM, MINIMUM_DEGREE):
        r, out = plan(planner, tmp_path, K, method)
        assert r["route"] == "columns", out
    S, pieces = block_star()
    for limits in (dict(max_front=7, max_front_wide=7, wide_fronts=1), dict(max_front=7, max_front_global=10, wide_fronts=0),      # a front limit nothing fits
                   dict(max_pool=100)):                                                                                              # panels + update matrices: 6 * (33 + 64) + 64 doubles
        r, out = plan(planner, tmp_path, S, NATURAL, pieces=pieces, **limits)
        assert r["route"] == "columns" and r["levels"] == 3 + 8 and r["widest"] == 6, out       # (the six leaf blocks side by side, three columns deep; then the root's eight)


@pytest.mark.parametrize("limits", [dict(mf_items=0), dict(max_item_bytes=64), dict(max_item_children=1)])
def test_without_extend_add_items(planner, tmp_path, limits):
    r, out = plan(planner, tmp_path, stage_chain(), NESTED_DISSECTION, **limits)
    assert r["route"] == "multifrontal" and r["width"] == 64 and r["item_nodes"] == 0 and r["items"] == 0, out


def test_a_callers_perm_on_a_random_quasidefinite_pattern(planner, tmp_path):
    rng = np.random.default_rng(11)
    K = quasidefinite(20, 12, rng)
    r, out = plan(planner, tmp_path, K, PERM, perm=rng.permutation(32) + 1)
    assert r["route"] == "columns", out
    # ... and with the dissection's own order handed over as a perm, pieces and all
    r, out = plan(planner, tmp_path, K, NESTED_DISSECTION)
    assert r["route"] == "multifrontal", out


def test_refusals_keep_their_status_and_text(planner, tmp_path):
    ARGUMENT = -4
    eye3 = (3, [1, 2, 3, 4], [1, 2, 3])
    cases = [((3, [1, 2, 4, 5], [1, 1, 1, 3]), NATURAL, None, "duplicate entry in the CSC pattern"),
             (np.array([[0.0, 0.0], [0.0, 1.0]]), NATURAL, None, "empty column in triu(A): QDLDL_etree! fails on this matrix (qdldl.jl:366-371)"),
             ((3, [1, 2, 3, 4], [1, 2, 4]), NATURAL, None, "row index out of range"),
             ((3, [1, 2, 3, 4], [1, 0, 3]), NATURAL, None, "row index out of range"),
             (eye3, PERM, [0, 1, 2], "perm is not a permutation of 1:n"),
             (eye3, PERM, [1, 2, 2], "perm is not a permutation of 1:n"),
             (eye3, PERM, [1, 2, 4], "perm is not a permutation of 1:n")]
    for pattern, method, perm, text in cases:
        r, out = plan(planner, tmp_path, pattern, method, perm=perm)
        assert r == dict(refused=ARGUMENT, message=text), out
