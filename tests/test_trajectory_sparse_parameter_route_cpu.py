"""The parameter destinations of the trajectory evaluators' sparse route without a GPU: include/calipso_trajectory_tables.hpp (SparseLayout with the stored parameter
patterns, sparse_route's fill segments) through tests/trajectory_host/sparse_parameter_route_main.cpp — a stand-alone program built with the host compiler under the
address and undefined-behaviour sanitizers and run as a child process, as tests/test_trajectory_sparse_route_cpu.py builds its own — against scipy's CSC of
TrajectoryProblem.sparse_parameter_patterns(); a non-zero outside the pattern; the table without the parameter pointers against sparse_route_main.cpp's, word for word;
sparse_parameter_patterns() against the numpy twin's dense theta-Jacobians, and its memory on a long horizon."""
import os
import subprocess
import sys
import tracemalloc

import numpy as np
import pytest
import scipy.sparse as sp

import problems as pr
from helpers import ROOT
from test_trajectory_codegen_cpu import covered, tp
from test_trajectory_sparse_route_cpu import build, positions

PARAMETER_FLAGS = (pr.OBJECTIVE_JACOBIAN_PARAMETERS | pr.EQUALITY_JACOBIAN_PARAMETERS | pr.EQUALITY_DUAL_JACOBIAN_PARAMETERS | pr.CONE_JACOBIAN_PARAMETERS |
                   pr.CONE_DUAL_JACOBIAN_PARAMETERS)


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    return (build(tmp_path_factory, os.path.join(ROOT, "tests", "trajectory_host", "sparse_parameter_route_main.cpp"), "sparse_parameter_route"),
            build(tmp_path_factory, os.path.join(ROOT, "tests", "trajectory_host", "sparse_route_main.cpp"), "sparse_route_plain"))


def input_lines(TP, patterns, parameter_patterns, flag=True):
    kinds = sys.modules[type(TP).__module__].KINDS
    blob = TP.tables()
    shape = [[kinds.index(t.kind) for t in TP.templates]] + [[getattr(t, a) for t in TP.templates] for a in ("nv", "m", "nth", "nd", "nq")]
    lines = [str(len(TP.templates))] + [" ".join(str(v) for v in vals) for vals in shape] + [str(blob.size), " ".join(str(int(v)) for v in blob)]
    lines.append(" ".join(str(v) for v in (TP.nx, TP.np, TP.ne, TP.nc)))
    pattern = lambda colptr, rowval: [str(len(rowval)), " ".join(str(int(v) + 1) for v in colptr), " ".join(str(int(v) + 1) for v in rowval)]
    for colptr, rowval in patterns:
        lines += pattern(colptr, rowval)
    if flag:
        lines.append("1" if parameter_patterns is not None else "0")
        for colptr, rowval in parameter_patterns or ():
            lines += pattern(colptr, rowval)
    return "\n".join(lines) + "\n"


def run(exe, tmp_path, text):
    (tmp_path / "route.txt").write_text(text)
    done = subprocess.run([exe, str(tmp_path / "route.txt")], capture_output=True, text=True, timeout=60)
    assert done.returncode == 0 and done.stdout.endswith("done\n"), done.stdout[-2000:] + done.stderr[-4000:]
    return done.stdout


def parse(stdout):
    out = stdout.splitlines()[:-1]
    got = {(f[0], int(f[1])): np.array([int(v) for v in f[2:]], dtype=np.int64) for f in (line.split() for line in out[1:])}
    return int(out[0].split()[1]), got


@pytest.mark.parametrize("name", ["ragged", "cone_3", "cone_65"])
def test_every_parameter_address_is_the_position_in_the_stored_parameter_pattern(hosts, tmp_path, name):
    TP = tp().trajectory(name)
    tr = sys.modules[type(TP).__module__]
    pats, ppats = TP.sparse_patterns(), TP.sparse_parameter_patterns()
    assert TP.np > 0 and all(len(c) == TP.np + 1 for c, _ in ppats)
    rc, got = parse(run(hosts[0], tmp_path, input_lines(TP, pats, ppats)))
    assert rc == 0
    where = {tr.D_LXX: positions(pats[0], TP.nx, TP.nx), tr.D_GX: positions(pats[1], TP.ne, TP.nx), tr.D_HX: positions(pats[2], TP.nc, TP.nx),
             tr.D_LGP: positions(ppats[0], TP.nx, TP.np), tr.D_GP: positions(ppats[1], TP.ne, TP.np), tr.D_HP: positions(ppats[2], TP.nc, TP.np)}
    seen = {tr.D_GP: [], tr.D_HP: []}
    for k, t in enumerate(TP.templates):
        want = np.zeros((t.nd, t.n), dtype=np.int64)
        for e, f in enumerate(t.d_field):
            want[e] = where[int(f)](t.d_i[e], t.d_j[e])
            if int(f) in seen:
                seen[int(f)].append(want[e])
        assert (want >= 0).all() and np.array_equal(got[("ad", k)], want.reshape(-1)), (k, t.kind)
    for f, pattern in ((tr.D_GP, ppats[1]), (tr.D_HP, ppats[2])):               # every stored non-zero of dg/dtheta, dh/dtheta has exactly one writer
        every = np.sort(np.concatenate(seen[f])) if seen[f] else np.zeros(0, dtype=np.int64)
        assert np.array_equal(every, np.arange(len(pattern[1]))), f
    want = np.where(np.isin(TP.g_field, (tr.D_GYX, tr.D_HZX)), TP.g_i, 0)
    for f in (tr.D_LXX, tr.D_LGP):
        at = TP.g_field == f
        want[at] = where[f](TP.g_i[at], TP.g_j[at])
    assert (want >= 0).all() and np.array_equal(got[("g_addr", 0)], want)
    P = TP.g_field == tr.D_LGP
    assert np.array_equal(np.sort(want[P]), np.arange(len(ppats[0][1])))          # ... and so has every one of the Lagrangian's theta-gradient
    for c, pattern in ((0, pats[1]), (1, pats[2]), (2, pats[0]), (3, ppats[1]), (4, ppats[2]), (5, ppats[0])):      # the fill: each nzval array exactly once
        assert np.array_equal(covered(got[("fill", c)]), np.arange(len(pattern[1]))), c


def test_a_parameter_non_zero_outside_the_pattern_and_bad_patterns(hosts, tmp_path):
    TP = tp().trajectory("ragged")
    pats = TP.sparse_patterns()
    ppats = [(c.copy(), r.copy()) for c, r in TP.sparse_parameter_patterns()]
    code = lambda pp: parse(run(hosts[0], tmp_path, input_lines(TP, pats, pp)))[0]
    assert code(ppats) == 0

    def without(pattern, at):
        colptr, rowval = pattern
        col = int(np.searchsorted(colptr, at, side="right") - 1)
        colptr = colptr.copy()
        colptr[col + 1:] -= 1
        return colptr, np.delete(rowval, at)

    for k in range(3):
        if len(ppats[k][1]):
            for at in (0, len(ppats[k][1]) - 1):
                assert code([without(p, at) if i == k else p for i, p in enumerate(ppats)]) == 4, (k, at)
    k = int(np.argmax([len(r) for _, r in ppats]))
    colptr, rowval = ppats[k]
    beyond = rowval.copy()
    beyond[-1] = (TP.nx, TP.ne, TP.nc)[k]
    assert code([(colptr, beyond) if i == k else p for i, p in enumerate(ppats)]) == 1          # a row index past the last row
    short = colptr.copy()
    short[-1] -= 1
    assert code([(short, rowval) if i == k else p for i, p in enumerate(ppats)]) == 1           # column pointers that do not end at nnz + 1


@pytest.mark.parametrize("name", ["ragged", "cone_3", "cone_65"])
def test_without_the_parameter_pointers_the_table_is_todays_word_for_word(hosts, tmp_path, name):
    TP = tp().trajectory(name)
    pats = TP.sparse_patterns()
    new = run(hosts[0], tmp_path, input_lines(TP, pats, None))
    old = run(hosts[1], tmp_path, input_lines(TP, pats, None, flag=False))
    assert new == old and new.startswith("rc 0\n")


PARAMETRISED = ["cartpole_mpc", "ragged", "cone_2", "cone_3", "cone_5", "cone_65", "cone_130"]      # (a static list: nothing is derived at collection time)


def test_the_static_list_names_every_built_problem_with_parameters():
    assert PARAMETRISED == [n for n in tp().BUILT if tp().trajectory(n).np > 0]


@pytest.mark.parametrize("name", PARAMETRISED)
def test_the_parameter_patterns_hold_every_non_zero_of_the_twins_dense_jacobians(name):
    TP, theta = tp().trajectory(name), tp().parameters(name)
    rng = np.random.default_rng(3)
    x, y, z = rng.standard_normal(TP.nx), rng.standard_normal(TP.ne), rng.standard_normal(TP.nc)
    sizes = dict(objective_jacobian_variables_parameters=TP.nx * TP.np, equality_dual_jacobian_variables_parameters=TP.nx * TP.np,
                 cone_dual_jacobian_variables_parameters=TP.nx * TP.np, equality_jacobian_parameters=TP.ne * TP.np, cone_jacobian_parameters=TP.nc * TP.np)
    out = {}
    TP.evaluate(PARAMETER_FLAGS, x, y, z, theta + 0.1 * rng.standard_normal(TP.np), lambda nm: out.setdefault(nm, np.zeros(sizes[nm])))
    get = lambda nm: out.get(nm, np.zeros(sizes[nm]))
    dense = (sum(get(n) for n in list(sizes)[:3]).reshape(TP.nx, TP.np, order="F"), get("equality_jacobian_parameters").reshape(TP.ne, TP.np, order="F"),
             get("cone_jacobian_parameters").reshape(TP.nc, TP.np, order="F"))
    assert any(np.count_nonzero(D) for D in dense)
    for (colptr, rowval), D, rows in zip(TP.sparse_parameter_patterns(), dense, (TP.nx, TP.ne, TP.nc)):
        assert colptr.dtype == rowval.dtype == np.int64 and colptr.shape == (TP.np + 1,) and colptr[0] == 0 and colptr[-1] == len(rowval)
        A = sp.csc_matrix((np.ones(len(rowval)), rowval, colptr), shape=(rows, TP.np))
        assert A.has_sorted_indices and (np.diff(colptr) >= 0).all()
        cols = np.repeat(np.arange(TP.np), np.diff(colptr))
        assert len(set(zip(rowval.tolist(), cols.tolist()))) == len(rowval)            # duplicate-free
        rest = D.copy()
        rest[rowval, cols] = 0.0
        assert not rest.any()
    if name == "ragged":                                                         # a stage without parameters: its functions touch no column
        counts = [len(p) for p in TP.indices.parameters]
        assert 0 in counts and any(counts)


def test_parameter_patterns_of_a_long_horizon_allocate_nothing_dense():
    codegen = tp().load_codegen()
    TP = codegen.TrajectoryProblem(name="trajectory_cone", **tp().functions("cone_130"))
    tracemalloc.start()
    pats = TP.sparse_parameter_patterns()
    _, peak = tracemalloc.get_traced_memory()
    tracemalloc.stop()
    nnz = sum(len(r) for _, r in pats)
    print("sparse_parameter_patterns: %d non-zeros, peak %d bytes (nx np bytes = %d)" % (nnz, peak, TP.nx * TP.np))
    assert nnz > 0 and peak < TP.nx * TP.np             # below even a boolean nx x np array
