"""The host side of the parameter Jacobians on the sparse handle without a GPU: calipso.jl_amd/csrc/sparse_parameters.hpp through
tests/sparse_parameters_host/main.cpp — a stand-alone program with its own main, built with the host compiler under the address and undefined-behaviour sanitizers and
run as a child process, as the other *_host_cpu tests do it: the pattern checks and their refusals (each names the array), the column selection's checks, the split into
short and long columns at SPLIT_LENGTH and the launch geometry of the gradient kernel and of the scatter."""
import os
import subprocess

import pytest

from helpers import ROOT
from test_trajectory_sparse_route_cpu import build


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = build(tmp_path_factory, os.path.join(ROOT, "tests", "sparse_parameters_host", "main.cpp"), "sparse_parameters")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.endswith("done\n"), run.stdout + run.stderr
    return run.stdout.splitlines()


def test_pattern_checks_name_the_array(lines):
    assert lines[0] == "ok"
    assert "no parameters (np = 0)" in lines[1]
    assert "gp_colptr is NULL" in lines[2]
    assert "gp_colptr: the first column pointer is 0, not 1" in lines[3]
    assert "gp_colptr: column 4 ends at 1" in lines[4]
    assert "hp_colptr: column 3 ends at 9" in lines[5]
    for k in (6, 7):                                            # unsorted rows, a duplicate
        assert "Lp_rowval: rows lie in 1 .. 300, ascending and without duplicates within a column" in lines[k], lines[k]
    for k in (8,):                                              # a row past the last row
        assert "hp_rowval: rows lie in 1 .. 4" in lines[k], lines[k]
    assert "gp_rowval: rows lie in 1 .. 5" in lines[9]          # row 0
    assert "Lp_rowval is NULL" in lines[10]
    assert lines[11] == "ok"
    assert all(l == "ok" or l.startswith("set_parameter_patterns: ") for l in lines[:12])


def test_column_selection_checks(lines):
    assert lines[12] == "ok" and lines[13] == "ok"
    assert "k: columns = NULL selects all 7 parameters, k is 6" in lines[14]
    assert "columns[1] = 0 is no parameter index (1 .. 7)" in lines[15]
    assert "columns[0] = 8 is no parameter index (1 .. 7)" in lines[16]
    assert "k: at least one column, not 0" in lines[17]
    assert "k: at most 65535 columns" in lines[18]
    assert all(l == "ok" or l.startswith("differentiate_parameters: ") for l in lines[12:19])


def test_split_and_geometry(lines):
    rest = lines[19:-1]
    split = rest[0].split()
    length = int(split[1])
    assert 1 < length < 300                                     # so that the columns of 63, 64, 65 and 300 non-zeros lie on both sides
    # column lengths 0, 1, 2 + 5 + 1, 63, 64, 65, 300 + 4 over the three arrays: a column empty in all of them, 63 a thread's, 64 a wavefront's
    totals = [0, 1, 8, 63, 64, 65, 304]
    assert split[2:4] == ["longest", "304"] and [int(v) for v in split[5:]] == [j for j, t in enumerate(totals) if t >= length]
    assert rest[1:6] == ["is_long 0 0", "is_long 1 0", "is_long %d 0" % (length - 1), "is_long %d 1" % length, "is_long %d 1" % (length + 1)]
    geo = {}
    for line in rest[6:16]:
        f = line.replace(":", "").split()
        geo[(int(f[1]), int(f[2]))] = (int(f[4]), int(f[6]), int(f[8]))
    for (n, nl), (long0, items, blocks) in geo.items():
        assert long0 % 64 == 0 and n <= long0 < n + 64          # the wavefront section starts at a multiple of 64: no wavefront spans both sections
        assert items == long0 + 64 * nl and blocks == max(1, -(-items // 256)) and blocks * 256 >= items
    assert geo[(64, 0)][0] == 64 and geo[(65, 3)] == (128, 320, 2) and geo[(1, 0)] == (64, 64, 1)
    assert rest[16:21] == ["scatter 0 1", "scatter 1 1", "scatter 256 1", "scatter 257 2", "scatter 300 2"]
    assert rest[21:25] == ["name lagrangian_gradient_parameters 0", "name equality_jacobian_parameters 1", "name cone_jacobian_parameters 2", "name -1 -1"]
