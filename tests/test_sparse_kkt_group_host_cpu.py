"""The host bookkeeping of search_direction! for groups of sparse problems (calipso.jl_amd/csrc/sparse_kkt_group.hpp) on the CPU: tests/sparse_kkt_group_host/main.cpp
includes only that header and step_decisions.hpp, is built with the plain host compiler under the address and undefined-behaviour sanitizers, and run as a child
process.  The replay is fed, per member, the inertias and residual norms that the ORACLE's search_direction! reads on the members of the mixed group
(tests/sparse_kkt_group_cases.py) and must come out with the oracle's counts, statuses and regularisation — member by member — and with the active sets a lockstep
call runs.  Also here: the new entries resolve in the built library, and without a HIP device SparseKKTGroup fails loudly, like every other handle type."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sparse_kkt_cases as kc
import sparse_kkt_group_cases as gc
from helpers import ROOT, load_pkg


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("sparse_kkt_group") / "sparse_kkt_group")
    # (gcc links the sanitizer runtimes dynamically unless told otherwise; clang links them statically by itself and does not know gcc's two flags)
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtimes = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"] +
                           static_runtimes + [os.path.join(ROOT, "tests", "sparse_kkt_group_host", "main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def run(program, *args):
    r = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def recordings(oracle_mod):
    """per member of the mixed group, recorded once: with the default options and with the failing max_regularization"""
    out = {}
    for limit in (None, gc.FAILING_MAX_REGULARIZATION):
        out[limit] = []
        for (pid, kind), _ in gc.MIXED:
            prob, w, lam = gc.member(oracle_mod.splitmix_uniform, kc.SMALL, pid, kind)
            out[limit].append((prob, gc.record(oracle_mod, prob, w, lam, limit)))
    return out


def replay(program, tmp_path, recs, max_regularization):
    prob = recs[0][0]
    lines = ["%d %d %d %r" % (prob.nx, prob.ne + prob.nc, len(recs), float(max_regularization))]
    for _, rec in recs:
        lines.append("%r 0.0 %d %d" % (kc.KAPPA, len(rec["inertias"]), len(rec["norms"])))
        lines += [" ".join(str(v) for v in t) for t in rec["inertias"]] + [repr(v) for v in rec["norms"]]
    path = tmp_path / "replay.txt"
    path.write_text("\n".join(lines) + "\n")
    out = run(program, "replay", path).splitlines()
    sets = [(l.split()[0], [int(v) for v in l.split()[1:]]) for l in out if l.split()[0] in ("factor", "solve", "norms", "round")]
    members = [dict(zip(l.split()[2::2], l.split()[3::2])) for l in out if l.startswith("member")]
    report = [l for l in out if l.startswith("report")][0].split()
    return sets, members, dict(zip(report[1::2], (int(v) for v in report[2::2])))


def test_the_oracle_does_on_the_members_what_the_cases_say(recordings):
    for ((pid, kind), (nfact, rounds, status)), (_, rec) in zip(gc.MIXED, recordings[None]):
        want = rec["want"]
        assert (want["factorizations"], want["rounds"], want["status"]) == (nfact, rounds, status), (pid, kind, want)
    assert [rec["want"]["status"] for _, rec in recordings[gc.FAILING_MAX_REGULARIZATION]] == gc.FAILING_STATUSES


def test_the_lockstep_replay_of_the_mixed_group(program, tmp_path, recordings):
    recs = recordings[None]
    sets, members, report = replay(program, tmp_path, recs, 1.0e40)
    for m, (_, rec) in zip(members, recs):
        want = rec["want"]
        assert (int(m["status"]), int(m["factorizations"]), int(m["rounds"])) == (want["status"], want["factorizations"], want["rounds"])
        assert (float(m["ep"]), float(m["ep_last"]), float(m["ed"])) == (want["ep"], want["ep_last"], want["ed"])       # bit for bit: repr and %.17g round-trip
    nfact, rounds = [w[0] for _, w in gc.MIXED], [w[1] for _, w in gc.MIXED]
    factor = [s for kind, s in sets if kind == "factor"]
    assert len(factor) == gc.MIXED_FACTOR_ROUNDS == max(nfact)
    for r, active in enumerate(factor):                                   # round r covers exactly the members that need more than r factorisations
        assert active == [k for k in range(len(recs)) if nfact[k] > r]
    assert [s for kind, s in sets if kind == "solve"] == [list(range(len(recs)))]
    norms, corrections = [s for kind, s in sets if kind == "norms"], [s for kind, s in sets if kind == "round"]
    assert len(corrections) == gc.MIXED_REFINE_ROUNDS == max(rounds) and len(norms) == max(rounds) + 1
    for r, active in enumerate(corrections):
        assert active == [k for k in range(len(recs)) if rounds[k] > r]
    assert report == dict(factor_rounds=14, refine_rounds=11, last_factor_active=3, last_refine_active=1, worst=2)


def test_the_lockstep_replay_with_failing_members(program, tmp_path, recordings):
    recs = recordings[gc.FAILING_MAX_REGULARIZATION]
    sets, members, report = replay(program, tmp_path, recs, gc.FAILING_MAX_REGULARIZATION)
    assert [int(m["status"]) for m in members] == gc.FAILING_STATUSES and report["worst"] == -1
    passing = [k for k, s in enumerate(gc.FAILING_STATUSES) if s == 0]
    assert [s for kind, s in sets if kind == "solve"] == [passing]        # the failed members leave, the others go on
    for k, (m, (_, rec)) in enumerate(zip(members, recs)):
        assert int(m["factorizations"]) == rec["want"]["factorizations"]
        if k in passing:
            assert int(m["rounds"]) == rec["want"]["rounds"] and float(m["ep"]) == rec["want"]["ep"]
        else:
            assert float(m["ep"]) > gc.FAILING_MAX_REGULARIZATION and int(m["rounds"]) == 0


def test_a_group_of_the_slowest_member_runs_the_same_rounds(program, tmp_path, recordings):
    """the launches and host waits of a lockstep call are a function of its rounds: a group of one holding the slowest member runs as many of both kinds"""
    k = [key for key, _ in gc.MIXED].index(gc.SLOWEST)
    _, _, report = replay(program, tmp_path, [recordings[None][k]], 1.0e40)
    assert (report["factor_rounds"], report["refine_rounds"]) == (gc.MIXED_FACTOR_ROUNDS, gc.MIXED_REFINE_ROUNDS)


def test_the_slab_layout_has_no_overlap_and_stays_in_bounds(program):
    out = run(program, "layout")
    assert out.startswith("layout ok cases=1728 largest="), out
    assert int(out.split("largest=")[1]) > 2**24                            # (the sweep reached 128 members of a 10^5-variable problem)


def test_the_argument_checks(program):
    create, option, matrix = "calipso_hip_sparse_kkt_group_create: ", "calipso_hip_sparse_kkt_group_set_option: ", "calipso_hip_sparse_kkt_group_get_matrix: "
    phase = "method: a group needs the multifrontal numeric phase (method 4, nested dissection), this plan has the column method (numeric phase %d), which factors a batch one matrix after the other"
    assert run(program, "checks").splitlines() == [
        "ok", "ok", create + "members: a group holds 1 .. 128 members, not 0", create + "members: a group holds 1 .. 128 members, not 129",
        create + "members: a group holds 1 .. 128 members, not -3",
        "ok", create + phase % 1, create + phase % 0,
        "ok", matrix + "member: 6 is not in 0 .. 5", matrix + "member: -1 is not in 0 .. 5",
        "ok", option + "krylov_fallback: the `H \\ residual` fallback is not built for groups (a member whose refinement fails gets status 2 and its last refined step)",
        option + "krylov_restart: the `H \\ residual` fallback is not built for groups", "ok",
        "ok", "calipso_hip_sparse_kkt_group_factorize: ep is NULL"]


def test_the_new_entries_resolve_in_the_built_library():
    load_pkg()
    from calipso_jl_amd._lib import SYMBOLS, lib
    names = ["create", "destroy", "last_error", "info", "pattern", "set_option", "set_values", "set_values_device", "factorize", "get_matrix", "mul", "solve_symmetric",
             "search_direction", "search_direction_device", "timing"]
    for n in names:
        assert "calipso_hip_sparse_kkt_group_" + n in SYMBOLS
        getattr(lib(), "calipso_hip_sparse_kkt_group_" + n)


def test_no_cpu_fallback():
    """without a HIP device SparseKKTGroup fails loudly: there is no CPU path behind the C ABI"""
    pkg = load_pkg()
    from calipso_jl_amd._lib import lib
    if lib().calipso_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    import scipy.sparse as sp
    with pytest.raises(pkg.CalipsoHipError) as e:
        pkg.SparseKKTGroup(sp.identity(4, format="csc"), sp.csc_matrix(np.ones((1, 4))), sp.csc_matrix(np.ones((2, 4))), members=3)
    assert "(-5)" in str(e.value) and "no HIP device" in str(e.value)
    with pytest.raises(pkg.CalipsoHipError) as e:                           # ... and the members are checked before anything else
        pkg.SparseKKTGroup(sp.identity(4, format="csc"), sp.csc_matrix(np.ones((1, 4))), sp.csc_matrix(np.ones((2, 4))), members=129)
    assert "(-4)" in str(e.value) and "members: a group holds 1 .. 128 members, not 129" in str(e.value)
