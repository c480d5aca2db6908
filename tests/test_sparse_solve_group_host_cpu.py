"""The host bookkeeping of solve! for groups of sparse conic QPs (calipso.jl_amd/csrc/sparse_solve_group.hpp) on the CPU: tests/sparse_solve_group_host/main.cpp
includes only that header (and the plain C++ headers behind it), is built with the host compiler under the address and undefined-behaviour sanitizers, and run as a
child process: nothing is loaded into Python under a sanitizer.

`main recorded` drives the lockstep as the device driver does on what the ORACLE read on SMALL pids 0 .. 3, step by step: published blocks, cone-search masks,
candidates, and per search_direction! the inertias and residual norms (sparse_solve_group_cases.record_solve walks the oracle's building blocks and asserts the walk
against the oracle's own solve!; the recording is kept in tests/golden and compared with a fresh one).  exit_kind, step_norms, cone_step_sizes,
line_search_accepts, filter_needs_augment, ic_after and refine_next decide on those numbers; every member must end with the oracle's status, counts, central path,
penalty and primal_regularization_last, and ticks and host waits must be the maximum over the members per tick, summed, computed here independently.
`main replay` runs made-up SCHEDULES for what the oracle's members do not show: line-search trials, and going on past a refinement failure."""
import os
import shutil
import subprocess

import pytest

import sparse_solve_cases as sc
import sparse_solve_group_cases as gc
from helpers import ROOT, load_pkg


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("sparse_solve_group") / "sparse_solve_group")
    # (gcc links the sanitizer runtimes dynamically unless told otherwise; clang links them statically by itself and does not know gcc's two flags)
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtimes = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"] +
                           static_runtimes + [os.path.join(ROOT, "tests", "sparse_solve_group_host", "main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def run(program, *args):
    r = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def schedule(accepted, outer, failing_step=None, trials=None):
    """a member's events: `accepted` steps spread over `outer` outer iterations (the earlier ones take the remainder), an outer update between two of them, then the
    exit; failing_step: that step's search_direction reports a refinement failure (status 2); trials: {step: line-search trials}"""
    per = [accepted // outer + (1 if j < accepted % outer else 0) for j in range(outer)]
    events, step = [], 0
    for j, count in enumerate(per):
        for _ in range(count):
            events.append(("S", (trials or {}).get(step, 0), 2 if step == failing_step else 0, 1 + step % 3, step % 5))
            step += 1
        events.append(("O",) if j < outer - 1 else ("X",))
    return events


def predicted(schedules, continue_after_failure):
    """ticks and vector-half host waits of the lockstep, from the schedules alone: per tick the maximum over the live members of their outer-update read-backs, one
    read-back for the masks and first candidate if anyone steps, the most trials of a stepping member, one for accept; and every member's own waits"""
    cursors, live = [0] * len(schedules), [True] * len(schedules)
    ticks, waits, own = 0, 1, [1] * len(schedules)                              # (the start group's read-back)
    outer_rounds = trial_rounds = 0
    while any(live):
        ticks += 1
        outers, stepping = [], []
        for k, ev in enumerate(schedules):
            if not live[k]:
                continue
            n = 0
            while ev[cursors[k]][0] == "O":
                n += 1; cursors[k] += 1
            outers.append(n); own[k] += n
            if ev[cursors[k]][0] == "X":
                live[k] = False
            else:
                stepping.append(k)
        waits += max(outers); outer_rounds += max(outers)
        on = []
        for k in stepping:
            e = schedules[k][cursors[k]]
            if e[2] == 2 and not continue_after_failure:
                live[k] = False
            else:
                on.append(k)
        if on:
            most = max(schedules[k][cursors[k]][1] for k in on)
            waits += 2 + most; trial_rounds += most
            for k in on:
                own[k] += 2 + schedules[k][cursors[k]][1]
                cursors[k] += 1
    return ticks, waits, outer_rounds, trial_rounds, own


def replay(program, tmp_path, sizes, schedules, continue_after_failure=False):
    lines = ["%d %d %d %d %d" % (sizes + (len(schedules), int(continue_after_failure)))]
    for ev in schedules:
        lines.append(str(len(ev)))
        lines += [" ".join(str(v) for v in e) for e in ev]
    path = tmp_path / "replay.txt"
    path.write_text("\n".join(lines) + "\n")
    out = run(program, "replay", path).splitlines()
    members = [dict(zip(l.split()[2::2], l.split()[3::2])) for l in out if l.startswith("member")]
    report = [l for l in out if l.startswith("report")][0].split()
    return members, dict(zip(report[1::2], (int(v) for v in report[2::2])))


GOLDEN = os.path.join(ROOT, "tests", "golden", "sparse_solve_group_small.txt")


@pytest.fixture(scope="module")
def recordings(oracle_mod):
    """SMALL pids 0 .. 3 walked through the oracle's building blocks, once: (records, want) per member"""
    return [gc.record_solve(oracle_mod, gc.SMALL, pid) for pid in gc.GROUP_SMALL_WITH_FAILURE[1]]


def schedule_of(records):
    """the events of a recording, for predicted(): a prologue behind the first is an outer update, S C T* A a step with its trials, a closing S a refinement failure"""
    events, i = [], 1
    while i < len(records):
        if records[i][0] == "P":
            events.append(("O",)); i += 1
        elif i + 1 == len(records):
            events.append(("S", 0, 2)); i += 1
        else:
            assert [r[0] for r in records[i:i + 2]] == ["S", "C"]
            j = i + 2
            while records[j][0] == "T":
                j += 1
            assert records[j][0] == "A"
            events.append(("S", j - i - 2, 0)); i = j + 1
    return events + [("X",)]


def test_the_golden_recording_is_the_oracles(recordings):
    assert gc.recording_text(recordings) == open(GOLDEN).read()


def test_the_lockstep_on_what_the_oracle_read_for_small_pids_0_to_3(program, recordings):
    """published blocks, masks, inertias and norms recorded from the oracle (tests/golden): every member ends with the oracle's status, counts, central path, penalty
    and primal_regularization_last; ticks and host waits are the maximum over the members per tick, summed"""
    out = run(program, "recorded", GOLDEN).splitlines()
    members = [dict(zip(l.split()[2::2], l.split()[3::2])) for l in out if l.startswith("member")]
    report = [l for l in out if l.startswith("report")][0].split()
    report = dict(zip(report[1::2], (int(v) for v in report[2::2])))
    schedules = [schedule_of(records) for records, _ in recordings]
    ticks, waits, outer_rounds, trial_rounds, own = predicted(schedules, False)
    for k, (m, (records, want)) in enumerate(zip(members, recordings)):
        pid = gc.GROUP_SMALL_WITH_FAILURE[1][k]
        assert int(m["status"]) == want["status"] == (-102 if pid in gc.FAILING[gc.SMALL] else 1)
        for name in ("total_iterations", "outer", "accepted", "factorizations", "max_rounds"):
            assert int(m[name]) == want[name], (pid, name, m[name], want[name])
        assert (float(m["kappa"]), float(m["rho"]), float(m["ep_last"])) == (want["kappa"], want["rho"], want["ep_last"])      # bit for bit: %.17g round-trips
        assert int(m["refinement_failures"]) == (1 if want["status"] == -102 else 0) and int(m["trials"]) == sum(r[0] == "T" for r in records)
        assert int(m["waits"]) == own[k]
        if want["status"] == 1:
            assert int(m["accepted"]) == gc.SOLVED[gc.SMALL][pid]
        else:
            assert int(m["accepted"]) == gc.FAILING[gc.SMALL][pid]
    sd_waits = report.pop("search_direction_waits")
    assert report == dict(ticks=ticks, outer_rounds=outer_rounds, trial_rounds=trial_rounds, host_waits=waits, worst=-102)
    # search_direction's own waits: per tick the most factorisations and the most norm passes of a stepping member, and the call's closing wait
    per_tick, cursors = 0, [1] * len(recordings)
    for _ in range(ticks):
        sds = []
        for k, (records, _) in enumerate(recordings):
            while cursors[k] < len(records) and records[cursors[k]][0] != "S":
                cursors[k] += 1
            if cursors[k] < len(records):
                sds.append(records[cursors[k]]); cursors[k] += 1
        if sds:
            per_tick += max(len(r[1]) for r in sds) + max(len(r[2]) for r in sds) + 1
    assert sd_waits == per_tick


def test_members_with_line_search_trials_and_a_group_of_the_slowest(program, tmp_path):
    """a member that takes trials in a step where its neighbours take none costs the group that step's trial rounds once; a group of one holding the slowest member
    waits as often as the group"""
    sizes = (56, 6, 6)
    slow = schedule(7, 3, trials={1: 3, 4: 25})
    schedules = [schedule(5, 3), slow, schedule(6, 2, trials={1: 1})]
    members, report = replay(program, tmp_path, sizes, schedules)
    ticks, waits, outer_rounds, trial_rounds, own = predicted(schedules, False)
    assert [int(m["trials"]) for m in members] == [0, 28, 1] and [int(m["worst"]) for m in members] == [0, 3, 0]      # 25 trials: the line-search warning
    assert report == dict(ticks=ticks, outer_rounds=outer_rounds, trial_rounds=trial_rounds, host_waits=waits, worst=1) and trial_rounds == 28
    assert [int(m["waits"]) for m in members] == own and max(own) <= waits < sum(own)
    _, alone = replay(program, tmp_path, sizes, [slow])
    assert alone["host_waits"] == own[1] and alone["ticks"] == report["ticks"]


def test_the_slab_layout_has_no_overlap_and_stays_in_bounds(program):
    out = run(program, "layout")
    assert out.startswith("layout ok cases=1800 largest="), out
    assert int(out.split("largest=")[1]) > 2**27                            # (the sweep reached 128 members of a 10^5-variable problem)


def test_the_argument_checks(program):
    attach, init, solve = "calipso_hip_sparse_kkt_group_qp_attach: ", "calipso_hip_sparse_kkt_group_initialize: ", "calipso_hip_sparse_kkt_group_solve: "
    get = "calipso_hip_sparse_kkt_group_get: "
    assert run(program, "checks").splitlines() == [
        "ok", "ok", attach + "q is NULL", attach + "b is NULL", attach + "hvec is NULL",
        "ok", init + "x0 is NULL",
        "ok", "ok", solve + "no gx resident (calipso_hip_sparse_kkt_group_set_values first)",
        solve + "no q, b, hvec resident (calipso_hip_sparse_kkt_group_qp_attach first)",
        solve + "no point resident (calipso_hip_sparse_kkt_group_initialize, or set_values with w, first)", "ok",
        solve + "status is NULL",
        "ok", "calipso_hip_sparse_kkt_group_keep_trace: rows: 1 .. 1048576 rows can be kept, not 0",
        "calipso_hip_sparse_kkt_group_trace: out is NULL with cap_rows > 0", "calipso_hip_sparse_kkt_group_trace: cap_rows is negative",
        "ok", get + "len: dual has 2 entries, not 3", get + "name: no resident vector of a group member called differentiate_slacks",
        get + "name: no resident vector of a group member called (null)", get + "member: 4 is not in 0 .. 3"]


def test_the_new_entries_resolve_in_the_built_library():
    load_pkg()
    from calipso_jl_amd._lib import SYMBOLS, lib
    for n in ["qp_attach", "qp_attach_device", "initialize", "initialize_device", "solve", "get", "solution_device", "keep_trace", "trace"]:
        assert "calipso_hip_sparse_kkt_group_" + n in SYMBOLS
        getattr(lib(), "calipso_hip_sparse_kkt_group_" + n)
    assert callable(load_pkg().SparseConicQPGroup) and "SparseConicQPGroup" in load_pkg().__all__
