"""GPU: where the prologue of a Newton step runs does not change its bits.  A single handle that queues a step ahead of its exit tests (csrc/api.hip: inner_iteration)
runs the step's prologue — gradients, barrier + gradient, merit + gradient, residual, the norms of the exit tests — on its second stream, beside the factorisation,
instead of on the main stream in front of it; CALIPSO_HIP_PROLOGUE_AHEAD=0 keeps the one-stream order.  Same kernels on the same data: every result must agree bit
for bit, in the cases that take the new order (advancing steps, steps in one call, a whole solve! with exits that undo a factorisation queued ahead, a step whose
inertia correction factors again) and in those that must not (a structured handle, a group).  The switch is read once per process, so each variant runs in a process
of its own, as in test_gpu_ldl_overlap.py."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import hashlib, sys, os
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
from helpers import load_pkg
from test_gpu_group import build, build_for_solve
from test_gpu_blocks import build_structured
pkg = load_pkg()
KEYS = ("status", "refinement_rounds", "factorizations", "step_size", "step_size_cone_slack_dual", "merit_candidate", "violation_candidate")
def sha(a): return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
def record(info): return repr(sorted((k, (v.hex() if isinstance(v, float) else v)) for k, v in info.items() if k in KEYS))
def state(s, info): return [sha(s.data("step").all), sha(s.solution.all), sha(s.data("residual").all), record(info)]
def emit(case, out, *figures): print("CASE %%s %%s %%s" %% (case, hashlib.sha256("\n".join(out).encode()).hexdigest(), " ".join(str(f) for f in figures)))

# (a step is queued ahead when the step before it ended well above the exit threshold of the inner loop, which scales with the central-path parameter: build()'s 0.17
# leaves most of these shapes below it after one step)
KAPPA = 1.0e-3
# advancing steps: the second and the third queue ahead.  NP = 1536 (1024 + 512), 1024 (one solve block + nothing below: the smallest the second stream takes), no cone, no equality
for k, shape in enumerate(((1500, 300, 60, 30, 3), (600, 300, 100, 50, 3), (1100, 200, 0, 0, 3), (1100, 0, 60, 30, 3))):
    s = build(pkg, 61 + k, shape)
    s.set("central_path", [KAPPA])
    out, ahead = [], []
    for it in range(3):
        info = s.newton_step(advance=True)
        assert info["status"] >= 0, info
        out += state(s, info)
        ahead.append(s.schedule_info()["last_prologue_mode"])
    emit("steps%%d" %% k, out, "".join(str(a) for a in ahead))

# four steps in one call against four calls (a step that does not advance restores the state it saved)
shape = (1100, 200, 40, 20, 3)
a, b = build(pkg, 71, shape), build(pkg, 71, shape)
a.set("central_path", [KAPPA]); b.set("central_path", [KAPPA])
ia = a.newton_steps(4, advance=False)
ib = [b.newton_step(advance=False) for _ in range(4)]
assert [record(i) for i in ia] == [record(i) for i in ib], (ia, ib)
assert state(a, ia[-1]) == state(b, ib[-1])
emit("nonadvancing", [record(i) for i in ia] + state(a, ia[-1]), a.schedule_info()["prologue_ahead_steps"], b.schedule_info()["prologue_ahead_steps"])

# a whole solve!: steps queued ahead, exits that undo a factorisation queued ahead
prob, s = build_for_solve(pkg, 72, shape)
rc = pkg.solve_b(s)
st = s.stats()
si = s.schedule_info()
emit("solve", [repr(int(rc)), repr(sorted(st.items())), sha(s.solution.all), sha(s.get("dual", prob.ne))], si["prologue_ahead_steps"], si["ahead_undone"],
     st["total_iterations"], st["factorizations"])

# the inertia correction factors again (the operands of the first solve are queued once per factorisation, the prologue once per step)
s = build(pkg, 73, shape, indefinite=6.0)
s.set("central_path", [KAPPA])
out, facts, ahead = [], [], []
for it in range(3):
    info = s.newton_step(advance=True)
    assert info["status"] >= 0, info
    out += state(s, info); facts.append(info["factorizations"]); ahead.append(s.schedule_info()["last_prologue_mode"])
emit("indefinite", out, "".join(str(a) for a in ahead), "".join(str(min(f, 9)) for f in facts))

# must not change: a structured handle, a group of two
_, s = build_structured(pkg, 7, 24, 30, 20, 4, 2, 3)
out = []
for it in range(3):
    info = s.newton_step(advance=True)
    out += state(s, info)
emit("structured", out, s.schedule_info()["prologue_ahead_steps"])
members = [build(pkg, 74 + k, shape) for k in range(2)]
g = pkg.Group(members)
out = []
for it in range(3):
    infos = g.newton_step(advance=True)
    for m, info in zip(members, infos): out += state(m, info)
emit("group", out, sum(m.schedule_info()["prologue_ahead_steps"] for m in members))
g.close()
'''


def run_variant(env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = {}
    for l in r.stdout.splitlines():
        if l.startswith("CASE "):
            w = l.split()
            cases[w[1]] = (w[2], w[3:])
    print(env, {k: v[1] for k, v in cases.items()})
    return cases


@pytest.fixture(scope="module")
def variants():
    return run_variant({}), run_variant({"CALIPSO_HIP_PROLOGUE_AHEAD": "0"}), run_variant({"CALIPSO_HIP_PROLOGUE_AHEAD": "1"})


CASES = ["steps0", "steps1", "steps2", "steps3", "nonadvancing", "solve", "indefinite", "structured", "group"]


@pytest.mark.parametrize("case", CASES)
def test_bits_do_not_depend_on_where_the_prologue_runs(variants, case):
    """default (handed over as a feed of the factorisation's plan) and the other placement (forked at the start of the step) against the one-stream order"""
    on, off, fork = variants
    assert set(on) == set(CASES) == set(off) == set(fork)
    assert on[case][0] == off[case][0], (case, on[case], off[case])
    assert fork[case][0] == off[case][0], (case, fork[case], off[case])
    if case == "solve":              # iterations, factorisations and refinement rounds are part of the digest; the figures are printed for the reader
        assert on[case][1][2:] == off[case][1][2:] == fork[case][1][2:]


def test_the_default_really_takes_the_new_order_and_the_others_never_do(variants):
    on, off, fork = variants
    for k in range(4):
        # the first step of a handle never queues ahead (no prediction yet); the second does, and takes the second stream
        assert on["steps%d" % k][1][0][:2] == "02" and set(on["steps%d" % k][1][0]) <= {"0", "2"}, on["steps%d" % k]
        assert fork["steps%d" % k][1][0] == on["steps%d" % k][1][0].replace("2", "1"), fork["steps%d" % k]
        assert off["steps%d" % k][1] == ["000"], off["steps%d" % k]
    assert on["nonadvancing"][1] == ["3", "3"] and off["nonadvancing"][1] == ["0", "0"]
    assert int(on["solve"][1][0]) >= 1 and int(off["solve"][1][0]) == 0
    assert int(on["solve"][1][1]) >= 1                       # an exit test held on a step whose factorisation was queued ahead: undo_ahead ran, with the prologue drained
    assert on["solve"][1][1] == off["solve"][1][1]           # (the prediction does not depend on the placement)
    modes, facts = on["indefinite"][1]
    assert any(m == "2" and int(f) >= 2 for m, f in zip(modes, facts)), (modes, facts)      # the regularisation loop ran on a step that took the new order
    assert set(off["indefinite"][1][0]) == {"0"} and off["indefinite"][1][1] == facts
    for v in (on, off, fork):
        assert v["structured"][1] == ["0"] and v["group"][1] == ["0"]
