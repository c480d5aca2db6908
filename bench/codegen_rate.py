#!/usr/bin/env python3
"""The generated cart-pole evaluator (calipso.jl_amd/codegen.py from the functions of tests/device_eval_generated/problems.py) beside the hand-written hyper-dual
one (tests/device_eval_small/cartpole_mpc.hip) in ONE process: python bench/codegen_rate.py [batch [--threads T] [--out FILE]] — `batch` (4096) cart-pole MPC
instances with the parameters of bench/small_newton_rate.py --evaluator cartpole, solve! then differentiate! with the evaluator's dR/dtheta.  The two handles
alternate: 2 warm-up rounds, then 7 timed repetitions each (the launches' own milliseconds), reported as median and quartiles; the yardstick is the hand-written
fixture of the same run.  Prints one JSON line and writes it to --out (default profiles/codegen_rate.json).  Both libraries come from
`python __graft_entry__.py build`; nothing is compiled here."""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
from __graft_entry__ import load_package
import problems as pr

WARMUP, REPEATS = 2, 7
GEN = os.path.join(ROOT, "tests", "device_eval_generated")


def quartiles(ms, B):
    q1, med, q3 = (float(v) for v in np.percentile(ms, [25, 50, 75]))
    return {"ms_median": med, "ms_q1": q1, "ms_q3": q3, "ms_all": [float(v) for v in ms], "per_s": B / (med * 1e-3)}


def main():
    a = sys.argv[1:]

    def opt(name, default):
        if name not in a:
            return default
        i = a.index(name); v = a[i + 1]; del a[i:i + 2]
        return v
    threads, out_path = int(opt("--threads", 0)), opt("--out", os.path.join(ROOT, "profiles", "codegen_rate.json"))
    B = int(a[0]) if a else 4096
    pkg = load_package()
    spec = importlib.util.spec_from_file_location("generated_problems", os.path.join(GEN, "problems.py"))
    gp = importlib.util.module_from_spec(spec); spec.loader.exec_module(gp)
    P = gp.generated("cartpole_mpc")
    if not os.path.exists(P.library_path(directory=GEN)):
        raise SystemExit("%s is not built: python __graft_entry__.py build" % P.library_path(directory=GEN))
    prob = pr.cartpole_mpc()
    rng = np.random.default_rng(0)
    th = np.repeat(prob.parameters[None], B, axis=0)
    th[:, 10:14] += 0.05 * rng.uniform(-1, 1, (B, 4))
    for t in range(9):
        o = 0 if t == 0 else 14 + 10 * (t - 1)
        th[:, o + 5:o + 10] *= 1.0 + 0.1 * rng.uniform(-1, 1, (B, 5))
    th[:, 98:102] *= 1.0 + 0.1 * rng.uniform(-1, 1, (B, 4))
    opts = dict(residual_tolerance=1e-3, optimality_tolerance=1e-3, equality_tolerance=1e-3, complementarity_tolerance=1e-3, slack_tolerance=1e-3, threads=threads)
    hand = pkg.SmallNewtonBatch(prob.nx, prob.ne, prob.nc, B, options=opts)
    hand.set_evaluator(ctypes.CDLL(os.path.join(ROOT, "tests", "device_eval_small", "libsmall_evaluators.so")), "cartpole_mpc_kernels", prob.np)
    gen = P.batch(B, options=opts, directory=GEN)
    x0 = np.repeat(prob.x0[None], B, axis=0)
    handles = (("hand_written", hand), ("generated", gen))
    times = {name: {"solve": [], "differentiate": []} for name, _ in handles}
    last = {}
    for name, sn in handles:
        sn.set_parameters(th)
    for rep in range(WARMUP + REPEATS):
        for name, sn in handles:
            sn.initialize(x0)
            res, ms = sn.solve()
            _, st, dms = sn.differentiate()
            if rep >= WARMUP:
                times[name]["solve"].append(ms); times[name]["differentiate"].append(dms)
            last[name] = (res, sn.get_state()["counters"])
    out = {"problem": "cartpole_mpc", "shape": [prob.nx, prob.ne, prob.nc], "n_parameters": prob.np, "batch": B, "threads": threads or "auto", "warmup": WARMUP, "repeats": REPEATS,
           "generated_operations": {hook: s["operations"] for hook, s in P.stats().items()}}
    for name, sn in handles:
        res, cn = last[name]
        out[name] = {"converged": int((res == 1).sum()), "mean_iterations": float(cn["total_iterations"].mean()), "newton_steps_total": int(cn["newton_steps"].sum()),
                     "solve": quartiles(times[name]["solve"], B), "differentiate": quartiles(times[name]["differentiate"], B),
                     "solve_then_differentiate": quartiles(np.add(times[name]["solve"], times[name]["differentiate"]), B)}
        sn.close()
    out["generated_over_hand_written"] = {k: out["generated"][k]["per_s"] / out["hand_written"][k]["per_s"] for k in ("solve", "differentiate", "solve_then_differentiate")}
    line = json.dumps(out)
    if out_path != "-":
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
