#!/usr/bin/env python3
"""Trajectory problems through the evaluators calipso.jl_amd/trajectory.py generates, beside the host-callback route on the same kind of handle and the oracle, in ONE
process: python bench/trajectory_codegen.py [--cases pendulum,cartpole_swingup_11,cartpole_swingup_101,cartpole_swingup_1025] [--repeats 3] [--out FILE]

Per case: ms per device_evaluate(ALL_VARIABLE_FLAGS) (200 calls, one synchronisation), ms per solve! (initialize! + solve!, median of the repeats after one warm-up
solve) on the generated device route; the same two on the host-callback route (TrajectoryProblem.evaluate, or tests/problems.py: pendulum for the pendulum) with the
same handle type; the oracle's solve! time on one core.  The host-callback route and the oracle hold dense nx x nx arrays on the host: they are left out (null)
beyond --host-limit variables (default 1000).  The pendulum is BASELINE config C2: the claim to check is that its device-route solve! beats the host-callback
route of the same run, and whether it is below the oracle's time.  Prints one JSON line and writes it to --out (default profiles/trajectory_codegen.json).  The
libraries come from `python __graft_entry__.py build` (the swing-up's text does not depend on the horizon: one library); nothing is compiled here."""
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
from __graft_entry__ import load_package
import problems as pr

FIXTURES = os.path.join(ROOT, "tests", "device_eval_trajectory")
EVALUATIONS = 200


def main():
    a = sys.argv[1:]

    def opt(name, default):
        if name not in a:
            return default
        i = a.index(name); v = a[i + 1]; del a[i:i + 2]
        return v
    cases = opt("--cases", "pendulum,cartpole_swingup_11,cartpole_swingup_101,cartpole_swingup_1025").split(",")
    repeats, host_limit = int(opt("--repeats", 3)), int(opt("--host-limit", 1000))
    out_path = opt("--out", os.path.join(ROOT, "profiles", "trajectory_codegen.json"))
    pkg = load_package()
    import oracle
    oracle.build()
    spec = importlib.util.spec_from_file_location("trajectory_problems", os.path.join(FIXTURES, "problems.py"))
    tp = importlib.util.module_from_spec(spec); spec.loader.exec_module(tp)
    out = {"evaluations": EVALUATIONS, "repeats": repeats, "cases": {}}
    for name in cases:
        t0 = time.perf_counter()
        TP = tp.trajectory(name)
        derive_s = time.perf_counter() - t0
        T = TP.T
        if name == "pendulum":
            x0 = TP.initialize_states(np.zeros(TP.nx), TP.linear_interpolation([0.0, 0.0], [np.pi, 0.0], T))
            host_problem = pr.pendulum(action_guess=np.zeros(T - 1))
        else:
            x0 = TP.initialize_actions(TP.initialize_states(np.zeros(TP.nx), TP.linear_interpolation(np.zeros(4), [0.0, np.pi, 0.0, 0.0], T)), [np.full(1, 0.01)] * (T - 1))
            host_problem = TP
        structure = TP.structure()
        t0 = time.perf_counter()
        dev = tp.solver(name)
        compile_s = time.perf_counter() - t0

        def measure(s, evaluate):
            s.set("solution", np.concatenate([x0, np.zeros(s.N - TP.nx)]))
            evaluate(s); s.synchronize()
            n = EVALUATIONS if evaluate is device else 5
            t0 = time.perf_counter()
            for _ in range(n):
                evaluate(s)
            s.synchronize()
            eval_ms = (time.perf_counter() - t0) / n * 1e3
            ms, ok = [], True
            for rep in range(repeats + 1):
                t0 = time.perf_counter()
                pkg.initialize_b(s, x0)
                ok = pkg.solve_b(s)
                s.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            return {"evaluate_ms": eval_ms, "solve_ms": float(np.median(ms[1:])), "solve_ms_all": ms[1:], "converged": bool(ok), "iterations": s.stats()["total_iterations"]}

        device = lambda s: s.device_evaluate(pr.ALL_VARIABLE_FLAGS, 0)
        hosted = lambda s: s.evaluate(pr.ALL_VARIABLE_FLAGS, 0)
        case = {"stages": T, "shape": [TP.nx, TP.ne, TP.nc], "structured": structure is not None, "derive_s": derive_s, "compile_or_load_s": compile_s,
                "templates": TP.stats()["templates"], "device": measure(dev, device), "enqueued_per_call": None, "host_callback": None, "oracle_solve_ms": None}
        device(dev); dev.synchronize()
        case["enqueued_per_call"] = TP.enqueued(dev)
        solution = dev.solution.variables
        dev.close()
        if TP.nx <= host_limit:
            host = pkg.Solver(host_problem, TP.nx, TP.np, TP.ne, TP.nc, nonnegative_indices=TP.nonnegative_indices, second_order_indices=TP.second_order_indices,
                              structure=structure)
            case["host_callback"] = measure(host, hosted)
            case["host_callback"]["solution_difference"] = float(np.abs(host.solution.variables - solution).max())
            host.close()
            ms = []
            for rep in range(2):
                o = oracle.OracleSolver(TP.nx, TP.np, TP.ne, TP.nc, TP.nonnegative_indices, TP.second_order_indices)
                o.point()["x"][:] = x0
                t0 = time.perf_counter()
                status = o.solve(host_problem)
                ms.append((time.perf_counter() - t0) * 1e3)
            case["oracle_solve_ms"], case["oracle_status"], case["oracle_iterations"] = min(ms), status, o.stats()["total_iterations"]
            case["device_over_host_callback"] = case["host_callback"]["solve_ms"] / case["device"]["solve_ms"]
            case["device_below_oracle"] = case["device"]["solve_ms"] < case["oracle_solve_ms"]
        out["cases"][name] = case
        print("%s: %s" % (name, json.dumps(case)), file=sys.stderr, flush=True)
    line = json.dumps(out)
    if out_path != "-":
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
