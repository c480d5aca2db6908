#!/usr/bin/env python3
"""Nonlinear trajectory problems on the sparse handle (TrajectoryProblem.sparse_solver: SparseKKT + the generated <name>_sparse_eval) beside the handle solver() gives
them today, alternating in ONE process: python bench/sparse_trajectory.py [--cases cartpole_swingup_11,cartpole_swingup_101,pendulum_11,pendulum_101,
cartpole_swingup_1001,pendulum_1001] [--reps 5] [--warmups 2] [--other-limit 2000] [--out FILE]

Per case, cold solve! from initialize! with krylov_fallback = 1, medians over the repeats after the warm-up solves: status, iterations, factorisations, fallbacks,
host waits, device ms of the vector half (the evaluator's kernels run inside its groups) and inside search_direction, wall ms; beside them the wall of one
synchronised evaluate() with every variable-side bit (median of 50), and initialize! + solve! of solver() — the structured handle for the cart-pole, the dense one for
the pendulum (implicit dynamics) — where the problem has at most --other-limit variables.  Prints one JSON line and writes it to --out (default
profiles/sparse_trajectory.json).  The libraries come from `python __graft_entry__.py build`: the text of a library does not depend on the horizon, nothing is
compiled here."""
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from __graft_entry__ import load_package

FIXTURES = os.path.join(ROOT, "tests", "device_eval_trajectory")
EVERYTHING = sum(1 << b for b in (0, 1, 2, 3, 4, 6, 7, 8, 10))


def pendulum(tp, T):
    """the pendulum of tests/device_eval_trajectory/problems.py at another horizon: the same stage functions, so the same library"""
    a = tp.functions("pendulum")
    stage, final, dyn, first, last = a["objective"][0], a["objective"][-1], a["dynamics"][0], a["equality"][0], a["equality"][-1]
    return dict(objective=[stage] * (T - 1) + [final], dynamics=[dyn] * (T - 1), num_states=[2] * T, num_actions=[1] * (T - 1), equality=[first] + [None] * (T - 2) + [last])


def main():
    a = sys.argv[1:]

    def opt(name, default):
        if name not in a:
            return default
        i = a.index(name); v = a[i + 1]; del a[i:i + 2]
        return v
    cases = opt("--cases", "cartpole_swingup_11,cartpole_swingup_101,pendulum_11,pendulum_101,cartpole_swingup_1001,pendulum_1001").split(",")
    reps, warmups, other_limit = int(opt("--reps", 5)), int(opt("--warmups", 2)), int(opt("--other-limit", 2000))
    out_path = opt("--out", os.path.join(ROOT, "profiles", "sparse_trajectory.json"))
    pkg = load_package()
    spec = importlib.util.spec_from_file_location("trajectory_problems", os.path.join(FIXTURES, "problems.py"))
    tp = importlib.util.module_from_spec(spec); spec.loader.exec_module(tp)
    codegen = tp.load_codegen()
    out = {"reps": reps, "warmups": warmups, "cases": {}}
    for name in cases:
        T = int(name.rsplit("_", 1)[1])
        if name.startswith("pendulum_"):
            TP = codegen.TrajectoryProblem(name="trajectory_pendulum", **pendulum(tp, T))
            x0 = TP.initialize_actions(TP.initialize_states(np.zeros(TP.nx), TP.linear_interpolation([0.0, 0.0], [np.pi, 0.0], T)), [np.zeros(1)] * (T - 1))
        else:
            TP = codegen.TrajectoryProblem(name=tp.library_name(name), **tp.functions(name))
            x0 = TP.initialize_actions(TP.initialize_states(np.zeros(TP.nx), TP.linear_interpolation(np.zeros(4), [0.0, np.pi, 0.0, 0.0], T)), [np.full(1, 0.01)] * (T - 1))
        t0 = time.perf_counter()
        s = TP.sparse_solver(directory=FIXTURES, options=dict(krylov_fallback=1))
        make_s = time.perf_counter() - t0
        other = None
        if TP.nx <= other_limit:
            other = TP.solver(directory=FIXTURES)
        rows, other_ms, other_ok, other_iterations = [], [], None, None
        for rep in range(warmups + reps):
            t0 = time.perf_counter()
            s.initialize(x0)
            status, info = s.solve()
            wall = (time.perf_counter() - t0) * 1e3
            fb = s.fallback_info()
            rows.append(dict(info, status=status, wall_with_initialize_ms=wall, fallbacks=fb["solve_fallbacks"], fallbacks_unconverged=fb["solve_unconverged"]))
            if other is not None:
                t0 = time.perf_counter()
                pkg.initialize_b(other, x0)
                other_ok = bool(pkg.solve_b(other))
                other.synchronize()
                other_ms.append((time.perf_counter() - t0) * 1e3)
                other_iterations = other.stats()["total_iterations"]
        kept = rows[warmups:]
        med = lambda key: float(np.median([r[key] for r in kept]))
        ev = []
        for _ in range(50):
            t0 = time.perf_counter()
            s.evaluate(EVERYTHING)
            ev.append((time.perf_counter() - t0) * 1e3)
        last = kept[-1]
        case = {"stages": T, "shape": [TP.nx, TP.ne, TP.nc], "N": s.N, "nnz": list(s.nnz), "handle": s.info, "make_handle_s": make_s, "status": last["status"],
                "statuses": [r["status"] for r in kept], "total_iterations": last["total_iterations"], "accepted_iterates": last["accepted_iterates"],
                "outer_iterations": last["outer_iterations"], "factorizations": last["factorizations"], "refinement_failures": last["refinement_failures"],
                "fallbacks": last["fallbacks"], "fallbacks_unconverged": last["fallbacks_unconverged"], "host_waits": last["host_waits"],
                "line_search_trials": last["line_search_trials"], "vector_ms": med("vector_ms"), "search_direction_ms": med("search_direction_ms"), "wall_ms": med("wall_ms"),
                "wall_with_initialize_ms": med("wall_with_initialize_ms"), "evaluate_synchronised_ms": float(np.median(ev)), "evaluations_enqueued": TP.enqueued(s),
                "other_handle": None}
        if other is not None:
            case["other_handle"] = {"kind": "structured" if other.structure is not None else "dense", "wall_with_initialize_ms": float(np.median(other_ms[warmups:])),
                                    "converged": other_ok, "total_iterations": other_iterations,
                                    "solution_difference": float(np.abs(other.solution.all - s.get("solution")).max())}
            other.close()
        s.close()
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
