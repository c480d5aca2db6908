"""A whole solve! for GROUPS of same-pattern sparse conic QPs in lockstep (calipso.jl_amd.SparseKKTGroup.solve, csrc/sparse_solve_group.hip) beside the same members
on single SparseKKT handles called one after the other, alternating in the same process: the T-stage conic QP of bench/sparse_kkt.py / bench/sparse_solve.py at
T = 128 and T = 2048, members = 1, 8, 32, 128, continue_after_refinement_failure = 1 on both routes, values cycling over generated problems of the one pattern
(seeds 0 .. 7), data resident, cold solves from x0 = 0.  Medians of --reps after 2 warm-ups with quartile distances: wall time and device time (vector half +
search_direction) of both routes, the group's ticks, launches and host waits, the single handles' host waits.  Every member's counts are asserted equal to its
single handle's.  Needs a GPU; there is no CPU path.

    python bench/sparse_solve_group.py [--stages 128 2048] [--members 1 8 32 128] [--reps 5] [--max-single-handles 128] [--out profiles/sparse_solve_group.json]

--max-single-handles: above it the sequential route cycles over that many single handles (one per distinct problem at the least) instead of holding `members` of
them; the row says so."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bench")):
    if p not in sys.path:
        sys.path.insert(0, p)

WARMUP, SEEDS = 2, 8
CONTINUE = dict(continue_after_refinement_failure=1)
COUNTED = ("status", "total_iterations", "outer_iterations", "accepted_iterates", "factorizations", "max_refinement_rounds", "refinement_failures", "worst_warning",
           "host_waits", "line_search_trials")


def quartiles(values):
    q1, q2, q3 = np.percentile(np.asarray(values, dtype=np.float64), [25, 50, 75])
    return dict(median=float(q2), quartile_distance=float(q3 - q1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stages", type=int, nargs="+", default=[128, 2048])
    ap.add_argument("--members", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-single-handles", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch      # (one HIP runtime per process: torch first, then the library)
    if not torch.cuda.is_available():
        raise SystemExit("bench/sparse_solve_group.py needs a GPU: there is no CPU path")
    torch.zeros(1, device="cuda:0")
    from helpers import load_pkg
    from sparse_kkt import DIM, ND, NN, NSOC, NV, staged_sparse
    from sparse_solve import sparse_handle
    pkg = load_pkg()
    dev = lambda v: torch.tensor(np.ascontiguousarray(v, dtype=np.float64).reshape(-1), dtype=torch.float64, device="cuda:0")
    rows = []
    for T in a.stages:
        data = [staged_sparse(T, seed) for seed in range(SEEDS)]
        for members in a.members:
            pick = [data[m % SEEDS] for m in range(members)]
            Lxx, gx, hx, _, _, _, n_nn, dims = pick[0][:8]
            g = pkg.SparseKKTGroup(Lxx, gx, hx, members, n_nonnegative=n_nn, second_order_dims=dims, options=CONTINUE)
            stack = lambda k, sparse: dev(np.concatenate([(d[k].data if sparse else np.asarray(d[k])).reshape(-1) for d in pick]))
            g.set_values(stack(0, True), stack(1, True), stack(2, True))
            g.attach_qp(stack(3, False), stack(4, False), stack(5, False))
            x0 = dev(np.zeros(members * g.nx))
            held = min(members, max(a.max_single_handles, min(members, SEEDS)))
            singles = [sparse_handle(pkg, pick[m], CONTINUE) for m in range(held)]
            group_runs, single_runs = [], []
            for k in range(WARMUP + a.reps):                                  # alternating: both routes see the same machine state
                t0 = time.perf_counter()
                g.initialize(x0)
                statuses, infos, report = g.solve()
                group_wall = 1e3 * (time.perf_counter() - t0)
                t0 = time.perf_counter()
                got = []
                for m in range(members):
                    s, sx0 = singles[m % held]
                    s.initialize(sx0)
                    try:
                        s.solve()
                    except pkg.CalipsoHipError:      # (one of the reference's error()s: the member's status says so on both routes)
                        pass
                    got.append(dict(s.solve_info))
                single_wall = 1e3 * (time.perf_counter() - t0)
                for m in range(members):
                    assert [infos[m][c] for c in COUNTED] == [got[m][c] for c in COUNTED], ("member %d differs from its single handle" % m, infos[m], got[m])
                if k >= WARMUP:
                    group_runs.append(dict(wall_ms=group_wall, device_ms=report["vector_ms"] + report["search_direction_ms"], report=report, statuses=statuses))
                    single_runs.append(dict(wall_ms=single_wall, device_ms=sum(r["vector_ms"] + r["search_direction_ms"] for r in got),
                                            host_waits=sum(r["host_waits"] for r in got)))
            last = group_runs[-1]
            gw, sw = quartiles([r["wall_ms"] for r in group_runs]), quartiles([r["wall_ms"] for r in single_runs])
            row = dict(stages=T, members=members, n=g.n, N=g.N, single_handles_held=held,
                       statuses=sorted(set(last["statuses"])), accepted_iterates=[min(i["accepted_iterates"] for i in infos), max(i["accepted_iterates"] for i in infos)],
                       ticks=last["report"]["ticks"], outer_update_rounds=last["report"]["outer_update_rounds"], line_search_trial_rounds=last["report"]["line_search_trial_rounds"],
                       group_launches=last["report"]["solve_launches"], group_host_waits=last["report"]["solve_host_waits"],
                       group_wall_ms=gw, group_device_ms=quartiles([r["device_ms"] for r in group_runs]),
                       sequential_wall_ms=sw, sequential_device_ms=quartiles([r["device_ms"] for r in single_runs]),
                       sequential_vector_host_waits=single_runs[-1]["host_waits"],
                       wall_ratio_sequential_over_group=sw["median"] / gw["median"],
                       group_faster_beyond_both_spreads=bool(sw["median"] - gw["median"] > sw["quartile_distance"] + gw["quartile_distance"]))
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            g.close()
            for s, _ in singles:
                s.close()
    result = dict(benchmark="sparse_solve_group", stage=dict(nv=NV, nd=ND, nonnegative=NN, second_order=NSOC, dimension=DIM), warmup=WARMUP, reps=a.reps, seeds=SEEDS,
                  options=CONTINUE, rows=rows,
                  not_measured=["the single handles' host waits inside search_direction (their info counts the vector half's only)",
                                "groups with krylov_fallback (not built)", "a captured-graph replay of the group's factorisation (not built)"])
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
