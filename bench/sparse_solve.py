"""A whole solve! on sparse, device-resident problem data (calipso.jl_amd.SparseKKT.solve, csrc/sparse_solve.hip) for the T-stage conic QP of bench/sparse_kkt.py
(stages of 12 variables, 8 dynamics rows, 2 nonnegative rows, 2 cones of dimension 3) at T = 128 and T = 2048: data resident, continue_after_refinement_failure = 1,
cold solves from x0 = 0, medians after a warm-up.  Per solve: iterations, factorisations, refinement failures, host waits outside search_direction, device time of
the vector half beside the device time inside search_direction, wall time.  In the same run, alternating with it, the T = 128 problem through the structured
dense handle (Solver(structure=...) + qp_attach + solve!): the way to solve this problem without the sparse solve.  Needs a GPU; there is no CPU path.

--fallback: the same rows with the `H \\ residual` fallback by preconditioned GMRES (krylov_fallback = 1, csrc/sparse_krylov.hip) AND with
continue_after_refinement_failure = 1, two handles alternating in the same run (and, at --dense-at stages, the dense handle, whose fallback is a dense LU).  Per row
and route: status, fallbacks, GMRES iterations per fallback, device ms inside search_direction (the fallbacks' included), wall.  The solve does not report its
fallbacks' device time apart, so the cost of an iteration is measured beside it: solve_nonsymmetric on a resident right-hand side of ones with the factorisation
the solve left (HIP events around the whole GMRES solve, divided by its iterations), and "ms per fallback" is that times the solve's iterations per fallback.

    python bench/sparse_solve.py [--stages 128 2048] [--seeds 0] [--reps 10] [--out profiles/sparse_solve.json]
    python bench/sparse_solve.py --fallback --seeds 0 1 2 3 --reps 5 --out profiles/sparse_solve_fallback.json"""
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

WARMUP = 2


CONTINUE, KRYLOV = dict(continue_after_refinement_failure=1), dict(krylov_fallback=1)


def sparse_handle(pkg, data, options=CONTINUE):
    import torch
    Lxx, gx, hx, q, b, h, n_nn, dims = data[:8]
    g = pkg.SparseKKT(Lxx, gx, hx, n_nonnegative=n_nn, second_order_dims=dims, options=options)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64).reshape(-1), dtype=torch.float64, device="cuda:0")
    g.set_values(dev(Lxx.data), dev(gx.data), dev(hx.data))
    g.attach_qp(dev(q), dev(b), dev(h))
    x0 = dev(np.zeros(g.nx))
    return g, x0


def sparse_solve_once(pkg, g, x0):
    t0 = time.perf_counter()
    g.initialize(x0)
    try:
        g.solve()
    except pkg.CalipsoHipError:      # (one of the reference's error()s: the row reports its status)
        pass
    return dict(g.solve_info, route_wall_ms=1e3 * (time.perf_counter() - t0), **{"fallback_" + k: v for k, v in g.fallback_info().items()})


def dense_handle(pkg, data):
    """the structured dense handle of the same problem (tests/test_gpu_blocks.build_structured's route)"""
    import problems as pr
    from sparse_kkt import DIM
    Lxx, gx, hx, q, b, h, n_nn, dims = data[:8]
    soc = [list(range(n_nn + k * DIM + 1, n_nn + (k + 1) * DIM + 1)) for k in range(len(dims))]
    prob = pr.ConicQP(Lxx.toarray(), q, gx.toarray(), b, -hx.toarray(), h, nonnegative_indices=list(range(1, n_nn + 1)), second_order_indices=soc)
    s = pkg.Solver(prob, prob.nx, 0, prob.ne, prob.nc, nonnegative_indices=prob.nonnegative_indices, second_order_indices=prob.second_order_indices,
                   structure=pr.declared_structure(prob))
    s.qp_attach(prob.P, prob.q, prob.A, prob.b, prob.G, prob.h, 0.5)
    return s, prob


def dense_solve_once(pkg, s, prob):
    t0 = time.perf_counter()
    pkg.initialize_b(s, np.zeros(prob.nx))
    try:
        ok = pkg.solve_b(s)
    except pkg.CalipsoHipError:
        ok = -1
    s.synchronize()
    wall = 1e3 * (time.perf_counter() - t0)
    st = s.stats()
    return dict(status=int(ok), wall_ms=wall, total_iterations=st["total_iterations"], factorizations=st["factorizations"], fallbacks=st["fallbacks"])


def median_row(rows, keys):
    return {k: float(np.median([r[k] for r in rows])) for k in keys}


STATUS_TEXT = {1: "solved", 0: "iteration caps", -1: "inertia correction failure", -2: "cone search failure", -102: "refinement failure"}


def gmres_probe(pkg, g, reps):
    """solve_nonsymmetric on ones with the factorisation the last solve left: median device ms, iterations, launches; None where the handle has no factorisation"""
    import torch
    r = torch.ones(g.N, dtype=torch.float64, device="cuda:0")
    runs = []
    try:
        for k in range(WARMUP + reps):
            g.solve_nonsymmetric(r)
            if k >= WARMUP:
                runs.append(g.fallback_info())
    except pkg.CalipsoHipError:
        return None
    last = runs[-1]
    ms = float(np.median([f["device_ms"] for f in runs]))
    return dict(iterations=last["iterations"], cycles=last["cycles"], converged=last["converged"], launches=last["launches"], residual_norm=last["residual_norm"],
                device_ms=ms, device_ms_per_iteration=ms / max(last["iterations"], 1))


def fallback_rows(pkg, a, staged_sparse):
    """--fallback: per (stages, seed) the GMRES fallback beside continue_after_refinement_failure (and the dense handle), alternating in the same run"""
    counted = ("status", "total_iterations", "accepted_iterates", "factorizations", "refinement_failures", "fallback_solve_fallbacks", "fallback_solve_iterations",
               "fallback_solve_most_iterations", "fallback_solve_unconverged")
    timed = ("vector_ms", "search_direction_ms", "wall_ms", "route_wall_ms")
    rows = []
    for T, seed in [(T, seed) for T in a.stages for seed in a.seeds]:
        data = staged_sparse(T, seed)
        handles = dict(krylov_fallback=sparse_handle(pkg, data, KRYLOV), continue_after_refinement_failure=sparse_handle(pkg, data, CONTINUE))
        dense = dense_handle(pkg, data) if T == a.dense_at else None
        runs, dense_runs = {k: [] for k in handles}, []
        for k in range(WARMUP + a.reps):
            got = {name: sparse_solve_once(pkg, *gx0) for name, gx0 in handles.items()}
            d = dense_solve_once(pkg, *dense) if dense else None
            if k >= WARMUP:
                for name in handles:
                    runs[name].append(got[name])
                if d:
                    dense_runs.append(d)
        g = handles["krylov_fallback"][0]
        row = dict(stages=T, seed=seed, n=g.n, N=g.N)
        for name, rs in runs.items():
            last = rs[-1]
            assert all(all(r[k] == last[k] for k in counted) for r in rs), "a solve did not repeat its counts"
            r = dict({k: last[k] for k in counted}, status_text=STATUS_TEXT.get(last["status"], str(last["status"])), **median_row(rs, timed))
            if name == "krylov_fallback":
                n = max(last["fallback_solve_fallbacks"], 1)
                probe = gmres_probe(pkg, g, a.reps)
                r.update(iterations_per_fallback=last["fallback_solve_iterations"] / n, workspace_bytes=g.fallback_info()["workspace_bytes"], gmres_probe=probe,
                         ms_per_fallback=None if probe is None else probe["device_ms_per_iteration"] * last["fallback_solve_iterations"] / n)
            row[name] = r
        if dense_runs:
            dl = dense_runs[-1]
            row["dense_handle"] = dict(status=dl["status"], total_iterations=dl["total_iterations"], factorizations=dl["factorizations"], fallbacks=dl["fallbacks"],
                                       wall_ms=float(np.median([d["wall_ms"] for d in dense_runs])))
        rows.append(row)
        for gx0 in handles.values():
            gx0[0].close()
        if dense:
            dense[0].close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stages", type=int, nargs="+", default=[128, 2048])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seeds", type=int, nargs="+", default=[0], help="seeds of bench/sparse_kkt.staged_sparse: one row per (stages, seed)")
    ap.add_argument("--dense-at", type=int, default=128, help="the stage count that is also solved through the structured dense handle")
    ap.add_argument("--fallback", action="store_true", help="krylov_fallback = 1 beside continue_after_refinement_failure = 1, alternating in the same run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch      # (one HIP runtime per process: torch first, then the library)
    if not torch.cuda.is_available():
        raise SystemExit("bench/sparse_solve.py needs a GPU: there is no CPU path")
    torch.zeros(1, device="cuda:0")
    from helpers import load_pkg
    from sparse_kkt import DIM, ND, NN, NSOC, NV, staged_sparse
    pkg = load_pkg()
    timed = ("vector_ms", "search_direction_ms", "wall_ms", "route_wall_ms")      # route_wall_ms: initialize + solve, as the dense handle's wall_ms
    counted = ("status", "total_iterations", "outer_iterations", "accepted_iterates", "factorizations", "max_refinement_rounds", "refinement_failures", "worst_warning",
               "host_waits", "line_search_trials")
    rows = fallback_rows(pkg, a, staged_sparse) if a.fallback else []
    for T, seed in [(T, seed) for T in a.stages for seed in a.seeds if not a.fallback]:
        data = staged_sparse(T, seed)
        g, x0 = sparse_handle(pkg, data)
        dense = dense_handle(pkg, data) if T == a.dense_at else None
        sparse_runs, dense_runs = [], []
        for k in range(WARMUP + a.reps):                                  # alternating: both routes see the same machine state
            r = sparse_solve_once(pkg, g, x0)
            d = dense_solve_once(pkg, *dense) if dense else None
            if k >= WARMUP:
                sparse_runs.append(r)
                if d:
                    dense_runs.append(d)
        last = sparse_runs[-1]
        assert all(all(r[k] == last[k] for k in counted) for r in sparse_runs), "a solve did not repeat its counts"
        row = dict(stages=T, seed=seed, nx=g.nx, ne=g.ne, nc=g.nc, n=g.n, N=g.N, **{k: last[k] for k in counted}, **median_row(sparse_runs, timed))
        steps = max(last["accepted_iterates"], 1)
        row.update(host_waits_per_step=last["host_waits"] / steps, vector_ms_per_step=row["vector_ms"] / steps, search_direction_ms_per_step=row["search_direction_ms"] / steps,
                   vector_share_of_device_time=row["vector_ms"] / (row["vector_ms"] + row["search_direction_ms"]))
        if dense_runs:
            dl = dense_runs[-1]
            row["dense_handle"] = dict(status=dl["status"], total_iterations=dl["total_iterations"], factorizations=dl["factorizations"], fallbacks=dl["fallbacks"],
                                       wall_ms=float(np.median([d["wall_ms"] for d in dense_runs])))
        rows.append(row)
        g.close()
        if dense:
            dense[0].close()
    result = dict(benchmark="sparse_solve_fallback" if a.fallback else "sparse_solve", stage=dict(nv=NV, nd=ND, nonnegative=NN, second_order=NSOC, dimension=DIM), warmup=WARMUP, reps=a.reps, rows=rows)
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
