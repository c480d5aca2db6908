"""differentiate! on sparse, device-resident problem data (SparseKKT.solve_columns / differentiate / vjp, csrc/sparse_differentiate.hip) on the T-stage conic QPs of
bench/sparse_kkt.py at T = 128 and T = 2048, for k = 1, 16 and 128 columns (recorded, not asserted in a test).  Device times come from HIP events on the handle's
stream (SparseKKT.timing, vjp_times); every figure is the median of --reps calls after --warmup.  Per (T, k):
  reverse    vjp(V, qp="LqgbHh") with CUDA tensors, split into assemble + factorisation, the transposed pre + ONE k-column LDL^T solve + post, the correction rounds
             (the problems have second-order cones, where the option is inert: 0) and the gradient kernel; wall time of the call beside them
  forward    differentiate(J): its pre + solve + post
  yardstick  k calls of the single-column solve_symmetric, in the same run: all a user could do for the forward direction before solve_columns existed.  That entry
             takes host arrays, so it is compared by wall clock with solve_columns on host arrays (both copy their columns in and out)
and at T = 128 the dense handle's differentiate_adjoint (Solver + qp_attach) on the same problem for k = 1 and 16, with the bytes each route holds for the call:
the dense handle's device_bytes and its k x (nx^2 + ...) gradient arrays against the sparse handle's differentiate_bytes and its gradients on the stored patterns.
Prints one JSON line; --out writes it to a file as well, --table prints the Markdown table of INTEGRATION.md.

    python bench/sparse_differentiate.py [--stages 128 2048] [--columns 1 16 128] [--reps 20] [--out profiles/sparse_differentiate.json] [--table]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "bench")):
    if p not in sys.path:
        sys.path.insert(0, p)

from sparse_kkt import DIM, KAPPA, RHO, residual, staged_sparse      # the problems of bench/sparse_kkt.py

median = lambda a: float(np.median(a))


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def measure(T, columns, reps, warmup):
    import torch
    from helpers import load_pkg
    pkg = load_pkg()
    Lxx, gx, hx, q, b, h, n_nn, dims, w, lam = staged_sparse(T)
    g = pkg.SparseKKT(Lxx, gx, hx, n_nonnegative=n_nn, second_order_dims=dims)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), dtype=torch.float64, device="cuda:0")
    g.set_values(dev(Lxx.data), dev(gx.data), dev(hx.data), dev(w), dev([RHO]), central_path=KAPPA)
    g.attach_qp(dev(q), dev(b), dev(h))
    # the regularisation a Newton step ends its inertia correction at: what a solve would leave the handle holding
    _, reg, _, status = g.search_direction(dev(residual(Lxx, gx, hx, q, b, h, n_nn, dims, w, lam)), (0.0, 0.0, 0.0))
    g.factorize(reg[0], reg[2])
    rng = np.random.default_rng(1)
    rows = []
    for k in columns:
        V = rng.standard_normal((g.N, k))
        Vd = dev(V)
        rec = {name: [] for name in ("reverse_wall", "reverse_device", "factorization", "reverse_map", "rounds", "gradients", "forward_map", "forward_wall", "columns_wall",
                                     "columns_map", "singles_wall")}
        for it in range(warmup + reps):
            t0 = g.timing()
            ms, out = wall(lambda: g.vjp(Vd, qp="LqgbHh"))
            t1, times = g.timing(), g.vjp_times()
            fwd_ms, _ = wall(lambda: g.differentiate(Vd))
            t2 = g.timing()
            g.factorize(reg[0], reg[2])
            col_ms, X = wall(lambda: g.solve_columns(V))
            t3 = g.timing()
            one_ms, x0 = wall(lambda: [g.solve_symmetric(V[:, j]) for j in range(k)])
            if it < warmup:
                continue
            rec["reverse_wall"].append(ms); rec["reverse_device"].append(times["device"]); rec["gradients"].append(times["gradients"])
            rec["factorization"].append((t1["assemble"] - t0["assemble"]) + (t1["factorize"] - t0["factorize"]))
            rec["reverse_map"].append(t1["columns_map"]); rec["rounds"].append(t1["columns_rounds"])
            rec["forward_map"].append(t2["columns_map"]); rec["forward_wall"].append(fwd_ms)
            rec["columns_wall"].append(col_ms); rec["columns_map"].append(t3["columns_map"]); rec["singles_wall"].append(one_ms)
        agree = float(np.abs(X[:, 0] - x0[0]).max() / max(1.0, np.abs(x0[0]).max()))
        grad_bytes = 8 * k * (sum(g.nnz) + g.nx + g.ne + g.nc)
        row = dict(stages=T, k=k, N=g.N, n=g.n, nnz=list(g.nnz), **{name + "_ms": median(a) for name, a in rec.items()}, vjp_info=g.vjp_info(),
                   singles_over_columns=median(rec["singles_wall"]) / median(rec["columns_wall"]), column_0_against_single=agree,
                   differentiate_bytes=g.differentiate_bytes(), gradient_bytes=grad_bytes)
        rows.append(row)
    return rows, (Lxx, gx, hx, q, b, h, n_nn, dims, w, lam, reg)


def dense_rows(data, columns, reps, warmup):
    """the dense handle's reverse mode on the same problem: Solver + qp_attach, the k x nx x nx gradient of P and the dense Jacobians' gradients"""
    import problems as pr
    from helpers import load_pkg
    pkg = load_pkg()
    Lxx, gx, hx, q, b, h, n_nn, dims, w, lam, reg = data
    soc = [list(range(n_nn + j * DIM + 1, n_nn + (j + 1) * DIM + 1)) for j in range(len(dims))]
    prob = pr.ConicQP(Lxx.toarray(), q, gx.toarray(), b, -hx.toarray(), h, nonnegative_indices=list(range(1, n_nn + 1)), second_order_indices=soc)
    s = pkg.Solver(prob, prob.nx, 0, prob.ne, prob.nc, nonnegative_indices=prob.nonnegative_indices, second_order_indices=prob.second_order_indices)
    s.set("solution", w)
    s.set("dual", lam)
    for name, v in (("central_path", KAPPA), ("penalty", RHO), ("primal_regularization", reg[0]), ("dual_regularization", reg[2])):
        s.set(name, [v])
    s.qp_attach(prob.P, prob.q, prob.A, prob.b, prob.G, prob.h, 0.5)
    s.qp_evaluate(pkg.FLAGS["objective"] | pkg.FLAGS["equality_constraint"] | pkg.FLAGS["cone_constraint"], 0)
    s.cone(product=True, jacobian=True, target=True)
    rng = np.random.default_rng(1)
    rows = []
    for k in columns:
        V = rng.standard_normal((s.N, k))
        rec = dict(wall=[], device=[], copy=[], gradients=[])
        for it in range(warmup + reps):
            ms, _ = wall(lambda: s.vjp(V, theta=False, qp=True))
            t = s.vjp_times()
            if it >= warmup:
                rec["wall"].append(ms); rec["device"].append(t["device"]); rec["copy"].append(t["copy"]); rec["gradients"].append(t["gradients"])
        rows.append(dict(k=k, N=int(s.N), **{"dense_" + name + "_ms": median(a) for name, a in rec.items()}, dense_device_bytes=int(s.device_bytes()),
                         dense_gradient_bytes=8 * k * (prob.nx * prob.nx + prob.nx + prob.ne * prob.nx + prob.ne + prob.nc * prob.nx + prob.nc)))
    return rows


def table(result):
    lines = ["| stages | N | k | factorisation | pre + solve + post (reverse) | rounds | gradient kernel | vjp device | vjp wall | forward pre + solve + post | solve_columns wall | k x solve_symmetric wall | ratio |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in result["rows"]:
        lines.append("| %d | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.2f | %.3f | %.2f | %.2f | %.1f |" % (
            r["stages"], r["N"], r["k"], r["factorization_ms"], r["reverse_map_ms"], r["rounds_ms"], r["gradients_ms"], r["reverse_device_ms"], r["reverse_wall_ms"],
            r["forward_map_ms"], r["columns_wall_ms"], r["singles_wall_ms"], r["singles_over_columns"]))
    lines.append("")
    lines.append("| k | dense vjp device | dense copies | dense wall | dense handle bytes | dense gradient bytes | sparse vjp wall | sparse workspace bytes | sparse gradient bytes |")
    lines.append("|---|---|---|---|---|---|---|---|---|")
    for d in result.get("dense", []):
        r = [x for x in result["rows"] if x["stages"] == result["dense_stages"] and x["k"] == d["k"]][0]
        lines.append("| %d | %.2f | %.2f | %.2f | %d | %d | %.2f | %d | %d |" % (d["k"], d["dense_device_ms"], d["dense_copy_ms"], d["dense_wall_ms"], d["dense_device_bytes"],
                                                                           d["dense_gradient_bytes"], r["reverse_wall_ms"], r["differentiate_bytes"], r["gradient_bytes"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stages", type=int, nargs="+", default=[128, 2048])
    ap.add_argument("--columns", type=int, nargs="+", default=[1, 16, 128])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dense-at", type=int, default=128, help="the stage count with the dense handle's rows (it forms nx x nx arrays)")
    ap.add_argument("--dense-columns", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--out", default=None)
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    import torch      # (one HIP runtime per process: torch first, then the library)
    torch.zeros(1, device="cuda:0")
    result = dict(benchmark="sparse_differentiate", reps=a.reps, warmup=a.warmup, rows=[], dense=[], dense_stages=a.dense_at)
    for T in a.stages:
        rows, data = measure(T, a.columns, a.reps, a.warmup)
        result["rows"] += rows
        if T == a.dense_at:
            result["dense"] = dense_rows(data, [k for k in a.dense_columns if k in a.columns], a.reps, a.warmup)
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if a.table:
        print(table(result))


if __name__ == "__main__":
    main()
