"""One search_direction! on sparse, device-resident problem data (calipso.jl_amd.SparseKKT, csrc/sparse_kkt.hip) for a T-stage conic QP with the structure of
tests/problems.staged_conic_qp — generated SPARSELY here, so that no nx^2 array exists — at T = 128 and T = 2048, split into its phases with the handle's HIP events
(assemble, factorise, first solve, refinement solves, the H v + norm of the refinement rounds), and beside it, at T = 128 only, the CPU oracle's search_direction on
one core (the oracle is dense: T = 2048 has no CPU row).  Prints one JSON line; --out writes it to a file as well.

    python bench/sparse_kkt.py [--stages 128 2048] [--reps 20] [--out profiles/sparse_kkt.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

NV, ND, NN, NSOC, DIM = 12, 8, 2, 2, 3        # per stage: variables, dynamics rows to the next stage, nonnegative rows, second-order cones and their dimension
KAPPA, RHO = 0.17, 52.0


def staged_sparse(T, seed=0):
    """(Lxx, gx, hx CSC, q, b, h, n_nonnegative, dims, point w, lam): staged_conic_qp's structure from a numpy generator, block by block"""
    rng = np.random.default_rng(seed)
    nx, ne, n_nn, n_soc = T * NV, (T - 1) * ND, T * NN, T * NSOC
    nc = n_nn + n_soc * DIM
    B = rng.uniform(-1, 1, (T, NV, NV))
    P = (B + np.transpose(B, (0, 2, 1))) / (2.0 * np.sqrt(NV)) + 2.0 * np.eye(NV)
    Lxx = sp.block_diag([P[t] for t in range(T)], format="csc")
    rows, cols, vals = [], [], []
    for t in range(T - 1):                                  # dynamics rows of the stage pair (t, t + 1)
        blk = rng.uniform(-1, 1, (ND, 2 * NV)) / np.sqrt(2 * NV)
        r, c = np.meshgrid(np.arange(ND) + t * ND, np.arange(2 * NV) + t * NV, indexing="ij")
        rows.append(r.ravel()); cols.append(c.ravel()); vals.append(blk.ravel())
    gx = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(ne, nx))
    stage_of_row = np.concatenate([np.arange(n_nn) // NN, np.repeat(np.arange(n_soc) // NSOC, DIM)])
    r, c = np.meshgrid(np.arange(nc), np.arange(NV), indexing="ij")
    hx = sp.csc_matrix((-(rng.uniform(-1, 1, (nc, NV)) / np.sqrt(NV)).ravel(), (r.ravel(), (c + stage_of_row[:, None] * NV).ravel())), shape=(nc, nx))

    def cone_point(lo_tail):
        v = np.zeros(nc)
        v[:n_nn] = rng.uniform(0.5, 1.5, n_nn)
        blocks = rng.uniform(-lo_tail, lo_tail, (n_soc, DIM))
        blocks[:, 0] = 1.0 + np.linalg.norm(blocks[:, 1:], axis=1)
        v[n_nn:] = blocks.ravel()
        return v
    xbar = rng.uniform(-1, 1, nx)
    q, b, h = rng.uniform(-1, 1, nx), gx @ xbar, -(hx @ xbar) + cone_point(0.3)
    w = np.concatenate([rng.uniform(-1, 1, nx), 0.1 * rng.uniform(-1, 1, ne), cone_point(0.3), rng.uniform(-1, 1, ne), rng.uniform(-1, 1, nc), cone_point(0.3)])
    return Lxx, gx, hx, q, b, h, n_nn, [DIM] * n_soc, w, rng.uniform(-1, 1, ne)


def residual(Lxx, gx, hx, q, b, h, n_nn, dims, w, lam):
    """residual! (residual.jl:1-51) of the QP at w, with sparse products"""
    nx, ne, nc = Lxx.shape[0], gx.shape[0], hx.shape[0]
    o = np.cumsum([0, nx, ne, nc, ne, nc, nc])
    x, r, s, y, z, t = (w[o[k]:o[k + 1]] for k in range(6))
    prod, target = s * t, np.zeros(nc)
    target[:n_nn] = 1.0
    S, Tt = s[n_nn:].reshape(len(dims), -1), t[n_nn:].reshape(len(dims), -1)      # (all cones of one dimension here)
    blk = np.empty_like(S)
    blk[:, 0] = (S * Tt).sum(axis=1)
    blk[:, 1:] = S[:, :1] * Tt[:, 1:] + Tt[:, :1] * S[:, 1:]
    prod[n_nn:] = blk.ravel()
    target[n_nn::S.shape[1]] = 1.0
    return np.concatenate([Lxx @ x + q + gx.T @ y + hx.T @ z, lam + RHO * r - y, -z - t, gx @ x - b - r, h + hx @ x - s, prod - KAPPA * target])


def measure(T, reps):
    import torch
    from helpers import load_pkg
    pkg = load_pkg()
    Lxx, gx, hx, q, b, h, n_nn, dims, w, lam = staged_sparse(T)
    R = residual(Lxx, gx, hx, q, b, h, n_nn, dims, w, lam)
    t0 = time.perf_counter()
    g = pkg.SparseKKT(Lxx, gx, hx, n_nonnegative=n_nn, second_order_dims=dims)
    analyse_s = time.perf_counter() - t0
    dev = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64).reshape(-1), dtype=torch.float64, device="cuda:0")
    g.set_values(dev(Lxx.data), dev(gx.data), dev(hx.data), dev(w), dev([RHO]), central_path=KAPPA)
    Rd = dev(R)
    rows = []
    for k in range(3 + reps):
        step, reg, info, status = g.search_direction(Rd, (0.0, 0.0, 0.0))
        if k >= 3:
            rows.append(g.timing())
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    device_ms = sum(med[k] for k in ("assemble", "factorize", "solve", "refinement_solves", "refinement_mul"))
    rounds = max(info["refinement_rounds"], 0)
    out = dict(stages=T, nx=g.nx, ne=g.ne, nc=g.nc, n=g.n, N=g.N, nnz_triu_K=g.info["nnz_upper"], nnz_L=g.info["nnzL"], tree_levels=g.info["levels"], numeric=g.info["numeric"],
               analyse_s=analyse_s, status=int(status), factorizations=info["factorizations"], refinement_rounds=rounds, residual_norm=info["residual_norm"],
               ms=med, device_ms=device_ms, wall_ms=med["wall"], assemble_share=med["assemble"] / device_ms, mul_share=med["refinement_mul"] / device_ms,
               mul_ms_per_evaluation=med["refinement_mul"] / (rounds + 1), refinement_solve_ms_per_round=med["refinement_solves"] / max(rounds, 1))
    return out, (Lxx, gx, hx, q, b, h, n_nn, dims, w, lam, R, step.cpu().numpy())


def oracle_row(data):
    """the oracle's search_direction on one core for the same problem, dense (and the GPU step held against it)"""
    import oracle
    import problems as pr
    from helpers import oracle_newton_state
    Lxx, gx, hx, q, b, h, n_nn, dims, w, lam, R, step = data
    nc = hx.shape[0]
    soc = [list(range(n_nn + k * DIM + 1, n_nn + (k + 1) * DIM + 1)) for k in range(len(dims))]
    prob = pr.ConicQP(Lxx.toarray(), q, gx.toarray(), b, -hx.toarray(), h, nonnegative_indices=list(range(1, n_nn + 1)), second_order_indices=soc)
    o = oracle_newton_state(oracle, prob, w, lam, kappa=KAPPA, rho=RHO)
    residual_difference = float(np.abs(o.buf("residual") - R).max())
    t0 = time.perf_counter()
    status = o.search_direction()
    ms = 1e3 * (time.perf_counter() - t0)
    so = o.buf("step")
    return dict(oracle_ms_one_core=ms, oracle_status=int(status), oracle_factorizations=o.stats()["factorizations"], oracle_refinement_rounds=o.stats()["last_refinement_rounds"],
                step_relative_difference=float(np.abs(step - so).max() / max(1.0, np.abs(so).max())), residual_difference=residual_difference, nc=nc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stages", type=int, nargs="+", default=[128, 2048])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--oracle-up-to", type=int, default=128, help="largest stage count with a CPU oracle row (the oracle is dense)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch      # (one HIP runtime per process: torch first, then the library)
    torch.zeros(1, device="cuda:0")
    rows = []
    for T in a.stages:
        row, data = measure(T, a.reps)
        if T <= a.oracle_up_to:
            row.update(oracle_row(data))
        rows.append(row)
    result = dict(benchmark="sparse_kkt", stage=dict(nv=NV, nd=ND, nonnegative=NN, second_order=NSOC, dimension=DIM), rows=rows)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
