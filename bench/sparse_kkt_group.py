"""One search_direction! of a GROUP of same-pattern sparse problems in lockstep (calipso.jl_amd.SparseKKTGroup, csrc/sparse_kkt_group.hip) against the same members on
`members` single SparseKKT handles called one after the other — what there was before the group.  The problems are those of bench/sparse_kkt.py (a T-stage conic QP,
generated sparsely) at T = 128 and T = 2048; members 1, 8, 32, 128.  Each member has its own values (the generator's seeds 0 .. 7, cycling) and its own point (the x
part drawn per member) and residual.  The two are alternated in the same process; medians after warm-up, with the quartiles' distance as the run-to-run spread;
device time from the handles' HIP events, wall time beside it.  A size that does not fit the device memory is skipped and listed.  Prints one JSON line; --out writes
it to a file as well.

    python bench/sparse_kkt_group.py [--stages 128 2048] [--members 1 8 32 128] [--reps 10] [--out profiles/sparse_kkt_group.json]"""
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

import sparse_kkt as single_bench      # staged_sparse, residual, KAPPA, RHO

BASES = 8
WARMUP = 3


def members_of(T, count):
    """per member: (Lxx, gx, hx, w, R); one pattern"""
    bases = [single_bench.staged_sparse(T, seed=s) for s in range(min(BASES, count))]
    out = []
    for m in range(count):
        Lxx, gx, hx, q, b, h, n_nn, dims, w, lam = bases[m % len(bases)]
        w = w.copy()
        w[:Lxx.shape[0]] = np.random.default_rng(1000 + m).uniform(-1, 1, Lxx.shape[0])
        out.append((Lxx, gx, hx, w, single_bench.residual(Lxx, gx, hx, q, b, h, n_nn, dims, w, lam)))
    return out, bases[0][6], bases[0][7]


def stats(values):
    v = np.asarray(values, dtype=np.float64)
    return dict(median=float(np.median(v)), spread=float(np.percentile(v, 75) - np.percentile(v, 25)), min=float(v.min()), max=float(v.max()))


def measure(T, count, reps):
    import torch
    from helpers import load_pkg
    pkg = load_pkg()
    ms, n_nn, dims = members_of(T, count)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), dtype=torch.float64, device="cuda:0")
    t0 = time.perf_counter()
    g = pkg.SparseKKTGroup(ms[0][0], ms[0][1], ms[0][2], members=count, n_nonnegative=n_nn, second_order_dims=dims)
    group_create_s = time.perf_counter() - t0
    g.set_values(dev(np.stack([m[0].data for m in ms])), dev(np.stack([m[1].data for m in ms])), dev(np.stack([m[2].data for m in ms])), dev(np.stack([m[3] for m in ms])),
                 dev(np.full(count, single_bench.RHO)), central_path=single_bench.KAPPA)
    Rg = dev(np.stack([m[4] for m in ms]))
    t0 = time.perf_counter()
    singles, Rs = [], []
    for Lxx, gx, hx, w, R in ms:
        s = pkg.SparseKKT(Lxx, gx, hx, n_nonnegative=n_nn, second_order_dims=dims)
        s.set_values(dev(Lxx.data), dev(gx.data), dev(hx.data), dev(w), dev([single_bench.RHO]), central_path=single_bench.KAPPA)
        singles.append(s); Rs.append(dev(R))
    singles_create_s = time.perf_counter() - t0
    torch.cuda.synchronize()
    rows = dict(group_device=[], group_wall=[], single_device=[], single_wall=[])
    phases, single_phases = [], []
    for k in range(WARMUP + reps):                                        # alternated in the same process
        t0 = time.perf_counter()
        steps, regs, infos, statuses, report = g.search_direction(Rg, (0.0, 0.0, 0.0))
        gw = 1e3 * (time.perf_counter() - t0)
        gt = g.timing()
        t0 = time.perf_counter()
        sd, sp_ = 0.0, dict(assemble=0.0, factorize=0.0, solve=0.0, refinement_solves=0.0, refinement_mul=0.0)
        outs = []
        for s, R in zip(singles, Rs):
            outs.append(s.search_direction(R, (0.0, 0.0, 0.0)))
            t = s.timing()
            for name in sp_:
                sp_[name] += t[name]
        sw = 1e3 * (time.perf_counter() - t0)
        sd = sum(sp_.values())
        if k >= WARMUP:
            rows["group_device"].append(gt["device"]); rows["group_wall"].append(gw); rows["single_device"].append(sd); rows["single_wall"].append(sw)
            phases.append(gt); single_phases.append(sp_)
    same = all(np.array_equal(steps[m].cpu().numpy(), outs[m][0].cpu().numpy()) and regs[m] == outs[m][1] and statuses[m] == outs[m][3] for m in range(count))
    st = {name: stats(v) for name, v in rows.items()}
    beats = {kind: st["single_" + kind]["median"] - st["group_" + kind]["median"] > st["single_" + kind]["spread"] + st["group_" + kind]["spread"] for kind in ("device", "wall")}
    med = lambda rs, name: float(np.median([r[name] for r in rs]))
    return dict(stages=T, members=count, N=g.N, n=g.n, nnz_triu_K=g.info["nnz_upper"], tree_levels=g.info["levels"], report=report, statuses=sorted(set(statuses)),
                factorizations=sorted(set(i["factorizations"] for i in infos)), refinement_rounds=sorted(set(i["refinement_rounds"] for i in infos)),
                members_equal_their_single_handles=bool(same), ms=st, speedup_device=st["single_device"]["median"] / st["group_device"]["median"],
                speedup_wall=st["single_wall"]["median"] / st["group_wall"]["median"], group_beats_sequential_by_more_than_the_spreads=beats,
                group_phases_ms={name: med(phases, name) for name in ("inertia_correction", "solve", "refinement")},
                sequential_phases_ms={name: med(single_phases, name) for name in single_phases[0]}, group_create_s=group_create_s, singles_create_s=singles_create_s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stages", type=int, nargs="+", default=[128, 2048])
    ap.add_argument("--members", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch      # (one HIP runtime per process: torch first, then the library)
    torch.zeros(1, device="cuda:0")
    from helpers import load_pkg
    rows, skipped = [], []
    for T in a.stages:
        for count in a.members:
            try:
                rows.append(measure(T, count, a.reps))
            except (load_pkg().CalipsoHipError, torch.cuda.OutOfMemoryError) as e:
                if "out of memory" not in str(e).lower():
                    raise
                skipped.append(dict(stages=T, members=count, reason="does not fit the device memory"))
            torch.cuda.empty_cache()
            print("# %d stages, %d members done" % (T, count), file=sys.stderr, flush=True)
    result = dict(benchmark="sparse_kkt_group", stage=dict(nv=single_bench.NV, nd=single_bench.ND, nonnegative=single_bench.NN, second_order=single_bench.NSOC, dimension=single_bench.DIM),
                  reps=a.reps, warmup=WARMUP, spread="distance of the quartiles over the repetitions", rows=rows, skipped=skipped)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
