"""Reverse-mode differentiate! for a group in lockstep against the same twelve reverse calls handle by handle (recorded, not asserted in a test).

For each shape — tests/test_gpu_group.py's SHAPE and bench.py's C4 — a group of 12 QP-attached members (bench.py's make_instance state, one Newton step taken) and
twelve twin handles in the same state are timed in one process, alternating, for k = 1 and k = 8 cotangent columns with all six QP data gradients:
  group   `ms` of calipso_hip_group_differentiate_adjoint: HIP events from the entry's first enqueue to its last kernel, ONE factorisation launch chain and one
          transposed condensed solve for all members
  single  the sum over the twelve twins of calipso_hip_differentiate_adjoint_times()[0] (the same interval of the single-handle entry), whose code path is the
          one the library had before the group entry existed: twelve launch chains
ratio = group / single (medians); >= 1 would mean that the launches are not shared.  One JSON line.

    python bench/group_differentiate_adjoint.py [--reps 10] [--warmup 2] [--members 12] [--shapes 300,140,40,20,3:2302,2208,244,240,2]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make(pkg, pr, pid, shape):
    nx, ne, n_nn, n_soc, dim = shape
    prob, pt, lam = pr.synthetic_conic_qp(pkg.splitmix_uniform, pid, nx, ne, n_nn, n_soc, dim)
    s = pkg.Solver(prob, prob.nx, 0, prob.ne, prob.nc, nonnegative_indices=prob.nonnegative_indices, second_order_indices=prob.second_order_indices)
    s.set("solution", np.concatenate([pt[k] for k in "xrsyzt"]))
    s.set("dual", lam)
    for name, v in (("central_path", 0.17), ("penalty", 52.0), ("fraction_to_boundary", 0.99)):
        s.set(name, [v])
    s.qp_attach(prob.P, prob.q, prob.A, prob.b, prob.G, prob.h, 0.5)
    fl = pkg.FLAGS
    s.qp_evaluate(fl["objective"] | fl["equality_constraint"] | fl["cone_constraint"], 0)
    s.cone(product=True, target=True)
    s.synchronize()
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--members", type=int, default=12)
    ap.add_argument("--shapes", default="300,140,40,20,3:2302,2208,244,240,2")
    args = ap.parse_args()
    import __graft_entry__ as entry
    pkg = entry.load_package()
    import problems as pr
    B = args.members
    results = []
    for text in args.shapes.split(":"):
        shape = tuple(int(v) for v in text.split(","))
        members = [make(pkg, pr, pid, shape) for pid in range(B)]
        twins = [make(pkg, pr, pid, shape) for pid in range(B)]
        grp = pkg.Group(members)
        grp.newton_step(advance=True)
        for t in twins:
            t.newton_step(advance=True)
        N = members[0].N
        row = {"shape": list(shape), "N": int(N), "padded_nx": int(members[0].padded_nx())}
        for k in (1, 8):
            V = np.random.default_rng(k).standard_normal((B, N, k))
            Vg = V[:, :, 0] if k == 1 else V

            def single():
                total = 0.0
                for i, t in enumerate(twins):
                    t.vjp(Vg[i], theta=False, qp=True)
                    total += t.vjp_times()["device"]
                return total

            def group():
                out = grp.vjp(Vg, theta=False, qp=True)
                assert not out["status"].any()
                return grp.vjp_ms()

            for _ in range(args.warmup):
                group(); single()
            g_ms, s_ms = [], []
            for _ in range(args.reps):                 # alternating: the two share whatever else the machine is doing
                g_ms.append(group()); s_ms.append(single())
            gm, sm = float(np.median(g_ms)), float(np.median(s_ms))
            gq, sq = np.percentile(g_ms, [25, 75]), np.percentile(s_ms, [25, 75])
            row["k%d" % k] = {"group_ms": gm, "group_quartiles_ms": [float(gq[0]), float(gq[1])], "sum_of_singles_ms": sm,
                              "sum_of_singles_quartiles_ms": [float(sq[0]), float(sq[1])], "ratio": gm / sm, "launches_shared": bool(gm < sm)}
        results.append(row)
        grp.close()
        del grp, members, twins
    print(json.dumps({"bench": "group_differentiate_adjoint", "members": B, "reps": args.reps, "warmup": args.warmup, "results": results}))


if __name__ == "__main__":
    main()
