"""Forward-mode differentiate! for a group in lockstep: the two forms of the batched GEMM against each other, and the group call against the same twelve calls handle
by handle (recorded, not asserted in a test).

For each shape a group of 12 parametric members (tests/problems.py: parametric_conic_qp, np = nx + ne + nc, host callbacks) at interior points and twelve twin handles in
the same state are timed in one process, alternating:
  tile16 / tile64  `ms[1]` of calipso_hip_group_differentiate with the tile forced: HIP events around the column pass alone (dR/dtheta formed -> last kernel), the
                   16-column form being the kernel the reverse mode has always had.  This A/B sets the column count from which tile = 0 takes the 64-column form
  group / singles  wall-clock of Group.differentiate() (tile = 0) against the sum of twelve Solver.differentiate() calls — the only way before the group entry existed;
                   both sides make the same twelve host callbacks
Shapes, by column count: np = 24 and 48 around the 16-column tile, a C5-like count (np = 102), tests/test_gpu_group.py's SHAPE (np = 540), and two shapes with more
than one solve block (np = 770, NP = 1024; np = 1200, NP = 1536).  One JSON line.

    python bench/group_differentiate.py [--reps 10] [--warmup 2] [--members 12] [--shapes 12,4,2,2,3:24,8,4,4,3:60,20,7,5,3:300,140,40,20,3:600,100,40,10,3:1100,60,10,10,3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make(pkg, pr, interior_point, pid, shape):
    prob = pr.parametric_conic_qp(*shape, seed=100 + pid)
    pt, lam = interior_point(prob, seed=pid)
    s = pkg.Solver(prob, prob.nx, prob.np, prob.ne, prob.nc, parameters=prob.parameters, nonnegative_indices=prob.nonnegative_indices,
                   second_order_indices=prob.second_order_indices)
    for name, v in (("central_path", 0.17), ("penalty", 52.0), ("primal_regularization", 1e-5), ("dual_regularization", 1e-5), ("fraction_to_boundary", 0.99)):
        s.set(name, [v])
    s.set("solution", np.concatenate([pt[k] for k in "xrsyzt"]))
    if prob.ne:
        s.set("dual", lam)
    s.evaluate(pr.ALL_VARIABLE_FLAGS, 0)
    s.cone(product=True, jacobian=True, target=True)
    s.synchronize()
    return s


def stats(v):
    q = np.percentile(v, [25, 75])
    return {"median_ms": float(np.median(v)), "quartiles_ms": [float(q[0]), float(q[1])]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--members", type=int, default=12)
    ap.add_argument("--shapes", default="12,4,2,2,3:24,8,4,4,3:60,20,7,5,3:300,140,40,20,3:600,100,40,10,3:1100,60,10,10,3")
    args = ap.parse_args()
    import __graft_entry__ as entry
    pkg = entry.load_package()
    import problems as pr
    from helpers import interior_point
    B = args.members
    results = []
    for text in args.shapes.split(":"):
        shape = tuple(int(v) for v in text.split(","))
        members = [make(pkg, pr, interior_point, pid, shape) for pid in range(B)]
        twins = [make(pkg, pr, interior_point, pid, shape) for pid in range(B)]
        grp = pkg.Group(members)

        def column_pass(tile):
            out = grp.differentiate(tile=tile)
            assert not out["status"].any()
            return grp.differentiate_ms()[1]

        def group_wall():
            t0 = time.perf_counter()
            grp.differentiate()
            return 1e3 * (time.perf_counter() - t0)

        def singles_wall():
            t0 = time.perf_counter()
            for t in twins:
                t.differentiate()
            return 1e3 * (time.perf_counter() - t0)

        for _ in range(args.warmup):
            column_pass(16); column_pass(64); group_wall(); singles_wall()
        t16, t64, gw, sw = [], [], [], []
        for _ in range(args.reps):                     # alternating: the four share whatever else the machine is doing
            t16.append(column_pass(16)); t64.append(column_pass(64)); gw.append(group_wall()); sw.append(singles_wall())
        a, b = stats(t16), stats(t64)
        spread = max(a["quartiles_ms"][1] - a["quartiles_ms"][0], b["quartiles_ms"][1] - b["quartiles_ms"][0])
        g, s = stats(gw), stats(sw)
        results.append({"shape": list(shape), "N": int(members[0].N), "np": int(members[0].np), "padded_nx": int(members[0].padded_nx()),
                        "column_pass_tile16": a, "column_pass_tile64": b, "tile64_faster_by_more_than_the_spread": bool(a["median_ms"] - b["median_ms"] > spread),
                        "group_wall": g, "sum_of_singles_wall": s, "ratio": g["median_ms"] / s["median_ms"], "group_cheaper": bool(g["median_ms"] < s["median_ms"])})
        grp.close()
        del grp, members, twins
    print(json.dumps({"bench": "group_differentiate", "members": B, "reps": args.reps, "warmup": args.warmup, "results": results}))


if __name__ == "__main__":
    main()
