"""Reverse-mode differentiate! on a Solver handle against a Newton step of the same handle (recorded, not asserted in a test).

A QP-attached handle of BASELINE config C3 (nx = 2500, ne = 1500, nc = 400 R+ + 200 x SOC3; bench.py's make_instance state: resident point, objective and
constraints evaluated, cone products formed) is timed, in one process, alternating the three so that they share the machine's state:
  (i)   vjp with k = 1 and no data gradients,
  (ii)  vjp with k = 1 and all six QP data gradients: device time and the copies to the host separately (calipso_hip_differentiate_adjoint_times),
  (iii) newton_step(advance=False) — the parent's code, the yardstick: (i) launches one factorisation and one of a step's several condensed solves.
Wall times are a host clock around calls that end in a stream synchronise; the device / copy split of a vjp is HIP-event timed by the library.  One JSON line: the
medians, the run-to-run spread of (iii) (its quartiles and extremes), the bytes the gradient kernels write and their share of the HBM peak over their own
event-timed duration.

    python bench/differentiate_adjoint.py [--reps 30] [--warmup 5] [--shape 2500,1500,400,200,3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12      # bytes / s (specification)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", default="2500,1500,400,200,3")
    ap.add_argument("--problem", type=int, default=0)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import __graft_entry__ as entry
    pkg = entry.load_package()
    import problems as pr
    nx, ne, n_nn, n_soc, dim = (int(v) for v in args.shape.split(","))
    prob, pt, lam = pr.synthetic_conic_qp(pkg.splitmix_uniform, args.problem, nx, ne, n_nn, n_soc, dim)
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
    v = np.random.default_rng(1).standard_normal(s.N)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return 1e3 * (time.perf_counter() - t0), out

    plain = lambda: s.vjp(v, adjoint=True, theta=False)
    full = lambda: s.vjp(v, adjoint=True, theta=False, qp=True)
    step = lambda: s.newton_step(advance=False)
    for _ in range(args.warmup):
        step(); plain(); full()
    rec = {k: [] for k in ("step_wall", "plain_wall", "plain_device", "full_wall", "full_device", "full_copy", "full_gradients")}
    for _ in range(args.reps):                     # alternating: the three share whatever else the machine is doing
        ms, info = timed(step)
        assert info["status"] >= 0
        rec["step_wall"].append(ms)
        ms, _ = timed(plain)
        t = s.vjp_times()
        rec["plain_wall"].append(ms); rec["plain_device"].append(t["device"])
        ms, _ = timed(full)
        t = s.vjp_times()
        rec["full_wall"].append(ms); rec["full_device"].append(t["device"]); rec["full_copy"].append(t["copy"]); rec["full_gradients"].append(t["gradients"])
    med = {k: float(np.median(a)) for k, a in rec.items()}
    q = np.percentile(rec["step_wall"], [0, 25, 75, 100])
    grad_bytes = 8.0 * (nx * nx + nx + prob.ne * nx + prob.ne + prob.nc * nx + prob.nc)
    extra = max(med["full_gradients"], 1e-9)                 # the gradient kernels between HIP events of their own (not a difference of two call times)
    gq = np.percentile(rec["full_gradients"], [25, 75])
    print(json.dumps({
        "bench": "differentiate_adjoint", "shape": [nx, prob.ne, prob.nc], "N": int(s.N), "reps": args.reps, "warmup": args.warmup,
        "i_vjp_k1_wall_ms": med["plain_wall"], "i_vjp_k1_device_ms": med["plain_device"],
        "ii_vjp_k1_all_gradients_wall_ms": med["full_wall"], "ii_device_ms": med["full_device"], "ii_host_copy_ms": med["full_copy"],
        "ii_gradient_bytes": grad_bytes, "ii_gradient_kernels_ms": extra, "ii_gradient_kernels_quartiles_ms": [float(gq[0]), float(gq[1])], "ii_share_of_hbm_peak": grad_bytes / (extra * 1e-3) / HBM_PEAK,
        "iii_newton_step_wall_ms": med["step_wall"], "iii_spread_ms": {"min": float(q[0]), "q25": float(q[1]), "q75": float(q[2]), "max": float(q[3])},
        "i_no_longer_than_iii": bool(med["plain_wall"] <= med["step_wall"]),
        "refinement_rounds_per_step": int(info["refinement_rounds"]), "vjp_info": s.vjp_info()}))


if __name__ == "__main__":
    main()
