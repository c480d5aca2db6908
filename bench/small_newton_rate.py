#!/usr/bin/env python3
"""Rate of the batched small-problem path (csrc/smallnewton.hip): python bench/small_newton_rate.py [nx ne nc [batch [steps]]] — whole solve!s of `batch` C5-shaped random
QPs (nx = 49, ne = 40: the shape of the reference's cart-pole MPC problem, examples/autotuning/cartpole.jl:85-146) in one launch, and `steps` non-advancing Newton
steps per instance in one launch; the same problems through the oracle on one host core for comparison (a sample of them).
  --soc q:d1,d2,...   cone layout: q nonnegative entries, then second-order cones of dimensions d1, d2, ... (nc = q + sum; replaces the positional nc)
  --lu-fallback       set_option("lu_fallback", 1): the reference's H \\ residual inside the kernel where refinement fails (else such instances stop with -102)
  --general K         also time K of the problems through the general path (calipso_hip_solve with the attached QP evaluator, one handle at a time)
  --evaluator cartpole   instead of random QPs: the cart-pole MPC problem itself (nx 49, ne 40, np 102) through the device evaluator of
                      tests/device_eval_small/cartpole_mpc.hip, per-instance parameters (x_init and weights moved by a few per cent): solve!s, Newton steps and
                      differentiate!s (dR/dtheta from the evaluator) per second for the batch (default 4096), beside the oracle's solve! + differentiate! on one core
  --vjp               also differentiate! in reverse mode (SmallNewtonBatch.vjp): VJPs per second for k = 1 cotangent per instance — with --evaluator cartpole the
                      autotuning row (e_{u_1}, the first action) contracted with the evaluator's dR/dtheta, beside the forward differentiates (102 columns); for
                      QPs a random cotangent on x with the gradients of all QP data (grad_qp)
  --layer [--repeats R]  instead of the launches: wall-clock milliseconds of torch_layer.QPLayer forward + backward (loss = sum(w * x), every input requires a gradient)
                      with torch.cuda.synchronize() around the timed region, the first call discarded, R >= 5 repeats (default 7) reported as min and all values —
                      (a) CPU tensors, (b) CUDA tensors, each with per-instance data and with ONE P shared by the batch
e.g. the cold-started SOC batch of DESIGN 5.00: python bench/small_newton_rate.py 48 12 0 4096 --soc 4:4,4,4,4 --lu-fallback --general 8"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
from __graft_entry__ import load_package
import problems as pr

def evaluator_rate(name, B, vjp=False):
    import ctypes
    if name != "cartpole":
        raise SystemExit("--evaluator: cartpole")
    pkg = load_package()
    prob = pr.cartpole_mpc()
    rng = np.random.default_rng(0)
    th = np.repeat(prob.parameters[None], B, axis=0)
    th[:, 10:14] += 0.05 * rng.uniform(-1, 1, (B, 4))
    for t in range(9):
        o = 0 if t == 0 else 14 + 10 * (t - 1)
        th[:, o + 5:o + 10] *= 1.0 + 0.1 * rng.uniform(-1, 1, (B, 5))
    th[:, 98:102] *= 1.0 + 0.1 * rng.uniform(-1, 1, (B, 4))
    opts = dict(residual_tolerance=1e-3, optimality_tolerance=1e-3, equality_tolerance=1e-3, complementarity_tolerance=1e-3, slack_tolerance=1e-3)
    sn = pkg.SmallNewtonBatch(prob.nx, prob.ne, prob.nc, B, options=opts)
    sn.set_evaluator(ctypes.CDLL(os.path.join(ROOT, "tests", "device_eval_small", "libsmall_evaluators.so")), "cartpole_mpc_kernels", prob.np)
    sn.set_parameters(th)
    x0 = np.repeat(prob.x0[None], B, axis=0)
    ms_all = []
    for rep in range(3):
        sn.initialize(x0)
        res, ms = sn.solve()
        ms_all.append(ms)
    st = sn.get_state()
    ms = min(ms_all)
    steps = int(st["counters"]["newton_steps"].sum())
    dms = min(sn.differentiate()[2] for _ in range(3))
    out = {"evaluator": "cartpole_mpc", "shape": [prob.nx, prob.ne, prob.nc], "n_parameters": prob.np, "batch": B,
           "solve": {"launch_ms": ms, "launch_ms_all": ms_all, "converged": int((res == 1).sum()), "solves_per_s": B / (ms * 1e-3), "newton_steps_total": steps,
                     "newton_steps_per_s": steps / (ms * 1e-3), "mean_iterations": float(st["counters"]["total_iterations"].mean())},
           "differentiate": {"launch_ms": dms, "differentiates_per_s": B / (dms * 1e-3)}}
    if vjp:      # reverse mode: one cotangent per instance, the autotuning row e_{u_1} (u_1 after the 4 states of stage 1), gradient over theta
        e = np.zeros((B, sn.N)); e[:, 4] = 1.0
        vms = [sn.vjp(e, adjoint=False)["ms"] for _ in range(3)]
        out["vjp"] = {"k": 1, "cotangent": "e_u1", "grad": "theta", "launch_ms": min(vms), "launch_ms_all": vms, "vjps_per_s": B / (min(vms) * 1e-3),
                      "forward_over_reverse_ms": dms / min(vms)}
    try:
        import oracle
        from test_oracle_solve import run as run_oracle
        ts = []
        for k in range(8):
            prob.parameters = th[k].copy()
            t0 = time.perf_counter(); run_oracle(oracle, prob, differentiate=1, **opts); ts.append(time.perf_counter() - t0)
        out["cpu_baseline"] = {"kind": "port", "cores": 1, "solve_and_differentiate_ms_median": 1e3 * float(np.median(ts)), "per_s": 1.0 / float(np.median(ts)),
                               "sample": "%d solve! + differentiate! by the oracle (evaluation through Python callbacks)" % len(ts)}
    except Exception as e:
        out["cpu_baseline"] = {"error": repr(e)}
    sn.close()
    print(json.dumps(out))


def layer_rate(nx, ne, nc, q, dims, soc_idx, B, repeats):
    import torch                                       # (one HIP runtime per process: torch first)
    pkg = load_package()
    from calipso_jl_amd.torch_layer import QPLayer
    nprob = min(B, 64)
    probs = [pr.random_qp(nx, ne, nc, seed=1000 + k, nonnegative_indices=list(range(1, q + 1)), second_order_indices=soc_idx or None) for k in range(nprob)]
    idx = np.arange(B) % nprob
    shape = {"P": (nx, nx), "q": (nx,), "A": (ne, nx), "b": (ne,), "G": (nc, nx), "h": (nc,)}
    st = lambda name: np.stack([np.asarray(getattr(probs[i], name), dtype=np.float64).reshape(shape[name]) for i in idx])
    data = {name: st(name) for name in "PqAbGh"}
    wx = np.random.default_rng(0).standard_normal((B, nx))
    out = {"layer": "QPLayer forward + backward, wall clock", "shape": [nx, ne, nc], "batch": B, "repeats": repeats, "torch": torch.__version__}
    for device in ("cpu", "cuda"):
        for variant in ("per_instance", "shared_P"):
            sn = pkg.SmallNewtonBatch(nx, ne, nc, B)
            if dims: sn.set_cones(q, dims)
            ts = [torch.tensor(data[name][0] if (variant == "shared_P" and name == "P") else data[name], device=device, requires_grad=True) for name in "PqAbGh"]
            w = torch.tensor(wx, device=device)
            ms = []
            for r in range(repeats + 1):
                for t_ in ts: t_.grad = None
                torch.cuda.synchronize(); t0 = time.perf_counter()
                x = QPLayer.apply(sn, *ts, False, probs[0].c)
                (x * w).sum().backward()
                torch.cuda.synchronize(); ms.append(1e3 * (time.perf_counter() - t0))
            ms = ms[1:]                                # (the first call sizes buffers and pools)
            out["%s_%s" % (device, variant)] = {"ms_min": min(ms), "ms_median": float(np.median(ms)), "ms_all": ms, "finite_gradients": bool(all(torch.isfinite(t_.grad).all() for t_ in ts))}
            sn.close()
    print(json.dumps(out))


def main():
    a = sys.argv[1:]
    flag = lambda name: name in a and (a.remove(name) or True)
    def opt(name):
        if name not in a: return None
        i = a.index(name); v = a[i + 1]; del a[i:i + 2]; return v
    ev = None
    vjp = flag("--vjp")
    if "--evaluator" in a:
        i = a.index("--evaluator"); ev = a[i + 1]; del a[i:i + 2]
        return evaluator_rate(ev, int(a[0]) if a else 4096, vjp)
    lu = flag("--lu-fallback")
    layer = max(5, int(opt("--repeats") or 7)) if flag("--layer") else None
    soc_arg, general = opt("--soc"), int(opt("--general") or 0)
    nx, ne, nc = (int(a[0]), int(a[1]), int(a[2])) if len(a) >= 3 else (49, 40, 0)
    q, dims = nc, []
    if soc_arg:
        q_s, d_s = soc_arg.split(":")
        q, dims = int(q_s), [int(x) for x in d_s.split(",") if x]
        nc = q + sum(dims)
    soc_idx, at = [], q + 1
    for dm in dims:
        soc_idx.append(list(range(at, at + dm))); at += dm
    B = int(a[3]) if len(a) > 3 else 4096
    K = int(a[4]) if len(a) > 4 else 20
    if layer: return layer_rate(nx, ne, nc, q, dims, soc_idx, B, layer)
    pkg = load_package()
    nprob = min(B, 64)                                 # distinct problems (the batch cycles through them with perturbed starting points)
    probs = [pr.random_qp(nx, ne, nc, seed=1000 + k, nonnegative_indices=list(range(1, q + 1)), second_order_indices=soc_idx or None) for k in range(nprob)]
    idx = np.arange(B) % nprob
    st = lambda name: np.stack([np.asarray(getattr(probs[i], name), dtype=np.float64) for i in idx])
    sn = pkg.SmallNewtonBatch(nx, ne, nc, B)
    if os.environ.get("SN_THREADS"): sn.set_option("threads", int(os.environ["SN_THREADS"]))      # threads per instance (0 / unset: chosen by the LDS footprint)
    if dims: sn.set_cones(q, dims)
    if lu: sn.set_option("lu_fallback", 1)
    sn.set_qp(st("P"), st("q"), st("A"), st("b"), st("G"), st("h"), objective_scale=probs[0].c, shared=False)
    rng = np.random.default_rng(0)
    x0 = np.stack([probs[i].x0 for i in idx]) + 0.01 * rng.standard_normal((B, nx))
    import ctypes as C
    from calipso_jl_amd._lib import lib
    dsc = np.zeros(4); f = lib().calipso_hip_debug_smallnewton_describe; f.argtypes = [C.c_void_p, C.POINTER(C.c_double)]; f(sn._h, dsc.ctypes.data_as(C.POINTER(C.c_double)))
    out = {"shape": [nx, ne, nc], "cones": {"nonnegative": q, "second_order": dims}, "lu_fallback": int(lu), "n": nx + ne + nc, "batch": B, "threads": os.environ.get("SN_THREADS", "auto"),
           "kernel": {"threads_per_instance": int(dsc[0]), "lds_bytes_per_instance": int(dsc[1]), "instances_per_compute_unit": int(dsc[2]), "compute_units": int(dsc[3])}}
    ms_all = []
    for rep in range(3):
        sn.initialize(x0)
        res, ms = sn.solve()
        ms_all.append(ms)
    stt = sn.get_state()
    its = stt["counters"]["total_iterations"]; steps = stt["counters"]["newton_steps"]
    ms = min(ms_all)
    out["solve"] = {"launch_ms": ms, "launch_ms_all": ms_all, "converged": int((res == 1).sum()), "solves_per_s": B / (ms * 1e-3), "newton_steps_total": int(steps.sum()),
                    "newton_steps_per_s": float(steps.sum()) / (ms * 1e-3), "mean_iterations": float(its.mean()), "max_iterations": int(its.max()),
                    "mean_factorizations": float(stt["counters"]["factorizations"].mean()), "max_refinement_rounds": int(stt["counters"]["max_refinement_rounds"].max()),
                    "status_counts": {str(int(v)): int((res == v).sum()) for v in np.unique(res)}, "fallbacks_per_solve": float(stt["counters"]["refinement_failures"].mean())}
    if vjp:          # reverse mode at the solutions: one random cotangent on x per instance, the gradients of all QP data
        v = rng.standard_normal((B, nx))
        vms = [sn.vjp(v, adjoint=False, qp=True)["ms"] for _ in range(3)]
        out["vjp"] = {"k": 1, "cotangent": "x", "grad": "qp", "launch_ms": min(vms), "launch_ms_all": vms, "vjps_per_s": B / (min(vms) * 1e-3)}
    if general:      # the general path on the first `general` problems, one handle at a time (its fallback: fallback.hip)
        tg, itg = [], []
        for k in range(min(general, nprob)):
            p = probs[k]
            s = pkg.Solver(p, p.nx, 0, p.ne, p.nc, nonnegative_indices=p.nonnegative_indices, second_order_indices=p.second_order_indices)
            s.qp_attach(p.P, p.q, p.A, p.b, p.G, p.h, p.c)
            pkg.initialize_b(s, p.x0)
            t0 = time.perf_counter(); pkg.solve_b(s); tg.append(time.perf_counter() - t0); itg.append(int(s.stats()["total_iterations"]))
            del s
        out["general_path"] = {"solves": len(tg), "solve_ms_median": 1e3 * float(np.median(tg)), "solves_per_s": 1.0 / float(np.median(tg)), "iterations": itg}
    # non-advancing steps from an interior state (the benchmark step of the headline, for the batch)
    w = stt["solution"].copy()
    if nc:
        w[:, nx + ne:nx + ne + nc] += 0.5; w[:, -nc:] += 0.5
    w[:, :nx] += 0.05 * rng.standard_normal((B, nx))
    sn.set_state(w=w, scalars=np.tile([0.17, 0.99, 52.0], (B, 1)))
    sn.steps(2, advance=False)
    t = [sn.steps(K, advance=False) for _ in range(3)]
    msk = min(x[2] for x in t)
    info, stat = t[0][0], t[0][1]
    out["steps"] = {"count_per_instance": K, "launch_ms": msk, "newton_steps_per_s": B * K / (msk * 1e-3), "ok": int((stat == 0).sum()), "stepped": int((info[:, 6] == 0).sum()),
                    "refinement_rounds_mean": float(info[:, 2].mean()), "us_per_step_of_a_resident_instance": msk * 1e3 / K / max(1.0, B / max(1.0, dsc[2] * dsc[3]))}
    # bytes an instance moves once per launch (problem data + state): the HBM side of the roofline is irrelevant here — say so with the number
    bytes_inst = 8.0 * (nx * nx + (ne + nc) * nx + nx + (ne + nc) + 2 * (nx + 2 * ne + 3 * nc))
    out["steps"]["hbm_fraction"] = B * bytes_inst / (msk * 1e-3) / 8e12
    # the oracle on the same problems (one host core)
    try:
        import oracle
        from test_oracle_solve import run as run_oracle
        ts = []
        for k in range(min(8, nprob)):
            t0 = time.perf_counter(); o, status = run_oracle(oracle, probs[k]); ts.append(time.perf_counter() - t0)
        out["cpu_baseline"] = {"kind": "port", "cores": 1, "solve_ms_median": 1e3 * float(np.median(ts)), "solves_per_s": 1.0 / float(np.median(ts)),
                               "sample": "%d solve!s by the oracle (evaluation through Python callbacks)" % len(ts)}
        out["solve"]["gpu_over_cpu"] = out["solve"]["solves_per_s"] / out["cpu_baseline"]["solves_per_s"]
    except Exception as e:
        out["cpu_baseline"] = {"error": repr(e)}
    sn.close()
    print(json.dumps(out))

if __name__ == "__main__":
    main()
