#!/usr/bin/env python3
"""differentiate! on the sparse handle with the evaluator's own dR/dtheta (SparseKKT.vjp(theta=True), differentiate(columns=...)) beside what the handle offered before
— the numpy twin on the host, a dense J for the same columns, differentiate(J) — in ONE process:
python bench/sparse_trajectory_differentiate.py [--cases cartpole_mpc_11,cartpole_mpc_101,cartpole_mpc_1001,cone_11,cone_101,cone_1001] [--reps 20] [--warmups 3] [--out FILE]

The problems are the two parametrised ones of tests/device_eval_trajectory/problems.py at other horizons (the text of a library does not depend on the horizon, nothing
is compiled here): the cart-pole MPC problem (14 / 10 / 8 parameters per stage) and the cone problem (2 per stage).  The pendulum of the other benches has no parameters.
Per case, after one solve! from initialize! (krylov_fallback = 1), medians over the repeats after the warm-ups: device (HIP events) and wall ms of vjp(theta=True) for
k = 1 and 16, of differentiate(columns = 16 parameters), the gradient kernel alone; the twin's wall ms for the five parameter bits, the wall of building the dense J of
the same 16 columns from it, and of differentiate(J); the bytes a full dense J (N x np doubles) would take.  Prints one JSON line and writes it to --out (default
profiles/sparse_trajectory_differentiate.json)."""
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
PARAMETER_BITS = 0x1f << 11


def cartpole_mpc(tp, T):
    """the cart-pole MPC problem of tests/device_eval_trajectory/problems.py at another horizon: the same stage functions, so the same library"""
    a = tp.functions("cartpole_mpc")
    stage, final, dyn, first = a["objective"][0], a["objective"][-1], a["dynamics"][0], a["equality"][0]
    return dict(objective=[stage] * (T - 1) + [final], dynamics=[dyn] * (T - 1), num_states=[4] * T, num_actions=[1] * (T - 1), equality=[first] + [None] * (T - 1),
                num_parameters=[14] + [10] * (T - 2) + [8])


def cartpole_parameters(T):
    """per stage: the reference state (upright at the origin) and action, unit weights; the initial state hanging down"""
    stage = [0.0, np.pi, 0.0, 0.0, 0.0] + [1.0] * 5
    return np.array(stage + [0.0, 0.0, 0.0, 0.0] + stage * (T - 2) + [0.0, np.pi, 0.0, 0.0] + [1.0] * 4)


def median_ms(call, reps, warmups):
    walls = []
    for _ in range(warmups + reps):
        t0 = time.perf_counter()
        call()
        walls.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(walls[warmups:]))


def main():
    a = sys.argv[1:]

    def opt(name, default):
        if name not in a:
            return default
        i = a.index(name); v = a[i + 1]; del a[i:i + 2]
        return v
    cases = opt("--cases", "cartpole_mpc_11,cartpole_mpc_101,cartpole_mpc_1001,cone_11,cone_101,cone_1001").split(",")
    reps, warmups = int(opt("--reps", 20)), int(opt("--warmups", 3))
    out_path = opt("--out", os.path.join(ROOT, "profiles", "sparse_trajectory_differentiate.json"))
    load_package()
    spec = importlib.util.spec_from_file_location("trajectory_problems", os.path.join(FIXTURES, "problems.py"))
    tp = importlib.util.module_from_spec(spec); spec.loader.exec_module(tp)
    codegen = tp.load_codegen()
    out = {"reps": reps, "warmups": warmups, "cases": {}}
    for name in cases:
        T = int(name.rsplit("_", 1)[1])
        if name.startswith("cartpole_mpc_"):
            TP, theta = codegen.TrajectoryProblem(name="trajectory_cartpole_mpc", **cartpole_mpc(tp, T)), cartpole_parameters(T)
        else:
            TP, theta = codegen.TrajectoryProblem(name=tp.library_name("cone_%d" % T), **tp.functions("cone_%d" % T)), tp.parameters("cone_%d" % T)
        s = TP.sparse_solver(parameters=theta, directory=FIXTURES, options=dict(krylov_fallback=1))
        s.initialize(np.zeros(TP.nx))
        status, info = s.solve()
        rng = np.random.default_rng(1)
        columns = np.sort(rng.choice(TP.np, size=16, replace=False))
        patterns = TP.sparse_parameter_patterns()
        case = {"stages": T, "shape": [TP.nx, TP.ne, TP.nc], "np": TP.np, "N": s.N, "status": status, "total_iterations": info["total_iterations"],
                "parameter_nnz": [int(len(r)) for _, r in patterns], "dense_J_bytes": 8 * s.N * TP.np}
        for k in (1, 16):
            V = rng.standard_normal((s.N, k))
            device, kernel = [], []

            def call():
                s.vjp(V, adjoint=False, theta=True)
                t = s.vjp_times(); device.append(t["device"]); kernel.append(t["gradients"])
            case["vjp_theta_k%d" % k] = {"wall_ms": median_ms(call, reps, warmups), "device_ms": float(np.median(device[warmups:])),
                                         "gradient_kernel_ms": float(np.median(kernel[warmups:]))}
        maps = []

        def forward():
            s.differentiate(columns=columns)
            maps.append(s.timing()["columns_map"])
        case["differentiate_16_columns"] = {"wall_ms": median_ms(forward, reps, warmups), "map_device_ms": float(np.median(maps[warmups:]))}
        # what the handle offered before: the twin on the host, a dense J for the same 16 columns, differentiate(J)
        w = s.get("solution")
        nx, ne, nc = TP.nx, TP.ne, TP.nc
        x, y, z = w[:nx], w[nx + ne + nc:nx + 2 * ne + nc], w[nx + 2 * ne + nc:nx + 2 * ne + 2 * nc]
        twin_bytes = 8 * (3 * nx + ne + nc) * TP.np
        if twin_bytes <= 1 << 30:                      # (the twin writes dense nx x np, ne x np and nc x np arrays)
            held = {}

            def twin():
                held.clear()
                rows = lambda nm: ne if nm == "equality_jacobian_parameters" else nc if nm == "cone_jacobian_parameters" else nx
                TP.evaluate(PARAMETER_BITS, x, y, z, theta, lambda nm: held.setdefault(nm, np.zeros(rows(nm) * TP.np)))

            def dense():
                J = np.zeros((s.N, 16))
                L = sum(v for nm, v in held.items() if nm.endswith("variables_parameters")).reshape(nx, TP.np, order="F")
                J[:nx] = L[:, columns]
                if ne:
                    J[nx + ne + nc:nx + 2 * ne + nc] = held["equality_jacobian_parameters"].reshape(ne, TP.np, order="F")[:, columns]
                if nc and "cone_jacobian_parameters" in held:
                    J[nx + 2 * ne + nc:nx + 2 * ne + 2 * nc] = held["cone_jacobian_parameters"].reshape(nc, TP.np, order="F")[:, columns]
                held["J"] = J
            few = max(3, reps // 4)
            case["host_twin"] = {"twin_wall_ms": median_ms(twin, few, 1), "dense_J_16_columns_wall_ms": median_ms(dense, few, 1), "twin_dense_bytes": twin_bytes}
            J = held["J"]
            case["host_twin"]["differentiate_J_wall_ms"] = median_ms(lambda: s.differentiate(J), reps, warmups)
            case["host_twin"]["sensitivity_difference"] = float(np.abs(s.differentiate(J) - s.differentiate(columns=columns)).max())
        else:
            case["host_twin"] = {"not_run": "the twin's dense theta-Jacobians would take %d bytes" % twin_bytes}
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
