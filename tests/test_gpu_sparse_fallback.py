"""GPU (run with -m gpu on an MI355X): the `H \\ residual` fallback of the sparse handle — restarted right-preconditioned GMRES (csrc/sparse_krylov.hip, driven by
search_direction of csrc/sparse_kkt.hip; options krylov_fallback, krylov_restart, krylov_max_cycles) — against the CPU oracle, which factorises H by a pivoted LU
there (search_direction.jl:22, 106-119).  The checker is always the oracle, or numpy on the oracle's H_dense, never the handle; the inputs are those of
tests/sparse_fallback_cases.py, which tests/test_sparse_fallback_inputs_cpu.py pins with the oracle alone.  Tolerances: |R - H step|_inf <= 1e-10 (the fallback's own
stopping tolerance, iterative_refinement_tolerance), which at cond(H) <= 1e4 (pinned there) puts the step within 1e-9 relative of the LU step, the tolerance of
tests/test_gpu_fallback.py; accepted iterates 1e-8 relative and integers exact, as tests/test_gpu_sparse_solve.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")      # (one HIP runtime per process: torch first, then the library)

import sparse_fallback_cases as fc
import sparse_solve_cases as sc
from test_gpu_sparse_solve import cold_solve, criteria, handle, rel

pytestmark = pytest.mark.gpu

ON = dict(krylov_fallback=1)
MOST_ITERATIONS = 32                      # the CPU prototype needed at most 14 at these points; the factor two covers different rounding


@pytest.fixture(scope="module")
def references(oracle_mod):
    """per row, computed once and left unchanged: the problem, the oracle's whole solve, and what the oracle makes of the first fallback point — the residual R, its
    `H \\ residual` step, H itself"""
    cache = {}

    def get(case):
        if case not in cache:
            prob = sc.problem(oracle_mod.splitmix_uniform, *case)
            ref = sc.oracle_solve(oracle_mod, prob)
            o, w, lam, R = fc.fixed_point(oracle_mod, prob, ref, fc.CASES[case]["first_row"])
            assert o.search_direction() == 2
            point = dict(w=w, lam=lam, R=R, step=o.buf("step").copy(), H=o.H_dense())
            for a in list(ref.values()) + list(point.values()):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            cache[case] = (prob, ref, point)
        return cache[case]
    return get


def at_the_fixed_point(prob, point, **options):
    """a handle with the fallback on at the first fallback point, and the residual its own prologue forms there"""
    g = handle(prob, options=dict(ON, **options))
    g.set_values(w=point["w"], penalty=fc.RHO, central_path=fc.KAPPA)
    g.set("dual", point["lam"])
    g.step_prologue()
    R = g.get("residual")
    assert rel(R, point["R"]) <= 1e-12
    return g, R


def true_norm(point, step):
    return float(np.abs(point["R"] - point["H"] @ step).max())


# ---- 1. the fallback at a fixed point --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(fc.CASES), ids=fc.CASE_IDS)
def test_the_fallback_at_the_first_fallback_point(references, case):
    prob, ref, point = references(case)
    g, R = at_the_fixed_point(prob, point)
    step, reg, info, status = g.search_direction(R)
    fb = g.fallback_info()
    print("N %d: status %d, %r, %r; |R - H step|_inf %.3e (numpy, the oracle's H), |step - LU step| %.3e" %
          (g.N, status, info, fb, true_norm(point, step), rel(step, point["step"])))
    assert status == 2
    assert info["fallback_iterations"] >= 1 and info["fallback_iterations"] == fb["iterations"]
    assert fb["taken"] == 1 and fb["converged"] == 1 and 1 <= fb["iterations"] <= MOST_ITERATIONS and fb["cycles"] >= 1
    assert fb["launches"] >= 6 * fb["iterations"] and fb["device_ms"] > 0.0
    assert fb["workspace_bytes"] >= 8 * (2 * 16 + 1) * g.N
    assert true_norm(point, step) <= fc.TOLERANCE
    assert rel(step, point["step"]) <= fc.STEP_AGREEMENT
    assert info["residual_norm"] == fb["residual_norm"] <= fc.TOLERANCE
    # solve_nonsymmetric on the same residual, with the factorisation search_direction left: the same bits, on the host and on the device route
    host = g.solve_nonsymmetric(R)
    assert np.array_equal(host, step)
    again = g.fallback_info()
    assert (again["taken"], again["iterations"], again["cycles"], again["converged"], again["residual_norm"]) == \
           (1, fb["iterations"], fb["cycles"], 1, fb["residual_norm"])
    dev = g.solve_nonsymmetric(torch.tensor(R, dtype=torch.float64, device="cuda:0"))
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), step)


def test_solve_nonsymmetric_refusals(references):
    pkg = __import__("helpers").load_pkg()
    prob, ref, point = references(fc.ROW_2)
    g = handle(prob)

    def refused(call, *texts):
        with pytest.raises(pkg.CalipsoHipError) as e:
            call()
        assert "(-4)" in str(e.value) and all(t in str(e.value) for t in texts), str(e.value)

    refused(lambda: g.solve_nonsymmetric(point["R"]), "calipso_hip_sparse_kkt_solve_nonsymmetric: factorize first")
    for name, value in (("krylov_fallback", 2), ("krylov_fallback", 0.5), ("krylov_restart", 0), ("krylov_restart", 33), ("krylov_max_cycles", 0), ("krylov_max_cycles", 17)):
        refused(lambda: g.set_option(name, value), name + ": an integer in")
    g.set_values(w=point["w"], penalty=fc.RHO, central_path=fc.KAPPA)
    g.factorize(1e-5, 1e-5)
    refused(lambda: g.solve_nonsymmetric(torch.zeros(g.N, dtype=torch.float64)), "calipso_hip_sparse_kkt_solve_nonsymmetric_device: residual is not device memory")
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.solve_nonsymmetric(np.zeros(g.N + 1))
    assert "the residual has" in str(e.value)
    # ... and it runs whatever krylov_fallback says (here: off), on the factorisation at hand
    step = g.solve_nonsymmetric(point["R"])
    fb = g.fallback_info()
    print("option off, ep = ed = 1e-5: %r" % fb)
    assert fb["taken"] == 1 and fb["converged"] == 1 and np.isfinite(step).all()


# ---- 2. restarts and the caps ------------------------------------------------------------------------------------------------------------------------------------------
def test_short_restarts_still_get_there(references):
    """krylov_restart = 4 at the point where full GMRES needs 15 columns: at least three cycles, and still everything test 1 asks — converged within MOST_ITERATIONS = 32
    iterations, which at four columns a cycle are eight cycles, so krylov_max_cycles = 8 lets the fallback go exactly as far as that bound does.  (Measured on an
    MI355X: 24 iterations in 6 cycles, |R - H step|_inf 5.3e-11.  Under the default krylov_max_cycles = 4 the same call stops after 16 iterations at 1.7e-7 and
    reports itself unconverged: restarts of four cannot do in 16 columns what takes the full space 15.)"""
    prob, ref, point = references(fc.ROW_4)
    g, R = at_the_fixed_point(prob, point, krylov_restart=4, krylov_max_cycles=MOST_ITERATIONS // 4)
    step, reg, info, status = g.search_direction(R)
    fb = g.fallback_info()
    print("krylov_restart = 4: %r; |R - H step|_inf %.3e, |step - LU step| %.3e" % (fb, true_norm(point, step), rel(step, point["step"])))
    assert status == 2 and info["fallback_iterations"] >= 1
    assert fb["cycles"] >= 3 and fb["iterations"] <= 4 * fb["cycles"]
    assert fb["converged"] == 1 and fb["iterations"] <= MOST_ITERATIONS
    assert true_norm(point, step) <= fc.TOLERANCE and rel(step, point["step"]) <= fc.STEP_AGREEMENT
    assert np.array_equal(g.solve_nonsymmetric(R), step)
    assert np.array_equal(g.solve_nonsymmetric(torch.tensor(R, dtype=torch.float64, device="cuda:0")).cpu().numpy(), step)


def test_a_capped_fallback_reports_unconverged_with_a_finite_step(references):
    prob, ref, point = references(fc.ROW_4)
    g, R = at_the_fixed_point(prob, point, krylov_restart=2, krylov_max_cycles=1)
    step, reg, info, status = g.search_direction(R)
    fb = g.fallback_info()
    want = true_norm(point, step)
    print("krylov_restart = 2, krylov_max_cycles = 1: %r; |R - H step|_inf %.17g (numpy)" % (fb, want))
    assert status == 2 and fb["taken"] == 1 and fb["converged"] == 0 and fb["cycles"] == 1 and fb["iterations"] == 2 == info["fallback_iterations"]
    assert np.isfinite(step).all() and want > fc.TOLERANCE
    assert abs(fb["residual_norm"] - want) <= 1e-12 * want
    assert info["residual_norm"] == fb["residual_norm"]


# ---- 3. whole solves -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(fc.CASES), ids=fc.CASE_IDS)
def test_whole_solves_with_the_fallback(references, case):
    prob, ref, point = references(case)
    want = fc.CASES[case]
    g = handle(prob, options=ON)
    status, info = cold_solve(g, prob)
    fb = g.fallback_info()
    print("status %d, %r, %r" % (status, info, fb))
    assert status == ref["status"] == 1
    assert (info["total_iterations"], info["outer_iterations"], info["accepted_iterates"]) == (ref["total_iterations"], ref["outer"], ref["accepted"])
    assert info["refinement_failures"] == fb["solve_fallbacks"] == ref["lu_fallbacks"] == want["fallbacks"]
    assert info["worst_warning"] >= 2 and fb["solve_unconverged"] == 0 and fb["solve_fallbacks"] <= fb["solve_iterations"] <= MOST_ITERATIONS * fb["solve_fallbacks"]
    tr = g.trace()
    assert tr.shape == ref["trace"].shape
    for r in range(tr.shape[0]):
        assert rel(tr[r], ref["trace"][r]) <= 1e-8, (r, rel(tr[r], ref["trace"][r]))
    assert rel(g.get("solution"), ref["w"]) <= 1e-8 and rel(g.get("dual"), ref["dual"]) <= 1e-8
    criteria(g, prob)


# ---- 4. same bits ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_solve_with_fallbacks_repeats_bit_for_bit_and_the_device_route_gives_the_host_routes_bits(references):
    import sparse_kkt_cases as kc
    from helpers import load_pkg
    prob, ref, point = references(fc.ROW_4)
    g = handle(prob, options=ON)
    status, info = cold_solve(g, prob)
    first, solution, fb = g.trace().copy(), g.get("solution"), g.fallback_info()
    assert status == 1 and fb["solve_fallbacks"] == fc.CASES[fc.ROW_4]["fallbacks"]
    status, again = cold_solve(g, prob)
    assert status == 1 and np.array_equal(g.trace(), first) and np.array_equal(g.get("solution"), solution)
    assert [again[k] for k in g.SOLVE_INFO[:12]] == [info[k] for k in g.SOLVE_INFO[:12]]
    fb2 = g.fallback_info()
    assert [fb2[k] for k in g.FALLBACK_INFO[:5] + g.FALLBACK_INFO[6:]] == [fb[k] for k in g.FALLBACK_INFO[:5] + g.FALLBACK_INFO[6:]]
    q, dims = kc.cone_layout(prob)
    Lxx, gx, hx = kc.sparse_inputs(prob)
    d = load_pkg().SparseKKT(Lxx, gx, hx, n_nonnegative=q, second_order_dims=dims, options=ON)
    dev = lambda a: torch.tensor(np.asarray(a, dtype=np.float64).reshape(-1), dtype=torch.float64, device="cuda:0")
    d.set_values(dev(Lxx.data), dev(gx.data), dev(hx.data))
    d.attach_qp(dev(prob.q), dev(prob.b), dev(prob.h))
    d.keep_trace(64)
    d.initialize(dev(np.zeros(prob.nx)))
    status, _ = d.solve()
    sol = d.solution_device()
    assert status == 1 and sol.is_cuda and np.array_equal(sol.cpu().numpy(), solution) and np.array_equal(d.trace(), first)


# ---- 5. the default ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_without_the_option_nothing_changes(references):
    prob, ref, point = references(fc.ROW_2)
    g = handle(prob)
    g.set_values(w=point["w"], penalty=fc.RHO, central_path=fc.KAPPA)
    g.set("dual", point["lam"])
    g.step_prologue()
    step, reg, info, status = g.search_direction(g.get("residual"))
    fb = g.fallback_info()
    assert status == 2 and info["fallback_iterations"] == 0 and np.isfinite(step).all()
    assert (fb["taken"], fb["iterations"], fb["cycles"], fb["converged"], fb["launches"], fb["workspace_bytes"]) == (0, 0, 0, 0, 0, 0)
    g = handle(prob)
    status, info = cold_solve(g, prob)
    fb = g.fallback_info()
    assert status == -102 and info["status"] == -102 and "no `H \\ residual` fallback" in g._error_text()
    assert info["accepted_iterates"] == fc.CASES[fc.ROW_2]["first_row"] and info["refinement_failures"] == 1
    assert (fb["taken"], fb["solve_fallbacks"], fb["solve_iterations"]) == (0, 0, 0)
    # ... and the option can be turned on and off on a living handle
    g.set_option("krylov_fallback", 1)
    status, info = cold_solve(g, prob)
    assert status == 1 and g.fallback_info()["solve_fallbacks"] == fc.CASES[fc.ROW_2]["fallbacks"]
    g.set_option("krylov_fallback", 0)
    status, info = cold_solve(g, prob)
    assert status == -102 and g.fallback_info()["solve_fallbacks"] == 0
