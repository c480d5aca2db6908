"""GPU (run with -m gpu on an MI355X): solve! on sparse problem data resident on the device — SparseKKT.attach_qp / initialize / solve and the building blocks of a
Newton step's vector half (csrc/sparse_solve.hip) — against the CPU oracle.  The checker is the oracle, never the code under test; the inputs are those of
tests/sparse_solve_cases.py, which tests/test_sparse_solve_inputs_cpu.py pins with the oracle alone.  Tolerances are the project's own for the same quantities:
vectors and products 1e-12 relative (test_gpu_sparse_kkt.py), accepted iterates 1e-8 relative, central_path 1e-15, penalty 1e-9 (test_gpu_smallnewton.py), integers exact."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")      # (one HIP runtime per process: torch first, then the library)

import helpers
import problems as pr
import sparse_kkt_cases as kc
import sparse_solve_cases as sc
from helpers import load_pkg

pytestmark = pytest.mark.gpu

MULTIFRONTAL, COLUMNS = "nested_dissection", "minimum_degree"
TRACE_ROWS = 64


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()) if np.asarray(b).size else 0.0


def close(a, b, tol):
    return abs(a - b) <= tol * max(1.0, abs(b))


def handle(prob, method=MULTIFRONTAL, **kw):
    """SparseKKT of the problem's sparse inputs with the values and q, b, h resident"""
    q, dims = kc.cone_layout(prob)
    Lxx, gx, hx = kc.sparse_inputs(prob)
    g = load_pkg().SparseKKT(Lxx, gx, hx, n_nonnegative=q, second_order_dims=dims, method=method, **kw)
    g.set_values(Lxx, gx, hx)
    g.attach_qp(prob.q, prob.b, prob.h)
    return g


def cold_solve(g, prob):
    g.keep_trace(TRACE_ROWS)
    g.initialize(np.zeros(prob.nx))
    return g.solve()


@pytest.fixture(scope="module")
def references(oracle_mod):
    """the oracle's whole solves, computed once and left unchanged"""
    cache = {}

    def get(shape, pid):
        if (shape, pid) not in cache:
            prob = sc.problem(oracle_mod.splitmix_uniform, shape, pid)
            ref = sc.oracle_solve(oracle_mod, prob)
            for a in ref.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            cache[(shape, pid)] = (prob, ref)
        return cache[(shape, pid)]
    return get


# ---- 1. building blocks at a fixed point -------------------------------------------------------------------------------------------------------------------------
def oracle_candidate(o, prob, w, a_s, a_t):
    """what solve.jl:206-250 makes of the oracle's step at the point w: (candidate, merit, constraint violation, merit_gradient . step.primals); the oracle's
    objective, constraints and barrier are left at the candidate"""
    n, ne, nc = prob.nx + prob.ne + prob.nc, prob.ne, prob.nc
    step = o.buf("step").copy()
    dd = float(np.dot(o.buf("merit_gradient"), step[:n]))
    cand = o.point("candidate")
    pt, sp_ = o.point(), dict(zip("xrsyzt", np.split(step, np.cumsum([prob.nx, ne, nc, ne, nc]))))
    for k in "xrs":
        cand[k][:] = pt[k] - a_s * sp_[k]
    cand["t"][:] = pt["t"] - a_t * sp_["t"]
    prob.evaluate(pr.OBJECTIVE | pr.EQUALITY | pr.CONE, cand["x"], pt["y"], pt["z"], np.zeros(0), o.buf)
    o.cone(which=1, barrier=True, barrier_gradient=True)
    Mh = o.merit(float(o.buf("objective")[0]), cand["r"], float(o.buf("barrier")[0]))
    thetah = o.constraint_violation(o.buf("equality_constraint"), cand["r"], o.buf("cone_constraint"), cand["s"])
    return cand, Mh, thetah, dd


@pytest.mark.parametrize("shape", sc.BLOCK_SHAPES, ids=["_".join(str(v) for v in s) for s in sc.BLOCK_SHAPES])
def test_building_blocks_at_a_fixed_point(oracle_mod, shape):
    prob, pt, lam = pr.staged_conic_qp(oracle_mod.splitmix_uniform, 0, *shape)
    w = np.concatenate([pt[k] for k in "xrsyzt"])
    o = helpers.oracle_newton_state(oracle_mod, prob, w, lam, kappa=kc.KAPPA, rho=kc.RHO)
    o.merit_gradient()
    op = o.point()
    f, barrier = float(o.buf("objective")[0]), float(o.buf("barrier")[0])
    M = o.merit(f, op["r"], barrier)
    theta = o.constraint_violation(o.buf("equality_constraint"), op["r"], o.buf("cone_constraint"), op["s"])
    R = o.buf("residual").copy()
    oy, oz = prob.nx + prob.ne + prob.nc, prob.nx + 2 * prob.ne + prob.nc
    inf = lambda v: float(np.abs(v).max()) if v.size else 0.0
    want = dict(objective=f, barrier=barrier, merit=M, constraint_violation=theta, residual_violation=float(np.abs(R).sum() / o.N), optimality_error=o.optimality_error(),
                slack_violation=max(inf(R[oy:oy + prob.ne]), inf(R[oz:oz + prob.nc])))
    g = handle(prob)
    g.set_values(w=w, penalty=kc.RHO, central_path=kc.KAPPA)
    g.set("dual", lam)
    got = g.step_prologue()
    for name in ("residual", "merit_gradient", "barrier_gradient", "cone_product", "cone_target", "equality_constraint", "cone_constraint", "objective_gradient_variables"):
        got_vector = g.get(name)
        ref_vector = o.buf(name)[:got_vector.size]                            # (the oracle's barrier_gradient buffer is longer than the cone part it fills)
        assert rel(got_vector, ref_vector) <= 1e-12, (name, rel(got_vector, ref_vector))
    for name, ref in want.items():
        print("%s: %r (oracle %r)" % (name, got[name], ref))
        assert close(got[name], ref, 1e-12), (name, got[name], ref)
    # the cone search on the oracle's step: the halvings of solve.jl:190-221, exactly
    o.search_direction()
    step = o.buf("step").copy()
    g.set("step", step)
    halvings = helpers.cone_search_halvings(o, w)
    a_s, a_t = g.cone_search()
    assert (a_s, a_t) == (halvings[0][0], halvings[1][0]), ((a_s, a_t), halvings)
    # the candidate at those step sizes, and accept
    y, z = op["y"].copy(), op["z"].copy()
    cand, Mh, thetah, dd = oracle_candidate(o, prob, w, a_s, a_t)
    gM, gtheta, gdd = g.candidate(a_s, a_t)
    print("candidate: merit %r (oracle %r), violation %r (%r), dd %r (%r)" % (gM, Mh, gtheta, thetah, gdd, dd))
    assert close(gM, Mh, 1e-12) and close(gtheta, thetah, 1e-12) and close(gdd, dd, 1e-12)
    nx, ne, nc = prob.nx, prob.ne, prob.nc
    new = np.concatenate([cand["x"], cand["r"], cand["s"], y - a_s * step[oy:oy + ne], z - a_s * step[oz:oz + nc], cand["t"]])
    assert rel(g.get("candidate")[:nx + ne + nc], new[:nx + ne + nc]) <= 1e-12 and rel(g.get("candidate")[oz + nc:], cand["t"]) <= 1e-12
    eq_violation = inf(o.buf("equality_constraint")[:ne])
    op["s"][:] = cand["s"]; op["t"][:] = cand["t"]
    o.cone(product=True)
    got_violations = g.accept(a_s)
    assert close(got_violations[0], eq_violation, 1e-12) and close(got_violations[1], inf(o.buf("cone_product")[:nc]), 1e-12)
    assert rel(g.get("solution"), new) <= 1e-12 and rel(g.get("cone_product"), o.buf("cone_product")[:nc]) <= 1e-12
    # the outer update of the dual (solve.jl:362-364), with the penalty given as an option this time
    g.set_option("penalty", 3.5)
    g.outer_update()
    assert rel(g.get("dual"), lam + 3.5 * cand["r"]) <= 1e-12


@pytest.mark.parametrize("shape", [s for s in sc.BLOCK_SHAPES if s[4] > 0], ids=["_".join(str(v) for v in s) for s in sc.BLOCK_SHAPES if s[4] > 0])
def test_cone_search_at_the_boundary(oracle_mod, shape):
    prob, pt, lam = pr.staged_conic_qp(oracle_mod.splitmix_uniform, 0, *shape)
    helpers.push_cones_to_the_boundary(prob, pt, np.random.default_rng(0))
    w = np.concatenate([pt[k] for k in "xrsyzt"])
    o = helpers.oracle_newton_state(oracle_mod, prob, w, lam, kappa=kc.KAPPA, rho=kc.RHO)
    o.search_direction()
    halvings = helpers.cone_search_halvings(o, w)
    assert max(k for _, k in halvings) <= helpers.CONE_SEARCH_LIMIT
    g = handle(prob, options=dict(max_cone_line_search=helpers.CONE_SEARCH_LIMIT))
    g.set_values(w=w, penalty=kc.RHO, central_path=kc.KAPPA)
    g.set("step", o.buf("step").copy())
    print("halvings", halvings)
    assert g.cone_search() == (halvings[0][0], halvings[1][0])


# ---- 2. whole solves ---------------------------------------------------------------------------------------------------------------------------------------------
def criteria(g, prob, tol=1e-4):
    """the four checks of every reference solver test (test/solver/test1.jl:21-30), as test_gpu_solve.criteria, on what a prologue at the final point leaves"""
    g.step_prologue()
    res = g.get("residual")
    oy, oz = prob.nx + prob.ne + prob.nc, prob.nx + 2 * prob.ne + prob.nc
    assert np.abs(res).sum() / g.N < tol
    assert max(np.abs(res[oy:oy + prob.ne]).max() if prob.ne else 0.0, np.abs(res[oz:oz + prob.nc]).max() if prob.nc else 0.0) < tol
    if prob.ne:
        assert np.abs(g.get("equality_constraint")).max() <= tol
    if prob.nc:
        assert np.abs(g.get("cone_product")).max() <= tol


def check_whole_solve(g, prob, ref, want):
    status, info = cold_solve(g, prob)
    print("status %d, %r" % (status, info))
    assert status == ref["status"] == 1
    assert (info["total_iterations"], info["outer_iterations"], info["accepted_iterates"]) == (ref["total_iterations"], ref["outer"], ref["accepted"])
    tr = g.trace()
    assert tr.shape == ref["trace"].shape
    for r in range(tr.shape[0]):
        assert rel(tr[r], ref["trace"][r]) <= 1e-8, (r, rel(tr[r], ref["trace"][r]))
    assert rel(g.get("solution"), ref["w"]) <= 1e-8 and rel(g.get("dual"), ref["dual"]) <= 1e-8
    assert abs(info["central_path"] - ref["kappa"]) <= 1e-15 and abs(info["penalty"] - ref["rho"]) <= 1e-9
    assert 1 <= info["factorizations"] <= ref["factorizations"]                 # (the oracle also counts the reference's hidden re-factorisations)
    if want["max_rounds"] <= sc.ROUNDS_PINNED_UP_TO:
        assert info["max_refinement_rounds"] == ref["max_refinement_rounds"] == want["max_rounds"]
    assert info["refinement_failures"] == 0
    assert info["host_waits"] <= 3 * info["accepted_iterates"] + info["line_search_trials"] + 2
    criteria(g, prob)


@pytest.mark.parametrize("case", list(sc.SOLVES), ids=sc.SOLVE_IDS)
def test_whole_solves(references, case):
    prob, ref = references(*case)
    check_whole_solve(handle(prob), prob, ref, sc.SOLVES[case])


def test_whole_solve_with_the_column_factorisation(references):
    case = ((3, 4, 2, 1, 1, 3), 1)
    prob, ref = references(*case)
    g = handle(prob, COLUMNS)
    assert g.info["numeric"].startswith("columns")
    check_whole_solve(g, prob, ref, sc.SOLVES[case])


# ---- 3. refinement failure -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(sc.FAILURES), ids=["%s-%d" % ("_".join(str(v) for v in s), p) for s, p in sc.FAILURES])
def test_refinement_failure(references, case):
    prob, ref = references(*case)
    k = ref["first_lu_fallback_row"]
    assert k == sc.FAILURES[case]["first_row"] and ref["lu_fallbacks"] == sc.FAILURES[case]["fallbacks"]
    g = handle(prob)
    status, info = cold_solve(g, prob)
    print("default: status %d, %r" % (status, info))
    assert status == -102 and info["status"] == -102 and "no `H \\ residual` fallback" in g._error_text()
    assert info["accepted_iterates"] == k and info["refinement_failures"] == 1 and info["worst_warning"] == 2
    tr = g.trace()
    assert tr.shape[0] == k
    for r in range(k):
        assert rel(tr[r], ref["trace"][r]) <= 1e-8, (r, rel(tr[r], ref["trace"][r]))
    assert rel(g.get("solution"), ref["trace"][k - 1]) <= 1e-8                    # the point is the last accepted iterate
    if case[0] == (3, 4, 2, 1, 1, 3):
        # the same handle then solves another problem of the pattern
        other, oref = references((3, 4, 2, 1, 1, 3), 1)
        g.set_values(*kc.sparse_inputs(other))
        g.attach_qp(other.q, other.b, other.h)
        status, info = cold_solve(g, other)
        assert status == 1 and rel(g.get("solution"), oref["w"]) <= 1e-8 and info["total_iterations"] == oref["total_iterations"]
    # ... and goes on past the failure when told to
    c = handle(prob, options=dict(continue_after_refinement_failure=1))
    status, info = cold_solve(c, prob)
    point = c.get("solution")
    print("continue_after_refinement_failure: status %d, %r, |solution - oracle| %.3e" % (status, info, rel(point, ref["w"])))
    tr = c.trace()
    assert status in (0, 1) and np.isfinite(point).all() and info["refinement_failures"] >= 1
    assert tr.shape[0] >= k
    for r in range(k):
        assert rel(tr[r], ref["trace"][r]) <= 1e-8


# ---- 4. same bits --------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_solve_repeats_bit_for_bit_and_the_device_route_gives_the_host_routes_bits(references):
    prob, ref = references((3, 4, 2, 1, 1, 3), 1)
    g = handle(prob)
    status, info = cold_solve(g, prob)
    first, point = g.trace().copy(), g.get("solution")
    assert status == 1 and first.shape[0] == ref["accepted"]
    status, again = cold_solve(g, prob)
    assert status == 1 and np.array_equal(g.trace(), first) and np.array_equal(g.get("solution"), point)
    assert [again[k] for k in g.SOLVE_INFO[:12]] == [info[k] for k in g.SOLVE_INFO[:12]]
    # CUDA tensors into set_values / attach_qp / initialize, the solution read on the device
    q, dims = kc.cone_layout(prob)
    Lxx, gx, hx = kc.sparse_inputs(prob)
    d = load_pkg().SparseKKT(Lxx, gx, hx, n_nonnegative=q, second_order_dims=dims)
    dev = lambda a: torch.tensor(np.asarray(a, dtype=np.float64).reshape(-1), dtype=torch.float64, device="cuda:0")
    d.set_values(dev(Lxx.data), dev(gx.data), dev(hx.data))
    d.attach_qp(dev(prob.q), dev(prob.b), dev(prob.h))
    d.keep_trace(TRACE_ROWS)
    d.initialize(dev(np.zeros(prob.nx)))
    status, _ = d.solve()
    sol = d.solution_device()
    assert status == 1 and sol.is_cuda and np.array_equal(sol.cpu().numpy(), point) and np.array_equal(d.trace(), first)


# ---- 5. warm start -------------------------------------------------------------------------------------------------------------------------------------------------
def test_warm_start(oracle_mod, references):
    prob, ref = references(*sc.WARM_START)
    warm = sc.oracle_solve(oracle_mod, prob, start=ref["w"])
    g = handle(prob, options=dict(warmstart=1))
    g.set("solution", ref["w"])
    g.keep_trace(TRACE_ROWS)
    status, info = g.solve()
    print("warm start: status %d, %r (oracle: %d iterations, %d outer)" % (status, info, warm["total_iterations"], warm["outer"]))
    assert status == warm["status"] == 1
    assert (info["total_iterations"], info["outer_iterations"], info["accepted_iterates"]) == (warm["total_iterations"], warm["outer"], warm["accepted"])
    assert rel(g.get("solution"), warm["w"]) <= 1e-8


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(references):
    pkg = load_pkg()
    prob, ref = references((2, 3, 1, 1, 0, 3), 0)
    q, dims = kc.cone_layout(prob)
    Lxx, gx, hx = kc.sparse_inputs(prob)
    g = pkg.SparseKKT(Lxx, gx, hx, n_nonnegative=q, second_order_dims=dims)

    def refused(call, *texts):
        with pytest.raises(pkg.CalipsoHipError) as e:
            call()
        assert "(-4)" in str(e.value) and all(t in str(e.value) for t in texts), str(e.value)

    refused(g.solve, "calipso_hip_sparse_kkt_solve: no Lxx resident")
    g.set_values(Lxx, gx, hx)
    refused(g.solve, "calipso_hip_sparse_kkt_solve: no q resident (calipso_hip_sparse_kkt_qp_attach first)")
    refused(lambda: g.initialize(np.zeros(prob.nx)), "calipso_hip_sparse_kkt_initialize: no q resident")
    g.attach_qp(prob.q, prob.b, prob.h)
    refused(g.solve, "calipso_hip_sparse_kkt_solve: no point resident")
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.attach_qp(q=np.zeros(prob.nx + 1))
    assert "q has %d entries, not %d" % (prob.nx + 1, prob.nx) in str(e.value)
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.initialize(np.zeros(prob.nx - 1))
    assert "x0 has" in str(e.value)
    refused(lambda: g.set("dual", np.zeros(prob.ne + 2)), "calipso_hip_sparse_kkt_set: len: dual has %d entries, not %d" % (prob.ne, prob.ne + 2))
    refused(lambda: g.set("residual", np.zeros(g.N)), "only solution, dual and step can be set")
    refused(lambda: g.get("no_such_vector"), "calipso_hip_sparse_kkt_get: name: no resident vector called no_such_vector")
    refused(lambda: g.attach_qp(q=torch.zeros(prob.nx, dtype=torch.float64)), "calipso_hip_sparse_kkt_qp_attach_device: q is not device memory")
    refused(lambda: g.initialize(torch.zeros(prob.nx, dtype=torch.float64)), "calipso_hip_sparse_kkt_initialize_device: x0 is not device memory")
    refused(lambda: g.keep_trace(0), "calipso_hip_sparse_kkt_keep_trace: rows")
    refused(lambda: g.set_option("no_such_option", 1.0), "unknown option")
    # ... and the handle works afterwards
    status, info = cold_solve(g, prob)
    assert status == 1 and info["total_iterations"] == ref["total_iterations"] and rel(g.get("solution"), ref["w"]) <= 1e-8
