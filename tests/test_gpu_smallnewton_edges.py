"""GPU (-m gpu): the one-launch batch kernel (csrc/smallnewton.hip, include/calipso_smallnewton_device.hpp) at the EDGES of the shapes it admits — 1 <= nx <= 128,
second-order cones of dimension 2 .. 16, any footprint up to the 160 KB of LDS of a compute unit — held to the CPU ORACLE:
  1. solve at nx = 1, 7, 8, 63, 64, 65, 127, 128 and every remainder of nx modulo the LDL^T's panel width (SN_JB = 8), m > nx, one and two chunks of 64 rows in the
     triangular solves, all three automatic workgroup sizes;
  2. the last shape the library admits before its "LDS" refusal, found by asking the library (equalities at nx = 128; cones of dimension 16 at nx = 96: step,
     sensitivities and whole solves with the in-kernel fallback);
  3. cones of dimension 2 and 16: one Newton step, whole solves, forward and reverse sensitivities;
  4. differentiate / vjp / grad_qp up to nx = 128 (two chunks of rows in the sensitivity kernels), k = 17 cotangents;
  5. 5000 instances with their own problem data (more than are resident at once): every instance indexed by its own number;
  6. problems without constraints, where the kernel departs from the reference on purpose (include/calipso_hip.h: quirk B-13).
Every comparison is against the oracle to the tolerances the other modules hold for the same quantities (1e-8 iterates, solutions, sensitivities; 1e-10 / 1e-9 the adjoint
against the forward mode of the same handle, which has itself just been held to the oracle).  Every instance of every case is compared, and each case asserts how many."""
import ctypes

import numpy as np
import pytest

import problems as pr
from helpers import interior_point, load_pkg
from test_gpu_smallnewton_adjoint import TIGHT, contract, qp_batch, qp_theta_columns
from test_gpu_smallnewton_fallback import batch, compare_with_oracle, rel, soc_qp, solved
from test_oracle_solve import run as run_oracle

pytestmark = pytest.mark.gpu

THREADS = [0, 64, 128, 256]
LDS = 160 * 1024
KAPPA, TAU, RHO = 0.17, 0.99, 52.0          # the scalars of the interior-point tests of test_gpu_smallnewton.py

# (nx, ne, nc), nonnegative cones only.  The last six are this module's own, one per remainder of nx modulo the panel width 8 that the listed shapes leave out
# or that never ran: 3, 5, 7 and 2, 4, 6 (with seeds 900..905 the oracle converges on all of them, status 1, in 8..14 iterations with no fallback — found on the
# CPU before any kernel ran them).  nx mod 8 over the list: 1, 7, 0, 5, 7, 0, 1, 7, 0, 0, 3, 5, 7, 2, 4, 6.
SIZE_EDGES = [(1, 1, 1), (7, 3, 2), (8, 0, 3), (5, 4, 12), (63, 20, 10), (64, 20, 10), (65, 21, 9), (127, 30, 14), (128, 30, 16), (128, 48, 0),
              (11, 4, 5), (13, 5, 6), (23, 8, 9), (18, 6, 7), (20, 7, 8), (22, 8, 9)]
SIZE_SEEDS = range(900, 906)


def describe(sn):
    """(threads per instance, LDS bytes per instance) of the launch the handle would make"""
    out = np.zeros(4)
    assert sn._L.calipso_hip_debug_smallnewton_describe(sn._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
    return int(out[0]), int(out[1])


def nonnegative_qps(shape, seeds):
    nx, ne, nc = shape
    return [pr.random_qp(nx, ne, nc, seed=s, nonnegative_indices=list(range(1, nc + 1))) for s in seeds]


def solve_and_compare(oracle_mod, probs, cones=None, rows=32, **opts):
    """whole solves of the batch against the oracle, EVERY instance (status, counters, every accepted iterate, solution; 1e-8): returns (the oracle's fallbacks, status)"""
    pkg = load_pkg()
    res, st, tr = solved(pkg, probs, cones, rows=rows, **opts)
    assert st["counters"]["accepted_iterates"].max() <= rows                # every accepted iterate is in the trace
    fb = compare_with_oracle(oracle_mod, probs, res, st, tr, rows_max=rows)
    assert len(fb) == len(probs)                                            # the number compared is the batch size
    return fb, res


# ---- 1. solve across the size edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("shape", SIZE_EDGES)
def test_solve_at_the_size_edges_matches_the_oracle(oracle_mod, shape, threads):
    """nx = 1 .. 8 (a single ragged panel of the LDL^T), 63 / 64 / 65 (the last row of the first chunk of 64, a second chunk of one row), 127 / 128 (the second chunk
    full; (128, 48, 0) leaves ONE instance per compute unit), m > nx.  The oracle converges on all of them (6..18 iterations, no fallback)."""
    probs = nonnegative_qps(shape, SIZE_SEEDS)
    fb, res = solve_and_compare(oracle_mod, probs, threads=threads)
    assert (res == 1).all() and max(fb) == 0


def test_the_automatic_workgroup_size_takes_all_three_values():
    """threads = 0 over the sweep above: 64, 128 and 256 threads per instance are each chosen (6, 3 or fewer instances per compute unit by the footprint the library
    reports), and (128, 48, 0) has room for exactly one instance"""
    pkg = load_pkg()
    seen = {}
    for shape in SIZE_EDGES:
        sn = pkg.SmallNewtonBatch(*shape, 2, options=dict(threads=0))
        nt, lds = describe(sn)
        sn.close()
        seen[shape] = (nt, lds)
    assert {nt for nt, _ in seen.values()} == {64, 128, 256}, seen
    assert seen[(1, 1, 1)][0] == 64 and seen[(64, 20, 10)][0] == 128 and seen[(128, 48, 0)][0] == 256
    assert LDS // seen[(128, 48, 0)][1] == 1                                # (before the kernel's static LDS, which only takes room away)


# ---- 2. the last admitted shape -------------------------------------------------------------------------------------------------------------------
def admits(pkg, nx, ne, nc, cones=None):
    """True when create (and set_cones) take the shape, False when they refuse it with the LDS message; anything else is an error"""
    try:
        sn = pkg.SmallNewtonBatch(nx, ne, nc, 2)
    except pkg.CalipsoHipError as e:
        assert "LDS" in str(e), e
        return False
    try:
        if cones is not None:
            sn.set_cones(*cones)
    except pkg.CalipsoHipError as e:
        assert "LDS" in str(e), e
        return False
    finally:
        sn.close()
    return True


def test_the_last_admitted_number_of_equalities_at_nx_128(oracle_mod):
    """nx = 128, nc = 0: ne upwards until the library refuses; the last admitted shape (ne = 63 with the committed layout(): 162 208 of 163 840 bytes) solves like the
    oracle at the automatic and the largest workgroup size"""
    pkg = load_pkg()
    ne = 48
    assert admits(pkg, 128, ne, 0)
    while ne < 400 and admits(pkg, 128, ne + 1, 0):
        ne += 1
    assert 48 <= ne < 400 and not admits(pkg, 128, ne + 1, 0)               # the refusal happened, past (128, 48, 0)
    probs = nonnegative_qps((128, ne, 0), range(900, 904))
    for threads in (0, 256):
        fb, res = solve_and_compare(oracle_mod, probs, threads=threads)
        assert (res == 1).all() and max(fb) == 0


def last_admitted_cone_layout(pkg):
    nx, ne, q = 96, 20, 4
    lay = lambda k: (nx, ne, q, (2,) + (16,) * k)
    fits = lambda k: admits(pkg, nx, ne, q + 2 + 16 * k, (q, lay(k)[3]))
    k = 1
    assert fits(k)
    while k < 40 and fits(k + 1):
        k += 1
    assert 1 <= k < 40 and not fits(k + 1)
    return lay(k)


# the cone layout that last_admitted_cone_layout finds with the committed layout() (160 944 of 163 840 bytes), and the seeds of soc_qp for which the ORACLE converges
# on it (status 1) in at most 100 iterations, with its iteration count and its fallbacks: the first six of 900..1059 that do (39 of those 160 seeds converge at all,
# in 72..195 iterations; the others end in the reference's cone-search error)
LAST_CONE_LAYOUT = (96, 20, 4, (2, 16, 16, 16, 16))
LAST_CONE_SEEDS = {902: (99, 33), 918: (90, 26), 919: (79, 40), 975: (92, 38), 986: (100, 29), 1006: (88, 34)}


@pytest.mark.parametrize("threads", THREADS)
def test_the_last_admitted_number_of_wide_cones_at_nx_96(oracle_mod, threads):
    """nx = 96, ne = 20, four nonnegative entries, one cone of dimension 2 and as many of dimension 16 as set_cones admits: one Newton step and the forward / reverse
    sensitivities at interior points, as section 3 (a) and (c)"""
    layout = last_admitted_cone_layout(load_pkg())
    assert layout[3].count(16) >= 1
    assert interior_step(oracle_mod, layout, threads) == 5
    assert interior_sensitivities(oracle_mod, layout, threads) == 5


@pytest.mark.parametrize("threads", [0, 256])
def test_whole_solves_at_the_last_admitted_number_of_wide_cones(oracle_mod, threads):
    """section 3 (b) at that layout: whole solves with lu_fallback = 1 — the in-kernel H \\ residual at N = 346 and the arrow-block storage at its admitted maximum, 26..40
    fallbacks each — every instance and every accepted iterate against the oracle.  The seeds belong to the layout: should layout() move the boundary, this fails
    until seeds are chosen (by the oracle alone) for the new one."""
    layout = last_admitted_cone_layout(load_pkg())
    assert layout == LAST_CONE_LAYOUT, (layout, "LAST_CONE_SEEDS were chosen for LAST_CONE_LAYOUT: search seeds for the new last admitted layout")
    assert len(LAST_CONE_SEEDS) >= 4
    probs = [soc_qp(layout, s) for s in LAST_CONE_SEEDS]
    fb, res = solve_and_compare(oracle_mod, probs, cones=(layout[2], layout[3]), rows=128, threads=threads, lu_fallback=1)
    assert (res == 1).all() and fb == [f for _, f in LAST_CONE_SEEDS.values()]


# ---- 3. cone dimensions 2 and 16 ------------------------------------------------------------------------------------------------------------------
CONE_LAYOUTS = [(11, 4, 0, (2,)), (15, 6, 1, (2, 2, 2, 2)), (13, 3, 0, (16,)), (40, 10, 3, (16,)), (21, 5, 3, (16, 16)), (96, 20, 4, (2, 16))]
# seeds of soc_qp for which the ORACLE converges (status 1) in at most 100 iterations, with its iteration count
CONE_SEEDS = {
    (11, 4, 0, (2,)): {900: 8, 901: 12, 902: 9, 903: 7, 904: 9, 905: 9},
    (15, 6, 1, (2, 2, 2, 2)): {900: 14, 901: 11, 902: 12, 903: 11, 904: 13, 905: 11},
    (13, 3, 0, (16,)): {900: 52, 901: 16, 903: 63, 904: 42, 907: 21, 909: 52},             # (902, 905, 906, 908: more than 100 iterations or not converged)
    (40, 10, 3, (16,)): {900: 25, 901: 25, 903: 23, 904: 32, 905: 13},                      # (902: 206 iterations)
    (21, 5, 3, (16, 16)): {900: 20, 902: 98, 908: 47, 916: 69, 919: 83, 932: 45},           # (the first six of 900..932 that meet the condition)
    (96, 20, 4, (2, 16)): {900: 50, 901: 48, 902: 29, 903: 65, 904: 75, 905: 60},
}


def interior_setup(layout, n=5):
    probs = [soc_qp(layout, 900 + k) for k in range(n)]
    pts = [interior_point(p, 40 + k) for k, p in enumerate(probs)]
    W = np.stack([np.concatenate([pt[f] for f in "xrsyzt"]) for pt, _ in pts])
    LAM = np.stack([lam for _, lam in pts])
    return probs, pts, W, LAM


def oracle_at(oracle_mod, prob, pt, lam):
    """the oracle at the interior point with the scalars of the batch: derivatives and cone Jacobians evaluated there"""
    o = oracle_mod.OracleSolver(prob.nx, prob.np, prob.ne, prob.nc, prob.nonnegative_indices, prob.second_order_indices)
    op = o.point()
    for f in "xrsyzt":
        op[f][:] = pt[f]
    if prob.ne:
        o.buf("dual")[:] = lam
    for name, v in (("central_path", KAPPA), ("penalty", RHO), ("primal_regularization", 1.0e-7), ("dual_regularization", 1.0e-7), ("fraction_to_boundary", TAU)):
        o.buf(name)[0] = v
    prob.evaluate(pr.ALL_VARIABLE_FLAGS, op["x"], op["y"], op["z"], prob.parameters, o.buf)
    o.cone(product=True, jacobian=True, target=True)
    return o


def batch_at(layout, probs, W, LAM, threads):
    sn = batch(load_pkg(), probs, cones=(layout[2], layout[3]), threads=threads)
    sn.keep_trace(1)
    sn.set_state(w=W, dual=LAM, scalars=np.tile([KAPPA, TAU, RHO], (len(probs), 1)))
    return sn


def interior_step(oracle_mod, layout, threads):
    """one non-advancing Newton step of five instances at interior points: the search direction against the oracle's search_direction! at the same point (1e-8).
    The kernel's direction is read off the iterate the step accepted (the trace's row: w - step_size * step, t with its own step size) — the state itself stays."""
    probs, pts, W, LAM = interior_setup(layout)
    sn = batch_at(layout, probs, W, LAM, threads)
    info, status, _ = sn.steps(1, advance=False)
    acc = sn.trace()[:, 0]
    after = sn.get_state()["solution"]
    sn.close()
    assert (status == 0).all() and (info[:, 6] == 0).all(), (status, info[:, 6])
    assert np.array_equal(after, W)
    ot = probs[0].nx + 2 * probs[0].ne + 2 * probs[0].nc
    compared = 0
    for k, prob in enumerate(probs):
        o = oracle_at(oracle_mod, prob, *pts[k])
        o.residual()
        assert o.search_direction() == 0                                    # (refinement converges at these points: no fallback in the reference either)
        so = o.buf("step")
        assert 0.0 < info[k, 0] <= 1.0 and 0.0 < info[k, 1] <= 1.0
        sg = (W[k] - acc[k]) / info[k, 0]
        sg[ot:] = (W[k, ot:] - acc[k, ot:]) / info[k, 1]
        assert rel(sg, so) <= 1e-8, (layout, k, rel(sg, so))
        assert int(info[k, 2]) == o.stats()["last_refinement_rounds"], (k, info[k, 2], o.stats()["last_refinement_rounds"])
        compared += 1
    return compared


def interior_sensitivities(oracle_mod, layout, threads):
    """differentiate at the same interior points, every column of theta = [dq; db; dh], against the oracle's factorisation there (1e-8); then vjp with k = 3 as the
    transpose of that forward mode (1e-10: the same unrefined map transposed, quirk B-3)"""
    probs, pts, W, LAM = interior_setup(layout)
    nx, ne, nc = probs[0].nx, probs[0].ne, probs[0].nc
    N, npar = nx + 2 * ne + 3 * nc, nx + ne + nc
    oy, oz = nx + ne + nc, nx + 2 * ne + nc
    J = np.zeros((N, npar))
    J[:nx, :nx] = np.eye(nx)
    J[oy:oy + ne, nx:nx + ne] = -np.eye(ne)
    J[oz:oz + nc, nx + ne:] = np.eye(nc)
    sn = batch_at(layout, probs, W, LAM, threads)
    _, status, _ = sn.steps(1, advance=False)                               # forms the cone Jacobians at these points (quirk B-12)
    assert (status == 0).all(), status
    S, st, _ = sn.differentiate(J)
    v = np.random.default_rng(7).standard_normal((len(probs), N, 3))
    out = sn.vjp(v, qp=False)
    sn.close()
    assert (st == 0).all() and (out["status"] == 0).all()
    g, ref = contract(np.repeat(J[None], len(probs), axis=0), out["adjoint"]), np.einsum("bnp,bnk->bpk", S, v)
    compared = 0
    for k, prob in enumerate(probs):
        o = oracle_at(oracle_mod, prob, *pts[k])
        o.residual_jacobian_variables(); o.residual_jacobian_variables_symmetric()
        for j in range(npar):
            o.buf("residual")[:] = J[:, j]
            o.search_direction_symmetric(0, fact=(j == 0))
            assert rel(S[k][:, j], -1.0 * o.buf("step")) <= 1e-8, (layout, k, j, rel(S[k][:, j], -1.0 * o.buf("step")))
        assert rel(g[k], ref[k]) <= 1e-10, (layout, k, rel(g[k], ref[k]))
        compared += 1
    return compared


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("layout", CONE_LAYOUTS)
def test_one_step_at_interior_points_with_cones_of_dimension_2_and_16(oracle_mod, layout, threads):
    """(a) the arrow blocks and their closed-form inverses (first-row quirk included) at the degenerate arrow (dimension 2) and at the width the block code was sized
    for (16), apart from the iteration's decisions"""
    assert interior_step(oracle_mod, layout, threads) == 5


@pytest.mark.parametrize("threads", [0, 256])
@pytest.mark.parametrize("layout", CONE_LAYOUTS)
def test_whole_solves_with_cones_of_dimension_2_and_16(oracle_mod, layout, threads):
    """(b) lu_fallback = 1, the seeds of CONE_SEEDS (the oracle converges within 100 iterations: longer runs part by rounding alone, as
    test_gpu_smallnewton_fallback.py documents), every instance and every accepted iterate.  The dimension-2 layouts never fall back and pass with lu_fallback = 0 too."""
    seeds = CONE_SEEDS[layout]
    assert len(seeds) >= 4
    probs = [soc_qp(layout, s) for s in seeds]
    fb, res = solve_and_compare(oracle_mod, probs, cones=(layout[2], layout[3]), rows=128, threads=threads, lu_fallback=1)
    assert (res == 1).all()
    if max(layout[3]) == 2:
        assert max(fb) == 0
        fb0, res0 = solve_and_compare(oracle_mod, probs, cones=(layout[2], layout[3]), rows=128, threads=threads, lu_fallback=0)
        assert (res0 == 1).all()


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("layout", CONE_LAYOUTS)
def test_sensitivities_at_interior_points_with_cones_of_dimension_2_and_16(oracle_mod, layout, threads):
    """(c)"""
    assert interior_sensitivities(oracle_mod, layout, threads) == 5


def test_cone_dimensions_1_and_17_are_refused_and_the_handle_lives_on(oracle_mod):
    pkg = load_pkg()
    layout = (11, 4, 0, (2,))
    probs = [soc_qp(layout, s) for s in (900, 901)]
    p0 = probs[0]
    sn = pkg.SmallNewtonBatch(p0.nx, p0.ne, p0.nc, len(probs))
    for dims in ([1, 1], [1], [17], [2, 17]):
        with pytest.raises(pkg.CalipsoHipError, match="dimension 2 .. 16"):
            sn.set_cones(0, dims)
    sn.set_cones(0, [2])
    stk = lambda name: np.stack([np.asarray(getattr(p, name), dtype=np.float64) for p in probs])
    sn.set_qp(stk("P"), stk("q"), stk("A"), stk("b"), stk("G"), stk("h"), objective_scale=p0.c, shared=False)
    sn.initialize(np.stack([p.x0 for p in probs]))
    sn.keep_trace(32)
    res, _ = sn.solve()
    st, tr = sn.get_state(), sn.trace()
    sn.close()
    assert len(compare_with_oracle(oracle_mod, probs, res, st, tr, rows_max=32)) == 2 and (res == 1).all()


# ---- 4. sensitivities above one chunk of rows -----------------------------------------------------------------------------------------------------
SENS_LAYOUTS = [(1, 1, 1, 0, 0), (7, 3, 2, 0, 0), (64, 20, 10, 0, 0), (65, 21, 9, 0, 0), (127, 30, 14, 0, 0), (128, 30, 16, 0, 0), (128, 48, 0, 0, 0)]


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("layout", SENS_LAYOUTS)
def test_forward_and_reverse_sensitivities_up_to_nx_128(oracle_mod, layout, threads):
    """at the ORACLE's solution (tolerances TIGHT; it converges on all 28 instances in 5..12 iterations, no fallback): differentiate, every column of theta = [dq; db;
    dh] (176 of them at (128, 48, 0)), against the oracle's solution_sensitivity, and vjp with k = 1 and k = 17 cotangents against solution_sensitivity' v; 1e-8"""
    pkg = load_pkg()
    sn, probs = qp_batch(pkg, layout, 4, 300, threads, **TIGHT)
    res, _ = sn.solve()
    nx, ne, nc, N = sn.nx, sn.ne, sn.nc, sn.N
    npar = nx + ne + nc
    oy, oz = nx + ne + nc, nx + 2 * ne + nc
    J = np.zeros((4, N, npar))
    J[:, :nx, :nx] = np.eye(nx)
    J[:, oy:oy + ne, nx:nx + ne] = -np.eye(ne)
    J[:, oz:oz + nc, nx + ne:] = np.eye(nc)
    own = sn.get_state()["solution"].copy()
    W, So = own.copy(), {}
    for k, prob in enumerate(probs):
        o, status = run_oracle(oracle_mod, prob, differentiate=1, **TIGHT)
        assert status == 1 and res[k] == 1 and o.stats()["lu_fallbacks"] == 0, (k, status, res[k])
        assert rel(own[k], o.point()["all"]) <= 1e-8, (k, rel(own[k], o.point()["all"]))
        assert np.abs(J[k] - o.mat("jacobian_parameters", o.N, prob.np)).max() == 0.0
        W[k] = o.point()["all"]
        So[k] = o.mat("solution_sensitivity", o.N, prob.np).copy()
    sn.set_state(w=W)
    vjps = {}
    for kc in (1, 17):                                                      # (k = 1 straight after set_state, before any differentiate: the adjoint entry's own set-up)
        v = np.random.default_rng(3 + kc).standard_normal((4, N, kc))
        out = sn.vjp(v, qp=False)
        assert (out["status"] == 0).all() and out["adjoint"].shape == (4, N, kc)
        vjps[kc] = (v, contract(J, out["adjoint"]))
        if kc == 1:
            S, st, _ = sn.differentiate(J)
            assert S.shape == (4, N, npar) and (st == 0).all()
    compared = 0
    for k in range(4):
        for j in range(npar):
            assert rel(S[k][:, j], So[k][:, j]) <= 1e-8, (layout, k, j, rel(S[k][:, j], So[k][:, j]))
        compared += 1
    for kc, (v, g) in vjps.items():
        for k in range(4):
            assert rel(g[k], So[k].T @ v[k]) <= 1e-8, (layout, k, kc, rel(g[k], So[k].T @ v[k]))
            compared += 1
    sn.close()
    assert compared == 12                                                   # four instances: forward, vjp k = 1, vjp k = 17


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("layout", [(7, 3, 2, 0, 0), (65, 21, 9, 0, 0)])
def test_qp_data_gradients_below_one_panel_and_above_one_chunk(layout, threads):
    """grad_qp against the forward mode (held to the oracle at these shapes by the test above) fed the closed-form dR/dtheta column of EVERY data entry — at nx = 65
    all 4190 of them, the 2145 symmetric pairs of P included — contracted with v; 1e-9, after solve, as test_qp_data_gradients_match_forward_mode_columns"""
    pkg = load_pkg()
    sn, probs = qp_batch(pkg, layout, 4, 300, threads, **TIGHT)
    res, _ = sn.solve()
    assert (res == 1).all()
    w = sn.get_state()["solution"]
    nx, ne, nc, N = sn.nx, sn.ne, sn.nc, sn.N
    Js, picks = zip(*[qp_theta_columns(nx, ne, nc, probs[0].c, w[b]) for b in range(4)])
    J = np.stack(Js)
    assert J.shape[2] == nx * (nx + 1) // 2 + nx + ne * nx + ne + nc * nx + nc
    S, st, _ = sn.differentiate(J)
    v = np.random.default_rng(5).standard_normal((4, N, 2))
    out = sn.vjp(v, adjoint=False)
    sn.close()
    fwd = np.einsum("bnp,bnk->bpk", S, v)
    compared = 0
    for b in range(4):
        assert st[b] == 0 and out["status"][b] == 0
        got = np.stack([sum(out[name][b][idx] for name, idx in pk) for pk in picks[b]])
        assert rel(got, fwd[b]) <= 1e-9, (layout, b, rel(got, fwd[b]))
        assert rel(out["P"][b], np.swapaxes(out["P"][b], 0, 1)) <= 1e-15
        compared += 1
    assert compared == 4


# ---- 5. more instances than fit at once -----------------------------------------------------------------------------------------------------------
def test_5000_instances_with_their_own_data_are_indexed_by_their_number(oracle_mod):
    """(24, 9, 11), per-instance QP data, 5000 instances (more than 256 compute units x 6 resident; no multiple of anything): instance b holds problem b mod 50.
    Instances 0..49 against the oracle; every later instance bitwise equal to instance b mod 50 — status, counters, solution, trace; then vjp (k = 1) with the same
    tiling of cotangents: adjoint and data gradients bitwise equal too.  A stride or a 32-bit offset into batch x N x k that is not the instance number shows here."""
    pkg = load_pkg()
    B, M, rows = 5000, 50, 32
    base = nonnegative_qps((24, 9, 11), range(1000, 1000 + M))
    probs = [base[b % M] for b in range(B)]
    sn = batch(pkg, probs, threads=0)
    assert describe(sn)[0] == 64
    sn.keep_trace(rows)
    res, _ = sn.solve()
    st, tr = sn.get_state(), sn.trace()
    assert st["counters"]["accepted_iterates"].max() <= rows
    head = dict(solution=st["solution"][:M], counters={n: c[:M] for n, c in st["counters"].items()})
    fb = compare_with_oracle(oracle_mod, base, res[:M], head, tr[:M], rows_max=rows)
    assert len(fb) == M and max(fb) == 0 and (res[:M] == 1).all()
    src = np.arange(B) % M
    assert np.array_equal(res, res[src])
    for n, c in st["counters"].items():
        assert np.array_equal(c, c[src]), n
    for name in ("solution", "dual", "scalars"):
        assert np.array_equal(st[name], st[name][src]), name
    assert np.array_equal(tr, tr[src])
    v0 = np.random.default_rng(11).standard_normal((M, sn.N))
    out = sn.vjp(v0[src])
    sn.close()
    assert (out["status"] == 0).all()
    for name in ("adjoint", "P", "q", "A", "b", "G", "h"):
        assert out[name].shape[0] == B and np.abs(out[name]).max() > 0.0 and np.array_equal(out[name], out[name][src]), name


# ---- 6. no constraints at all ---------------------------------------------------------------------------------------------------------------------
UNCONSTRAINED = [(15, 9), (1, 900), (128, 900)]                             # (nx, seed of random_qp(nx, 0, 0))


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("nx,seed", UNCONSTRAINED)
def test_unconstrained_kernel_reaches_the_minimiser_where_the_reference_crawls(oracle_mod, nx, seed, threads):
    """ne = nc = 0: the reference's constraint violation is norm(c) / length(c) = 0 / 0 = NaN (constraint_violation.jl:13), no comparison of its line search holds, every
    iteration takes all 25 halvings and moves by 2^-25 of the Newton step: solve! returns false after its 10 x 100 iterations, 5.8 from the minimiser at (15, 0, 0).
    The oracle restates that (tests/test_oracle_solve.py pins it).  The batch kernel takes the violation of an empty constraint set as 0 — a deliberate departure,
    quirk B-13 of include/calipso_hip.h — and so takes the full Newton step: status 1 and the closed-form minimiser -(2cP)^-1 q, to the solver's tolerances (1e-4)."""
    pkg = load_pkg()
    prob = pr.random_qp(nx, 0, 0, seed=seed, nonnegative_indices=[])
    o, status = run_oracle(oracle_mod, prob)
    assert status == 0 and o.stats()["total_iterations"] > 500              # the reference's behaviour, for the record
    res, st, tr = solved(pkg, [prob, prob], threads=threads)
    xs = np.linalg.solve(2.0 * prob.c * prob.P, -prob.q)
    # the first accepted iterate IS the full Newton step from x0 (step size 1), the direction being the oracle's search_direction! there
    empty = np.zeros(0)
    o1 = oracle_at(oracle_mod, prob, dict(x=prob.x0, r=empty, s=empty, y=empty, z=empty, t=empty), empty)
    o1.residual()
    assert o1.search_direction() == 0
    for k in range(2):
        # a quadratic objective: one full step per value of the central-path parameter at most, ten outer iterations
        assert res[k] == 1 and st["counters"]["total_iterations"][k] <= 20, (k, res[k], st["counters"]["total_iterations"][k])
        assert rel(st["solution"][k, :nx], xs) <= 1e-4, (nx, k, rel(st["solution"][k, :nx], xs))
        assert rel(tr[k, 0], prob.x0 - o1.buf("step")) <= 1e-8, (nx, k, rel(tr[k, 0], prob.x0 - o1.buf("step")))


def test_unconstrained_general_path_follows_the_reference(oracle_mod):
    """the same (15, 0, 0) problem through calipso_hip_solve: the general path keeps the reference's NaN violation, so it crawls exactly like the oracle — not converged,
    the same iteration count, and after 1001 steps of 2^-25 the same point to 1e-8"""
    pkg = load_pkg()
    prob = pr.random_qp(15, 0, 0, seed=9, nonnegative_indices=[])
    o, status = run_oracle(oracle_mod, prob)
    assert status == 0
    s = pkg.Solver(prob, prob.nx, 0, prob.ne, prob.nc, nonnegative_indices=prob.nonnegative_indices)
    s.qp_attach(prob.P, prob.q, prob.A, prob.b, prob.G, prob.h, prob.c)
    pkg.initialize_b(s, prob.x0)
    ok = pkg.solve_b(s)
    assert not ok
    assert s.stats()["total_iterations"] == o.stats()["total_iterations"], (s.stats()["total_iterations"], o.stats()["total_iterations"])
    assert rel(s.solution.all, o.point()["all"]) <= 1e-8, (15, rel(s.solution.all, o.point()["all"]))
    xs = np.linalg.solve(2.0 * prob.c * prob.P, -prob.q)
    assert np.abs(s.solution.all[:15] - xs).max() > 1.0                     # (nowhere near the minimiser)
