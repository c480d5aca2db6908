"""GPU: the cache of the Schur complement's equality products (csrc/lfac.hip: LfacAux) moves no bit.  A dense handle with an attached QP stepped alone keeps
every tile's accumulator after the equality stages in a buffer E (a CAPTURE run of the full plan stores it), and later factorisations with the same gx, penalty and
regularisation start from E and run the cone stages only (a HIT, the cached plan); the retries of an inertia correction go without (a BYPASS).  Two handles of one problem
in one process, one with opt.schur_cache = 0 — the code path of every handle before the cache existed — are driven through the same sequence and compared with
np.array_equal after every step."""
import numpy as np
import pytest

import problems as pr
from helpers import load_pkg

pytestmark = pytest.mark.gpu

# (nx, ne, n_nonneg, n_soc, dim) of synthetic_conic_qp: the smallest shapes that reach each corner (tests/test_lfac_cached_plan_cpu.py plans the same ones on the CPU)
SHAPES = [(1000, 40, 0, 0, 3),          # nc = 0: the accumulators are kept after stage nst - 2 (the last stage stays: it carries the epilogue); a partial stage
          (1024, 64, 32, 0, 3),         # ne a multiple of 32, one cone stage
          (1100, 33, 5, 4, 3),          # padded size 1536 != nx, a stage of one row
          (1300, 700, 100, 50, 4)]      # tiles split over several workgroups in the head


def make(pkg, prob, pt, lam, cache):
    s = pkg.Solver(prob, prob.nx, 0, prob.ne, prob.nc, nonnegative_indices=prob.nonnegative_indices, second_order_indices=prob.second_order_indices)
    if not cache:
        s.set_option("schur_cache", 0)
    s.set("solution", np.concatenate([pt[k] for k in "xrsyzt"]))
    if prob.ne:
        s.set("dual", lam)
    for name, v in (("central_path", 0.17), ("penalty", 52.0), ("fraction_to_boundary", 0.99)):
        s.set(name, [v])
    attach(pkg, s, prob, prob.A, prob.b)
    return s


def attach(pkg, s, prob, A, b):
    s.qp_attach(prob.P, prob.q, A, b, prob.G, prob.h, 0.5)
    fl = pkg.FLAGS
    s.qp_evaluate(fl["objective"] | fl["equality_constraint"] | fl["cone_constraint"], 0)
    s.cone(product=True, target=True)
    s.synchronize()


def counts(s):
    i = s.schur_cache_info()
    return np.array([i["captures"], i["hits"], i["bypasses"]])


def step_both(handles, advance=False):
    """one Newton step on every handle, each compared with the last one (the handle without the cache); returns the step record and what the step added to the first
    handle's [captures, hits, bypasses]"""
    before = counts(handles[0])
    infos = [s.newton_step(advance=advance) for s in handles]
    delta = counts(handles[0]) - before
    assert infos[0]["status"] >= 0, infos[0]
    ref = handles[-1]
    want = [ref.data("step").all, ref.data("residual").all, ref.candidate.all, ref.solution.all]
    want_inertia = ref.factorize()              # the same matrix once more (with the regularisation the step ended on): its inertia triple
    for s, info in zip(handles[:-1], infos[:-1]):
        assert info == infos[-1], (info, infos[-1])
        for name, got, w in zip(("step", "residual", "candidate", "solution"), [s.data("step").all, s.data("residual").all, s.candidate.all, s.solution.all], want):
            assert np.array_equal(got, w), name
        assert s.factorize() == want_inertia
    return infos[0], delta


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "_".join(str(v) for v in s))
def test_steps_with_the_cache_are_the_steps_without_it(shape):
    pkg = load_pkg()
    nx, ne, n_nn, n_soc, dim = shape
    prob, pt, lam = pr.synthetic_conic_qp(pkg.splitmix_uniform, 61, nx, ne, n_nn, n_soc, dim)
    other, _, _ = pr.synthetic_conic_qp(pkg.splitmix_uniform, 62, nx, ne, n_nn, n_soc, dim)          # another A (and its b)
    a, b = make(pkg, prob, pt, lam, True), make(pkg, prob, pt, lam, False)
    assert a.scalar("opt.schur_cache") == 1.0 and b.scalar("opt.schur_cache") == 0.0

    # 1. two steps that do not advance: the first stores the products, the second starts from them
    _, d = step_both([a, b]); assert d.tolist() == [1, 0, 0], d
    assert int(a.kernel_times()[6]) == 1 and int(b.kernel_times()[6]) == 1                            # both took the left-looking schedule
    _, d = step_both([a, b]); assert d.tolist() == [0, 1, 0], d
    # 2. another penalty: omega_y changes, the products are stored again
    for s in (a, b):
        s.set("penalty", [7.5])
    _, d = step_both([a, b]); assert d.tolist() == [1, 0, 0], d
    _, d = step_both([a, b]); assert d.tolist() == [0, 1, 0], d
    # 3. a Hessian with negative curvature: IC-1 (a hit: gx, the penalty and the initial regularisation are what they were) fails its inertia test, the retries have
    # another regularisation and go without the cache, which is kept for the IC-1 of the next step
    for s in (a, b):
        s.set("lagrangian_hessian", prob.P - 6.0 * np.eye(nx))
    info, d = step_both([a, b])
    assert info["factorizations"] >= 2, info
    assert d.tolist() == [0, 1, info["factorizations"] - 1], (d, info)
    info, d = step_both([a, b])
    assert d[0] == 0 and d[1] == 1, d
    # 4. another A: nothing of the old one is used again — the step is that of a handle that never saw the old A
    fresh = make(pkg, prob, pt, lam, True)
    fresh.set("penalty", [7.5])
    for s in (a, b, fresh):
        attach(pkg, s, prob, other.A, other.b)
    for name in ("primal_regularization", "primal_regularization_last", "dual_regularization"):       # (what the retries of 3. left in the scalars)
        fresh.set(name, [a.scalar(name)])
    _, d = step_both([a, fresh, b]); assert d.tolist() == [1, 0, 0], d
    fresh.close()
    # 5. three steps that advance.  A full step ends the inner problem of a QP (the next step would find its residual converged and compute nothing), so the second
    # follows a smaller central-path parameter and the third a larger penalty as well, as after solve!'s outer updates: the penalty is part of the key
    for k, (kappa, rho) in enumerate(((0.17, 7.5), (0.017, 7.5), (0.0017, 75.0))):
        for s in (a, b):
            s.set("central_path", [kappa]); s.set("penalty", [rho])
        info, d = step_both([a, b], advance=True)
        nf, new_key = info["factorizations"], int(k == 2)
        assert nf >= 1 or k > 0, info
        assert d.tolist() == ([new_key, 1 - new_key, nf - 1] if nf else [0, 0, 0]), (k, d, info)
    ia, ib = a.schur_cache_info(), b.schur_cache_info()
    assert ia["captures"] >= 3 and ia["hits"] >= 5 and ia["bypasses"] >= 1, ia
    assert ia["bytes"] == 8 * a.padded_nx() ** 2
    assert ib == dict(captures=0, hits=0, bypasses=0, bytes=0), ib
    a.close(); b.close()


def test_handles_that_cannot_use_the_cache_report_it_off():
    """no equality rows, a host-callback handle (no attached QP: its gx may change with every evaluation) and a member stepped by its group (k_schur forms its products)"""
    pkg = load_pkg()
    off = dict(captures=0, hits=0, bypasses=0, bytes=0)
    # ne = 0
    prob, pt, lam = pr.synthetic_conic_qp(pkg.splitmix_uniform, 63, 1024, 0, 64, 0, 3)
    a, b = make(pkg, prob, pt, lam, True), make(pkg, prob, pt, lam, False)
    for _ in range(2):
        step_both([a, b])
    assert int(a.kernel_times()[6]) == 1 and a.schur_cache_info() == off
    a.close(); b.close()
    # host callbacks: the factorisation of the evaluated data, beside an attached handle without the cache at the same point
    prob, pt, lam = pr.synthetic_conic_qp(pkg.splitmix_uniform, 64, 1000, 40, 0, 0, 3)
    b = make(pkg, prob, pt, lam, False)
    h = pkg.Solver(prob, prob.nx, 0, prob.ne, prob.nc, nonnegative_indices=prob.nonnegative_indices, second_order_indices=prob.second_order_indices)
    h.set("solution", np.concatenate([pt[k] for k in "xrsyzt"]))
    h.set("dual", lam)
    for name, v in (("central_path", 0.17), ("penalty", 52.0), ("fraction_to_boundary", 0.99)):
        h.set(name, [v])
    h.evaluate(pr.ALL_VARIABLE_FLAGS, 0)
    h.cone(product=True, target=True)
    for _ in range(2):
        got = h.factorize()
        assert got == b.factorize() and got[0][2] == 0, got
    assert int(h.kernel_times()[6]) == 1 and h.schur_cache_info() == off
    h.close()
    # a group of two: its members' steps are the step of the handle alone, and nothing is cached for them
    members = [make(pkg, prob, pt, lam, True) for _ in range(2)]
    g = pkg.Group(members)
    want = b.newton_step(advance=False)
    got = g.newton_step(advance=False)
    for m, info in zip(members, got):
        assert info == want
        assert np.array_equal(m.data("step").all, b.data("step").all)
        assert m.schur_cache_info() == off
    g.close()
    for s in members + [b]:
        s.close()
