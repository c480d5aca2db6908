"""GPU (run with -m gpu on an MI355X): calipso.jl_amd.SparseKKTGroup — search_direction! for groups of same-pattern sparse problems in lockstep
(csrc/sparse_kkt_group.hip) — against the CPU oracle and against single SparseKKT handles on the same data.  The checker is the oracle or the single handle, never
the group itself.  Members are those of tests/sparse_kkt_group_cases.py, whose walks tests/test_sparse_kkt_group_host_cpu.py pins with the oracle alone.  Tolerances
are those of tests/test_gpu_sparse_kkt.py for the same quantities: matrices and products 1e-12 relative, steps 1e-8 relative, integers and the regularisation walk
exact; a member against its single handle: every output bit for bit."""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")      # (one HIP runtime per process: torch first, then the library)

import helpers
import sparse_kkt_cases as kc
import sparse_kkt_group_cases as gc
from helpers import load_pkg

pytestmark = pytest.mark.gpu

ERR_INERTIA = -1
ZERO = (0.0, 0.0, 0.0)


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()) if np.asarray(b).size else 0.0


@pytest.fixture(scope="module")
def members(oracle_mod):
    """per (shape, pid, kind), computed once and left unchanged: the problem, its sparse inputs, the point, the residual and what the oracle's search_direction! makes
    of it; and per (member, options) what a fresh single SparseKKT returns on the same data"""
    cache, singles = {}, {}

    def get(shape, pid, kind):
        key = (shape, pid, kind)
        if key not in cache:
            prob, w, lam = gc.member(oracle_mod.splitmix_uniform, shape, pid, kind)
            o, ref = kc.oracle_search_direction(oracle_mod, prob, w, lam)
            m = dict(prob=prob, w=w, inputs=kc.sparse_inputs(prob), R=o.buf("residual").copy(), step=o.buf("step").copy(), H=o.H_dense().copy(), ref=ref)
            for a in (m["w"], m["R"], m["step"], m["H"]):
                a.setflags(write=False)
            cache[key] = m
        return cache[key]

    def single(shape, pid, kind, **options):
        key = (shape, pid, kind, tuple(sorted(options.items())))
        if key not in singles:
            m = get(shape, pid, kind)
            q, dims = kc.cone_layout(m["prob"])
            s = load_pkg().SparseKKT(*m["inputs"], n_nonnegative=q, second_order_dims=dims, options=options)
            s.set_values(*m["inputs"], m["w"], kc.RHO, central_path=kc.KAPPA)
            try:
                out = s.search_direction(m["R"], ZERO)
            except load_pkg().CalipsoHipError as e:                        # inertia correction failure: the regularisation is where the walk stopped
                assert "(-1)" in str(e)
                out = (None, s.regularization, None, ERR_INERTIA)
            singles[key] = out
        return singles[key]
    get.single = single
    return get


def group_of(ms, **kw):
    """a SparseKKTGroup holding the members ms (one pattern), values set"""
    first = ms[0]
    for m in ms:
        for A, B in zip(m["inputs"], first["inputs"]):
            assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)      # one pattern: what makes them a group
    q, dims = kc.cone_layout(first["prob"])
    g = load_pkg().SparseKKTGroup(*first["inputs"], members=len(ms), n_nonnegative=q, second_order_dims=dims, **kw)
    g.set_values([m["inputs"][0] for m in ms], [m["inputs"][1] for m in ms], [m["inputs"][2] for m in ms], [m["w"] for m in ms], kc.RHO, central_path=kc.KAPPA)
    return g


def residuals(ms):
    return np.stack([m["R"] for m in ms])


def mixed(members):
    return [members(kc.SMALL, pid, kind) for (pid, kind), _ in gc.MIXED]


def assert_member_is_its_single_handle(out, k, want):
    steps, regs, infos, statuses, _ = out
    step, reg, info, status = want
    assert statuses[k] == status and regs[k] == reg
    if status != ERR_INERTIA:
        assert np.array_equal(steps[k], step)
        assert infos[k] == dict((name, info[name]) for name in ("factorizations", "refinement_rounds", "residual_norm"))


def test_mixed_walks_against_the_oracle(members):
    ms = mixed(members)
    g = group_of(ms)
    assert g.info["members"] == 6 and g.info["N"] == 56 and g.info["numeric"] == "multifrontal"
    steps, regs, infos, statuses, report = g.search_direction(residuals(ms), ZERO)
    for k, (m, (key, (nfact, rounds, status))) in enumerate(zip(ms, gc.MIXED)):
        ref = m["ref"]
        print("%s: factorisations %d (oracle %d), refinement rounds %d (oracle %d), ep %r, status %d, |R - H step| %.3e" %
              (key, infos[k]["factorizations"], ref["factorizations"], infos[k]["refinement_rounds"], ref["rounds"], regs[k][0], statuses[k], infos[k]["residual_norm"]))
        assert statuses[k] == ref["status"] == status
        assert regs[k] == (ref["ep"], ref["ep_last"], ref["ed"])                               # bit for bit
        assert infos[k]["factorizations"] == ref["factorizations"] == nfact
        assert infos[k]["refinement_rounds"] == ref["rounds"] == rounds
        if status == 0:
            assert rel(steps[k], m["step"]) <= 1e-8
            assert np.abs(m["R"] - m["H"] @ steps[k]).max() <= 1e-9 * max(1.0, np.abs(m["R"]).max())
    assert g.status == 2
    assert report["factorization_rounds"] == gc.MIXED_FACTOR_ROUNDS and report["refinement_rounds"] == gc.MIXED_REFINE_ROUNDS      # the maxima over the members
    assert report["last_factorization_active"] == 3 and report["last_refinement_active"] == 1
    # the cost of the call is that of its slowest member: a group of ONE holding it alone waits and launches as often
    alone = group_of([members(kc.SMALL, *gc.SLOWEST)])
    one = alone.search_direction(residuals([members(kc.SMALL, *gc.SLOWEST)]), ZERO)[4]
    print("group of six: %s\ngroup of one: %s" % (report, one))
    assert (report["host_waits"], report["launches"]) == (one["host_waits"], one["launches"])
    assert (one["factorization_rounds"], one["refinement_rounds"]) == (gc.MIXED_FACTOR_ROUNDS, gc.MIXED_REFINE_ROUNDS)


@pytest.mark.parametrize("which", ["mixed", "one", "tree"])
def test_a_member_is_its_single_handle_bit_for_bit(members, which):
    """a member's arithmetic depends neither on the number of members nor on its slot"""
    if which == "tree":
        keys = [(kc.TREE, pid, kind) for (pid, kind), _ in gc.TREE_GROUP]
    else:
        keys = [(kc.SMALL, pid, kind) for (pid, kind), _ in gc.MIXED] if which == "mixed" else [(kc.SMALL,) + gc.SLOWEST]
    ms = [members(*key) for key in keys]
    g = group_of(ms)
    out = g.search_direction(residuals(ms), ZERO)
    for k, key in enumerate(keys):
        assert_member_is_its_single_handle(out, k, members.single(*key))
    if which == "tree":
        assert g.info["N"] == 954 and g.info["levels"] > 1
        assert [(i["factorizations"], i["refinement_rounds"]) for i in out[2]] == [want for _, want in gc.TREE_GROUP]


def test_order_and_repetition(members):
    ms = mixed(members)
    g = group_of(ms)
    first = g.search_direction(residuals(ms), ZERO)
    again = g.search_direction(residuals(ms), ZERO)                       # a second call on the same group: the same bits
    assert np.array_equal(first[0], again[0]) and first[1:4] == again[1:4]
    perm = [4, 2, 5, 0, 3, 1]
    p = group_of([ms[k] for k in perm])
    permuted = p.search_direction(residuals([ms[k] for k in perm]), ZERO)
    for at, k in enumerate(perm):                                          # permuting the members permutes every output bitwise
        assert np.array_equal(permuted[0][at], first[0][k])
        assert (permuted[1][at], permuted[2][at], permuted[3][at]) == (first[1][k], first[2][k], first[3][k])
    assert [permuted[4][n] for n in ("factorization_rounds", "refinement_rounds", "host_waits", "launches")] == [first[4][n] for n in ("factorization_rounds", "refinement_rounds", "host_waits", "launches")]
    # the device route (CUDA tensors) returns the host route's bits
    dev = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), dtype=torch.float64, device="cuda:0")
    q, dims = kc.cone_layout(ms[0]["prob"])
    d = load_pkg().SparseKKTGroup(*ms[0]["inputs"], members=len(ms), n_nonnegative=q, second_order_dims=dims)
    d.set_values(dev(np.stack([m["inputs"][0].data for m in ms])), dev(np.stack([m["inputs"][1].data for m in ms])), dev(np.stack([m["inputs"][2].data for m in ms])),
                 dev(np.stack([m["w"] for m in ms])), dev(np.full(len(ms), kc.RHO)), central_path=kc.KAPPA)
    steps, regs, infos, statuses, _ = d.search_direction(dev(residuals(ms)), ZERO)
    assert steps.is_cuda and np.array_equal(steps.cpu().numpy(), first[0])
    assert (regs, infos, statuses) == first[1:4]


BLOCK_GROUPS = ["staged_3_4_2_1_1_3", "staged_5_7_3_0_1_5", "qp_noeq_7_0_4", "qp_nocone_9_4_0", "qp_soc64_70_5_66"]


@pytest.mark.parametrize("name", BLOCK_GROUPS)
def test_building_blocks_at_fixed_regularisations(oracle_mod, name):
    """the same problem at interior_point seeds 1, 2 and 3, every member at its OWN (ep, ed) in one factorize call: as check_blocks of tests/test_gpu_sparse_kkt.py
    asserts per handle"""
    prob, _, _ = kc.block_case(oracle_mod.splitmix_uniform, name)
    tail = kc.DENSE_CASES[name][1] if name in kc.DENSE_CASES else 0.3
    seeds = [1, 2, 3] if prob.nx < 50 else [1, 2]
    eps, eds = [kc.EP, 0.5 * kc.EP, 2.0 * kc.EP][:len(seeds)], [kc.ED, 3.0 * kc.ED, 0.25 * kc.ED][:len(seeds)]
    refs = []
    for seed, ep, ed in zip(seeds, eps, eds):
        pt, lam = helpers.interior_point(prob, seed=seed, tail=tail)
        o = helpers.make_oracle(oracle_mod, prob, pt, lam, kappa=kc.KAPPA, rho=kc.RHO, ep=ep, ed=ed)
        o.cone(product=True, jacobian=True, target=True)
        o.residual()
        o.residual_jacobian_variables(); o.residual_jacobian_variables_symmetric()
        v = np.random.default_rng(9 + seed).standard_normal(o.N)
        o.factorize(update=False)
        inertia = o.compute_inertia()
        o.search_direction_symmetric(0, fact=False)
        refs.append(dict(prob=prob, inputs=kc.sparse_inputs(prob), w=np.concatenate([pt[k] for k in "xrsyzt"]), K=np.triu(o.K_dense()).copy(), v=v, Hv=o.H_mul(v).copy(),
                         inertia=inertia, R=o.buf("residual").copy(), step=o.buf("step").copy()))
    g = group_of(refs)
    assert g.info["max_cone_dimension"] == max(kc.cone_layout(prob)[1] + [0])
    warn = g.factorize(eps, eds)
    Hv, steps = g.mul(np.stack([r["v"] for r in refs])), g.solve_symmetric(np.stack([r["R"] for r in refs]))
    for k, r in enumerate(refs):
        K = g.matrix(k)
        assert K.shape == r["K"].shape and sp.triu(K).nnz == K.nnz
        assert rel(K.toarray(), r["K"]) <= 1e-12                            # every member's K carries its own (ep, ed)
        assert rel(Hv[k], r["Hv"]) <= 1e-12
        assert g.inertia[k] == r["inertia"] == (g.nx, g.ne + g.nc, 0)
        assert rel(steps[k], r["step"]) <= 1e-8
    assert warn == 0
    assert not np.allclose(g.matrix(0).toarray(), g.matrix(1).toarray())


def test_a_failing_member_leaves_and_the_others_go_on(members):
    ms = mixed(members)
    g = group_of(ms, options=dict(max_regularization=gc.FAILING_MAX_REGULARIZATION))
    given = np.full((len(ms), g.N), 7.0)
    out = g.search_direction(residuals(ms), ZERO)
    steps, regs, infos, statuses, report = out
    assert statuses == gc.FAILING_STATUSES and g.status == ERR_INERTIA
    plain = group_of(ms).search_direction(residuals(ms), ZERO)
    for k, ((pid, kind), _) in enumerate(gc.MIXED):
        want = members.single(kc.SMALL, pid, kind, max_regularization=gc.FAILING_MAX_REGULARIZATION)
        assert_member_is_its_single_handle(out, k, want)
        if statuses[k] == 0:                                               # the passing members' outputs are bitwise those without the limit
            assert np.array_equal(steps[k], plain[0][k]) and (regs[k], infos[k]) == (plain[1][k], plain[2][k])
        else:                                                              # the regularisation a single handle reports after its error; the step untouched
            assert want[3] == ERR_INERTIA and regs[k] == want[1] and regs[k][0] > gc.FAILING_MAX_REGULARIZATION
            assert infos[k]["refinement_rounds"] == 0 and np.array_equal(steps[k], np.zeros(g.N))
    # the walk 1e-20 -> 1e-18 -> .. reaches ep = 100 at the 13th factorisation: the indefinite member passes there, the three boundary members would go on to 1e4 > 1e3
    # and fail there — the last round holds those four
    assert report["factorization_rounds"] == 13 and report["last_factorization_active"] == 4
    # ... untouched on the device route too: the caller's own step stays in place
    dev = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), dtype=torch.float64, device="cuda:0")
    L = load_pkg()._lib.lib()
    import ctypes as C
    step, R = dev(given), dev(residuals(ms))
    reg, info, status, rep = np.zeros(3 * len(ms)), np.zeros(4 * len(ms)), np.zeros(len(ms), dtype=np.int32), np.zeros(8)
    torch.cuda.synchronize()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = L.calipso_hip_sparse_kkt_group_search_direction_device(g._h, C.c_void_p(R.data_ptr()), C.c_void_p(step.data_ptr()), pd(reg), pd(info),
                                                                status.ctypes.data_as(C.POINTER(C.c_int32)), pd(rep))
    assert rc == ERR_INERTIA and list(status) == gc.FAILING_STATUSES
    got = step.cpu().numpy()
    for k, s in enumerate(gc.FAILING_STATUSES):
        assert np.array_equal(got[k], steps[k] if s == 0 else given[k])


def test_the_limit_of_128_members(oracle_mod):
    pkg = load_pkg()
    base = []
    for pid in range(4):
        prob, w, lam = gc.member(oracle_mod.splitmix_uniform, gc.LIMIT_SHAPE, pid, "interior")
        o = helpers.oracle_newton_state(oracle_mod, prob, w, lam, kappa=kc.KAPPA, rho=kc.RHO)
        m = dict(prob=prob, w=w, inputs=kc.sparse_inputs(prob), R=o.buf("residual").copy())
        q, dims = kc.cone_layout(prob)
        s = pkg.SparseKKT(*m["inputs"], n_nonnegative=q, second_order_dims=dims)
        s.set_values(*m["inputs"], w, kc.RHO, central_path=kc.KAPPA)
        m["single"] = s.search_direction(m["R"], ZERO)
        base.append(m)
    ms = [base[k % 4] for k in range(128)]
    g = group_of(ms)
    out = g.search_direction(residuals(ms), ZERO)
    for k in range(128):                                                   # every member is bitwise equal to its single handle
        assert_member_is_its_single_handle(out, k, ms[k]["single"])
    q, dims = kc.cone_layout(base[0]["prob"])
    for count in (129, 0):
        with pytest.raises(pkg.CalipsoHipError) as e:
            pkg.SparseKKTGroup(*base[0]["inputs"], members=count, n_nonnegative=q, second_order_dims=dims)
        assert "(-4)" in str(e.value) and "members: a group holds 1 .. 128 members, not %d" % count in str(e.value)


def test_refusals(members):
    pkg = load_pkg()
    ms = mixed(members)[:2]
    q, dims = kc.cone_layout(ms[0]["prob"])
    with pytest.raises(pkg.CalipsoHipError) as e:                           # the column method factors a batch one matrix after the other
        pkg.SparseKKTGroup(*ms[0]["inputs"], members=2, n_nonnegative=q, second_order_dims=dims, method="minimum_degree")
    assert "(-4)" in str(e.value) and "a group needs the multifrontal numeric phase" in str(e.value) and "numeric phase" in str(e.value)
    g = group_of(ms)
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.set_option("krylov_fallback", 1)
    assert "bad argument" in str(e.value) and "not built for groups" in str(e.value)
    g.set_option("krylov_fallback", 0)
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.set_option("no_such_option", 1.0)
    assert "unknown option" in str(e.value)
    with pytest.raises(pkg.CalipsoHipError) as e:                           # arrays of the wrong length
        g.search_direction(np.ones((2, g.N - 1)), ZERO)
    assert "the residual has" in str(e.value)
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.set_values(w=np.ones((3, g.N)))
    assert "w has" in str(e.value)
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.set_values(Lxx=[ms[0]["inputs"][0], ms[0]["inputs"][0].data[:-1]])
    assert "Lxx has" in str(e.value)
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.mul(np.ones(g.N))
    assert "v has" in str(e.value)
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.matrix(2)
    assert "member: 2 is not in 0 .. 1" in str(e.value)
    with pytest.raises(pkg.CalipsoHipError) as e:                           # a CPU tensor on the device route: refused, naming the argument, before anything is enqueued
        g.set_values(w=torch.tensor(np.stack([m["w"] for m in ms]), dtype=torch.float64))
    assert "bad argument" in str(e.value) and "calipso_hip_sparse_kkt_group_set_values_device: w is not device memory" in str(e.value)
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.search_direction(torch.tensor(residuals(ms), dtype=torch.float64), ZERO)
    assert "calipso_hip_sparse_kkt_group_search_direction_device: residual is not device memory" in str(e.value)
    out = g.search_direction(residuals(ms), ZERO)                         # ... and the group is as it was
    for k, ((pid, kind), _) in enumerate(gc.MIXED[:2]):
        assert_member_is_its_single_handle(out, k, members.single(kc.SMALL, pid, kind))
