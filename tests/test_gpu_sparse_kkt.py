"""GPU (run with -m gpu on an MI355X): calipso.jl_amd.SparseKKT — search_direction! on sparse problem data resident on the device (csrc/sparse_kkt.hip) — against the
CPU oracle.  The checker is the oracle, never the code under test; the inputs are those of tests/sparse_kkt_cases.py, which tests/test_sparse_kkt_inputs_cpu.py pins
with the oracle alone.  Tolerances are those tests/test_gpu_parity.py uses for the same quantities on the dense path: matrices and products 1e-12 relative, steps 1e-8
relative, integers (inertia, factorisation counts) and the regularisation walk exact."""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")      # (one HIP runtime per process: torch first, then the library)

import helpers
import sparse_kkt_cases as kc
from helpers import load_pkg

pytestmark = pytest.mark.gpu

MULTIFRONTAL, COLUMNS = "nested_dissection", "minimum_degree"       # methods 4 and 2 of calipso_hip_sparse_create


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()) if np.asarray(b).size else 0.0


def handle(prob, method=MULTIFRONTAL, extra=None, **kw):
    """(SparseKKT of the problem's sparse inputs, those inputs)"""
    q, dims = kc.cone_layout(prob)
    Lxx, gx, hx = kc.sparse_inputs(prob, extra)
    return load_pkg().SparseKKT(Lxx, gx, hx, n_nonnegative=q, second_order_dims=dims, method=method, **kw), (Lxx, gx, hx)


@pytest.fixture(scope="module")
def block_references(oracle_mod):
    """per building-block case, computed once and left unchanged: the problem, the point and what the oracle makes of it at the fixed regularisation"""
    cache = {}

    def get(name):
        if name not in cache:
            prob, pt, lam = kc.block_case(oracle_mod.splitmix_uniform, name)
            o = helpers.make_oracle(oracle_mod, prob, pt, lam, kappa=kc.KAPPA, rho=kc.RHO, ep=kc.EP, ed=kc.ED)
            o.cone(product=True, jacobian=True, target=True)
            o.residual()
            o.residual_jacobian_variables(); o.residual_jacobian_variables_symmetric()
            v = np.random.default_rng(9).standard_normal(o.N)
            o.factorize(update=False)
            inertia = o.compute_inertia()
            o.search_direction_symmetric(0, fact=False)
            ref = dict(prob=prob, w=np.concatenate([pt[k] for k in "xrsyzt"]), K=np.triu(o.K_dense()).copy(), v=v, Hv=o.H_mul(v).copy(), inertia=inertia,
                       R=o.buf("residual").copy(), step=o.buf("step").copy())
            for a in ref.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            cache[name] = ref
        return cache[name]
    return get


def check_blocks(g, inputs, ref):
    Lxx, gx, hx = inputs
    g.set_values(Lxx, gx, hx, ref["w"], kc.RHO, central_path=kc.KAPPA)
    warn = g.factorize(kc.EP, kc.ED)
    K = g.matrix()
    assert K.shape == ref["K"].shape and sp.triu(K).nnz == K.nnz
    assert rel(K.toarray(), ref["K"]) <= 1e-12
    assert rel(g.mul(ref["v"]), ref["Hv"]) <= 1e-12
    assert warn == 0 and g.inertia == ref["inertia"] == (g.nx, g.ne + g.nc, 0)
    assert rel(g.solve_symmetric(ref["R"]), ref["step"]) <= 1e-8


@pytest.mark.parametrize("method", [MULTIFRONTAL, COLUMNS])
@pytest.mark.parametrize("name", kc.BLOCK_CASES)
def test_building_blocks_at_a_fixed_regularisation(block_references, name, method):
    ref = block_references(name)
    g, inputs = handle(ref["prob"], method)
    assert g.info["n"] == g.n and g.info["N"] == g.N and g.info["assemble_launches"] == 1
    assert g.info["max_cone_dimension"] == max(kc.cone_layout(ref["prob"])[1] + [0])
    if method == COLUMNS:
        assert g.info["numeric"].startswith("columns")
    check_blocks(g, inputs, ref)


def test_a_superset_pattern_with_stored_zeros_moves_nothing(block_references):
    ref = block_references("staged_3_4_2_1_1_3")
    g, inputs = handle(ref["prob"], extra=np.random.default_rng(1))
    exact = kc.sparse_inputs(ref["prob"])
    assert all(a.nnz > b.nnz for a, b in zip(inputs, exact))
    check_blocks(g, inputs, ref)


@pytest.mark.parametrize("name", ["staged_2_3_1_1_0_3", "staged_3_4_2_1_1_3", "qp_soc64_70_5_66"])
def test_the_single_column_solve_is_the_one_column_map(block_references, name):
    """solve_symmetric and search_direction go through the multi-column map with one column: the same bits as solve_columns, and a handle that used the column
    entries steps as one that never did (the dense-pattern case takes the wavefront-per-row H v in its refinement)"""
    ref = block_references(name)
    g, (Lxx, gx, hx) = handle(ref["prob"])
    g.set_values(Lxx, gx, hx, ref["w"], kc.RHO, central_path=kc.KAPPA)
    assert g.factorize(kc.EP, kc.ED) == 0
    R, R2 = ref["R"], np.random.default_rng(3).standard_normal(g.N)
    one = g.solve_symmetric(R)
    assert np.array_equal(g.solve_columns(R), one)
    assert np.array_equal(g.solve_columns(np.stack([R, R2], axis=1))[:, 0], one)
    fresh, _ = handle(ref["prob"])
    fresh.set_values(Lxx, gx, hx, ref["w"], kc.RHO, central_path=kc.KAPPA)
    step, reg, info, status = g.search_direction(R, (0.0, 0.0, 0.0))
    want = fresh.search_direction(R, (0.0, 0.0, 0.0))
    assert np.array_equal(step, want[0]) and (reg, info, status) == want[1:]


@pytest.mark.parametrize("name", sorted(kc.WHOLE))
def test_whole_search_direction(oracle_mod, name):
    shape, pid, kind, want = kc.WHOLE[name]
    prob, w, lam = kc.whole_case(oracle_mod.splitmix_uniform, shape, pid, kind)
    o, ref = kc.oracle_search_direction(oracle_mod, prob, w, lam)
    assert ref["status"] == 0 and ref["fallbacks"] == 0
    R = o.buf("residual").copy()
    g, (Lxx, gx, hx) = handle(prob)
    g.set_values(Lxx, gx, hx, w, kc.RHO, central_path=kc.KAPPA)
    step, reg, info, status = g.search_direction(R, (0.0, 0.0, 0.0))
    print("%s: factorisations %d (oracle %d), refinement rounds %d (oracle %d), ep %r, |R - H step| %.3e" %
          (name, info["factorizations"], ref["factorizations"], info["refinement_rounds"], ref["rounds"], reg[0], info["residual_norm"]))
    assert status == 0
    assert reg == (ref["ep"], ref["ep_last"], ref["ed"])                  # bit for bit
    assert info["factorizations"] == ref["factorizations"] == want["factorizations"]
    assert rel(step, o.buf("step")) <= 1e-8
    assert np.abs(R - o.H_dense() @ step).max() <= 1e-9 * max(1.0, np.abs(R).max())
    if want["rounds_stable"]:                                            # (pinned in tests/test_sparse_kkt_inputs_cpu.py: the oracle decides the same count on perturbed points)
        assert info["refinement_rounds"] == ref["rounds"]


def test_refinement_failure_is_a_warning_and_leaves_the_handle_usable(oracle_mod):
    prob, w, lam = helpers.staged_step_case(oracle_mod.splitmix_uniform, kc.FAILURE_ID, kc.FAILURE_SHAPE, True)
    o, ref = kc.oracle_search_direction(oracle_mod, prob, w, lam)
    assert ref["status"] == 2 and ref["fallbacks"] == 1
    g, (Lxx, gx, hx) = handle(prob)
    g.set_values(Lxx, gx, hx, w, kc.RHO, central_path=kc.KAPPA)
    step, reg, info, status = g.search_direction(o.buf("residual").copy(), (0.0, 0.0, 0.0))
    assert status == 2                                                   # CALIPSO_WARN_REFINEMENT: no `H \ residual` here
    assert reg == (ref["ep"], ref["ep_last"], ref["ed"]) and info["factorizations"] == ref["factorizations"]
    assert np.isfinite(step).all()
    # the same handle, the interior point of the same problem
    prob, w, lam = helpers.staged_step_case(oracle_mod.splitmix_uniform, kc.FAILURE_ID, kc.FAILURE_SHAPE, False)
    o, ref = kc.oracle_search_direction(oracle_mod, prob, w, lam)
    assert ref["status"] == 0
    g.set_values(w=w)
    R = o.buf("residual").copy()
    step, reg, info, status = g.search_direction(R, (0.0, 0.0, 0.0))
    assert status == 0 and reg == (ref["ep"], ref["ep_last"], ref["ed"]) and info["factorizations"] == ref["factorizations"]
    assert rel(step, o.buf("step")) <= 1e-8
    assert np.abs(R - o.H_dense() @ step).max() <= 1e-9 * max(1.0, np.abs(R).max())


def test_device_route_gives_the_bits_of_the_host_route(oracle_mod):
    shape, pid, kind, _ = kc.WHOLE["interior_small"]
    prob, w, lam = kc.whole_case(oracle_mod.splitmix_uniform, shape, pid, kind)
    o, ref = kc.oracle_search_direction(oracle_mod, prob, w, lam)
    R = o.buf("residual").copy()
    g, (Lxx, gx, hx) = handle(prob)
    g.set_values(Lxx, gx, hx, w, kc.RHO, central_path=kc.KAPPA)
    host = g.search_direction(R, (0.0, 0.0, 0.0))
    d, _ = handle(prob)
    dev = lambda a: torch.tensor(np.asarray(a, dtype=np.float64).reshape(-1), dtype=torch.float64, device="cuda:0")
    d.set_values(dev(Lxx.data), dev(gx.data), dev(hx.data), dev(w), dev([kc.RHO]), central_path=kc.KAPPA)
    step, reg, info, status = d.search_direction(dev(R), (0.0, 0.0, 0.0))
    assert step.is_cuda and np.array_equal(step.cpu().numpy(), host[0])
    assert (reg, info, status) == host[1:]
    assert rel(host[0], o.buf("step")) <= 1e-8
    # a host pointer in a device entry: refused, naming the argument, before anything is enqueued
    pkg = load_pkg()
    with pytest.raises(pkg.CalipsoHipError) as e:
        d.set_values(w=torch.tensor(w, dtype=torch.float64))
    assert "bad argument" in str(e.value) and "calipso_hip_sparse_kkt_set_values_device: w is not device memory" in str(e.value)
    with pytest.raises(pkg.CalipsoHipError) as e:
        d.search_direction(torch.tensor(R, dtype=torch.float64))
    assert "calipso_hip_sparse_kkt_search_direction_device: residual is not device memory" in str(e.value)
    again = d.search_direction(dev(R), (0.0, 0.0, 0.0))                  # ... and the handle is as it was
    assert np.array_equal(again[0].cpu().numpy(), host[0])


def test_refusals():
    pkg = load_pkg()
    eye = sp.identity(4, format="csc")
    none, two = sp.csc_matrix((0, 4)), sp.csc_matrix(np.ones((2, 4)))
    unsorted = sp.csc_matrix((np.ones(2), np.array([1, 0]), np.array([0, 2, 2, 2, 2])), shape=(4, 4))
    duplicate = sp.csc_matrix((np.ones(2), np.array([1, 1]), np.array([0, 2, 2, 2, 2])), shape=(4, 4))
    for make, text in [(lambda: pkg.SparseKKT(unsorted, none, two), "Lxx: row indices must ascend within a column"),
                       (lambda: pkg.SparseKKT(eye, none, sp.csc_matrix((np.ones(2), np.array([1, 1]), np.array([0, 2, 2, 2, 2])), shape=(2, 4))), "hx: duplicate entry in the CSC pattern"),
                       (lambda: pkg.SparseKKT(duplicate, none, two), "Lxx: duplicate entry in the CSC pattern"),
                       (lambda: pkg.SparseKKT(eye, none, two, n_nonnegative=1, second_order_dims=[1]), "a second-order cone has dimension >= 2"),
                       (lambda: pkg.SparseKKT(eye, none, two, n_nonnegative=1, second_order_dims=[2]), "the cone dimensions exceed nc = 2"),
                       (lambda: pkg.SparseKKT(eye, none, two, n_nonnegative=0, second_order_dims=[3]), "the cone dimensions exceed nc = 2")]:
        with pytest.raises(pkg.CalipsoHipError) as e:
            make()
        assert "(-4)" in str(e.value) and text in str(e.value)
    g = pkg.SparseKKT(eye, none, two)
    g.set_values(eye, None, two, np.ones(g.N), 1.0)
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.solve_symmetric(np.ones(g.N))
    assert "bad argument" in str(e.value) and "factorize first" in str(e.value)
    with pytest.raises(pkg.CalipsoHipError) as e:
        g.set_option("no_such_option", 1.0)
    assert "unknown option" in str(e.value)
    assert g.factorize(0.1, 0.1) == 0 and g.inertia == (4, 2, 0)          # ... and the handle works
    assert np.isfinite(g.solve_symmetric(np.ones(g.N))).all()
