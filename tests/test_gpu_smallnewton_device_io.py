"""GPU (-m gpu): the device-resident, stream-ordered entries of the one-launch batch kernel (calipso_hip_smallnewton_*_device, SmallNewtonBatch.*_device,
torch_layer.QPLayer on CUDA tensors, torch_layer.ParametricLayer).  The kernels k_smallnewton / k_smallnewton_adj are the host path's, and they are pinned as
bit-reproducible at a fixed workgroup size: so everything here is held to the HOST path to the bit (np.array_equal) — the packed data through whole solves, the
state, the solution slices, the adjoints and per-instance gradients — and only the batch sums of shared inputs' gradients, which the device adds in another order
than numpy, to the worst-case bound for two summation orders of B terms, |g_dev - sum_k g_k| <= 2 (B - 1) 2^-53 sum_k |g_k| elementwise."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")      # (one HIP runtime per process: torch first, then the library)

from helpers import load_pkg
from test_gpu_smallnewton_adjoint import C5, MIXED, RPLUS, THREADS, TIGHT, evlib

pytestmark = pytest.mark.gpu

NAMES = "PqAbGh"
EDGES = [(1, 0, 0, 0, 0), (7, 0, 5, 0, 0), (9, 4, 0, 0, 0), (128, 63, 0, 0, 0)]      # nx = 1, ne = 0, nc = 0, the widest admitted R+ shape
U = 2.0 ** -53


def gen(layout, B, seed):
    """the recipe of problems.parametric_conic_qp, batched: P = Q'Q + I, A, G ~ N(0, 1/nx), q, b ~ N(0, 1), h in [1, 2)"""
    nx, ne, nnn, nsoc, sdim = layout
    nc = nnn + nsoc * sdim
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((B, nx, nx)) / np.sqrt(nx)
    return dict(P=np.transpose(Q, (0, 2, 1)) @ Q + np.eye(nx), q=rng.standard_normal((B, nx)), A=rng.standard_normal((B, ne, nx)) / np.sqrt(nx),
                b=rng.standard_normal((B, ne)), G=rng.standard_normal((B, nc, nx)) / np.sqrt(nx), h=rng.random((B, nc)) + 1.0)


def handle(pkg, layout, B, threads=0, **opts):
    nx, ne, nnn, nsoc, sdim = layout
    sn = pkg.SmallNewtonBatch(nx, ne, nnn + nsoc * sdim, B, options=dict(threads=threads, **opts))
    if nsoc:
        sn.set_cones(nnn, [sdim] * nsoc)
    return sn


def cuda(a, **kw):
    return torch.tensor(np.ascontiguousarray(a), device="cuda", **kw)


def shared_view(d, shared):
    """the data with the arrays named in `shared` taken from instance 0: (what the device path gets, what the host path gets: broadcast)"""
    B = d["P"].shape[0]
    one = {n: (d[n][0] if n in shared else d[n]) for n in NAMES}
    full = {n: (np.broadcast_to(d[n][0], d[n].shape).copy() if n in shared else d[n]) for n in NAMES}
    return one, full


def host_solve(sn, full, c, x0=None):
    sn.set_qp(*[full[n] for n in NAMES], objective_scale=c, shared=False)
    sn.initialize(np.zeros((sn.batch, sn.nx)) if x0 is None else x0)
    return sn.solve()[0]


def device_solve(sn, one, c, row_major=True, x0=None):
    sn.set_stream(torch.cuda.current_stream())      # (the tensors below are torch's: the handle works on the stream that owns them)
    t = lambda n: cuda(one[n] if (row_major or one[n].ndim < 2 or n in "qbh") else np.swapaxes(one[n], -1, -2))
    mask = sn.set_qp_device(*[t(n) for n in NAMES], objective_scale=c, row_major=row_major)
    sn.initialize_device(x0)
    sn.solve_device()
    return mask


def assert_same_state(D, H, res=None):
    a, b = D.get_state(), H.get_state()
    for key in ("solution", "dual", "scalars"):
        assert np.array_equal(a[key], b[key]), key
    for key in a["counters"]:
        assert np.array_equal(a["counters"][key], b["counters"][key]), key
    if res is not None:
        assert np.array_equal(D.status_device().cpu().numpy(), res)


def buffers(sn):
    out = (ctypes.c_int64 * 8)()
    f = sn._L.calipso_hip_debug_smallnewton_buffers
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)], ctypes.c_int32
    assert f(sn._h, out) == 0
    return list(out)


def reduced_ratio(g_dev, g_per):
    """max over the entries of |g_dev - sum_k g_k| / (2 (B - 1) 2^-53 sum_k |g_k|) against numpy's float64 sum of the per-instance gradients: <= 1 is the bound"""
    B = g_per.shape[0]
    dev, bound = np.abs(g_dev - g_per.sum(axis=0)), 2.0 * (B - 1) * U * np.abs(g_per).sum(axis=0)
    assert np.all(dev <= bound), float((dev - bound).max())
    return float((dev[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ---- 1. the pack kernel writes the host's bits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("layout", RPLUS + MIXED + EDGES)
def test_device_pack_and_solve_equal_the_host_path_to_the_bit(layout, threads):
    pkg = load_pkg()
    B, c = 5, 0.7
    d = gen(layout, B, 500)
    opts = C5 if layout[0] >= 49 else TIGHT
    H = handle(pkg, layout, B, threads, **opts)
    res = host_solve(H, d, c)
    for row_major in (True, False):
        D = handle(pkg, layout, B, threads, **opts)
        assert device_solve(D, d, c, row_major) == 0
        torch.cuda.synchronize()
        assert_same_state(D, H, res)
        D.close()
    H.close()


# ---- 2. sharing masks ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", ["PqAbGh", "", "P", "PAG", "A"])
def test_sharing_masks_store_shared_arrays_once_and_keep_their_buffers(shared):
    pkg = load_pkg()
    layout, B, c = (12, 5, 6, 0, 0), 6, 0.5
    one, full = shared_view(gen(layout, B, 510), shared)
    H = handle(pkg, layout, B, **TIGHT)
    res = host_solve(H, full, c)
    D = handle(pkg, layout, B, **TIGHT)
    mask = device_solve(D, one, c)
    assert mask == sum(1 << NAMES.index(n) for n in shared)
    first = buffers(D)
    nx, m = 12, 11
    assert first[4] == (0 if "P" in shared else nx * nx) and first[5] == (0 if "q" in shared else nx)
    assert first[6] == (0 if ("A" in shared and "G" in shared) else m * nx)          # A without G: Z falls back to per-instance storage
    assert first[7] == (0 if ("b" in shared and "h" in shared) else m)
    torch.cuda.synchronize()
    assert_same_state(D, H, res)
    device_solve(D, one, c)                                                           # the same mask and shapes again: the same buffers
    assert buffers(D) == first
    torch.cuda.synchronize()
    assert_same_state(D, H, res)
    # and against the host's own all-shared storage
    if shared == "PqAbGh":
        H.set_qp(*[one[n] for n in NAMES], objective_scale=c, shared=True)
        H.initialize(np.zeros((B, nx)))
        assert np.array_equal(H.solve()[0], res)
        assert_same_state(D, H, res)
    D.close(); H.close()


# ---- 3. state in, solution out ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [RPLUS[0], MIXED[0], EDGES[0], EDGES[1], EDGES[2]])
def test_state_and_solution_entries_equal_the_host_entries(layout):
    pkg = load_pkg()
    B, c = 5, 0.5
    d = gen(layout, B, 520)
    H, D = handle(pkg, layout, B, **TIGHT), handle(pkg, layout, B, **TIGHT)
    x0 = np.random.default_rng(1).standard_normal((B, layout[0])) * 0.1
    res = host_solve(H, d, c, x0)
    device_solve(D, d, c, x0=cuda(x0))
    sol = D.solution_device(parts="xyzws")
    torch.cuda.synchronize()
    assert_same_state(D, H, res)
    st = H.get_state()
    w = st["solution"]
    nx, ne, nc = H.nx, H.ne, H.nc
    oy, oz = nx + ne + nc, nx + 2 * ne + nc
    assert np.array_equal(sol["x"].cpu().numpy(), w[:, :nx]) and np.array_equal(sol["y"].cpu().numpy(), w[:, oy:oy + ne])
    assert np.array_equal(sol["z"].cpu().numpy(), w[:, oz:oz + nc]) and np.array_equal(sol["w"].cpu().numpy(), w)
    assert sol["status"].dtype == torch.int32 and np.array_equal(sol["status"].cpu().numpy(), res)
    out = dict(x=torch.empty((B, nx), dtype=torch.float64, device="cuda"))           # a caller's buffer
    assert D.solution_device(out=out, parts="")["x"] is out["x"]
    assert np.array_equal(out["x"].cpu().numpy(), w[:, :nx])
    # warm start from a given state: points, duals and the three scalars
    rng = np.random.default_rng(2)
    w2 = w * (1.0 + 1e-3 * rng.standard_normal(w.shape))
    lam2 = st["dual"] + 1e-2 * rng.standard_normal(st["dual"].shape)
    sc2 = np.tile([0.05, 0.995, 30.0], (B, 1)) * (1.0 + 0.1 * rng.random((B, 3)))
    for sn in (H, D):
        sn.set_option("warmstart", 1.0)
    H.set_state(w=w2, dual=lam2 if ne else None, scalars=sc2)
    D.set_state_device(w=cuda(w2), dual=cuda(lam2) if ne else None, scalars=cuda(sc2))
    assert_same_state(D, H)                                                           # (the scatter of the scalars, before any launch)
    res2 = H.solve()[0]
    D.solve_device()
    assert_same_state(D, H, res2)
    D.set_state_device(scalars=cuda(sc2 * 1.5))                                       # the scalars alone: points and duals stay
    H.set_state(scalars=sc2 * 1.5)
    assert_same_state(D, H)
    D.close(); H.close()


# ---- 4. the reverse mode ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("layout", [RPLUS[0], MIXED[0], EDGES[0], EDGES[1], EDGES[2]])
def test_vjp_device_equals_vjp_to_the_bit(layout, k):
    pkg = load_pkg()
    B, c = 5, 0.7
    d = gen(layout, B, 530)
    H, D = handle(pkg, layout, B, **TIGHT), handle(pkg, layout, B, **TIGHT)
    res = host_solve(H, d, c)
    device_solve(D, d, c)
    N, nx, ne, nc = H.N, H.nx, H.ne, H.nc
    v = np.random.default_rng(3).standard_normal((B, N, k))
    ref = H.vjp(v if k > 1 else v[:, :, 0])
    out = D.vjp_device(cotangent=cuda(v if k > 1 else v[:, :, 0]), adjoint=True)
    assert np.array_equal(out["status"].cpu().numpy(), ref["status"])
    good = res == 1
    for name in ("adjoint",) + tuple(NAMES):
        got = out[name].cpu().numpy()
        assert got.shape == ref[name].shape, name
        if name == "adjoint":
            assert np.array_equal(got, ref[name]), name
        else:
            assert np.array_equal(got[good], ref[name][good]) and np.isnan(got[~good]).all(), name
    # the cotangent by parts = the full cotangent with zeros elsewhere
    oy, oz = nx + ne + nc, nx + 2 * ne + nc
    vp = np.zeros_like(v)
    vp[:, :nx], vp[:, oy:oy + ne], vp[:, oz:oz + nc] = v[:, :nx], v[:, oy:oy + ne], v[:, oz:oz + nc]
    sq = (lambda a: a) if k > 1 else (lambda a: a[:, :, 0])
    full = D.vjp_device(cotangent=cuda(sq(vp)), adjoint=True)
    parts = D.vjp_device(x=cuda(sq(vp[:, :nx])), y=cuda(sq(vp[:, oy:oy + ne])), z=cuda(sq(vp[:, oz:oz + nc])), adjoint=True)
    for name in ("adjoint",) + tuple(NAMES):
        assert np.array_equal(full[name].cpu().numpy(), parts[name].cpu().numpy(), equal_nan=True), name
    xonly = D.vjp_device(x=cuda(sq(v[:, :nx])), qp="q")
    refx = H.vjp(sq(v[:, :nx]), adjoint=False)
    assert set(xonly) == {"status", "q"} and np.array_equal(xonly["q"].cpu().numpy()[good], refx["q"][good])
    D.close(); H.close()


@pytest.mark.parametrize("B", [5, 4096])
def test_reduced_gradients_within_the_bound_of_two_summation_orders(B):
    """the batch sums on the device against numpy's float64 sum of the device's own per-instance gradients (bit-equal to the host's: the test above); k = 1 and 3;
    two runs bit-equal.  Largest |deviation| / bound: printed; seen 0.005 at B = 4096 and 0.000 at B = 5"""
    pkg = load_pkg()
    worst = 0.0
    for layout, opts in (((12, 5, 6, 0, 0), TIGHT), ((49, 40, 0, 0, 0), C5)):
        D = handle(pkg, layout, B, **opts)
        d = gen(layout, B, 540)
        device_solve(D, d, 0.5)
        st = D.status_device().cpu().numpy()
        if (st != 1).any():                             # (a sum needs every term: an instance that did not converge takes the data of one that did)
            for n in NAMES:
                d[n][st != 1] = d[n][int(np.argmax(st == 1))]
            device_solve(D, d, 0.5)
        assert (D.status_device() == 1).all()
        for k in (1, 3):
            v = cuda(np.random.default_rng(4).standard_normal((B, D.N, k) if k > 1 else (B, D.N)))
            per = D.vjp_device(cotangent=v)
            red = D.vjp_device(cotangent=v, reduce=NAMES)
            again = D.vjp_device(cotangent=v, reduce=NAMES)
            mixed = D.vjp_device(cotangent=v, reduce="PA")
            for name in NAMES:
                g = red[name].cpu().numpy()
                assert g.shape == per[name].shape[1:]
                assert np.array_equal(g, again[name].cpu().numpy()), name
                worst = max(worst, reduced_ratio(g, per[name].cpu().numpy()))
                assert np.array_equal(mixed[name].cpu().numpy(), (red if name in "PA" else per)[name].cpu().numpy()), name
        D.close()
    print("largest deviation of a device batch sum / bound, B = %d: %.3f" % (B, worst))


def test_non_converged_instances_give_nan_rows_and_nan_sums():
    """the construction of test_torch_layer_gradcheck_and_non_converged_instances (one outer, one residual iteration: solve status 0) on a batch where instances 0
    and 3 start at their solution (q = 0, b = 0, x0 = 0), which is the one way such a solve can still end with status 1; rows are held by the statuses the host
    path reports: status != 1 gives NaN, status 1 the host's bits"""
    pkg = load_pkg()
    layout, B, c = (4, 2, 0, 0, 0), 6, 0.5
    d = gen(layout, B, 550)
    for k in (0, 3):
        d["q"][k] = 0.0; d["b"][k] = 0.0
    opts = dict(max_outer_iterations=1, max_residual_iterations=1)
    H, D = handle(pkg, layout, B, **opts), handle(pkg, layout, B, **opts)
    res = host_solve(H, d, c)
    device_solve(D, d, c)
    print("solve statuses:", res)
    bad = res != 1
    assert bad.any() and (~bad).any(), res                                            # both groups: NaN rows and rows held to the host's bits
    v = np.random.default_rng(5).standard_normal((B, H.N))
    ref = H.vjp(v, adjoint=False)
    per = D.vjp_device(cotangent=cuda(v))
    red = D.vjp_device(cotangent=cuda(v), reduce="PqAb")
    assert np.array_equal(D.status_device().cpu().numpy(), res)                       # (the solve's statuses survive the differentiate launches)
    for name in "PqAb":
        g = per[name].cpu().numpy()
        assert np.isnan(g[bad]).all() and np.array_equal(g[~bad], ref[name][~bad]), name
        assert torch.isnan(red[name]).all(), name
    D.close(); H.close()


# ---- 5. stream order, no host synchronisation ------------------------------------------------------------------------------------------------------
def test_forward_and_backward_return_while_the_stream_is_still_busy():
    from calipso_jl_amd.torch_layer import QPLayer
    pkg = load_pkg()
    layout, B, c = (12, 5, 6, 0, 0), 64, 0.5
    nx = layout[0]
    d = gen(layout, B, 560)
    D, H = handle(pkg, layout, B, **TIGHT), handle(pkg, layout, B, **TIGHT)
    rest = [cuda(d[n], requires_grad=True) for n in "qAbGh"]
    wx = cuda(np.random.default_rng(6).standard_normal((B, nx)))
    stream = torch.cuda.Stream()
    n = 4096
    with torch.cuda.stream(stream):
        warm = torch.eye(nx, dtype=torch.float64, device="cuda").requires_grad_()     # the handle's buffers and torch's pools: sized once, before the timed part
        (QPLayer.apply(D, warm, *rest, False, c) * wx).sum().backward()
        for t in rest:
            t.grad = None
        W = torch.randn((n, n), dtype=torch.float64, device="cuda") / math.sqrt(n)
        M = torch.randn((n, n), dtype=torch.float64, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        M = M @ W
        e0.record(stream); M = M @ W; e1.record(stream)
        stream.synchronize()
        one_ms = e0.elapsed_time(e1)
        count = int(math.ceil(400.0 / one_ms)) + 1                                     # a chain of >= 400 ms, twice the 200 ms asked for
        for _ in range(count):
            M = M @ W
        L = M[:nx, :nx] / M[:nx, :nx].abs().max()
        P = (L @ L.T + torch.eye(nx, dtype=torch.float64, device="cuda")).detach().requires_grad_()      # the chain's last op makes the layer's input
        x = QPLayer.apply(D, P, *rest, False, c)
        (x * wx).sum().backward()
        busy = not stream.query()
    assert busy, "forward + backward drained the stream: an entry synchronised (one matmul %.2f ms, %d in the chain)" % (one_ms, count)
    stream.synchronize()
    assert x.is_cuda and P.grad.is_cuda
    # the host path on the values the inputs finally hold
    Pc = P.detach().cpu().requires_grad_()
    restc = [t.detach().cpu().requires_grad_() for t in rest]
    xc = QPLayer.apply(H, Pc, *restc, False, c)
    (xc * wx.cpu()).sum().backward()
    assert np.array_equal(x.detach().cpu().numpy(), xc.detach().numpy())
    for name, t, tc in zip("qAbGh", rest, restc):
        assert np.array_equal(t.grad.cpu().numpy(), tc.grad.numpy()), name
    v = np.zeros((B, H.N)); v[:, :nx] = wx.cpu().numpy()
    ratio = reduced_ratio(P.grad.cpu().numpy(), H.vjp(v, adjoint=False)["P"])
    print("one matmul %.2f ms, chain of %d, shared P's gradient: deviation / bound = %.3f" % (one_ms, count, ratio))
    D.close(); H.close()


# ---- 6. the layer on CUDA tensors against the layer on CPU tensors -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", ["", "PqAbGh", "PAG"])
def test_qp_layer_on_cuda_tensors_equals_the_layer_on_cpu_tensors(shared):
    from calipso_jl_amd.torch_layer import QPLayer
    pkg = load_pkg()
    layout, B, c = (6, 2, 4, 0, 0), 4, 0.5
    one, _ = shared_view(gen(layout, B, 570), shared)
    D, H = handle(pkg, layout, B, **TIGHT), handle(pkg, layout, B, **TIGHT)
    cpu = [torch.tensor(one[n], requires_grad=True) for n in NAMES]
    dev = [cuda(one[n], requires_grad=True) for n in NAMES]
    wx, wz = np.random.default_rng(1).standard_normal((B, 6)), np.random.default_rng(2).standard_normal((B, 4))
    outs_c = QPLayer.apply(H, *cpu, True, c)
    outs_d = QPLayer.apply(D, *dev, True, c)
    # the handle solves another batch before the backward pass: the key check must solve the first again
    other, _ = shared_view(gen(layout, B, 571), shared)
    QPLayer.apply(D, *[cuda(other[n]) for n in NAMES], False, c)
    ((outs_c[0] * torch.tensor(wx)).sum() + (outs_c[2] * torch.tensor(wz)).sum()).backward()
    ((outs_d[0] * cuda(wx)).sum() + (outs_d[2] * cuda(wz)).sum()).backward()
    for a, b in zip(outs_d, outs_c):
        assert a.is_cuda and a.device == dev[0].device and np.array_equal(a.detach().cpu().numpy(), b.detach().numpy())
    v = np.zeros((B, H.N)); v[:, :6] = wx; v[:, 6 + 2 * 2 + 4:6 + 2 * 2 + 8] = wz
    per = H.vjp(v, adjoint=False)
    for name, td, tc in zip(NAMES, dev, cpu):
        assert td.grad.is_cuda and td.grad.shape == td.shape
        if name in shared:
            reduced_ratio(td.grad.cpu().numpy(), per[name])
        else:
            assert np.array_equal(td.grad.cpu().numpy(), tc.grad.numpy()), name
    D.close(); H.close()


def test_qp_layer_gradcheck_on_the_device_path():
    """the settings of test_torch_layer_gradcheck_and_non_converged_instances: eps 1e-6, atol 1e-5, rtol 1e-3; then the non-converged batch: NaN gradients, no
    warning on this path, the statuses through status_device()"""
    from calipso_jl_amd.torch_layer import QPLayer
    import problems as pr
    pkg = load_pkg()
    nx, ne = 4, 2
    p = pr.parametric_conic_qp(nx, ne, 0, 0, 0, seed=77)
    tol = dict(residual_tolerance=1e-10, optimality_tolerance=1e-10, equality_tolerance=1e-10, complementarity_tolerance=1e-10, slack_tolerance=1e-10, penalty_initial=1e8)
    sn = pkg.SmallNewtonBatch(nx, ne, 0, 2, options=tol)
    P = cuda(np.asarray(p.P))
    q = cuda(np.stack([np.asarray(p.q), np.asarray(p.q) + 0.5]), requires_grad=True)
    A = cuda(np.asarray(p.A).reshape(ne, nx), requires_grad=True)
    b = cuda(np.asarray(p.b), requires_grad=True)
    G, h = torch.zeros((0, nx), dtype=torch.float64, device="cuda"), torch.zeros(0, dtype=torch.float64, device="cuda")
    f = lambda q_, A_, b_: QPLayer.apply(sn, P, q_, A_, b_, G, h, False, p.c)
    assert torch.autograd.gradcheck(f, (q, A, b), eps=1e-6, atol=1e-5, rtol=1e-3)
    sn.close()
    sn = pkg.SmallNewtonBatch(nx, ne, 0, 2, options=dict(max_outer_iterations=1, max_residual_iterations=1))
    x = QPLayer.apply(sn, P, q, A, b, G, h, False, p.c)
    x.sum().backward()
    assert (sn.status_device() != 1).all() and torch.isnan(q.grad).all() and torch.isnan(A.grad).all()
    sn.close()


# ---- 7. evaluators ---------------------------------------------------------------------------------------------------------------------------------
def test_cartpole_parameters_on_the_device_and_the_parametric_layer():
    import test_gpu_smallnewton_evaluator as te
    from calipso_jl_amd.torch_layer import ParametricLayer
    pkg = load_pkg()
    prob = te.cartpole()
    B = 64
    th = te.cartpole_thetas(B)
    x0 = np.repeat(np.asarray(prob.x0, dtype=np.float64)[None], B, axis=0)

    def make():
        sn = pkg.SmallNewtonBatch(prob.nx, prob.ne, prob.nc, B, options=C5)
        sn.set_evaluator(evlib(), "cartpole_mpc_kernels", prob.np)
        return sn

    H, D, Lyr = make(), make(), make()
    H.set_parameters(th); H.initialize(x0)
    res = H.solve()[0]
    assert (res == 1).all()
    D.set_stream(torch.cuda.current_stream())
    D.set_parameters_device(cuda(th)); D.initialize_device(cuda(x0)); D.solve_device()
    assert_same_state(D, H, res)
    for k in (1, 3):
        v = np.random.default_rng(9).standard_normal((B, H.N, k))
        v = v if k > 1 else v[:, :, 0]
        ref, out = H.vjp(v), D.vjp_device(cotangent=cuda(v), adjoint=True)
        assert "P" not in out
        for name in ("theta", "adjoint", "status"):
            assert np.array_equal(out[name].cpu().numpy(), ref[name]), (name, k)
    # the layer
    theta = cuda(th, requires_grad=True)
    w = ParametricLayer.apply(Lyr, theta, cuda(x0))
    assert w.is_cuda and np.array_equal(w.detach().cpu().numpy(), H.get_state()["solution"])
    v1 = np.random.default_rng(10).standard_normal((B, H.N))
    (w * cuda(v1)).sum().backward()
    assert np.array_equal(theta.grad.cpu().numpy(), H.vjp(v1, adjoint=False)["theta"])
    # set_qp_device replaces the evaluator, and an evaluator replaces it, as the host entries do
    layout = (prob.nx, prob.ne, prob.nc, 0, 0)
    d = gen(layout, B, 580)
    resq = host_solve(H, d, 0.5)
    device_solve(D, d, 0.5)
    assert_same_state(D, H, resq)
    assert "P" in D.vjp_device(x=cuda(v1[:, :prob.nx]))
    for sn in (H, D):
        sn.set_evaluator(evlib(), "cartpole_mpc_kernels", prob.np)
    with pytest.raises(pkg.CalipsoHipError, match="parameters"):
        D.solve_device()                                                              # (the parameters went with the evaluator's replacement)
    H.set_parameters(th); H.initialize(x0)
    D.set_parameters_device(cuda(th)); D.initialize_device(cuda(x0)); D.solve_device()
    assert np.array_equal(H.solve()[0], res)
    assert_same_state(D, H, res)
    for sn in (H, D, Lyr):
        sn.close()


# ---- 8. refusals that never reach the GPU ------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle():
    import test_gpu_smallnewton_evaluator as te
    pkg = load_pkg()
    layout, B = (3, 1, 2, 0, 0), 2
    sn = handle(pkg, layout, B)
    d = gen(layout, B, 590)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)
    with pytest.raises(ValueError, match="CUDA"):
        sn.set_qp_device(*[torch.tensor(d[n]) for n in NAMES])
    with pytest.raises(pkg.CalipsoHipError, match="no problem data"):
        sn.solve_device()
    with pytest.raises(pkg.CalipsoHipError, match="no problem data"):
        sn.vjp_device(cotangent=f64(B, sn.N).cuda(), qp=False)
    device_solve(sn, d, 0.5)
    for call in (lambda: sn.initialize_device(f64(B, 3)), lambda: sn.set_state_device(w=f64(B, sn.N)), lambda: sn.vjp_device(cotangent=f64(B, sn.N)),
                 lambda: sn.solution_device(out=dict(x=f64(B, 3)))):
        with pytest.raises(ValueError, match="CUDA"):
            call()
    with pytest.raises(ValueError, match="float64"):
        sn.initialize_device(f64(B, 3).cuda().float())
    with pytest.raises(ValueError, match="shape"):
        sn.initialize_device(f64(B, 4).cuda())
    with pytest.raises(ValueError, match="contiguous"):
        sn.initialize_device(f64(3, B).cuda().t())
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="handle on device"):
            sn.initialize_device(f64(B, 3).to("cuda:1"))
    # the host entry's refusals, carried over with its messages (valid device pointers: refused on the arguments alone)
    fn, last = sn._L.calipso_hip_smallnewton_differentiate_adjoint_device, lambda h: h._L.calipso_hip_smallnewton_last_error(h._h).decode()
    cot = f64(B, sn.N).cuda()
    none = None
    assert fn(sn._h, 0, ctypes.c_void_p(cot.data_ptr()), none, none, none, none, none, none, 0, 1, none) == -4 and "k >= 1" in last(sn)
    assert fn(sn._h, 1, none, none, none, none, none, none, none, 0, 1, none) == -4 and "no cotangent" in last(sn)
    with pytest.raises(pkg.CalipsoHipError, match="grad_theta"):
        sn.vjp_device(cotangent=cot, theta=True)
    with pytest.raises(pkg.CalipsoHipError, match="no evaluator"):
        sn.n_parameters = 3
        sn.set_parameters_device(f64(3).cuda())
    sn.close()
    prob = te.nonlinear_cone()
    E = pkg.SmallNewtonBatch(prob.nx, prob.ne, prob.nc, 2)
    E.set_evaluator(evlib(), "nonlinear_cone_kernels", prob.np)
    with pytest.raises(pkg.CalipsoHipError, match="parameters and none were set"):
        E.solve_device()
    E.set_stream(torch.cuda.current_stream())
    E.set_parameters_device(cuda(te.nonlinear_thetas(2)))
    with pytest.raises(pkg.CalipsoHipError, match="grad_qp"):
        E.vjp_device(cotangent=f64(2, E.N).cuda(), qp=True)
    E.close()
    E0 = pkg.SmallNewtonBatch(prob.nx, prob.ne, prob.nc, 2)
    E0.set_evaluator(evlib(), "nonlinear_cone_kernels", 0)                            # (no parameters: grad_theta is refused before any launch)
    with pytest.raises(pkg.CalipsoHipError, match="grad_theta"):
        E0.vjp_device(cotangent=f64(2, E0.N).cuda(), theta=True)
    E0.close()


def test_host_entries_keep_their_bits_on_a_borrowed_stream():
    """after set_stream the host entries run on the caller's stream and still wait for their own work: the same bits as on the handle's own stream"""
    pkg = load_pkg()
    layout, B, c = RPLUS[0], 5, 0.5
    d = gen(layout, B, 600)
    H, S = handle(pkg, layout, B, **TIGHT), handle(pkg, layout, B, **TIGHT)
    res = host_solve(H, d, c)
    stream = torch.cuda.Stream()
    S.set_stream(stream)
    assert np.array_equal(host_solve(S, d, c), res)
    assert_same_state(S, H)
    v = np.random.default_rng(1).standard_normal((B, H.N))
    a, b = S.vjp(v), H.vjp(v)
    for name in ("adjoint",) + tuple(NAMES):
        assert np.array_equal(a[name], b[name]), name
    S.set_stream(0)                                                                   # the legacy default stream (torch's default), then back to its own
    assert np.array_equal(host_solve(S, d, c), res)
    assert_same_state(S, H)
    S.set_stream(None)
    assert np.array_equal(host_solve(S, d, c), res)
    assert_same_state(S, H)
    S.close(); H.close()


# ---- 9. one data path behind the host and the device entries -----------------------------------------------------------------------------------------
# Both kinds of entry pack through k_sn_pack, so "device equals host" no longer anchors the pack by itself: the scale is pinned here, transposes and signs by the
# oracle comparisons of test_gpu_smallnewton.py and test_gpu_smallnewton_edges.py.
def set_and_solve(sn, kind, data, c):
    """the QP through the host ("host") or the device ("device") entry — arrays without a batch axis are shared —, a cold start, the solve: its statuses"""
    if kind == "host":
        sn.set_qp(*[data[n] for n in NAMES], objective_scale=c, shared=data["P"].ndim == 2)
        sn.initialize(np.zeros((sn.batch, sn.nx)))
        return sn.solve()[0]
    sn.set_qp_device(*[cuda(data[n]) for n in NAMES], objective_scale=c)
    sn.initialize_device(None)
    sn.solve_device()
    return sn.status_device().cpu().numpy()


def on_torch_stream(sn):
    sn.set_stream(torch.cuda.current_stream())
    return sn


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("kind", ["host", "device"])
def test_objective_scale_is_one_multiply_of_P(kind, shared):
    """Lxx = (2c) P is all the solve reads of P and c.  With P' = (2.0 * c) * P from numpy, 2 * 0.5 * P' = P' exactly: set_qp(P', objective_scale=0.5) must give
    the bits of set_qp(P, objective_scale=c) — the pack multiplies once, by the rounded 2c"""
    pkg = load_pkg()
    c = 0.7
    for layout in [(12, 5, 6, 0, 0), (1, 0, 0, 0, 0)]:
        B = 5
        d = gen(layout, B, 610)
        data = {n: (d[n][0] if shared else d[n]) for n in NAMES}
        scaled = dict(data, P=(2.0 * c) * data["P"])
        X, Y = on_torch_stream(handle(pkg, layout, B, **TIGHT)), on_torch_stream(handle(pkg, layout, B, **TIGHT))
        rx, ry = set_and_solve(X, kind, data, c), set_and_solve(Y, kind, scaled, 0.5)
        assert np.array_equal(rx, ry) and (rx == 1).any(), (rx, ry)
        assert_same_state(X, Y)
        X.close(); Y.close()


def test_one_handle_alternating_host_and_device_entries():
    """buffers grow and never shrink, strides change with every call: after each step the handle solves as a fresh handle given only that step's data"""
    pkg = load_pkg()
    layout, B, c = (12, 5, 6, 0, 0), 6, 0.5
    nx, m = 12, 11
    full, zero = [nx * nx, nx, m * nx, m], [0, 0, 0, 0]
    steps = [("host", "", full), ("device", "PAG", [0, nx, 0, m]), ("host", NAMES, zero), ("device", "", full), ("host", "", full)]
    sn = on_torch_stream(handle(pkg, layout, B, **TIGHT))
    for i, (kind, shared, strides) in enumerate(steps):
        d = gen(layout, B, 620 + i)
        data = {n: (d[n][0] if n in shared else d[n]) for n in NAMES}
        fresh = on_torch_stream(handle(pkg, layout, B, **TIGHT))
        res, ref = set_and_solve(sn, kind, data, c), set_and_solve(fresh, kind, data, c)
        assert np.array_equal(res, ref) and (ref == 1).any(), (i, res, ref)
        assert_same_state(sn, fresh)
        assert buffers(sn)[4:] == strides and buffers(fresh)[4:] == strides, (i, buffers(sn))
        fresh.close()
    sn.close()


def test_repeated_host_set_qp_keeps_its_buffers():
    pkg = load_pkg()
    layout, B = (12, 5, 6, 0, 0), 5
    sn = handle(pkg, layout, B, **TIGHT)
    host_solve(sn, gen(layout, B, 630), 0.5)
    first = buffers(sn)
    assert all(first[:4]) and first[4:] == [144, 12, 132, 11]
    res = host_solve(sn, gen(layout, B, 631), 0.5)
    assert buffers(sn) == first
    fresh = handle(pkg, layout, B, **TIGHT)
    assert np.array_equal(host_solve(fresh, gen(layout, B, 631), 0.5), res)
    assert_same_state(sn, fresh)
    sn.close(); fresh.close()


def test_host_set_state_with_one_argument_leaves_the_other_two():
    pkg = load_pkg()
    layout, B = (12, 5, 6, 0, 0), 5
    sn = handle(pkg, layout, B, **TIGHT)
    host_solve(sn, gen(layout, B, 640), 0.5)
    rng = np.random.default_rng(7)
    before = sn.get_state()
    assert (before["scalars"][:, 3:] != 0).any()                                      # (the regularisations the solve left: slots 3..5 hold something to lose)
    sc = np.tile([0.05, 0.995, 30.0], (B, 1)) * (1.0 + 0.1 * rng.random((B, 3)))
    sn.set_state(scalars=sc)
    after = sn.get_state()
    assert np.array_equal(after["scalars"][:, :3], sc) and np.array_equal(after["scalars"][:, 3:], before["scalars"][:, 3:])
    assert np.array_equal(after["solution"], before["solution"]) and np.array_equal(after["dual"], before["dual"])
    lam = before["dual"] + rng.standard_normal(before["dual"].shape)
    sn.set_state(dual=lam)
    third = sn.get_state()
    assert np.array_equal(third["dual"], lam) and np.array_equal(third["solution"], before["solution"]) and np.array_equal(third["scalars"], after["scalars"])
    w = before["solution"] + rng.standard_normal(before["solution"].shape)
    sn.set_state(w=w)
    last = sn.get_state()
    assert np.array_equal(last["solution"], w) and np.array_equal(last["dual"], lam) and np.array_equal(last["scalars"], after["scalars"])
    for key in before["counters"]:
        assert np.array_equal(last["counters"][key], before["counters"][key]), key
    sn.close()


def test_host_set_qp_replaces_an_evaluator_and_an_evaluator_comes_back():
    import test_gpu_smallnewton_evaluator as te
    pkg = load_pkg()
    prob = te.nonlinear_cone()
    B = 5
    th = te.nonlinear_thetas(B)
    E, ref = te.make(pkg, prob, "nonlinear_cone_kernels", th), te.make(pkg, prob, "nonlinear_cone_kernels", th)
    res_ev = ref.solve()[0]
    assert (res_ev == 1).all() and np.array_equal(E.solve()[0], res_ev)
    layout = (prob.nx, prob.ne, prob.nc, 0, 0)
    d = gen(layout, B, 650)
    Q = handle(pkg, layout, B)
    res = host_solve(Q, d, 0.5)
    assert np.array_equal(host_solve(E, d, 0.5), res) and (res == 1).any()           # the QP on the handle that held the evaluator
    assert_same_state(E, Q)
    assert "P" in E.vjp(np.ones((B, E.N)))
    with pytest.raises(pkg.CalipsoHipError, match="calipso_hip_smallnewton_set_parameters: no evaluator"):
        E.set_parameters(th)
    E.set_evaluator(evlib(), "nonlinear_cone_kernels", prob.np)
    E.initialize(np.repeat(prob.x0[None], B, axis=0))
    with pytest.raises(pkg.CalipsoHipError, match="parameters and none were set"):
        E.solve()                                                                     # (the parameters went with the first evaluator)
    E.set_parameters(th)
    assert np.array_equal(E.solve()[0], res_ev)
    assert_same_state(E, ref)
    for sn in (E, ref, Q):
        sn.close()
