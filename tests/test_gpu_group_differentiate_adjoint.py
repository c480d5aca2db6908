"""differentiate! in reverse mode for a group in lockstep (calipso_hip_group_differentiate_adjoint, csrc/group.hip + the group pass of csrc/columns.hip + the batched
GEMM of csrc/gemm.hip + the instance dimension of the kernels of csrc/adjoint.hip / csrc/soc_wide.hip) and torch_layer.GroupQPLayer: Group.vjp against the ORACLE's
forward maps per member (the transposed map at interior points, every cone branch; grad_theta = S' v at solutions), against Solver.vjp on twin handles (more than one
solve block, the QP data gradients), and the properties of a group call (no cross-talk, member order, repetition, coexistence with the other entries, refusals).

Bounds: those of test_gpu_differentiate_adjoint.py.  Against the oracle 1e-8 relative to max(1, |M|), and for S' v the forward's entrywise bound carried through the
contraction, 1e-8 max(1, |S|) ||v||_1.  Between two of our own paths 1e-8 relative to max(1, |reference|)."""
import warnings

import numpy as np
import pytest

import problems as pr
from helpers import SHAPE_L, SHAPE_S, interior_point, load_pkg, make_oracle, make_pair
from test_gpu_differentiate_adjoint import LAYOUTS, QP_SHAPE, interior_state, qp_handle
from test_gpu_differentiate_refined import handle_point, pair_at_solution
from test_gpu_group import build, same

pytestmark = pytest.mark.gpu

QP_NAMES = "PqAbGh"


def member_scalars(i):
    """different kappa, rho, ep, ed per member: a launch that read another member's row of the scalar table would be off by order one"""
    return dict(kappa=0.17 + 0.05 * i, rho=52.0 + 7.0 * i, ep=0.05 + 0.01 * i, ed=0.03 + 0.01 * i)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_transposed_map_against_the_oracles_forward_map_per_member(oracle_mod, layout):
    pkg = load_pkg()
    nx, ne, nnn, nsoc, sdim = layout
    pairs = []
    for i in range(3):
        prob = pr.parametric_conic_qp(nx, ne, nnn, nsoc, sdim, seed=900 + nx + 17 * i)
        pt, lam = interior_point(prob, seed=5 + i, tail=0.05 if sdim > 16 else 0.3)
        o, g = make_pair(oracle_mod, prob, pt, lam, **member_scalars(i))
        o.cone(product=True, jacobian=True, target=True)
        g.cone(product=True, jacobian=True, target=True)
        o.residual_jacobian_variables(); o.residual_jacobian_variables_symmetric()
        pairs.append((o, g))
    N = pairs[0][0].N
    grp = pkg.Group([g for _, g in pairs])
    out = grp.vjp(np.broadcast_to(np.eye(N), (3, N, N)), theta=False)      # ONE call, k = N unit cotangents per member: column j = M_i' e_j
    assert out["adjoint"].shape == (3, N, N) and not out["status"].any()
    for i, (o, g) in enumerate(pairs):
        M = np.zeros((N, N))
        for j in range(N):                                   # M_i column by column, factored once
            o.buf("residual")[:] = 0.0
            o.buf("residual")[j] = 1.0
            o.search_direction_symmetric(0, fact=(j == 0))
            M[:, j] = o.buf("step")
        err = np.abs(out["adjoint"][i] - M.T).max()
        print("%s member %d: N = %d, |M| = %.2e, |Lambda - M'| = %.2e" % (layout, i, N, np.abs(M).max(), err))
        assert err <= 1e-8 * max(1.0, np.abs(M).max())
        assert g.vjp_info() == dict(columns=N, rounds=0, failed_columns=0, final_norm=0.0)
    grp.close()


@pytest.mark.parametrize("names", [("qp12_5_6_s300", "qp12_5_6_s301"), ("cartpole",)])
def test_grad_theta_against_the_oracles_sensitivities(oracle_mod, names):
    pkg = load_pkg()
    trio = [pair_at_solution(oracle_mod, name) for name in names]       # host callbacks: the parameter Jacobians come one member after the other
    grp = pkg.Group([g for _, _, g in trio])
    N = trio[0][1].N
    V = np.stack([np.random.default_rng(17 + i).standard_normal((N, 3)) for i in range(len(trio))])
    out = grp.vjp(V)
    assert out["adjoint"].shape == (len(trio), N, 3) and not out["status"].any()
    for i, (prob, o, g) in enumerate(trio):
        S_cpu = o.mat("solution_sensitivity", o.N, prob.np)
        want = S_cpu.T @ V[i]
        assert out["theta"][i].shape == (prob.np, 3)
        for j in range(3):
            err, bound = np.abs(out["theta"][i][:, j] - want[:, j]).max(), 1e-8 * max(1.0, np.abs(S_cpu).max()) * np.abs(V[i][:, j]).sum()
            print("%s column %d: |S| = %.2e, |theta - S'v| = %.2e, bound %.2e" % (names[i], j, np.abs(S_cpu).max(), err, bound))
            assert err <= bound, (names[i], j, err, bound)
    grp.close()


def close(a, ref):
    return np.abs(a - ref).max() <= 1e-8 * max(1.0, np.abs(ref).max())


# (shape, problem ids, opt.solve_block, padded nx, solve blocks).  nx pads to a power of two up to 512 and to a multiple of 512 beyond, so nx = 600 gives NP = 1024: with solve blocks of
# 512 (what a group wants, internal.hpp) two equal blocks, the forward and backward update products of the schedule both live; SHAPE_L (NP = 1536) under the default
# limit a 1024-wide block and a narrower last one
BLOCKED = [((600, 100, 40, 10, 3), [41, 42, 43], 512, 1024, "512 + 512"), (SHAPE_L, [41, 42], 1024, 1536, "1024 + 512")]


@pytest.mark.parametrize("shape,ids,solve_block,padded,blocks", BLOCKED)
def test_more_than_one_solve_block_against_twin_handles(shape, ids, solve_block, padded, blocks):
    pkg = load_pkg()
    twins = [build(pkg, p, shape=shape) for p in ids]
    members = [build(pkg, p, shape=shape) for p in ids]
    for h in twins + members:
        h.set_option("solve_block", solve_block)
    assert members[0].padded_nx() == padded
    grp = pkg.Group(members)
    grp.newton_step(advance=True)
    for t in twins:
        t.newton_step(advance=True)
    N = members[0].N
    for k in (1, 17):
        V = np.random.default_rng(50 + k).standard_normal((len(ids), N, k))
        out = grp.vjp(V[:, :, 0] if k == 1 else V, theta=False, qp=True)
        assert not out["status"].any()
        for i, t in enumerate(twins):
            ref = t.vjp(V[i][:, 0] if k == 1 else V[i], theta=False, qp=True)
            for name in ("adjoint",) + tuple(QP_NAMES):
                assert out[name][i].shape == ref[name].shape, name
                assert close(out[name][i], ref[name]), (k, i, name, np.abs(out[name][i] - ref[name]).max(), np.abs(ref[name]).max())
            gP = out["P"][i]
            assert np.array_equal(gP, np.swapaxes(gP, 0, 1))
    grp.close()


def test_no_cross_talk_and_member_order():
    pkg = load_pkg()
    ids = [3, 4, 5, 6]
    members = [build(pkg, p, shape=SHAPE_S) for p in ids]
    N = members[0].N
    V = np.random.default_rng(61).standard_normal((4, N, 2))
    V[2] = 0.0
    grp = pkg.Group(members)
    out = grp.vjp(V, theta=False, qp=True)
    for name in ("adjoint",) + tuple(QP_NAMES):
        assert not out[name][2].any(), name                      # exactly zero
        for i in (0, 1, 3):
            assert np.abs(out[name][i]).max() > 0.0, (name, i)
    grp.close()
    order = [2, 0, 3, 1]                                          # the same problems as another member list: results land in member order
    again = [build(pkg, ids[j], shape=SHAPE_S) for j in order]
    grp2 = pkg.Group(again)
    out2 = grp2.vjp(V[order], theta=False, qp=True)
    for name in ("adjoint",) + tuple(QP_NAMES):
        for pos, j in enumerate(order):
            assert same(out2[name][pos], out[name][j]), (name, pos, j)
    grp2.close()


def test_repetition_and_coexistence_with_the_other_entries():
    pkg = load_pkg()
    ids = [11, 12, 13]
    twins = [build(pkg, p, shape=SHAPE_S) for p in ids]
    members = [build(pkg, p, shape=SHAPE_S) for p in ids]
    grp = pkg.Group(members)
    N = members[0].N
    V = np.random.default_rng(71).standard_normal((3, N, 3))
    before = grp.newton_step(advance=False)
    first = grp.vjp(V, theta=False, qp=True)
    second = grp.vjp(V, theta=False, qp=True)
    for name in first:
        assert same(first[name], second[name]), name
    assert grp.vjp_ms() > 0.0
    after = grp.newton_step(advance=False)
    assert before == after
    for t in twins:                                               # the twins in the members' state: the same step, not advanced
        t.newton_step(advance=False)
    for i, (m, t) in enumerate(zip(members, twins)):              # a member's own reverse call (its own workspace, the single-handle kernels as a batch of one)
        a, b = m.vjp(V[i], theta=False, qp=True), t.vjp(V[i], theta=False, qp=True)
        for name in a:
            assert same(a[name], b[name]), (i, name)
        assert close(first["adjoint"][i], a["adjoint"])
    grp.close()


def test_refusals_name_the_cause(oracle_mod):
    pkg = load_pkg()
    prob, pt, lam, sc = interior_state()
    qps = [qp_handle(pkg, prob, pt, lam, sc) for _ in range(2)]          # np = 0, QP attached
    par = []
    for _ in range(2):                                                   # parameters, no QP
        _, g = make_pair(oracle_mod, prob, pt, lam, **sc)
        g.cone(product=True, jacobian=True, target=True)
        par.append(g)
    gq, gp = pkg.Group(qps), pkg.Group(par)
    N = qps[0].N
    v = np.ones((2, N))
    calls = [(lambda: gp.vjp(np.zeros((2, N, 0))), "k must be"), (lambda: gp.vjp(None), "cotangent"), (lambda: gq.vjp(v, theta=True), "grad_theta"),
             (lambda: gp.vjp(v, qp=True), "grad_qp")]
    for call, word in calls:
        with pytest.raises(pkg.CalipsoHipError) as e:
            call()
        assert word in str(e.value), (word, str(e.value))
    assert gp.vjp(v)["theta"].shape == (2, prob.np)                     # a refused call leaves the group usable
    ok = gq.vjp(v, qp=True)
    qps[1].set_option("differentiate_refinement", 1)
    with pytest.raises(pkg.CalipsoHipError) as e:
        gq.vjp(v, qp=True)
    assert "member 1" in str(e.value) and "differentiate_refinement" in str(e.value), str(e.value)
    qps[1].set_option("differentiate_refinement", 0)
    qps[0].analyze_structure()
    with pytest.raises(pkg.CalipsoHipError) as e:
        gq.vjp(v, qp=True)
    assert "member 0" in str(e.value) and "structure" in str(e.value), str(e.value)
    qps[0].clear_structure()
    again = gq.vjp(v, qp=True)                                           # the next valid call succeeds, with the bits of the one before
    for name in ok:
        assert same(ok[name], again[name]), name
    gq.close(); gp.close()


def test_group_qp_layer(oracle_mod):
    import torch
    pkg = load_pkg()
    from calipso_jl_amd.torch_layer import GroupQPLayer
    probs = [pr.parametric_conic_qp(*QP_SHAPE, seed=300 + i) for i in range(3)]
    hs = [pkg.Solver(p, p.nx, 0, p.ne, p.nc, nonnegative_indices=p.nonnegative_indices, second_order_indices=p.second_order_indices) for p in probs]
    grp = pkg.Group(hs)
    nx, c0 = probs[0].nx, probs[0].c
    stacked = lambda k: np.stack([np.asarray(getattr(p, k)) for p in probs])
    leaves = lambda arrays: {k: torch.tensor(a, dtype=torch.float64, requires_grad=True) for k, a in arrays.items()}
    C = np.random.default_rng(31).standard_normal((3, nx))
    T = leaves({k: stacked(k) for k in QP_NAMES})
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                   # every solve converges: no warning, no NaN
        x = GroupQPLayer.apply(grp, *[T[k] for k in QP_NAMES], False, c0)
        (torch.from_numpy(C) * x).sum().backward()
    assert x.shape == (3, nx) and all(T[k].grad is not None and T[k].grad.shape == T[k].shape for k in QP_NAMES)
    for i, (prob, h) in enumerate(zip(probs, hs)):                       # the oracle differentiated at the member's own point and fields
        pt, lam, sc = handle_point(h)
        o = make_oracle(oracle_mod, prob, pt, lam, **sc)
        o.buf("parameters")[:] = prob.parameters
        o.buf("objective_jacobian_variables_variables")[:] = h.get("lagrangian_hessian", prob.nx * prob.nx)
        o.buf("equality_dual_jacobian_variables_variables")[:] = 0.0
        o.buf("cone_dual_jacobian_variables_variables")[:] = 0.0
        o.buf("equality_jacobian_variables")[:] = h.get("equality_jacobian_variables", prob.ne * prob.nx)
        o.cone(product=True, jacobian=True, target=True)
        assert o.differentiate(prob) >= 0
        S_cpu = o.mat("solution_sensitivity", o.N, prob.np)
        v = np.zeros(o.N); v[:nx] = C[i]
        want = S_cpu.T @ v                                               # theta = [dq; db; dh] moves q, b, h themselves
        bound = 1e-8 * max(1.0, np.abs(S_cpu).max()) * np.abs(v).sum()
        got = np.concatenate([T[k].grad[i].numpy() for k in "qbh"])
        print("GroupQPLayer member %d: |[grad q; b; h] - S'v| = %.2e, bound %.2e, |S| = %.2e" % (i, np.abs(got - want).max(), bound, np.abs(S_cpu).max()))
        assert np.abs(got - want).max() <= bound
        gP = T["P"].grad[i].numpy()
        assert np.array_equal(gP, gP.T)
    # a shared P: its gradient is the member-order sum of the per-member gradients of the run that gives every member that P as its own
    P0 = np.asarray(probs[0].P)
    rest = {k: stacked(k) for k in "qAbGh"}
    Tb = leaves(dict(P=np.stack([P0] * 3), **rest))
    Ts = leaves(dict(P=P0, **rest))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for U in (Tb, Ts):
            (torch.from_numpy(C) * GroupQPLayer.apply(grp, *[U[k] for k in QP_NAMES], False, c0)).sum().backward()
    acc = Tb["P"].grad[0].numpy().copy()
    for i in (1, 2):
        acc += Tb["P"].grad[i].numpy()
    assert Ts["P"].grad.shape == (nx, nx) and np.abs(acc).max() > 0.0
    assert np.array_equal(Ts["P"].grad.numpy(), acc)
    assert np.array_equal(Ts["q"].grad.numpy(), Tb["q"].grad.numpy())
    # the cotangents of the duals reach the backward pass
    Td = leaves(dict(P=P0, **rest))
    rng = np.random.default_rng(32)
    Cy, Cz = rng.standard_normal((3, probs[0].ne)), rng.standard_normal((3, probs[0].nc))
    x, y, z = GroupQPLayer.apply(grp, *[Td[k] for k in QP_NAMES], True, c0)
    ((torch.from_numpy(C) * x).sum() + (torch.from_numpy(Cy) * y).sum() + (torch.from_numpy(Cz) * z).sum()).backward()
    ne, nc, N = probs[0].ne, probs[0].nc, hs[0].N
    v = np.zeros((3, N))
    v[:, :nx] = C; v[:, nx + ne + nc:nx + 2 * ne + nc] = Cy; v[:, nx + 2 * ne + nc:nx + 2 * ne + 2 * nc] = Cz
    direct = grp.vjp(v, adjoint=False, theta=False, qp="qh")              # the same state, the same bits as the backward pass saw
    assert np.array_equal(Td["q"].grad.numpy(), direct["q"]) and np.array_equal(Td["h"].grad.numpy(), direct["h"])
    only_x = np.zeros((3, N)); only_x[:, :nx] = C
    assert not np.array_equal(grp.vjp(only_x, adjoint=False, theta=False, qp="q")["q"], direct["q"])
    grp.close()
