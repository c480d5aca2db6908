"""differentiate! in forward mode for a group in lockstep (calipso_hip_group_differentiate, csrc/group.hip + the group pass of csrc/columns.hip + the instance dimension
of the multi-column k_residual_symmetric / k_recover of csrc/vectors.hip and csrc/soc_wide.hip + the two forms of the batched GEMM of csrc/gemm.hip): Group.differentiate
against the ORACLE's differentiate! per member (every cone branch at interior points, at solutions, at the edges of both GEMM tiles), against Solver.differentiate on
twin handles (more than one solve block), and the properties of a group call (no cross-talk, member order, repetition, coexistence with the other entries, refusals).

Bounds: against the oracle that of test_gpu_multirhs.py, |S_gpu - S_cpu| <= 1e-8 max(1, |S_cpu|); between two of our own paths 1e-8 relative to max(1, |reference|);
S' v against Group.vjp with the reverse test's bound, 1e-8 max(1, |S|) ||v||_1.  The 16- and the 64-column form of the batched GEMM feed every element of C the same chain
of MFMAs, so they are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import problems as pr
from helpers import SHAPE_S, interior_point, load_pkg, make_pair
from test_gpu_differentiate_adjoint import LAYOUTS, interior_state, qp_handle
from test_gpu_differentiate_refined import pair_at_solution
from test_gpu_group import build, same
from test_gpu_group_differentiate_adjoint import member_scalars

pytestmark = pytest.mark.gpu

CALIPSO_ERR_ARGUMENT = -4
SCALAR_FIELDS = (("central_path", "kappa"), ("penalty", "rho"), ("primal_regularization", "ep"), ("dual_regularization", "ed"), ("fraction_to_boundary", "tau"))
PARAMETER_FLAGS = (pr.OBJECTIVE_JACOBIAN_PARAMETERS | pr.EQUALITY_JACOBIAN_PARAMETERS | pr.EQUALITY_DUAL_JACOBIAN_PARAMETERS | pr.CONE_JACOBIAN_PARAMETERS |
                   pr.CONE_DUAL_JACOBIAN_PARAMETERS)


def close(a, ref):
    return np.abs(a - ref).max() <= 1e-8 * max(1.0, np.abs(ref).max())


def pair(oracle_mod, prob, seed, tail=0.3, **sc):
    """(oracle, handle) at an interior point of prob, cone Jacobians formed on both sides (differentiate! uses those of the last cone! call)"""
    pt, lam = interior_point(prob, seed=seed, tail=tail)
    o, g = make_pair(oracle_mod, prob, pt, lam, **sc)
    o.cone(product=True, jacobian=True, target=True)
    g.cone(product=True, jacobian=True, target=True)
    return o, g


def handle(pkg, prob, seed, attach=False, kappa=0.17, rho=52.0, ep=0.12, ed=0.21, tau=0.99):
    """the handle of helpers.make_pair without its oracle (host callbacks); attach: the QP's data attached as well — a device evaluator, which leaves the (constant)
    parameter Jacobians the callback uploaded where they are"""
    pt, lam = interior_point(prob, seed=seed)
    g = pkg.Solver(prob, prob.nx, prob.np, prob.ne, prob.nc, parameters=prob.parameters, nonnegative_indices=prob.nonnegative_indices,
                   second_order_indices=prob.second_order_indices)
    sc = dict(kappa=kappa, rho=rho, ep=ep, ed=ed, tau=tau)
    for field, kw in SCALAR_FIELDS:
        g.set(field, [sc[kw]])
    g.set("solution", np.concatenate([pt[k] for k in "xrsyzt"]))
    if prob.ne:
        g.set("dual", lam)
    g.evaluate(pr.ALL_VARIABLE_FLAGS | (PARAMETER_FLAGS if attach else 0), 0)
    if attach:
        g.qp_attach(prob.P, prob.q, prob.A, prob.b, prob.G, prob.h, prob.c)
        g.qp_evaluate(pr.ALL_VARIABLE_FLAGS, 0)
    g.cone(product=True, jacobian=True, target=True)
    return g


def check_members_against_oracle(prob_of, pairs, out, what):
    assert not out["status"].any()
    for i, (o, g) in enumerate(pairs):
        prob = prob_of(i)
        assert o.differentiate(prob) >= 0
        S_cpu = o.mat("solution_sensitivity", o.N, prob.np)
        S = out["sensitivity"][i]
        assert S.shape == (o.N, prob.np)
        err, scale = np.abs(S - S_cpu).max(), max(1.0, np.abs(S_cpu).max())
        print("%s member %d: N = %d, np = %d, |S| = %.2e, |S_gpu - S_cpu| = %.2e" % (what, i, o.N, prob.np, np.abs(S_cpu).max(), err))
        assert err <= 1e-8 * scale, (what, i, err, scale)
        assert same(g.data("solution_sensitivity"), S)
        assert g.differentiate_info() == dict(columns=prob.np, rounds=0, failed_columns=0, final_norm=0.0)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_cone_branch_against_the_oracle_per_member(oracle_mod, layout):
    pkg = load_pkg()
    nx, ne, nnn, nsoc, sdim = layout
    probs = [pr.parametric_conic_qp(nx, ne, nnn, nsoc, sdim, seed=900 + nx + 17 * i) for i in range(3)]
    pairs = [pair(oracle_mod, probs[i], 5 + i, tail=0.05 if sdim > 16 else 0.3, **member_scalars(i)) for i in range(3)]
    grp = pkg.Group([g for _, g in pairs])
    out = grp.differentiate()                                            # ONE call
    assert out["sensitivity"].shape == (3, pairs[0][0].N, probs[0].np) and out["status"].shape == (3,)
    check_members_against_oracle(lambda i: probs[i], pairs, out, str(layout))
    grp.close()


@pytest.mark.parametrize("names", [("qp12_5_6_s300", "qp12_5_6_s301"), ("cartpole",)])
def test_at_solutions_against_the_oracle(oracle_mod, names):
    pkg = load_pkg()
    trio = [pair_at_solution(oracle_mod, name) for name in names]       # host callbacks; the oracle is differentiated already
    grp = pkg.Group([g for _, _, g in trio])
    out = grp.differentiate()
    assert not out["status"].any()
    for i, (prob, o, g) in enumerate(trio):
        S_cpu = o.mat("solution_sensitivity", o.N, prob.np)
        err, scale = np.abs(out["sensitivity"][i] - S_cpu).max(), max(1.0, np.abs(S_cpu).max())
        print("%s: np = %d, |S| = %.2e, |S_gpu - S_cpu| = %.2e" % (names[i], prob.np, np.abs(S_cpu).max(), err))
        assert err <= 1e-8 * scale, (names[i], err, scale)
        assert same(g.data("solution_sensitivity"), out["sensitivity"][i])
    grp.close()


# np = 1: one column; np = 61: one ragged 64-column tile, four 16-column tiles with the last ragged; np = 111 = 64 + 47 with N = 173, m = 41, NP = 128: ragged in
# rows, columns and K
EDGES = {"np1": lambda i: pr.one_parameter_conic_qp_dims(14, 6, 4, [3, 3], seed=40 + i), "np61": lambda i: pr.parametric_conic_qp(40, 12, 9, 0, 3, seed=40 + i),
         "np111": lambda i: pr.parametric_conic_qp(70, 20, 6, 5, 3, seed=70 + i)}


@pytest.mark.parametrize("case,columns", [("np1", 1), ("np61", 61), ("np111", 111)])
def test_column_counts_at_the_edges_of_both_tiles_give_the_same_bits(oracle_mod, case, columns):
    pkg = load_pkg()
    probs = [EDGES[case](i) for i in range(3)]
    assert probs[0].np == columns
    pairs = [pair(oracle_mod, probs[i], 3 + i, kappa=0.17 + 0.05 * i, rho=52.0 + 7.0 * i, ep=1e-5, ed=1e-5) for i in range(3)]
    grp = pkg.Group([g for _, g in pairs])
    narrow, wide, chosen = grp.differentiate(tile=16), grp.differentiate(tile=64), grp.differentiate(tile=0)
    assert np.array_equal(narrow["sensitivity"], wide["sensitivity"])
    assert np.array_equal(chosen["sensitivity"], narrow["sensitivity"])
    check_members_against_oracle(lambda i: probs[i], pairs, chosen, case)
    grp.close()


def test_more_than_one_solve_block_against_twin_handles():
    """nx = 600 pads to NP = 1024: with solve blocks of 512 two equal blocks, the forward and the backward update product of trsm_multi both live; np = 770"""
    pkg = load_pkg()
    shape = (600, 100, 40, 10, 3)
    probs = [pr.parametric_conic_qp(*shape, seed=41 + i) for i in range(2)]
    sc = [dict(kappa=0.17 + 0.05 * i, rho=52.0 + 7.0 * i, ep=1e-5, ed=1e-5) for i in range(2)]
    twins = [handle(pkg, probs[i], 3 + i, **sc[i]) for i in range(2)]
    members = [handle(pkg, probs[i], 3 + i, **sc[i]) for i in range(2)]
    for h in twins + members:
        h.set_option("solve_block", 512)
    assert members[0].padded_nx() == 1024 and members[0].np == 770 and members[0].N == 1010
    grp = pkg.Group(members)
    out = grp.differentiate()
    assert not out["status"].any()
    for i, t in enumerate(twins):
        t.differentiate()
        ref = t.data("solution_sensitivity")
        print("member %d: |S| = %.2e, |group - twin| = %.2e" % (i, np.abs(ref).max(), np.abs(out["sensitivity"][i] - ref).max()))
        assert close(out["sensitivity"][i], ref)
    grp.close()


class FrozenParameters(pr.ParametricConicQP):
    """the same QP with parameters that move nothing: every parameter Jacobian zero, so dR/dtheta = 0"""

    def evaluate(self, flags, x, y, z, theta, out):
        super().evaluate(flags, x, y, z, theta, out)
        for bit, name, rows in ((pr.OBJECTIVE_JACOBIAN_PARAMETERS, "objective_jacobian_variables_parameters", self.nx),
                                (pr.EQUALITY_JACOBIAN_PARAMETERS, "equality_jacobian_parameters", self.ne), (pr.CONE_JACOBIAN_PARAMETERS, "cone_jacobian_parameters", self.nc)):
            if flags & bit and rows:
                pr._put(out, name, np.zeros((rows, self.np)))


def shape_s_problem(pid, frozen=False):
    p = pr.parametric_conic_qp(*SHAPE_S, seed=500 + pid)
    if frozen:
        p = FrozenParameters(p.P, p.q, p.A, p.b, p.G, p.h, nonnegative_indices=p.nonnegative_indices, second_order_indices=p.second_order_indices, name="frozen")
    return p


def test_no_cross_talk_and_member_order():
    pkg = load_pkg()
    ids = [3, 4, 5, 6]
    make = lambda j: handle(pkg, shape_s_problem(ids[j], frozen=(j == 2)), 10 + j, **member_scalars(j))
    grp = pkg.Group([make(j) for j in range(4)])
    out = grp.differentiate()
    assert not out["sensitivity"][2].any()                                # exactly zero
    for i in (0, 1, 3):
        assert np.abs(out["sensitivity"][i]).max() > 0.0, i
    grp.close()
    order = [2, 0, 3, 1]                                                  # the same problems as another member list: results land in member order
    grp2 = pkg.Group([make(j) for j in order])
    out2 = grp2.differentiate()
    for pos, j in enumerate(order):
        assert same(out2["sensitivity"][pos], out["sensitivity"][j]), (pos, j)
    grp2.close()


def test_repetition_and_coexistence_with_the_other_entries():
    pkg = load_pkg()
    ids = [11, 12, 13]
    make = lambda j: handle(pkg, shape_s_problem(ids[j]), 20 + j, attach=True, **member_scalars(j))      # device evaluators: the group can step them
    twins, members = [make(j) for j in range(3)], [make(j) for j in range(3)]
    grp = pkg.Group(members)
    N, npar = members[0].N, members[0].np
    V = np.random.default_rng(71).standard_normal((3, N, 3))
    before = grp.newton_step(advance=False)
    vjp_before = grp.vjp(V)
    first = grp.differentiate()
    bytes_first = members[0].device_bytes()
    second = grp.differentiate()
    assert same(first["sensitivity"], second["sensitivity"]) and same(first["status"], second["status"])
    assert members[0].device_bytes() == bytes_first                      # the workspace is kept: a repeated call allocates nothing
    ms = grp.differentiate_ms()
    assert ms[0] >= ms[1] > 0.0
    vjp_after = grp.vjp(V)
    for name in vjp_before:
        assert same(vjp_before[name], vjp_after[name]), name             # the forward and the reverse workspace do not disturb each other
    for i in range(3):                                                    # S_i' V_i, the reverse test's bound
        S = first["sensitivity"][i]
        assert S.shape == (N, npar)
        want = S.T @ V[i]
        for j in range(3):
            err, bound = np.abs(vjp_after["theta"][i][:, j] - want[:, j]).max(), 1e-8 * max(1.0, np.abs(S).max()) * np.abs(V[i][:, j]).sum()
            assert err <= bound, (i, j, err, bound)
    after = grp.newton_step(advance=False)
    assert before == after
    for t in twins:                                                       # the twins in the members' state: the same step, not advanced
        t.newton_step(advance=False)
    for i, (m, t) in enumerate(zip(members, twins)):                      # a member's own call (its own workspace, the same kernels as a batch of one)
        m.differentiate(); t.differentiate()
        assert same(m.data("solution_sensitivity"), t.data("solution_sensitivity")), i
        assert close(first["sensitivity"][i], m.data("solution_sensitivity"))
    grp.close()


def last_error(pkg, h):
    return h._L.calipso_hip_last_error(h._h).decode()


def test_refusals_name_the_cause(oracle_mod):
    pkg = load_pkg()
    prob, pt, lam, sc = interior_state()
    par = []
    for _ in range(2):
        _, g = make_pair(oracle_mod, prob, pt, lam, **sc)
        g.cone(product=True, jacobian=True, target=True)
        par.append(g)
    gp = pkg.Group(par)
    L = gp._L
    ok = gp.differentiate()
    status = (C.c_int32 * 2)()
    assert L.calipso_hip_group_differentiate(None, None, status, 0, None) == CALIPSO_ERR_ARGUMENT                 # a NULL group
    assert L.calipso_hip_group_differentiate(gp._g, None, None, 0, None) == CALIPSO_ERR_ARGUMENT                  # a NULL status
    assert "status" in last_error(pkg, par[0])
    for tile in (7, 32, -16):
        with pytest.raises(pkg.CalipsoHipError) as e:
            gp.differentiate(tile=tile)
        assert "tile" in str(e.value), str(e.value)
    par[1].set_option("differentiate_refinement", 1)
    with pytest.raises(pkg.CalipsoHipError) as e:
        gp.differentiate()
    assert "member 1" in str(e.value) and "differentiate_refinement" in str(e.value), str(e.value)
    par[1].set_option("differentiate_refinement", 0)
    par[0].analyze_structure()
    with pytest.raises(pkg.CalipsoHipError) as e:
        gp.differentiate()
    assert "member 0" in str(e.value) and "structure" in str(e.value), str(e.value)
    par[0].clear_structure()
    L.calipso_hip_group_set_evaluators(gp._g, None, None)                 # no callback and no device evaluator on any member
    assert L.calipso_hip_group_differentiate(gp._g, None, status, 0, None) == CALIPSO_ERR_ARGUMENT
    assert "member 0" in last_error(pkg, par[0]) and "evaluator" in last_error(pkg, par[0]), last_error(pkg, par[0])
    again = gp.differentiate()                                            # the next valid call succeeds, with the bits of the one before
    assert same(ok["sensitivity"], again["sensitivity"]) and not again["status"].any()
    gp.close()
    qps = [qp_handle(pkg, prob, pt, lam, sc) for _ in range(2)]          # np = 0
    gq = pkg.Group(qps)
    with pytest.raises(pkg.CalipsoHipError) as e:
        gq.differentiate()
    assert "np = 0" in str(e.value), str(e.value)
    assert all(i["status"] >= 0 for i in gq.newton_step(advance=False))  # the group stays usable
    gq.close()
    dead = [build(pkg, p, shape=SHAPE_S) for p in (3, 4)]                # a dead group: its members were destroyed first
    gd = pkg.Group(dead)
    for s in dead:
        s._L.calipso_hip_destroy(s._h)
        s._h = C.c_void_p()
    assert L.calipso_hip_group_differentiate(gd._g, None, status, 0, None) == CALIPSO_ERR_ARGUMENT
    gd.close()
