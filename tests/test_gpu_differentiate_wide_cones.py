"""differentiate! in both directions through WIDE second-order cones (dimension > 4: one wavefront per cone, csrc/soc_wide.hip) with more than one column: the forward
pass (calipso_hip_differentiate -> launch_residual_symmetric_multi / launch_recover_multi -> k_residual_symmetric_wide / k_recover_wide with the column in blockIdx.y),
the reverse pass on a handle (calipso_hip_differentiate_adjoint -> k_recover_t_wide / k_residual_symmetric_t_wide) and on a group in lockstep
(calipso_hip_group_differentiate_adjoint: the member in blockIdx.z, column_shift), at the layouts of wide_cone_cases.LAYOUTS — every value of the kernels' template
parameter E (elements per lane: 1, 2, 4, 8, 16), the block of a cone in LDS and in the cone scratch, a wavefront exactly full (64) and two (128), a narrow wide cone and a
register cone under a larger E, two wide cones in one handle, no equalities, no nonnegative rows.

References: the oracle (differentiate!, search_direction_symmetric! column by column) and test_smallnewton_adjoint_cpu's Condensed, which
tests/test_differentiate_wide_cones_cpu.py pins to the oracle on the same layouts, points and scalars to 6e-15 — it stands in where the oracle's column loop is too slow
(layout F, dimension 513: 528 columns) and gives the transposed map directly.

Bounds.  Against a reference 1e-8 max(1, max|reference array|), the project's step tolerance against the oracle (test_gpu_multirhs.py, test_gpu_differentiate_adjoint.py,
test_gpu_shapes.py up to dimension 1024); for grad_theta the forward's entrywise bound carried through the contraction, 1e-8 max(1, |S|) ||v||_1.  The references' own
error is at most 6e-15, so the bound is the project's, not the reference's; it is NOT fitted to what the kernels deliver — they sit seven orders below it.

Measured on an MI355X (worst |got - reference| / max(1, max|reference|) per layout and direction; "oracle / Condensed" where both references exist):
  layout                    N     forward (p columns)             forward p = 1        reverse (k columns)          reverse k = 1: Condensed / column 0 of k = 17
  A (12,3,2,[64])           216   p = 81   1.6e-15 / 1.1e-15                           k = 216  1.1e-15             2.3e-16 / 6.8e-16
  B (12,3,2,[65])           219   p = 82   1.1e-15 / 7.9e-16      8.0e-16 / 1.2e-15    k = 219  7.9e-16             7.2e-16 / 8.6e-16
  C (14,4,3,[128,5])        430   p = 154  2.6e-16 / 2.6e-16                           k = 430  2.6e-16             6.3e-16 / 2.7e-16
  D (14,4,3,[129,3,70])     637   p = 223  4.8e-16 / 3.6e-16      1.3e-15 / 8.8e-16    k = 637  4.8e-16 / 3.6e-16   8.2e-16 / 8.2e-16
  E (12,3,2,[257])          795   p = 274  3.1e-16 / 3.1e-16                           k = 17   1.1e-15             5.1e-16 / 2.2e-16
  F (12,3,0,[513])          1557  p = 528  - / 5.1e-16                                 k = 17   6.5e-16             1.3e-15 / 3.8e-16
  G (10,0,0,[5,6])          43    p = 21   4.4e-16 / 3.3e-16                           k = 43   4.4e-16             2.4e-16 / 1.2e-16
F's three columns against the oracle's search_direction_symmetric!: 6.9e-17, 1.2e-16, 6.2e-16.  grad_theta on E and F (k = 17): 3.6e-18 and 1.5e-18 of
max(1, |S|) ||v||_1.  Groups of three (k = 17): D 4.1e-16 / 0 / 8.6e-16, E 1.1e-15 / 0 / 8.9e-16 against Condensed per member, and every member's columns are the bits of
Solver.vjp on a twin handle.  The whole file takes 6 s; the longest tests are F's (forward 1.2 s, one column 1.0 s with its two calls, k = 17 0.5 s): about half a second per
differentiate / vjp call, the d^3 factorisation of the 513-cone's block on one wavefront, plus the numpy reference columns, computed once.

Shown to bite on scratch builds with one in-bounds mistake each (csrc/soc_wide.hip), the rest of the suite run against the same builds:
  t1 without its blockIdx.y * d.m column offset in k_residual_symmetric_wide: the forward tests of all seven layouts fail (p = 1 passes, as it must); the rest green
  k_recover_t_wide taking the weight block of the handle's FIRST wide cone for every cone: the reverse tests of C, D, G and D's group fail; the rest green
  wide_E returning 2 where it returns 4: every test on D fails; of the rest only test_gpu_shapes.py's Newton steps at dimensions 130 and 200 notice
  w_t_times without the slot offset of its broadcast index: the reverse tests of B to F and both groups fail; of the rest only the dimension-70 layout of the adjoint tests
Swapping the indices of W in w_t_times fails nothing and cannot: W = -(B_sym)^-1 is the inverse of a symmetrised block, symmetric to 2e-16 relative, so W and W' give
the same lambda to rounding (at most 7e-16 in numpy on these layouts).
"""
import gc

import numpy as np
import pytest

import wide_cone_cases as wc
from helpers import load_pkg, make_pair
from test_gpu_group_differentiate_adjoint import member_scalars

pytestmark = pytest.mark.gpu

K = 17       # cotangent columns of the reverse tests: one more than the 16-column tile of k_gemm_batch


@pytest.fixture(autouse=True)
def handles_are_destroyed_with_their_test():
    """a Solver is part of a reference cycle (its evaluation callback holds it), so its handle and streams live until the collector runs: collect at the end of every
    test, so that what this module leaves behind for the tests after it — live streams on the hardware queues among them — does not depend on when that happens"""
    yield
    gc.collect()


def handle(oracle_mod, c):
    """a handle at the case's point with its scalars, evaluated, cone Jacobians formed (differentiate! uses those of the last cone! call)"""
    o, g = make_pair(oracle_mod, c.prob, c.pt, c.lam, **c.sc)
    o.cone(product=True, jacobian=True, target=True)
    g.cone(product=True, jacobian=True, target=True)
    return g


def check(got, ref, c, what, bound=None):
    """|got - ref| <= 1e-8 max(1, |ref|) on the rows of every wide cone first (the failure names the cone), then on the whole array; returns the relative error"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = 1e-8 * max(1.0, np.abs(ref).max()) if bound is None else bound
    for label, rows in c.wide_cone_rows():
        err = np.abs(got[rows] - ref[rows]).max()
        assert err <= bound, "%s, layout %s, %s (its z, s, t rows): error %.3e > %.3e" % (what, c.key, label, err, bound)
    err = np.abs(got - ref).max()
    assert err <= bound, "%s, layout %s: error %.3e > %.3e" % (what, c.key, err, bound)
    return err / max(1.0, np.abs(ref).max())


def cotangents(c, seed=17):
    return np.random.default_rng(seed).standard_normal((c.N, K))


_lam_ref = {}


def reference_adjoints(c, seed=17):
    """(V, M' V through Condensed.transposed), once per case"""
    k = (c.key, c.member, seed)
    if k not in _lam_ref:
        V = cotangents(c, seed)
        _lam_ref[k] = (wc.frozen(V), wc.frozen(c.transposed_columns(V)))
    return _lam_ref[k]


def check_theta(theta, lam_ref, c, V, what):
    """grad_theta = S' v = -J' lambda column by column, to the contraction bound 1e-8 max(1, |S|) ||v||_1; returns the largest error relative to max(1, |S|) ||v||_1"""
    want = -c.J.T @ lam_ref
    assert theta.shape == want.shape, (what, theta.shape, want.shape)
    err = np.abs(theta - want).max(axis=0)
    scale = max(1.0, np.abs(c.sensitivities()).max()) * np.abs(V).sum(axis=0)
    assert (err <= 1e-8 * scale).all(), "%s, layout %s: errors %s, bounds %s" % (what, c.key, err, 1e-8 * scale)
    return float((err[scale > 0.0] / scale[scale > 0.0]).max()) if (scale > 0.0).any() else 0.0


# ---- forward ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(wc.LAYOUTS))
def test_forward_all_columns(oracle_mod, key):
    c = wc.case(key)
    g = handle(oracle_mod, c)
    g.differentiate()
    S, J = g.data("solution_sensitivity"), g.data("jacobian_parameters")
    assert np.abs(J - c.J).max() <= 1e-12
    S_cond = c.sensitivities()
    if key in wc.ORACLE_DIFFERENTIATES:
        S_ref, J_cpu = wc.oracle_differentiate(oracle_mod, c)
        assert np.abs(J - J_cpu).max() <= 1e-12
        name = "the oracle's differentiate!"
    else:
        S_ref, name = S_cond, "-Condensed.forward"
    err = check(S, S_ref, c, "forward, p = %d, against %s" % (c.prob.np, name))
    err_c = check(S, S_cond, c, "forward, p = %d, against -Condensed.forward" % c.prob.np)
    line = "forward  %s %-22s N = %4d, p = %3d, |S| = %.2e: error %.2e against %s, %.2e against Condensed" % (key, wc.LAYOUTS[key], c.N, c.prob.np, np.abs(S_ref).max(), err, name, err_c)
    if key not in wc.ORACLE_DIFFERENTIATES:
        o = c.oracle(oracle_mod)
        for n, j in enumerate((0, c.prob.nx + 1, c.prob.np - 1)):      # a q column, a b column and the h column of the cone's last element
            col = -wc.oracle_step(o, c.J[:, j], n == 0)
            e = check(S[:, j], col, c, "forward, column %d against the oracle's search_direction_symmetric!" % j)
            line += "; column %d against the oracle %.2e" % (j, e)
    print(line)
    info = g.differentiate_info()
    assert info["columns"] == c.prob.np and info["rounds"] == 0 and info["failed_columns"] == 0


@pytest.mark.parametrize("key", ["B", "D"])
def test_forward_one_parameter(oracle_mod, key):
    """p == 1 takes the other branch of `p > 1 ? 1 : B.b.n` in both wide launchers"""
    c = wc.case(key, one_parameter=True)
    assert c.prob.np == 1
    g = handle(oracle_mod, c)
    g.differentiate()
    S, J = g.data("solution_sensitivity"), g.data("jacobian_parameters")
    S_cpu, J_cpu = wc.oracle_differentiate(oracle_mod, c)
    assert J.shape == (c.N, 1) and np.abs(J - J_cpu).max() <= 1e-12 and np.abs(J - c.J).max() <= 1e-12
    err = check(S, S_cpu, c, "forward, p = 1, against the oracle's differentiate!")
    err_c = check(S, c.sensitivities(), c, "forward, p = 1, against -Condensed.forward")
    print("forward  %s %-22s N = %4d, p =   1, |S| = %.2e: error %.2e against the oracle's differentiate!, %.2e against Condensed" % (
        key, wc.LAYOUTS[key], c.N, np.abs(S_cpu).max(), err, err_c))
    assert np.abs(S_cpu).max() > 1e-3      # (the single column is far from zero)


# ---- reverse ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(wc.WHOLE_MAP))
def test_reverse_whole_map(oracle_mod, key):
    c = wc.case(key)
    g = handle(oracle_mod, c)
    Lam = g.vjp(np.eye(c.N), theta=False)["adjoint"]          # ONE call, k = N unit cotangents: column j = M' e_j
    MT = c.transposed_map()
    err = check(Lam, MT, c, "reverse, k = N, against Condensed.transposed")
    line = "reverse  %s %-22s N = %4d, k = %3d, |M| = %.2e: error %.2e against Condensed" % (key, wc.LAYOUTS[key], c.N, c.N, np.abs(MT).max(), err)
    if key == "D":
        e = check(Lam, wc.oracle_map(oracle_mod, c).T, c, "reverse, k = N, against the oracle's M transposed")
        line += ", %.2e against the oracle's M'" % e
    print(line)
    assert g.vjp_info() == dict(columns=c.N, rounds=0, failed_columns=0, final_norm=0.0)


@pytest.mark.parametrize("key", ["E", "F"])
def test_reverse_wide_elements_per_lane(oracle_mod, key):
    c = wc.case(key)
    g = handle(oracle_mod, c)
    V, Lam_ref = reference_adjoints(c)
    out = g.vjp(V)
    err = check(out["adjoint"], Lam_ref, c, "reverse, k = %d, against Condensed.transposed" % K)
    err_t = check_theta(out["theta"], Lam_ref, c, V, "grad_theta, k = %d, against -J' lambda" % K)
    print("reverse  %s %-22s N = %4d, k = %3d, |lambda| = %.2e: error %.2e against Condensed; grad_theta %.2e of max(1, |S|) ||v||_1" % (
        key, wc.LAYOUTS[key], c.N, K, np.abs(Lam_ref).max(), err, err_t))
    assert g.vjp_info() == dict(columns=K, rounds=0, failed_columns=0, final_norm=0.0)


@pytest.mark.parametrize("key", sorted(wc.LAYOUTS))
def test_reverse_one_column(oracle_mod, key):
    """a single cotangent takes the mat-vec middle (columns.hip: condensed_middle) and the wide transposed kernels with p = 1"""
    c = wc.case(key)
    g = handle(oracle_mod, c)
    V, Lam_ref = reference_adjoints(c)
    many = g.vjp(V)
    one = g.vjp(V[:, 0])
    assert one["adjoint"].shape == (c.N,) and one["theta"].shape == (c.prob.np,) and g.vjp_info()["columns"] == 1
    err = check(one["adjoint"], Lam_ref[:, 0], c, "reverse, k = 1, against Condensed.transposed")
    diff = check(one["adjoint"], many["adjoint"][:, 0], c, "reverse, k = 1, against column 0 of k = %d" % K)
    check(many["adjoint"], Lam_ref, c, "reverse, k = %d, against Condensed.transposed" % K)
    check_theta(one["theta"][:, None], Lam_ref[:, :1], c, V[:, :1], "grad_theta, k = 1")
    print("one col. %s %-22s N = %4d, |lambda| = %.2e: error %.2e against Condensed, %.2e from column 0 of k = %d" % (
        key, wc.LAYOUTS[key], c.N, np.abs(Lam_ref[:, 0]).max(), err, diff, K))


def test_columns_are_independent_and_repeat_their_bits(oracle_mod):
    c = wc.case("D")
    g = handle(oracle_mod, c)
    g.differentiate()
    S = g.data("solution_sensitivity")
    assert g.differentiate_info()["rounds"] == 0
    g.differentiate()
    assert np.array_equal(g.data("solution_sensitivity"), S)
    V = np.array(reference_adjoints(c)[0][:, :3])
    first = g.vjp(V)
    assert g.vjp_info()["rounds"] == 0
    second = g.vjp(V)
    Vz = V.copy(); Vz[:, 1] = 0.0
    holed = g.vjp(Vz)
    for name in ("adjoint", "theta"):
        assert np.array_equal(first[name], second[name]), name
        assert not holed[name][:, 1].any(), name                      # exactly zero
        for j in (0, 2):
            assert np.array_equal(holed[name][:, j], first[name][:, j]), (name, j)
            assert np.abs(first[name][:, j]).max() > 0.0
    g.set_option("differentiate_refinement", 1)                        # correction rounds are inert with second-order cones
    g.differentiate()
    assert np.array_equal(g.data("solution_sensitivity"), S) and g.differentiate_info()["rounds"] == 0
    third = g.vjp(V)
    assert np.array_equal(third["adjoint"], first["adjoint"]) and np.array_equal(third["theta"], first["theta"]) and g.vjp_info()["rounds"] == 0


# ---- group -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["D", "E"])
def test_group_reverse_per_member(oracle_mod, key):
    pkg = load_pkg()
    cases = [wc.case(key, member=i, scalars=member_scalars(i)) for i in range(3)]
    members = [handle(oracle_mod, c) for c in cases]
    twins = [handle(oracle_mod, c) for c in cases]
    N = cases[0].N
    refs = [reference_adjoints(c, seed=17 + i) for i, c in enumerate(cases)]
    V = np.stack([np.array(v) for v, _ in refs])
    V[1] = 0.0                                                        # member 1: zero cotangents
    grp = pkg.Group(members)
    out = grp.vjp(V)                                                   # ONE call, k = 17 columns per member
    assert out["adjoint"].shape == (3, N, K) and out["theta"].shape == (3, cases[0].prob.np, K) and not out["status"].any()
    for i, (c, t) in enumerate(zip(cases, twins)):
        lam_ref = np.zeros((N, K)) if i == 1 else refs[i][1]
        err = check(out["adjoint"][i], lam_ref, c, "group member %d, k = %d, against Condensed.transposed" % (i, K))
        err_t = check_theta(out["theta"][i], lam_ref, c, V[i], "group member %d, grad_theta" % i)
        alone = t.vjp(V[i])
        d = check(out["adjoint"][i], alone["adjoint"], c, "group member %d against Solver.vjp on a twin" % i)
        d_t = np.abs(out["theta"][i] - alone["theta"]).max()
        assert d_t <= 1e-8 * max(1.0, np.abs(alone["theta"]).max()), (i, d_t)
        if i == 1:
            assert not out["adjoint"][i].any() and not out["theta"][i].any()      # exactly zero
        else:
            assert np.abs(out["adjoint"][i]).max() > 0.0
        print("group    %s %-22s member %d, k = %d, |lambda| = %.2e: error %.2e against Condensed, %.2e from its twin's Solver.vjp; grad_theta %.2e of max(1, |S|) ||v||_1" % (
            key, wc.LAYOUTS[key], i, K, np.abs(lam_ref).max(), err, d, err_t))
    grp.close()
