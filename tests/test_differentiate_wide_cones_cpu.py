"""CPU (no GPU): the references of tests/test_gpu_differentiate_wide_cones.py, pinned before any device run.  On every layout of wide_cone_cases.LAYOUTS (second-order
cones of dimension 5 to 513, one and several per problem) test_smallnewton_adjoint_cpu's Condensed IS the oracle's search_direction_symmetric! and its transposed() is the
transpose of that map; where the oracle's own column loop is affordable (all layouts but F, dimension 513) -Condensed.forward(dR/dtheta) IS the oracle's differentiate!,
entry by entry, and the numpy assembly of dR/dtheta is the oracle's.  That makes Condensed the reference of the device tests at the one size where the oracle's
differentiate! is too slow for a test, and tests/problems.py's builders are pinned on the way.

Bounds: those of test_smallnewton_adjoint_cpu.py / test_differentiate_adjoint_cpu.py (1e-10 relative for a forward map, 1e-12 for the dot-product identity).  Measured:
forward at most 2.3e-15, identity at most 1.1e-16, sensitivities at most 5.3e-15 (|S| between 1 and 15)."""
import numpy as np
import pytest

import problems as pr
import wide_cone_cases as wc


def test_dims_builder_is_parametric_conic_qp_for_equal_dimensions():
    for (nx, ne, n_nn, k, d, seed) in ((12, 5, 3, 2, 3, 4), (14, 6, 4, 1, 5, 914), (10, 4, 6, 0, 0, 7), (9, 0, 0, 3, 4, 1)):
        a, b = pr.parametric_conic_qp(nx, ne, n_nn, k, d, seed), pr.parametric_conic_qp_dims(nx, ne, n_nn, [d] * k, seed)
        for name in "PqAbGh":
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        assert a.nonnegative_indices == b.nonnegative_indices and a.second_order_indices == b.second_order_indices
        assert (a.nx, a.ne, a.nc, a.np) == (b.nx, b.ne, b.nc, b.np)
    p = pr.parametric_conic_qp_dims(14, 4, 3, [129, 3, 70], 914)
    assert p.nc == 205 and [len(c) for c in p.second_order_indices] == [129, 3, 70]
    assert sorted(p.nonnegative_indices + sum(p.second_order_indices, [])) == list(range(1, 206))       # one index list per cone, in order, nothing shared


def test_one_parameter_problem_moves_h_along_its_direction():
    prob = pr.one_parameter_conic_qp_dims(14, 4, 3, [5, 3], seed=914)
    base = pr.parametric_conic_qp_dims(14, 4, 3, [5, 3], seed=914)
    assert prob.np == 1 and prob.parameters.shape == (1,) and np.array_equal(prob.G, base.G) and np.array_equal(prob.h, base.h)
    rng = np.random.default_rng(2)
    pt = dict(x=rng.standard_normal(prob.nx), y=rng.standard_normal(prob.ne), z=rng.standard_normal(prob.nc))
    J = wc.parameter_jacobian(prob, pt)
    want = np.zeros((prob.nx + 2 * prob.ne + 3 * prob.nc, 1))
    want[prob.nx + 2 * prob.ne + prob.nc:prob.nx + 2 * prob.ne + 2 * prob.nc, 0] = prob.direction
    assert np.array_equal(J, want) and np.abs(prob.direction).min() > 0.0
    h = lambda th: _cone_constraint(prob, pt, th)
    assert np.abs((h(0.5) - h(-0.5)) - prob.direction).max() <= 1e-14 * max(1.0, np.abs(prob.direction).max())      # linear in theta: exact up to rounding


def _cone_constraint(prob, pt, th):
    store = {}
    prob.evaluate(pr.CONE, pt["x"], pt["y"], pt["z"], np.array([th]), lambda name: store.setdefault(name, np.zeros(prob.nc)))
    return store["cone_constraint"].copy()


@pytest.mark.parametrize("key", sorted(wc.LAYOUTS))
def test_condensed_is_the_oracles_map_and_its_transpose(oracle_mod, key):
    c = wc.case(key)
    o = c.oracle(oracle_mod)
    rng = np.random.default_rng(11)
    worst_f = worst_t = 0.0
    for j in range(3):
        r, v = rng.standard_normal(c.N), rng.standard_normal(c.N)
        Mr = wc.oracle_step(o, r, j == 0)
        err = np.abs(c.cm.forward(r) - Mr).max()
        worst_f = max(worst_f, err / max(1.0, np.abs(Mr).max()))
        assert err <= 1e-10 * max(1.0, np.abs(Mr).max()), (key, j, err)
        MTv = c.cm.transposed(v)
        gap, scale = abs(np.dot(MTv, r) - np.dot(v, Mr)), np.linalg.norm(MTv) * np.linalg.norm(r)
        worst_t = max(worst_t, gap / scale)
        assert gap <= 1e-12 * scale, (key, j, gap, scale)
    print("%s %s: N = %d, |Condensed.forward - oracle| = %.1e, |<M'v, r> - <v, M r>| = %.1e (relative)" % (key, wc.LAYOUTS[key], c.N, worst_f, worst_t))


@pytest.mark.parametrize("key", list(wc.ORACLE_DIFFERENTIATES))
def test_condensed_sensitivities_are_the_oracles_differentiate(oracle_mod, key):
    c = wc.case(key)
    S_cpu, J_cpu = wc.oracle_differentiate(oracle_mod, c)
    assert np.abs(c.J - J_cpu).max() <= 1e-12
    S = c.sensitivities()
    err, scale = np.abs(S - S_cpu).max(), max(1.0, np.abs(S_cpu).max())
    print("%s %s: N = %d, p = %d, |S| = %.2e, |-Condensed.forward(J) - oracle| = %.1e" % (key, wc.LAYOUTS[key], c.N, c.prob.np, np.abs(S_cpu).max(), err))
    assert S.shape == S_cpu.shape and err <= 1e-10 * scale, (key, err, scale)
