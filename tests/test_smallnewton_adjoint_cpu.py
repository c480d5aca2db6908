"""CPU (no GPU): the reverse mode of the batch kernel's differentiate! (k_smallnewton_adj, include/calipso_smallnewton_device.hpp) restated in numpy stage by stage —
search_direction_symmetric_t, arrow_inverse_t and the first-row Cbar_t of the dt recovery — and held to the ORACLE's search_direction_symmetric! at interior points,
for nonnegative and second-order-cone layouts: <M' v, r> = <v, M r> with M r from the oracle, to 1e-12.  This pins the transposed map and its quirk handling
(second_order.jl:63-65: arrow_inverse uses the first row of its matrix only) without a device."""
import numpy as np
import pytest

import problems as pr
from helpers import interior_point


def arrow_inverse(u, x):
    """second_order_vector_inverse (cones/second_order.jl:50-60), the kernel's operation order"""
    g = u[1:] / u[0]
    beta = 1.0 / (1.0 + (-1.0 / (u[0] * u[0]) * np.dot(u[1:], u[1:])))
    x0_1 = x[0] - np.dot(g, x[1:])
    o = x[1:] - beta * (g * x0_1)
    return np.concatenate([[1.0 / u[0] * (x[0] - np.dot(g, o))], 1.0 / u[0] * o])


def arrow_inverse_t(u, y):
    """the transpose of arrow_inverse's operation sequence (the device's arrow_inverse_t)"""
    g = u[1:] / u[0]
    beta = 1.0 / (1.0 + (-1.0 / (u[0] * u[0]) * np.dot(u[1:], u[1:])))
    x2_1 = 1.0 / u[0] * y[0]
    o = 1.0 / u[0] * y[1:] - g * x2_1
    x0_1 = -beta * np.dot(g, o)
    return np.concatenate([[x2_1 + x0_1], o - g * x0_1])


def arrow(a):
    """arrow(a) = [a0 a1'; a1 a0 I]"""
    M = a[0] * np.eye(len(a))
    M[0, 1:] = a[1:]
    M[1:, 0] = a[1:]
    return M


class Condensed:
    """the kernel's condensed search_direction_symmetric! (factorize + search_direction_symmetric) and its transpose, for a QP at the point w"""

    def __init__(self, Lxx, A, G, w, q, dims, rho, ep, ed):
        nx, ne, nc = Lxx.shape[0], A.shape[0], G.shape[0]
        self.nx, self.ne, self.nc, self.q, self.rho, self.ep, self.ed = nx, ne, nc, q, rho, ep, ed
        self.orr, self.os, self.oy, self.oz, self.ot = nx, nx + ne, nx + ne + nc, nx + 2 * ne + nc, nx + 2 * ne + 2 * nc
        self.N = nx + 2 * ne + 3 * nc
        self.s, self.t = w[self.os:self.os + nc].copy(), w[self.ot:self.ot + nc].copy()
        self.Z = np.vstack([A, -G])
        self.cones, at = [], q
        for dm in dims:
            self.cones.append(slice(at, at + dm)); at += dm
        self.hrr = rho + ep
        self.omega_y = -1.0 / (-1.0 / self.hrr - ed)
        Sb, T = self.s[:q] - ed, self.t[:q]
        self.wz = -1.0 / (-Sb / (T + Sb * ep) - ed)
        self.W, self.u, self.ct = [], [], []
        for c in self.cones:
            sl, t = self.s[c], self.t[c]
            e0 = np.zeros(len(sl)); e0[0] = 1.0
            u = t + (sl - ed * e0) * ep
            Cbar = arrow(sl) - ed * np.eye(len(sl))
            B = np.stack([-arrow_inverse(u, Cbar[:, i]) for i in range(len(sl))], axis=1) - ed * np.eye(len(sl))
            Bs = np.triu(B) + np.triu(B, 1).T                   # what a factorisation of triu(K) sees
            self.W.append(-np.linalg.inv(Bs)); self.u.append(u); self.ct.append(sl - ed * e0)
        Om = np.zeros((ne + nc, ne + nc))
        Om[:ne, :ne] = self.omega_y * np.eye(ne)
        Om[ne:ne + q, ne:ne + q] = np.diag(self.wz)
        for c, W in zip(self.cones, self.W):
            Om[ne + c.start:ne + c.stop, ne + c.start:ne + c.stop] = W
        S = np.tril(Lxx.T) + np.tril(Lxx.T, -1).T + ep * np.eye(nx) + self.Z.T @ Om @ self.Z
        self.S = np.tril(S) + np.tril(S, -1).T

    def forward(self, r):
        nx, ne, q, ed, ep, hrr = self.nx, self.ne, self.q, self.ed, self.ep, self.hrr
        R = lambda o, n: r[o:o + n]
        rx, rr, rs, ry, rz, rt = R(0, nx), R(self.orr, ne), R(self.os, self.nc), R(self.oy, ne), R(self.oz, self.nc), R(self.ot, self.nc)
        by = ry + rr / hrr
        Sb, T = self.s[:q] - ed, self.t[:q]
        den = T + Sb * ep
        bz = np.zeros(self.nc)
        bz[:q] = rz[:q] + (rt[:q] + Sb * rs[:q]) / den
        t1 = np.zeros(ne + self.nc)
        t1[:ne] = self.omega_y * by
        t1[ne:ne + q] = self.wz * bz[:q]
        for c, W, u in zip(self.cones, self.W, self.u):
            bz[c] = rz[c] + arrow_inverse(u, (arrow(self.s[c]) - ed * np.eye(c.stop - c.start)) @ rs[c] + rt[c])
            t1[ne + c.start:ne + c.stop] = W @ bz[c]
        dx = np.linalg.solve(self.S, self.Z.T @ t1 + rx)
        t2 = self.Z @ dx
        out = np.zeros(self.N)
        out[:nx] = dx
        dy = -self.omega_y * (by - t2[:ne])
        out[self.oy:self.oy + ne] = dy
        out[self.orr:self.orr + ne] = (rr + dy) / hrr
        dz = np.zeros(self.nc)
        dz[:q] = -self.wz * (bz[:q] - t2[ne:ne + q])
        ds = (rt[:q] + Sb * (rs[:q] + dz[:q])) / den
        out[self.oz:self.oz + q] = dz[:q]
        out[self.os:self.os + q] = ds
        out[self.ot:self.ot + q] = (rt[:q] - T * ds) / Sb
        for c, W, u, ct in zip(self.cones, self.W, self.u, self.ct):
            dzc = -W @ (bz[c] - t2[ne + c.start:ne + c.stop])
            dsc = arrow_inverse(u, rt[c] + (arrow(self.s[c]) - ed * np.eye(len(ct))) @ (rs[c] + dzc))
            dtc = arrow_inverse(ct, rt[c] - arrow(self.t[c]) @ dsc)      # the first row of Cbar_t only
            out[self.oz + c.start:self.oz + c.stop] = dzc
            out[self.os + c.start:self.os + c.stop] = dsc
            out[self.ot + c.start:self.ot + c.stop] = dtc
        return out

    def transposed(self, v):
        """M' v: the stages of forward() in reverse order, each transposed — the arithmetic of search_direction_symmetric_t"""
        nx, ne, nc, q, ed, ep, hrr = self.nx, self.ne, self.nc, self.q, self.ed, self.ep, self.hrr
        V = lambda o, n: v[o:o + n]
        vx, vr, vs, vy, vz, vt = V(0, nx), V(self.orr, ne), V(self.os, nc), V(self.oy, ne), V(self.oz, nc), V(self.ot, nc)
        out = np.zeros(self.N)
        rsym, t2 = np.zeros(ne + nc), np.zeros(ne + nc)
        dyb = vy + vr / hrr
        out[self.orr:self.orr + ne] = vr / hrr
        rsym[:ne], t2[:ne] = -self.omega_y * dyb, self.omega_y * dyb
        Sb, T = self.s[:q] - ed, self.t[:q]
        den = T + Sb * ep
        g = (vs[:q] - T * vt[:q] / Sb) / den
        out[self.ot:self.ot + q] = vt[:q] / Sb + g
        out[self.os:self.os + q] = Sb * g
        dzb = vz[:q] + Sb * g
        rsym[ne:ne + q], t2[ne:ne + q] = -self.wz * dzb, self.wz * dzb
        for c, W, u, ct in zip(self.cones, self.W, self.u, self.ct):
            Cbar = arrow(self.s[c]) - ed * np.eye(len(ct))
            a = arrow_inverse_t(ct, vt[c])
            b = vs[c] - arrow(self.t[c]).T @ a
            a2 = arrow_inverse_t(u, b)
            gb = Cbar.T @ a2
            out[self.ot + c.start:self.ot + c.stop] = a + a2
            out[self.os + c.start:self.os + c.stop] = gb
            wv = W.T @ (vz[c] + gb)
            rsym[ne + c.start:ne + c.stop], t2[ne + c.start:ne + c.stop] = -wv, wv
        xb = np.linalg.solve(self.S.T, self.Z.T @ t2 + vx)
        t1 = self.Z @ xb
        out[:nx] = xb
        tot = rsym[:ne] + self.omega_y * t1[:ne]
        out[self.oy:self.oy + ne] = tot
        out[self.orr:self.orr + ne] += tot / hrr
        tot = rsym[ne:ne + q] + self.wz * t1[ne:ne + q]
        out[self.oz:self.oz + q] = tot
        out[self.ot:self.ot + q] += tot / den
        out[self.os:self.os + q] += Sb * tot / den
        for c, W, u in zip(self.cones, self.W, self.u):
            bz = rsym[ne + c.start:ne + c.stop] + W.T @ t1[ne + c.start:ne + c.stop]
            out[self.oz + c.start:self.oz + c.stop] = bz
            a = arrow_inverse_t(u, bz)
            out[self.ot + c.start:self.ot + c.stop] += a
            out[self.os + c.start:self.os + c.stop] += (arrow(self.s[c]) - ed * np.eye(c.stop - c.start)).T @ a
        return out


def test_arrow_inverse_t_is_the_transpose_of_the_quirky_arrow_inverse():
    rng = np.random.default_rng(3)
    for dm in (2, 3, 5, 16):
        u = np.concatenate([[2.0 + rng.random()], 0.4 * rng.standard_normal(dm - 1)])
        T = np.stack([arrow_inverse(u, e) for e in np.eye(dm)], axis=1)
        Tt = np.stack([arrow_inverse_t(u, e) for e in np.eye(dm)], axis=1)
        assert np.abs(Tt - T.T).max() <= 1e-14 * max(1.0, np.abs(T).max())
        # (the quirk: T is not arrow(u)^-1 for every u — the transpose is of THIS map)


@pytest.mark.parametrize("layout", [(10, 4, 6, 0, 0), (12, 5, 3, 2, 3), (16, 5, 0, 3, 4), (14, 6, 4, 1, 5), (9, 0, 2, 2, 3)])
def test_transposed_map_against_the_oracles_search_direction(oracle_mod, layout):
    nx, ne, nnn, nsoc, sdim = layout
    prob = pr.parametric_conic_qp(nx, ne, nnn, nsoc, sdim, seed=900 + nx)
    kappa, tau, rho, ep, ed = 0.17, 0.99, 52.0, 0.05, 0.03
    pt, lam = interior_point(prob, seed=5)
    o = oracle_mod.OracleSolver(prob.nx, prob.np, prob.ne, prob.nc, prob.nonnegative_indices, prob.second_order_indices)
    op = o.point()
    for f in "xrsyzt":
        op[f][:] = pt[f]
    o.buf("dual")[:] = lam
    for name, val in (("central_path", kappa), ("penalty", rho), ("primal_regularization", ep), ("dual_regularization", ed), ("fraction_to_boundary", tau)):
        o.buf(name)[0] = val
    prob.evaluate(pr.ALL_VARIABLE_FLAGS, op["x"], op["y"], op["z"], prob.parameters, o.buf)
    o.cone(product=True, jacobian=True, target=True)
    o.residual_jacobian_variables(); o.residual_jacobian_variables_symmetric()
    w = op["all"].copy()
    cm = Condensed(2.0 * prob.c * np.asarray(prob.P), np.asarray(prob.A).reshape(ne, nx), np.asarray(prob.G).reshape(prob.nc, nx), w, nnn,
                   [sdim] * nsoc, rho, ep, ed)
    rng = np.random.default_rng(11)
    N = cm.N
    for j in range(6):
        r, v = rng.standard_normal(N), rng.standard_normal(N)
        o.buf("residual")[:] = r
        o.search_direction_symmetric(0, fact=(j == 0))
        Mr = o.buf("step").copy()
        # the restatement IS the oracle's map ...
        assert np.abs(cm.forward(r) - Mr).max() <= 1e-10 * max(1.0, np.abs(Mr).max())
        # ... and its transpose is the transpose of the oracle's
        MTv = cm.transposed(v)
        lhs, rhs = np.dot(MTv, r), np.dot(v, Mr)
        assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(MTv) * np.linalg.norm(r), (j, lhs, rhs)
    # column by column: M' as a matrix is the transpose of M
    M = np.stack([cm.forward(e) for e in np.eye(N)], axis=1)
    MT = np.stack([cm.transposed(e) for e in np.eye(N)], axis=1)
    assert np.abs(MT - M.T).max() <= 1e-12 * np.abs(M).max()
