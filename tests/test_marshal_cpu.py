"""CPU-side checks (no GPU, no library call) of the index layouts behind Solver.vjp, Group.vjp and SmallNewtonBatch.vjp, and of the plumbing the handle classes
share.  The handles are stand-ins made with object.__new__; where the loaded library would stand, a recording fake copies out the cotangent buffer it is handed,
fills every output buffer with base(array) + flat index and returns 0.  The expected arrays are index formulas written out here, not calls of the package's own
layout code: a cotangent must arrive as buf[(i*k + j)*N + n] == v[i, n, j], and e.g. a group's out["A"][i, r, c, j] == base_A + ((i*k + j)*nx + c)*ne + r."""
import ctypes as C
import re

import numpy as np
import pytest

from helpers import load_pkg

NAMES = "PqAbGh"
BASE = dict(adjoint=1e6, theta=2e6, P=3e6, q=4e6, A=5e6, b=6e6, G=7e6, h=8e6, packed=9e6)
INFO = dict(columns=7, rounds=3, failed_columns=1, final_norm=0.25)
TEXT = "the known text"
DIMS = [(3, 2, 1, 2), (3, 0, 1, 0)]      # (nx, ne, nc, np): all distinct; no equalities and no parameters (the one-double buffers, the empty arrays)
COUNT = 2


def qp_table(nx, ne, nc):
    return dict(P=(nx, nx), q=(nx,), A=(ne, nx), b=(ne,), G=(nc, nx), h=(nc,))


def expected(count, k, shape, base, item=None, at=0):
    """out[i, r[, c], j] = base + (i*k + j)*item + at + (c*rows + r, or r): column j of item i is one block of `item` doubles, a matrix column-major in it"""
    item = int(np.prod(shape)) if item is None else item
    out = np.empty((count,) + tuple(shape) + (k,))
    for i in range(count):
        for j in range(k):
            for r in range(shape[0]):
                if len(shape) == 1:
                    out[i, r, j] = base + (i * k + j) * item + at + r
                else:
                    for c in range(shape[1]):
                        out[i, r, c, j] = base + (i * k + j) * item + at + c * shape[0] + r
    return out


def check_received(buf, v, N):
    """v: (count, N, k)"""
    count, _, k = v.shape
    assert buf.shape == (count * k * N,)
    for i in range(count):
        for j in range(k):
            for n in range(N):
                assert buf[(i * k + j) * N + n] == v[i, n, j]


class FakeLib:
    """the entries reverse-mode differentiate! reaches, recording"""

    def __init__(self, count, nx, ne, nc, npar):
        self.count, self.N, self.npar, self.table = count, nx + 2 * ne + 3 * nc, npar, qp_table(nx, ne, nc)
        self.calls, self.destroyed, self.asked, self.received, self.k, self.nonnull = [], [], [], None, None, set()

    def __getattr__(self, name):
        if name.endswith("last_error"):
            return lambda h: (self.asked.append((name, h)), TEXT.encode())[1]
        if name.endswith("destroy"):
            return lambda h: (self.destroyed.append((name, h)), 0)[1]
        raise AttributeError(name)

    def _fill(self, ptr, name, n):
        if ptr is None or not ptr:
            return
        self.nonnull.add(name)
        if n:
            np.ctypeslib.as_array(ptr, shape=(n,))[:] = BASE[name] + np.arange(n)

    def _columns(self, k, v, adj, gth):
        per = self.count * k
        self.k, self.nonnull = k, set()
        self.received = np.ctypeslib.as_array(v, shape=(per * self.N,)).copy() if v is not None and v else None
        self._fill(adj, "adjoint", per * self.N)
        self._fill(gth, "theta", per * self.npar)
        return per

    def _six(self, k, v, adj, gth, ptrs):
        per = self._columns(k, v, adj, gth)
        if ptrs is not None:
            for i, name in enumerate(NAMES):
                self._fill(ptrs[i], name, per * int(np.prod(self.table[name])))
        return 0

    def calipso_hip_differentiate_adjoint(self, h, cb, user, k, v, adj, gth, ptrs):
        self.calls.append("adjoint")
        return self._six(k, v, adj, gth, ptrs)

    def calipso_hip_group_set_evaluators(self, g, evals, user):
        self.calls.append("set_evaluators")
        assert len(evals) == self.count and user is None
        return 0

    def calipso_hip_group_differentiate_adjoint(self, g, k, v, adj, gth, ptrs, status, ms):
        self.calls.append("group_adjoint")
        for i in range(self.count):
            status[i] = 10 + i
        ms._obj.value = 1.5
        return self._six(k, v, adj, gth, ptrs)

    def calipso_hip_smallnewton_differentiate_adjoint(self, h, k, v, adj, gth, gqp, status, ms):
        self.calls.append("smallnewton_adjoint")
        per = self._columns(k, v, adj, gth)
        self._fill(gqp, "packed", per * sum(int(np.prod(s)) for s in self.table.values()))
        for i in range(self.count):
            status[i] = 10 + i
        ms._obj.value = 2.5
        return 0

    def _info(self, name, out):
        self.calls.append(name)
        np.ctypeslib.as_array(out, shape=(4,))[:] = [INFO["columns"], INFO["rounds"], INFO["failed_columns"], INFO["final_norm"]]
        return 0

    def calipso_hip_differentiate_info(self, h, out):
        return self._info("differentiate_info", out)

    def calipso_hip_differentiate_adjoint_info(self, h, out):
        return self._info("differentiate_adjoint_info", out)

    def calipso_hip_comm_size(self, c, out):
        return -1


def make_solver(pkg, L, nx, ne, nc, npar):
    from calipso_jl_amd._lib import EVAL_FN
    s = object.__new__(pkg.Solver)
    s._L, s._h, s._cb = L, C.c_void_p(1), EVAL_FN(lambda *a: 0)
    s.nx, s.ne, s.nc, s.np, s.N = nx, ne, nc, npar, nx + 2 * ne + 3 * nc
    return s


def make_group(pkg, L, count, nx, ne, nc, npar):
    g = object.__new__(pkg.Group)
    g.solvers, g._L, g._g = [make_solver(pkg, L, nx, ne, nc, npar) for _ in range(count)], L, C.c_void_p(2)
    return g


def make_batch(pkg, L, batch, nx, ne, nc, n_parameters=None):
    sn = object.__new__(pkg.SmallNewtonBatch)
    sn._L, sn._h = L, C.c_void_p(3)
    sn.nx, sn.ne, sn.nc, sn.batch, sn.device, sn.N = nx, ne, nc, batch, 0, nx + 2 * ne + 3 * nc
    if n_parameters is not None:
        sn.n_parameters, sn._evaluator = n_parameters, True
    return sn


def requested(qp):
    return NAMES if qp is True else (qp or "")


def check_six(out, count, k, squeeze, L, names, adjoint, theta, lead):
    """the arrays of a handle (lead False: no item axis) or a group, each filled by its own pointer"""
    pick = lambda a: (a if lead else a[0])[..., 0] if squeeze else (a if lead else a[0])
    want = dict(adjoint=(L.N,), theta=(L.npar,), **L.table)
    keys = (["adjoint"] if adjoint else []) + (["theta"] if theta else []) + list(names)
    assert [key for key in out if key != "status"] == keys
    assert L.nonnull == set(keys)      # every requested array got a buffer, an empty one too; nothing else did
    for key in keys:
        e = pick(expected(count, k, want[key], BASE[key]))
        assert out[key].shape == e.shape and np.array_equal(out[key], e), key


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("qp", [True, "Ab", None])
def test_solver_vjp_layout(dims, k, qp):
    pkg = load_pkg()
    nx, ne, nc, npar = dims
    L = FakeLib(1, *dims)
    s = make_solver(pkg, L, *dims)
    v = np.random.default_rng(0).standard_normal((s.N,) if k is None else (s.N, k))
    out = s.vjp(v, qp=qp)
    assert L.calls == ["adjoint"] and L.k == (k or 1)
    check_received(L.received, v.reshape(1, s.N, k or 1), s.N)
    check_six(out, 1, k or 1, k is None, L, requested(qp), True, npar > 0, lead=False)
    out = s.vjp(v, adjoint=False, theta=True, qp=qp)      # theta asked for by name: with np = 0 an empty array from a one-double buffer
    check_six(out, 1, k or 1, k is None, L, requested(qp), False, True, lead=False)
    assert out["theta"].shape == ((npar,) if k is None else (npar, k))


def test_solver_vjp_without_a_cotangent_passes_null_and_one_column():
    pkg = load_pkg()
    L = FakeLib(1, *DIMS[0])
    s = make_solver(pkg, L, *DIMS[0])
    out = s.vjp(None, qp="q")
    assert L.received is None and L.k == 1
    check_six(out, 1, 1, True, L, "q", True, True, lead=False)


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("qp", [True, "Ab", None])
def test_group_vjp_layout(dims, k, qp):
    pkg = load_pkg()
    nx, ne, nc, npar = dims
    L = FakeLib(COUNT, *dims)
    g = make_group(pkg, L, COUNT, *dims)
    N = g.solvers[0].N
    v = np.random.default_rng(1).standard_normal((COUNT, N) if k is None else (COUNT, N, k))
    out = g.vjp(v, qp=qp)
    assert L.calls == ["set_evaluators", "group_adjoint"] and L.k == (k or 1)
    check_received(L.received, v.reshape(COUNT, N, k or 1), N)
    check_six(out, COUNT, k or 1, k is None, L, requested(qp), True, npar > 0, lead=True)
    assert list(out)[-1] == "status" and out["status"].dtype == np.int32 and out["status"].tolist() == [10, 11] and g.vjp_ms() == 1.5
    out = g.vjp(v, adjoint=False, theta=True, qp=qp)
    check_six(out, COUNT, k or 1, k is None, L, requested(qp), False, True, lead=True)


@pytest.mark.parametrize("k", [None, 2])
def test_group_of_one_member_equals_the_handle_with_a_leading_axis(k):
    pkg = load_pkg()
    dims = DIMS[0]
    Ls, Lg = FakeLib(1, *dims), FakeLib(1, *dims)
    s, g = make_solver(pkg, Ls, *dims), make_group(pkg, Lg, 1, *dims)
    v = np.random.default_rng(2).standard_normal((s.N,) if k is None else (s.N, k))
    a, b = s.vjp(v, qp=True), g.vjp(v[None], qp=True)
    assert np.array_equal(Ls.received, Lg.received)
    assert list(a) + ["status"] == list(b)
    for key in a:
        assert b[key].shape == (1,) + a[key].shape and np.array_equal(b[key][0], a[key]), key


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("qp", [True, "Ab", None, False])
@pytest.mark.parametrize("rows", ["N", "nx"])
def test_batch_kernel_vjp_layout(dims, k, qp, rows):
    """the six QP gradients come in ONE packed buffer, k outermost per instance; any true qp gives all six (as it always did); the (batch, nx[, k]) cotangent is the
    x rows, the rest zero"""
    pkg = load_pkg()
    nx, ne, nc, _ = dims
    L = FakeLib(COUNT, nx, ne, nc, 0)
    sn = make_batch(pkg, L, COUNT, nx, ne, nc)
    n = sn.N if rows == "N" else nx
    v = np.random.default_rng(3).standard_normal((COUNT, n) if k is None else (COUNT, n, k))
    out = sn.vjp(v, qp=qp)
    kk = k or 1
    assert L.calls == ["smallnewton_adjoint"] and L.k == kk
    full = np.zeros((COUNT, sn.N, kk))
    full[:, :n] = v.reshape(COUNT, n, kk)
    check_received(L.received, full, sn.N)
    names = NAMES if (qp is None or qp) else ""
    assert list(out) == ["status", "ms", "adjoint"] + list(names)
    assert L.nonnull == {"adjoint"} | ({"packed"} if names else set())
    assert out["status"].dtype == np.int32 and out["status"].tolist() == [10, 11] and out["ms"] == 2.5
    pick = lambda a: a[..., 0] if k is None else a
    e = pick(expected(COUNT, kk, (sn.N,), BASE["adjoint"]))
    assert out["adjoint"].shape == e.shape and np.array_equal(out["adjoint"], e)
    table, at = qp_table(nx, ne, nc), 0
    nqp = sum(int(np.prod(s)) for s in table.values())
    for name in names:
        e = pick(expected(COUNT, kk, table[name], BASE["packed"], item=nqp, at=at))
        at += int(np.prod(table[name]))
        assert out[name].shape == e.shape and np.array_equal(out[name], e), name


@pytest.mark.parametrize("k", [None, 2])
def test_batch_kernel_vjp_with_an_evaluator_defaults_to_theta(k):
    pkg = load_pkg()
    nx, ne, nc, npar = DIMS[0]
    L = FakeLib(COUNT, nx, ne, nc, npar)
    sn = make_batch(pkg, L, COUNT, nx, ne, nc, n_parameters=npar)
    v = np.random.default_rng(4).standard_normal((COUNT, sn.N) if k is None else (COUNT, sn.N, k))
    out = sn.vjp(v, adjoint=False)
    assert list(out) == ["status", "ms", "theta"] and L.nonnull == {"theta"}
    e = expected(COUNT, k or 1, (npar,), BASE["theta"])
    assert np.array_equal(out["theta"], e[..., 0] if k is None else e)


def test_wrong_cotangent_shapes_and_qp_letters_are_refused_with_their_texts():
    pkg = load_pkg()
    dims = DIMS[0]
    L = FakeLib(COUNT, *dims)
    s, g, sn = make_solver(pkg, L, *dims), make_group(pkg, L, COUNT, *dims), make_batch(pkg, L, COUNT, *dims[:3])
    N = s.N
    for bad in (np.zeros(N + 1), np.zeros((N + 1, 2)), np.zeros((1, N, 2)), np.zeros((2, N))):
        with pytest.raises(ValueError, match=re.escape("cotangent must be (N,) or (N, k)")):
            s.vjp(bad)
    for bad in (np.zeros(N), np.zeros((COUNT + 1, N)), np.zeros((COUNT, N + 1, 2)), np.zeros((COUNT, N, 2, 1)), np.zeros((N, COUNT))):
        with pytest.raises(ValueError, match=re.escape("cotangent must be (count, N) or (count, N, k)")):
            g.vjp(bad)
    for bad in (np.zeros(N), np.zeros((COUNT + 1, N)), np.zeros((COUNT, N - 1)), np.zeros((COUNT, dims[0] + 1, 2)), np.zeros((COUNT, N, 0)), np.zeros((COUNT, N, 2, 1))):
        with pytest.raises(ValueError, match=re.escape("cotangent must be (batch, N), (batch, N, k), (batch, nx) or (batch, nx, k)")):
            sn.vjp(bad)
    for handle, v in ((s, np.zeros(N)), (g, np.zeros((COUNT, N)))):
        for bad in ("Px", "x", "pq"):
            with pytest.raises(ValueError, match=re.escape("qp must be True or a string of names out of 'PqAbGh'")):
                handle.vjp(v, qp=bad)
    assert L.calls == []      # all refused before any C call


def test_vjp_info_and_differentiate_info_decode_the_same_four_doubles():
    pkg = load_pkg()
    L = FakeLib(1, *DIMS[0])
    s = make_solver(pkg, L, *DIMS[0])
    a, b = s.differentiate_info(), s.vjp_info()
    assert L.calls == ["differentiate_info", "differentiate_adjoint_info"]
    assert a == INFO and b == INFO
    assert [type(a[key]) for key in INFO] == [int, int, int, float] and [type(b[key]) for key in INFO] == [int, int, int, float]


# class -> (attribute of the handle, last_error entry, destroy entry, the message of _check(-1, "what") today)
HANDLES = {"Solver": ("_h", "calipso_hip_last_error", "calipso_hip_destroy", "what: inertia correction failure (-1): " + TEXT),
           "LDLSolver": ("_h", "calipso_hip_last_error", "calipso_hip_destroy", "what: inertia correction failure (-1): " + TEXT),
           "SparseLDL": ("_h", "calipso_hip_sparse_last_error", "calipso_hip_sparse_destroy", "what failed (-1): " + TEXT),
           "SmallBatch": ("_h", "calipso_hip_small_last_error", "calipso_hip_small_destroy", "what failed (-1): " + TEXT),
           "SmallNewtonBatch": ("_h", "calipso_hip_smallnewton_last_error", "calipso_hip_smallnewton_destroy", "what failed (-1): " + TEXT),
           "Comm": ("_c", "calipso_hip_comm_last_error", "calipso_hip_comm_destroy", "comm_size failed (-1): " + TEXT)}


def make_handle(pkg, cls, L):
    attr = HANDLES[cls][0]
    obj = object.__new__(getattr(pkg, cls))
    obj._L = L
    setattr(obj, attr, C.c_void_p(5))
    return obj, getattr(obj, attr)


@pytest.mark.parametrize("cls", sorted(HANDLES))
def test_a_negative_status_raises_with_the_message_of_its_class(cls):
    pkg = load_pkg()
    L = FakeLib(1, *DIMS[0])
    obj, h = make_handle(pkg, cls, L)
    with pytest.raises(pkg.CalipsoHipError) as err:
        obj.size() if cls == "Comm" else obj._check(-1, "what")      # (a communicator's calls check their status themselves)
    assert str(err.value) == HANDLES[cls][3]
    assert L.asked == [(HANDLES[cls][1], h)]
    if cls != "Comm":
        assert obj._check(0, "what") == 0 and obj._check(1, "what") == 1 and len(L.asked) == 1
    if cls in ("Solver", "LDLSolver"):      # a status without a name of its own
        with pytest.raises(pkg.CalipsoHipError) as err:
            obj._check(-7, "what")
        assert str(err.value) == "what: error (-7): " + TEXT


@pytest.mark.parametrize("cls", sorted(HANDLES))
def test_close_destroys_once(cls):
    pkg = load_pkg()
    L = FakeLib(1, *DIMS[0])
    obj, h = make_handle(pkg, cls, L)
    close = getattr(obj, "close", None) or obj.__del__      # (a Solver is closed by its finaliser)
    close()
    assert L.destroyed == [(HANDLES[cls][2], h)]
    close()
    del obj, close
    assert len(L.destroyed) == 1
