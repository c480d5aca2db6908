"""CPU-side checks (no GPU, no library call) of the host paths of QPLayer, SolverQPLayer and GroupQPLayer over duck-typed fakes of the handles: the cotangent that
reaches vjp() has gx, gy, gz at rows 0, nx+ne+nc and nx+2ne+nc and zeros elsewhere; gradients of batched inputs come back per item, those of shared inputs summed
over the items with the layer's own reduction, bit for bit; inputs that need no gradient get None and are not asked of vjp() where the layer names what it wants;
items that did not converge give NaN before the sum and ONE warning; wrong dtypes and shapes are refused with the layers' texts; a handle that solved other data
since forward solves the same data again, once."""
import warnings

import numpy as np
import pytest

from helpers import load_pkg

torch = pytest.importorskip("torch")

NAMES = "PqAbGh"
COUNT = 3
DIMS = [(3, 2, 1), (3, 0, 1)]      # (nx, ne, nc): all distinct; no equalities


def table(nx, ne, nc):
    return dict(P=(nx, nx), q=(nx,), A=(ne, nx), b=(ne,), G=(nc, nx), h=(nc,))


class _Shape:
    def __init__(self, nx, ne, nc, seed):
        self.nx, self.ne, self.nc, self.N = nx, ne, nc, nx + 2 * ne + 3 * nc
        self.rng = np.random.default_rng(seed)
        self.solves, self.cotangents, self.asked = 0, [], []

    def _vjp(self, lead, v, adjoint, qp):
        assert adjoint is False
        v = np.asarray(v)
        assert v.shape == lead + (self.N,) and v.dtype == np.float64
        self.cotangents.append(v.copy())
        self.asked.append(qp)
        return {name: self.gradients[name].copy() for name in (NAMES if qp is True else qp)}

    def _known(self, lead):
        self.gradients = {name: self.rng.standard_normal(lead + s) for name, s in table(self.nx, self.ne, self.nc).items()}
        self.W = self.rng.standard_normal(lead + (self.N,))


class _Point:
    def __init__(self, w, nx, ne, nc):
        oy, oz = nx + ne + nc, nx + 2 * ne + nc
        self.variables, self.equality_dual, self.cone_dual = w[:nx], w[oy:oy + ne], w[oz:oz + nc]


class FakeBatch(_Shape):
    """what QPLayer's host path calls of a SmallNewtonBatch"""

    def __init__(self, nx, ne, nc, status):
        super().__init__(nx, ne, nc, 11)
        self.batch, self.device, self.status = len(status), 0, np.array(status, dtype=np.int32)
        self._known((self.batch,))

    def set_qp(self, P, q, A, b, G, h, objective_scale=0.5, shared=None):
        self.data = [np.array(a) for a in (P, q, A, b, G, h)]

    def initialize(self, x0):
        assert np.array_equal(x0, np.zeros((self.batch, self.nx)))

    def solve(self):
        self.solves += 1
        return self.status.copy(), 0.0

    def get_state(self):
        return dict(solution=self.W.copy())

    def vjp(self, v, adjoint=True, theta=None, qp=None):
        return dict(self._vjp((self.batch,), v, adjoint, qp), status=np.zeros(self.batch, dtype=np.int32), ms=0.0)


class _FakeEntries:
    def __init__(self, owner, result):
        self.owner, self.result = owner, result

    def calipso_hip_initialize(self, h, guess):
        return 0

    def calipso_hip_solve(self, h, cb, user):
        self.owner.solves += 1
        return self.result


class FakeSolver(_Shape):
    """what SolverQPLayer (through initialize_b / solve_b) and GroupQPLayer's members call of a Solver"""

    def __init__(self, nx, ne, nc, result=1, seed=12):
        super().__init__(nx, ne, nc, seed)
        self._L, self._h, self._cb = _FakeEntries(self, result), None, None
        self._known(())
        self.attached = []

    def _check(self, rc, what):
        assert rc >= 0
        return rc

    def qp_attach(self, P, q, A, b, G, h, objective_scale=0.5):
        self.attached.append([np.array(a) for a in (P, q, A, b, G, h)])

    @property
    def solution(self):
        return _Point(self.W, self.nx, self.ne, self.nc)

    def vjp(self, v, adjoint=True, theta=None, qp=None):
        assert theta is False
        return self._vjp((), v, adjoint, qp)


class FakeGroup(_Shape):
    """what GroupQPLayer calls of a Group"""

    def __init__(self, nx, ne, nc, results):
        super().__init__(nx, ne, nc, 13)
        self.solvers = [FakeSolver(nx, ne, nc, seed=20 + i) for i in range(len(results))]
        self.results = list(results)
        self._known((len(results),))

    def solve(self):
        self.solves += 1
        return list(self.results)

    def vjp(self, v, adjoint=True, theta=None, qp=None):
        assert theta is False
        return dict(self._vjp((len(self.solvers),), v, adjoint, qp), status=np.zeros(len(self.solvers), dtype=np.int32))


def layers():
    load_pkg()
    from calipso_jl_amd import torch_layer
    return torch_layer


def make(kind, dims, converged=(True, True, True)):
    """(layer, handle, lead, what vjp() is asked for given the wanted names, the parent's reduction of a shared input's gradient)"""
    L = layers()
    if kind == "batch":
        in_order = lambda g: g.sum(axis=0)
        return L.QPLayer, FakeBatch(*dims, status=[1 if c else 0 for c in converged]), (COUNT,), lambda want: True, in_order
    if kind == "solver":
        return L.SolverQPLayer, FakeSolver(*dims, result=1 if converged[1] else 0), (), lambda want: want, None

    def in_order(g):
        acc = g[0].copy()
        for i in range(1, COUNT):
            acc += g[i]
        return acc
    return L.GroupQPLayer, FakeGroup(*dims, results=[1 if c else 0 for c in converged]), (COUNT,), lambda want: want, in_order


def inputs(dims, lead, batched, requires, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for name, s in table(*dims).items():
        t = torch.from_numpy(rng.standard_normal((lead if name in batched else ()) + s))
        out.append(t.requires_grad_(name in requires))
    return out


def solution_of(handle, lead):
    if isinstance(handle, FakeGroup):
        return np.stack([s.W for s in handle.solvers])
    return handle.W


KINDS = ["batch", "solver", "group"]


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("converged", [(True, True, True), (True, False, True)])
def test_cotangent_rows_gradients_sums_and_nan(kind, dims, converged):
    nx, ne, nc = dims
    layer, handle, lead, asked, reduce = make(kind, dims, converged)
    batched = "PbG" if lead else ""                 # the others are shared by the items
    requires = "PqAG"                               # b and h need no gradient
    data = inputs(dims, lead, batched, requires)
    x, y, z = layer.apply(handle, *data, True)
    N, oy, oz = handle.N, nx + ne + nc, nx + 2 * ne + nc
    W = solution_of(handle, lead)
    assert x.shape == lead + (nx,) and y.shape == lead + (ne,) and z.shape == lead + (nc,)
    for part, at, n in ((x, 0, nx), (y, oy, ne), (z, oz, nc)):
        assert np.array_equal(part.detach().numpy(), W[..., at:at + n])
    rng = np.random.default_rng(6)
    cx, cy, cz = (rng.standard_normal(lead + (n,)) for n in (nx, ne, nc))
    loss = (x * torch.from_numpy(cx)).sum() + (y * torch.from_numpy(cy)).sum() + (z * torch.from_numpy(cz)).sum()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        loss.backward()
    # the cotangent: three parts at their rows, zeros elsewhere
    assert len(handle.cotangents) == 1 and handle.solves == 1
    v = handle.cotangents[0]
    expect = np.zeros(lead + (N,))
    expect[..., 0:nx], expect[..., oy:oy + ne], expect[..., oz:oz + nc] = cx, cy, cz
    assert np.array_equal(v, expect)
    assert np.count_nonzero(v) == np.count_nonzero(cx) + np.count_nonzero(cy) + np.count_nonzero(cz)
    assert handle.asked == [asked(requires)]
    # the gradients
    bad = ~np.array(converged) if lead else (not converged[1])
    for name, t in zip(NAMES, data):
        if name not in requires:
            assert t.grad is None
            continue
        g = handle.gradients[name].copy()
        if lead:
            g[bad] = np.nan
            if name not in batched:
                g = reduce(g)
        elif bad:
            g = np.full_like(g, np.nan)
        assert t.grad.shape == t.shape and t.grad.dtype == torch.float64
        assert np.array_equal(t.grad.numpy(), g, equal_nan=True), name
        if name not in batched and np.any(bad):
            assert np.isnan(t.grad.numpy()).all()      # NaN went in before the sum
    # one warning, with the layer's text, only when something did not converge
    texts = dict(batch="QPLayer: 1 of 3 instances did not converge (solve status != 1): their gradients are NaN",
                 solver="SolverQPLayer: the solve did not converge: the gradients are NaN",
                 group="GroupQPLayer: 1 of 3 members did not converge: their gradients are NaN")
    assert [str(w.message) for w in caught] == ([] if all(converged) else [texts[kind]])


@pytest.mark.parametrize("kind", KINDS)
def test_only_the_solution_without_duals(kind):
    dims = DIMS[0]
    layer, handle, lead, asked, _ = make(kind, dims)
    data = inputs(dims, lead, NAMES if lead else "", "q")
    x = layer.apply(handle, *data)
    assert isinstance(x, torch.Tensor) and x.shape == lead + (dims[0],)
    x.sum().backward()
    v = handle.cotangents[0]
    assert np.array_equal(v[..., :dims[0]], np.ones(lead + (dims[0],))) and not v[..., dims[0]:].any()
    assert handle.asked == [asked("q")]
    assert np.array_equal(data[1].grad.numpy(), handle.gradients["q"]) and all(t.grad is None for i, t in enumerate(data) if i != 1)


@pytest.mark.parametrize("kind", KINDS)
def test_wrong_dtype_and_shape_are_refused_with_the_layers_texts(kind):
    dims = DIMS[0]
    nx, ne, nc = dims
    layer, handle, lead, _, _ = make(kind, dims)
    title = dict(batch="QPLayer", solver="SolverQPLayer", group="GroupQPLayer")[kind]
    data = inputs(dims, lead, "", "")
    data[2] = data[2].to(torch.float32)
    with pytest.raises(TypeError) as err:
        layer.apply(handle, *data)
    assert str(err.value) == "%s: A must be float64" % title
    data = inputs(dims, lead, "", "")
    data[4] = torch.zeros((nc + 1, nx), dtype=torch.float64)
    with pytest.raises(ValueError) as err:
        layer.apply(handle, *data)
    assert str(err.value) == ("%s: G must be %s" % (title, (nc, nx))) + (" or %s" % ((COUNT, nc, nx),) if lead else "")
    data = inputs(dims, lead, "", "")
    data[1] = torch.zeros((COUNT + 1, nx), dtype=torch.float64)      # a leading axis of the wrong length
    with pytest.raises(ValueError) as err:
        layer.apply(handle, *data)
    assert str(err.value) == ("%s: q must be %s" % (title, (nx,))) + (" or %s" % ((COUNT, nx),) if lead else "")
    assert handle.solves == 0


@pytest.mark.parametrize("kind", KINDS)
def test_backward_solves_the_same_data_again_once_after_the_handle_was_used_elsewhere(kind):
    dims = DIMS[0]
    layer, handle, lead, _, _ = make(kind, dims)
    data = inputs(dims, lead, "PA" if lead else "", NAMES)
    x = layer.apply(handle, *data)
    y = layer.apply(handle, *data)      # the same handle solves again: x's key is stale, y's is current
    assert handle.solves == 2
    y.sum().backward()
    assert handle.solves == 2
    x.sum().backward()
    assert handle.solves == 3
    x2 = layer.apply(handle, *data)
    handle._qp_layer_key = object()
    x2.sum().backward()
    assert handle.solves == 5
    if kind == "solver":
        for got, t in zip(handle.attached[-1], data):
            assert np.array_equal(got, t.detach().numpy())
    if kind == "group":
        for i, s in enumerate(handle.solvers):
            assert len(s.attached) == 5
            for got, t, name in zip(s.attached[-1], data, NAMES):
                assert np.array_equal(got, t.detach().numpy()[i] if name in "PA" else t.detach().numpy())
    if kind == "batch":
        for got, t, name in zip(handle.data, data, NAMES):
            a = t.detach().numpy()
            assert np.array_equal(got, a if name in "PA" else np.broadcast_to(a, (COUNT,) + a.shape))
