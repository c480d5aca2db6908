"""CPU-side checks (no GPU, no library call) of torch_layer.SparseTrajectoryLayer over a duck-typed stand-in of a SparseKKT with an evaluator and parameter patterns,
in the style of tests/test_torch_layer_cpu.py: forward is set_parameters + initialize + solve and returns the handle's point; backward is ONE vjp(theta=True) whose
cotangent is dLoss/dw as it is, and theta's gradient is what vjp returned, bit for bit; x0 gets none; a solve that did not converge gives NaN and one warning; wrong
dtypes, shapes and a handle without patterns are refused with the layer's texts; a handle that solved other data since forward solves the same data again, once."""
import warnings

import numpy as np
import pytest

from helpers import load_pkg

torch = pytest.importorskip("torch")


class FakeSparse:
    """what SparseTrajectoryLayer's host path calls of a SparseKKT"""

    def __init__(self, nx=4, ne=2, nc=1, num_parameters=5, status=1, patterns=True):
        self.nx, self.ne, self.nc, self.N, self.num_parameters, self.device = nx, ne, nc, nx + 2 * ne + 3 * nc, num_parameters, 0
        rng = np.random.default_rng(3)
        self.W, self.gradient = rng.standard_normal(self.N), rng.standard_normal(num_parameters)
        self.status, self.patterns = status, patterns
        self.calls, self.cotangents, self.theta, self.x0 = [], [], None, None

    def _has_parameter_patterns(self):
        return self.patterns

    def set_parameters(self, theta):
        self.calls.append("set_parameters"); self.theta = np.array(theta)

    def initialize(self, x0):
        self.calls.append("initialize"); self.x0 = np.array(x0)

    def solve(self):
        self.calls.append("solve")
        return self.status, {}

    def get(self, name):
        assert name == "solution"
        return self.W + self.theta.sum()          # (the point moves with theta: a solve of other data leaves another one)

    def vjp(self, V, adjoint=True, qp="", theta=None):
        assert adjoint is False and theta is True and not qp
        V = np.asarray(V)
        assert V.shape == (self.N,) and V.dtype == np.float64
        self.calls.append("vjp"); self.cotangents.append(V.copy())
        return {"theta": self.gradient.copy()}


def layer():
    load_pkg()
    from calipso_jl_amd.torch_layer import SparseTrajectoryLayer
    return SparseTrajectoryLayer


def tensors(h, requires=True):
    rng = np.random.default_rng(8)
    return (torch.tensor(rng.standard_normal(h.num_parameters), dtype=torch.float64, requires_grad=requires), torch.tensor(rng.standard_normal(h.nx), dtype=torch.float64))


def test_forward_solves_and_backward_is_one_vjp_with_the_cotangent_as_it_is():
    h = FakeSparse()
    theta, x0 = tensors(h)
    w = layer().apply(h, theta, x0)
    assert h.calls == ["set_parameters", "initialize", "solve"]
    assert np.array_equal(h.theta, theta.detach().numpy()) and np.array_equal(h.x0, x0.numpy())
    assert w.shape == (h.N,) and w.dtype == torch.float64 and np.array_equal(w.detach().numpy(), h.W + h.theta.sum())
    weights = torch.tensor(np.random.default_rng(2).standard_normal(h.N))
    (w * weights).sum().backward()
    assert h.calls[3:] == ["vjp"] and np.array_equal(h.cotangents[0], weights.numpy())
    assert np.array_equal(theta.grad.numpy(), h.gradient) and x0.grad is None


def test_no_gradient_wanted_no_vjp():
    h = FakeSparse()
    theta, x0 = tensors(h, requires=False)
    x0.requires_grad_(True)
    w = layer().apply(h, theta, x0)
    w.sum().backward()
    assert "vjp" not in h.calls and x0.grad is None


def test_a_solve_that_did_not_converge_gives_nan_and_one_warning():
    h = FakeSparse(status=0)
    theta, x0 = tensors(h)
    w = layer().apply(h, theta, x0)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        w.sum().backward()
    assert len(caught) == 1 and "SparseTrajectoryLayer: the solve did not converge" in str(caught[0].message)
    assert theta.grad.shape == (h.num_parameters,) and np.isnan(theta.grad.numpy()).all()


def test_refusals_carry_the_layers_texts():
    h = FakeSparse()
    theta, x0 = tensors(h)
    with pytest.raises(TypeError, match="SparseTrajectoryLayer: theta must be float64"):
        layer().apply(h, theta.detach().float(), x0)
    with pytest.raises(ValueError, match=r"SparseTrajectoryLayer: x0 must be \(4,\)"):
        layer().apply(h, theta, x0[:3])
    with pytest.raises(ValueError, match=r"SparseTrajectoryLayer: theta must be \(5,\)"):
        layer().apply(h, theta.detach()[None, :], x0)
    with pytest.raises(ValueError, match="set_parameter_patterns"):
        layer().apply(FakeSparse(patterns=False), theta, x0)
    assert h.calls == []


def test_backward_solves_the_same_data_again_once_after_the_handle_was_used_elsewhere():
    h = FakeSparse()
    theta, x0 = tensors(h)
    w = layer().apply(h, theta, x0)
    other = layer().apply(h, (2.0 * theta).detach(), x0)          # the handle solves other data
    assert np.array_equal(h.theta, 2.0 * theta.detach().numpy()) and not np.array_equal(other.numpy(), w.detach().numpy())
    before = len(h.calls)
    w.sum().backward()
    assert h.calls[before:] == ["set_parameters", "initialize", "solve", "vjp"]
    assert np.array_equal(h.theta, theta.detach().numpy()) and np.array_equal(theta.grad.numpy(), h.gradient)
