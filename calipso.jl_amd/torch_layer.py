"""calipso.jl_amd.torch_layer — a batch of conic QPs as a differentiable PyTorch layer (OptNet / cvxpylayers style) over SmallNewtonBatch.

    from calipso_jl_amd.torch_layer import QPLayer
    sn = SmallNewtonBatch(nx, ne, nc, batch)            # (set_cones / options as for solve)
    x = QPLayer.apply(sn, P, q, A, b, G, h)              # min c x'Px + q'x  s.t. Ax = b, h - Gx >= 0
    x, y, z = QPLayer.apply(sn, P, q, A, b, G, h, True)  # with the duals

Every input is a float64 tensor, batched (leading axis = batch) or unbatched and shared by the batch.  The forward pass is one solve! launch of the batch kernel,
the backward pass one reverse-mode differentiate! launch (SmallNewtonBatch.vjp): gradients of shared inputs are summed over the batch.  Tensors travel through
host numpy arrays and come back on the inputs' device.  An instance whose solve did not converge (status != 1) gets NaN gradients, with a warning.  torch is
imported on first use of QPLayer: the package itself loads without it."""
import warnings

import numpy as np

__all__ = ["QPLayer"]

_cls = {}


def _np(t):
    return t.detach().to("cpu", dtype=t.dtype).numpy().astype(np.float64, copy=False) if t is not None else None


def _build():
    import torch

    class QPLayer(torch.autograd.Function):
        """apply(sn, P, q, A, b, G, h, return_duals=False, objective_scale=0.5): the QP solution x (batch, nx), or (x, y, z) with return_duals"""

        @staticmethod
        def forward(ctx, sn, P, q, A, b, G, h, return_duals=False, objective_scale=0.5):
            data = (P, q, A, b, G, h)
            dims = ((sn.nx, sn.nx), (sn.nx,), (sn.ne, sn.nx), (sn.ne,), (sn.nc, sn.nx), (sn.nc,))
            shared = []
            for name, t, dm in zip("PqAbGh", data, dims):
                if t.dtype != torch.float64:
                    raise TypeError("QPLayer: %s must be float64" % name)
                if tuple(t.shape) == dm:
                    shared.append(True)
                elif tuple(t.shape) == (sn.batch,) + dm:
                    shared.append(False)
                else:
                    raise ValueError("QPLayer: %s must be %s or %s" % (name, dm, (sn.batch,) + dm))
            arrays = [_np(t) for t in data]
            all_shared = all(shared)
            if not all_shared:      # (set_qp takes one problem for all or one per instance: the shared inputs are repeated)
                arrays = [np.broadcast_to(a, (sn.batch,) + a.shape) if s else a for a, s in zip(arrays, shared)]
            key = object()
            _solve(sn, arrays, all_shared, objective_scale, key)
            st = sn.get_state()
            w = st["solution"]
            nx, ne, nc = sn.nx, sn.ne, sn.nc
            oy, oz = nx + ne + nc, nx + 2 * ne + nc
            ctx.sn, ctx.key, ctx.arrays, ctx.all_shared, ctx.c = sn, key, arrays, all_shared, objective_scale
            ctx.shared, ctx.status, ctx.device = shared, sn._qp_layer_status.copy(), P.device
            ctx.return_duals = bool(return_duals)
            dev = P.device
            x = torch.from_numpy(w[:, :nx].copy()).to(dev)
            if not return_duals:
                return x
            return x, torch.from_numpy(w[:, oy:oy + ne].copy()).to(dev), torch.from_numpy(w[:, oz:oz + nc].copy()).to(dev)

        @staticmethod
        def backward(ctx, gx, gy=None, gz=None):
            sn = ctx.sn
            if getattr(sn, "_qp_layer_key", None) is not ctx.key:      # the handle solved another batch since: the same data solve again (deterministic)
                _solve(sn, ctx.arrays, ctx.all_shared, ctx.c, ctx.key)
            nx, ne, nc = sn.nx, sn.ne, sn.nc
            oy, oz = nx + ne + nc, nx + 2 * ne + nc
            v = np.zeros((sn.batch, sn.N))
            if gx is not None:
                v[:, :nx] = _np(gx)
            if gy is not None and ne:
                v[:, oy:oy + ne] = _np(gy)
            if gz is not None and nc:
                v[:, oz:oz + nc] = _np(gz)
            out = sn.vjp(v, adjoint=False, qp=True)
            bad = ctx.status != 1
            if bad.any():
                warnings.warn("QPLayer: %d of %d instances did not converge (solve status != 1): their gradients are NaN" % (int(bad.sum()), sn.batch))
            grads = []
            for name, s, need in zip("PqAbGh", ctx.shared, ctx.needs_input_grad[1:7]):
                if not need:
                    grads.append(None)
                    continue
                g = out[name].copy()
                g[bad] = np.nan
                if s:
                    g = g.sum(axis=0)
                grads.append(torch.from_numpy(g).to(ctx.device))
            return (None, *grads, None, None)

    return QPLayer


def _solve(sn, arrays, shared, objective_scale, key):
    sn.set_qp(*arrays, objective_scale=objective_scale, shared=shared)
    sn.initialize(np.zeros((sn.batch, sn.nx)))
    res, _ = sn.solve()
    sn._qp_layer_key, sn._qp_layer_status = key, res


def __getattr__(name):
    if name == "QPLayer":
        if name not in _cls:
            _cls[name] = _build()
        return _cls[name]
    raise AttributeError(name)
