"""calipso.jl_amd.torch_layer — a batch of conic QPs as a differentiable PyTorch layer (OptNet / cvxpylayers style) over SmallNewtonBatch.

    from calipso_jl_amd.torch_layer import QPLayer
    sn = SmallNewtonBatch(nx, ne, nc, batch)            # (set_cones / options as for solve)
    x = QPLayer.apply(sn, P, q, A, b, G, h)              # min c x'Px + q'x  s.t. Ax = b, h - Gx >= 0
    x, y, z = QPLayer.apply(sn, P, q, A, b, G, h, True)  # with the duals

Every input is a float64 tensor, batched (leading axis = batch) or unbatched and shared by the batch.  The forward pass is one solve! launch of the batch kernel,
the backward pass one reverse-mode differentiate! launch (SmallNewtonBatch.vjp): gradients of shared inputs are summed over the batch.  An instance whose solve
did not converge (status != 1) gets NaN gradients.

With CPU tensors the data travel through host numpy arrays, and non-converged instances are reported with a warning.  When EVERY input is a CUDA tensor on the
handle's device the layer takes the device path and never leaves the GPU: the handle is put on torch's current stream (set_stream), the data are packed by a
kernel with each array shared or per instance by its own shape (a shared P is stored once, never broadcast), the solution is gathered on the device
(set_qp_device, initialize_device(None), solve_device, solution_device), and backward is vjp_device with the cotangent parts and the gradients of shared inputs
summed on the device — no host copy and no synchronisation in forward or backward.  The host cannot know the statuses there without waiting, so there is no
warning on that path: sn.status_device() gives the solve statuses as an int32 CUDA tensor (1 = converged) for the caller to look at when it suits.

    w = ParametricLayer.apply(sn, theta)                 # the points (batch, N) of a handle with a device evaluator that provides dR/dtheta; CUDA tensors only

ParametricLayer is the auto-tuning loop of examples/autotuning/cartpole.jl as a layer: forward = set_parameters_device + initialize_device + solve_device,
backward = vjp_device with grad_theta (theta (batch, n_parameters), or (n_parameters,) shared: summed).  torch is imported on first use of a layer: the package
itself loads without it.

    x = SolverQPLayer.apply(solver, P, q, A, b, G, h)    # ONE unbatched QP on a Solver handle (dense, stage-structured or stage-parallel: any size the handle admits)

SolverQPLayer is the same layer over the general path: forward = qp_attach + initialize! with zeros + solve!, backward = Solver.vjp(qp=...) — one transposed
condensed solve for the cotangent and the closed-form data gradients of the inputs that need them.  The data travel through host arrays; a solve that did not
converge gives NaN gradients and a warning, as on the host path of QPLayer.

    x = GroupQPLayer.apply(group, P, q, A, b, G, h)      # a batch of QPs too large for the batch kernel (nx in the hundreds or thousands) on a Group of Solver handles

GroupQPLayer is the batched layer over the general path: every input (count, ...) or unbatched and shared by the members; forward = qp_attach per member + initialize!
with zeros + Group.solve (all members in lockstep through the same launches), backward = ONE Group.vjp(qp=...) for the inputs that need gradients — one factorisation
launch chain and one transposed condensed solve for the whole group instead of one per member.  Gradients of shared inputs are summed over the members on the host, in
member order.  Host tensors only: the handles take host arrays.  Members that did not converge get NaN gradients and one warning counts them.

    x = SparseQPLayer.apply(kkt, P_values, q, A_values, b, G_values, h)   # ONE large sparse QP on a handle from SparseConicQP: no dense block anywhere

SparseQPLayer is the layer over the sparse route: the matrices are given as the VALUES on the stored patterns of the P, A, G the handle was made from (CSC order,
row indices ascending), and their gradients come back on those patterns — no nx x nx array exists in forward or backward.  forward = set_values + attach_qp +
initialize with zeros + solve, backward = ONE SparseKKT.vjp for the cotangent.  Host tensors, or CUDA tensors on the handle's device: then the data, the solution and
the gradients stay on the device and nothing but the solve's own read-backs crosses to the host.  A solve that does not end with status 1 warns and gives NaN gradients.

    w = SparseTrajectoryLayer.apply(handle, theta, x0)   # the point (N,) of a nonlinear problem on a sparse handle whose evaluator provides dR/dtheta

SparseTrajectoryLayer is the auto-tuning loop on the sparse route (TrajectoryProblem.sparse_solver(), or any SparseKKT with set_evaluator + set_parameter_patterns):
forward = set_parameters + initialize + solve, backward = ONE SparseKKT.vjp(theta=True) — dLoss/dtheta from the evaluator's parameter Jacobians on their stored
patterns, with no host evaluation and no dense array of any x num_parameters size.  theta and x0: float64 host tensors, or CUDA tensors on the handle's device (then
theta, the point and the gradient stay on the device).  x0 gets no gradient."""
import warnings

import numpy as np

from ._marshal import QP_NAMES, cotangent_from_parts, dual_rows, qp_shapes

__all__ = ["QPLayer", "ParametricLayer", "SolverQPLayer", "GroupQPLayer", "SparseQPLayer", "SparseTrajectoryLayer"]

_cls = {}


def _np(t):
    return t.detach().to("cpu", dtype=t.dtype).numpy().astype(np.float64, copy=False) if t is not None else None


# ---- what the layers share; `h` is the handle or, for a group, its first member: whatever carries nx, ne, nc --------------------------------------------------------
def _classify(torch, layer, h, data, count=None, host_only=False, shapes=None):
    """the inputs' dtypes and shapes: per input True for the unbatched shape (shared by the items), False for a leading axis of `count`; count None: one item, no
    leading axis admitted.  shapes: the six unbatched shapes where they are not those of the dense QP arrays"""
    shared = []
    for name, t, dm in zip(QP_NAMES, data, shapes or qp_shapes(h.nx, h.ne, h.nc).values()):
        if t.dtype != torch.float64:
            raise TypeError("%s: %s must be float64" % (layer, name))
        if host_only and t.is_cuda:
            raise ValueError("%s: %s must be a host tensor (the handles take host arrays)" % (layer, name))
        if tuple(t.shape) == dm:
            shared.append(True)
        elif count is not None and tuple(t.shape) == (count,) + dm:
            shared.append(False)
        else:
            raise ValueError("%s: %s must be %s" % (layer, name, dm) + (" or %s" % ((count,) + dm,) if count is not None else ""))
    return shared


def _cotangent(h, lead, gx, gy, gz):
    return cotangent_from_parts(_np(gx), _np(gy), _np(gz), lead, h.nx, h.ne, h.nc)


def _outputs(torch, x, y, z, return_duals, device):
    out = [torch.from_numpy(a.copy()).to(device) for a in ((x, y, z) if return_duals else (x,))]
    return tuple(out) if return_duals else out[0]


def _want(ctx):
    """the names of the inputs that need a gradient"""
    return "".join(name for name, need in zip(QP_NAMES, ctx.needs_input_grad[1:7]) if need)


def _solved_again(handle, ctx, solve, modified=None):
    """the handle solved other data since forward: the same data solve again (deterministic), and True.  modified: the layer kept the input tensors themselves, not
    copies — the text of the error if one of them was written to since"""
    if getattr(handle, "_qp_layer_key", None) is not ctx.key:
        if modified and any(t._version != v for t, v in zip(ctx.inputs, ctx.versions)):
            raise RuntimeError(modified)
        solve()
        return True
    return False


def _gradients(torch, out, want, shared, bad, warning, reduce, device):
    """vjp()'s arrays -> the gradients of the six inputs: None where none is wanted, NaN for the items of the mask `bad` (a 0-d mask: the one item) with ONE warning,
    then shared inputs summed over the items by `reduce`"""
    bad = np.asarray(bad)
    if bad.any():
        warnings.warn(warning)
    grads = []
    for name, s in zip(QP_NAMES, shared):
        if name not in want:
            grads.append(None)
            continue
        g = out[name].copy()
        g[bad] = np.nan
        if s and reduce:
            g = reduce(g)
        grads.append(torch.from_numpy(np.ascontiguousarray(g)).to(device))
    return grads


def _sum_in_member_order(g):
    acc = g[0].copy()
    for i in range(1, g.shape[0]):
        acc += g[i]
    return acc


def _build():
    import torch

    class QPLayer(torch.autograd.Function):
        """apply(sn, P, q, A, b, G, h, return_duals=False, objective_scale=0.5): the QP solution x (batch, nx), or (x, y, z) with return_duals"""

        @staticmethod
        def forward(ctx, sn, P, q, A, b, G, h, return_duals=False, objective_scale=0.5):
            data = (P, q, A, b, G, h)
            shared = _classify(torch, "QPLayer", sn, data, sn.batch)
            if all(t.is_cuda and t.device.index == sn.device for t in data):      # the device path: nothing leaves the GPU, nothing waits for it
                tensors = [t.detach().contiguous() for t in data]
                key = object()
                _solve_device(torch, sn, tensors, objective_scale, key)
                sol = sn.solution_device(parts="xyz" if return_duals else "x")
                ctx.sn, ctx.key, ctx.tensors, ctx.c, ctx.shared, ctx.on_device = sn, key, tensors, objective_scale, shared, True
                ctx.inputs, ctx.versions = data, [t._version for t in data]      # (ctx.tensors may alias the inputs' storage: the re-solve in backward checks them)
                return (sol["x"], sol["y"], sol["z"]) if return_duals else sol["x"]
            ctx.on_device = False
            arrays = [_np(t) for t in data]
            all_shared = all(shared)
            if not all_shared:      # (set_qp takes one problem for all or one per instance: the shared inputs are repeated)
                arrays = [np.broadcast_to(a, (sn.batch,) + a.shape) if s else a for a, s in zip(arrays, shared)]
            key = object()
            _solve(sn, arrays, all_shared, objective_scale, key)
            ctx.sn, ctx.key, ctx.arrays, ctx.all_shared, ctx.c = sn, key, arrays, all_shared, objective_scale
            ctx.shared, ctx.status, ctx.device = shared, sn._qp_layer_status.copy(), P.device
            w = sn.get_state()["solution"]
            oy, oz = dual_rows(sn.nx, sn.ne, sn.nc)
            return _outputs(torch, w[:, :sn.nx], w[:, oy:oy + sn.ne], w[:, oz:oz + sn.nc], return_duals, P.device)

        @staticmethod
        def backward(ctx, gx, gy=None, gz=None):
            sn = ctx.sn
            if ctx.on_device:
                if not _solved_again(sn, ctx, lambda: _solve_device(torch, sn, ctx.tensors, ctx.c, ctx.key), "QPLayer: an input was modified in place after forward and the "
                                     "handle has solved another batch since: backward cannot solve the same data again"):
                    sn.set_stream(torch.cuda.current_stream(ctx.tensors[0].device))
                part = lambda g, n: g.contiguous() if (g is not None and n) else None
                out = sn.vjp_device(x=part(gx, sn.nx), y=part(gy, sn.ne), z=part(gz, sn.nc), qp=_want(ctx), reduce="".join(name for name, s in zip(QP_NAMES, ctx.shared) if s))
                return (None, *[out.get(name) for name in QP_NAMES], None, None)
            _solved_again(sn, ctx, lambda: _solve(sn, ctx.arrays, ctx.all_shared, ctx.c, ctx.key))
            out = sn.vjp(_cotangent(sn, (sn.batch,), gx, gy, gz), adjoint=False, qp=True)
            bad = ctx.status != 1
            warning = "QPLayer: %d of %d instances did not converge (solve status != 1): their gradients are NaN" % (int(bad.sum()), sn.batch)
            return (None, *_gradients(torch, out, _want(ctx), ctx.shared, bad, warning, lambda g: g.sum(axis=0), ctx.device), None, None)

    class ParametricLayer(torch.autograd.Function):
        """apply(sn, theta, x0=None): the points w (batch, N) of solve! with the handle's device evaluator at the parameters theta (CUDA, float64; (batch,
        n_parameters) or (n_parameters,) shared by the batch); x0 (batch, nx): the guess of initialize!, zeros by default"""

        @staticmethod
        def forward(ctx, sn, theta, x0=None):
            if not theta.is_cuda:
                raise ValueError("ParametricLayer: theta must be a CUDA tensor (the layer has no host path)")
            th = theta.detach().contiguous()
            x0 = x0.detach().contiguous() if x0 is not None else None
            key = object()
            _solve_parameters(torch, sn, th, x0, key)
            ctx.sn, ctx.key, ctx.theta, ctx.x0 = sn, key, th, x0
            ctx.inputs, ctx.versions = (theta,), [theta._version]
            return sn.solution_device(parts="w")["w"]

        @staticmethod
        def backward(ctx, gw):
            sn = ctx.sn
            if not _solved_again(sn, ctx, lambda: _solve_parameters(torch, sn, ctx.theta, ctx.x0, ctx.key), "ParametricLayer: theta was modified in place after forward and "
                                 "the handle has solved another batch since: backward cannot solve the same data again"):
                sn.set_stream(torch.cuda.current_stream(ctx.theta.device))
            g = sn.vjp_device(cotangent=gw.contiguous(), theta=True, qp=False)["theta"]
            return None, (g.sum(dim=0) if ctx.theta.dim() == 1 else g), None

    class SolverQPLayer(torch.autograd.Function):
        """apply(solver, P, q, A, b, G, h, return_duals=False, objective_scale=0.5): the solution x (nx,) of one QP on a Solver handle, or (x, y, z) with return_duals"""

        @staticmethod
        def forward(ctx, solver, P, q, A, b, G, h, return_duals=False, objective_scale=0.5):
            data = (P, q, A, b, G, h)
            _classify(torch, "SolverQPLayer", solver, data)
            arrays = [_np(t) for t in data]
            key = object()
            _solve_handle(solver, arrays, objective_scale, key)
            ctx.solver, ctx.key, ctx.arrays, ctx.c, ctx.converged, ctx.device = solver, key, arrays, objective_scale, solver._qp_layer_converged, P.device
            w = solver.solution
            return _outputs(torch, w.variables, w.equality_dual, w.cone_dual, return_duals, P.device)

        @staticmethod
        def backward(ctx, gx, gy=None, gz=None):
            solver, want = ctx.solver, _want(ctx)
            _solved_again(solver, ctx, lambda: _solve_handle(solver, ctx.arrays, ctx.c, ctx.key))
            v = _cotangent(solver, (), gx, gy, gz)
            out = solver.vjp(v, adjoint=False, theta=False, qp=want) if want else {}
            warning = "SolverQPLayer: the solve did not converge: the gradients are NaN"
            return (None, *_gradients(torch, out, want, (False,) * 6, not ctx.converged, warning, None, ctx.device), None, None)

    class GroupQPLayer(torch.autograd.Function):
        """apply(group, P, q, A, b, G, h, return_duals=False, objective_scale=0.5): the solutions x (count, nx) of one QP per member of a Group, or (x, y, z) with
        return_duals.  Inputs: float64 HOST tensors (the handles take host arrays), batched (count, ...) or unbatched and shared by the members"""

        @staticmethod
        def forward(ctx, group, P, q, A, b, G, h, return_duals=False, objective_scale=0.5):
            s0, count = group.solvers[0], len(group.solvers)
            data = (P, q, A, b, G, h)
            shared = _classify(torch, "GroupQPLayer", s0, data, count, host_only=True)
            arrays = [_np(t).copy() for t in data]
            key = object()
            _solve_group(group, arrays, shared, objective_scale, key)
            ctx.group, ctx.key, ctx.arrays, ctx.shared, ctx.c, ctx.converged = group, key, arrays, shared, objective_scale, group._qp_layer_converged.copy()
            W = [s.solution for s in group.solvers]
            return _outputs(torch, *[np.stack([getattr(w, part) for w in W]) for part in ("variables", "equality_dual", "cone_dual")], return_duals, "cpu")

        @staticmethod
        def backward(ctx, gx, gy=None, gz=None):
            group, want = ctx.group, _want(ctx)
            _solved_again(group, ctx, lambda: _solve_group(group, ctx.arrays, ctx.shared, ctx.c, ctx.key))
            count = len(group.solvers)
            v = _cotangent(group.solvers[0], (count,), gx, gy, gz)
            out = group.vjp(v, adjoint=False, theta=False, qp=want) if want else {}
            bad = ~ctx.converged
            warning = "GroupQPLayer: %d of %d members did not converge: their gradients are NaN" % (int(bad.sum()), count)
            return (None, *_gradients(torch, out, want, ctx.shared, bad, warning, _sum_in_member_order, "cpu"), None, None)

    class SparseQPLayer(torch.autograd.Function):
        """apply(kkt, P_values, q, A_values, b, G_values, h, return_duals=False): the solution x (nx,) of one sparse QP on a handle from SparseConicQP, or (x, y, z) with
        return_duals.  P_values, A_values, G_values: the values on the stored patterns of the P, A, G the handle was made from"""

        @staticmethod
        def forward(ctx, kkt, P_values, q, A_values, b, G_values, h, return_duals=False):
            data = (P_values, q, A_values, b, G_values, h)
            if not hasattr(kkt, "_conic_qp"):
                raise ValueError("SparseQPLayer: the handle must come from SparseConicQP")
            shapes = [(int(kkt._conic_qp[0].size),), (kkt.nx,), (kkt.nnz[1],), (kkt.ne,), (kkt.nnz[2],), (kkt.nc,)]
            _classify(torch, "SparseQPLayer", kkt, data, shapes=shapes)
            on_device = all(t.is_cuda and t.device.index == kkt.device for t in data)
            if not on_device and any(t.is_cuda for t in data):
                raise ValueError("SparseQPLayer: the inputs are all host tensors or all CUDA tensors on the handle's device")
            tensors = [t.detach().contiguous() if on_device else _np(t) for t in data]
            key = object()
            _solve_sparse(torch, kkt, tensors, on_device, key)
            ctx.kkt, ctx.key, ctx.tensors, ctx.on_device, ctx.converged, ctx.device = kkt, key, tensors, on_device, kkt._qp_layer_converged, q.device
            ctx.inputs, ctx.versions = data, [t._version for t in data]
            oy, oz = dual_rows(kkt.nx, kkt.ne, kkt.nc)
            if on_device:
                w = kkt.solution_device()
                out = (w[:kkt.nx].clone(), w[oy:oy + kkt.ne].clone(), w[oz:oz + kkt.nc].clone())
                return out if return_duals else out[0]
            w = kkt.get("solution")
            return _outputs(torch, w[:kkt.nx], w[oy:oy + kkt.ne], w[oz:oz + kkt.nc], return_duals, q.device)

        @staticmethod
        def backward(ctx, gx, gy=None, gz=None):
            kkt, want = ctx.kkt, _want(ctx)
            _solved_again(kkt, ctx, lambda: _solve_sparse(torch, kkt, ctx.tensors, ctx.on_device, ctx.key), "SparseQPLayer: an input was modified in place after forward and the "
                          "handle has solved other data since: backward cannot solve the same data again" if ctx.on_device else None)
            warning = "SparseQPLayer: the solve did not converge (status != 1): the gradients are NaN"
            if not ctx.on_device:
                out = kkt.vjp(_cotangent(kkt, (), gx, gy, gz), adjoint=False, qp=want) if want else {}
                return (None, *_gradients(torch, out, want, (False,) * 6, not ctx.converged, warning, None, ctx.device), None)
            oy, oz = dual_rows(kkt.nx, kkt.ne, kkt.nc)
            v = torch.zeros(kkt.N, dtype=torch.float64, device=ctx.device)
            for g, at, n in ((gx, 0, kkt.nx), (gy, oy, kkt.ne), (gz, oz, kkt.nc)):
                if g is not None and n:
                    v[at:at + n] = g
            out = kkt.vjp(v, adjoint=False, qp=want) if want else {}
            if not ctx.converged:
                warnings.warn(warning)
                out = {name: torch.full_like(g, float("nan")) for name, g in out.items()}
            return (None, *[out[name].contiguous() if name in out else None for name in QP_NAMES], None)

    class SparseTrajectoryLayer(torch.autograd.Function):
        """apply(handle, theta, x0): the point w (N,) solve! returns for the parameters theta (num_parameters,) from the initial variables x0 (nx,), on a SparseKKT whose
        evaluator provides dR/dtheta (set_parameter_patterns; TrajectoryProblem.sparse_solver() sets them)"""

        @staticmethod
        def forward(ctx, handle, theta, x0):
            if not handle._has_parameter_patterns():
                raise ValueError("SparseTrajectoryLayer: the handle needs an evaluator with parameters and set_parameter_patterns (TrajectoryProblem.sparse_solver() sets them)")
            for name, t, n in (("theta", theta, handle.num_parameters), ("x0", x0, handle.nx)):
                if t.dtype != torch.float64:
                    raise TypeError("SparseTrajectoryLayer: %s must be float64" % name)
                if tuple(t.shape) != (n,):
                    raise ValueError("SparseTrajectoryLayer: %s must be (%d,)" % (name, n))
            on_device = all(t.is_cuda and t.device.index == handle.device for t in (theta, x0))
            if not on_device and (theta.is_cuda or x0.is_cuda):
                raise ValueError("SparseTrajectoryLayer: theta and x0 are both host tensors or both CUDA tensors on the handle's device")
            tensors = [t.detach().contiguous() if on_device else _np(t).copy() for t in (theta, x0)]
            key = object()
            _solve_sparse_parameters(handle, tensors, key)
            ctx.handle, ctx.key, ctx.tensors, ctx.on_device, ctx.converged, ctx.device = handle, key, tensors, on_device, handle._qp_layer_converged, theta.device
            ctx.inputs, ctx.versions = (theta, x0), [t._version for t in (theta, x0)]
            return handle.solution_device() if on_device else torch.from_numpy(handle.get("solution").copy()).to(theta.device)

        @staticmethod
        def backward(ctx, gw):
            handle = ctx.handle
            _solved_again(handle, ctx, lambda: _solve_sparse_parameters(handle, ctx.tensors, ctx.key), "SparseTrajectoryLayer: an input was modified in place after forward "
                          "and the handle has solved other data since: backward cannot solve the same data again" if ctx.on_device else None)
            if not ctx.needs_input_grad[1]:
                return None, None, None
            g = handle.vjp(gw.detach().contiguous() if ctx.on_device else _np(gw), adjoint=False, theta=True)["theta"]
            if not ctx.on_device:
                g = torch.from_numpy(np.ascontiguousarray(g)).to(ctx.device)
            if not ctx.converged:
                warnings.warn("SparseTrajectoryLayer: the solve did not converge (status != 1): the gradient is NaN")
                g = torch.full_like(g, float("nan"))
            return None, g.contiguous(), None

    return {"QPLayer": QPLayer, "ParametricLayer": ParametricLayer, "SolverQPLayer": SolverQPLayer, "GroupQPLayer": GroupQPLayer, "SparseQPLayer": SparseQPLayer,
            "SparseTrajectoryLayer": SparseTrajectoryLayer}


def _solve_device(torch, sn, tensors, objective_scale, key):
    sn.set_stream(torch.cuda.current_stream(tensors[0].device))
    sn.set_qp_device(*tensors, objective_scale=objective_scale)
    sn.initialize_device(None)
    sn.solve_device()
    sn._qp_layer_key, sn._qp_layer_status = key, None


def _solve_parameters(torch, sn, theta, x0, key):
    sn.set_stream(torch.cuda.current_stream(theta.device))
    sn.set_parameters_device(theta)
    sn.initialize_device(x0)
    sn.solve_device()
    sn._qp_layer_key, sn._qp_layer_status = key, None


def _solve_handle(solver, arrays, objective_scale, key):
    from . import initialize_b, solve_b
    solver.qp_attach(*arrays, objective_scale=objective_scale)
    initialize_b(solver, np.zeros(solver.nx))
    converged = solve_b(solver)
    solver._qp_layer_key, solver._qp_layer_converged = key, bool(converged)


def _solve_group(group, arrays, shared, objective_scale, key):
    from . import initialize_b
    for i, solver in enumerate(group.solvers):
        solver.qp_attach(*[a if s else a[i] for a, s in zip(arrays, shared)], objective_scale=objective_scale)
        initialize_b(solver, np.zeros(solver.nx))
    res = group.solve()
    group._qp_layer_key, group._qp_layer_converged = key, np.array([r == 1 for r in res])


def _solve_sparse(torch, kkt, data, on_device, key):
    """data: the six inputs as numpy arrays, or as CUDA tensors on the handle's device: Lxx = c (P + P') on its own pattern from P's values, gx = A, hx = -G"""
    Pv, q, Av, b, Gv, h = data
    ij, ji, c = kkt._conic_qp_positions(on_device)
    if on_device:
        Lxx = torch.zeros(kkt.nnz[0], dtype=torch.float64, device=Pv.device)
        Lxx.index_add_(0, ij, c * Pv)      # (the positions of a pattern are distinct: each add touches an entry once, in a fixed order)
        Lxx.index_add_(0, ji, c * Pv)
        x0 = torch.zeros(kkt.nx, dtype=torch.float64, device=Pv.device)
        pick = lambda t, n: t if n else None      # (an empty tensor has no device pointer to check)
        kkt.set_values(pick(Lxx, kkt.nnz[0]), pick(Av, kkt.nnz[1]), pick(-Gv, kkt.nnz[2]))
        kkt.attach_qp(q, pick(b, kkt.ne), pick(h, kkt.nc))
    else:
        Lxx = np.zeros(kkt.nnz[0])
        Lxx[ij] += c * Pv
        Lxx[ji] += c * Pv
        x0 = np.zeros(kkt.nx)
        kkt.set_values(Lxx, Av, -Gv)
        kkt.attach_qp(q, b, h)
    kkt.initialize(x0)
    status, _ = kkt.solve()
    kkt._qp_layer_key, kkt._qp_layer_converged = key, status == 1


def _solve_sparse_parameters(kkt, data, key):
    """data: theta and x0 as numpy arrays, or as CUDA tensors on the handle's device"""
    theta, x0 = data
    kkt.set_parameters(theta)
    kkt.initialize(x0)
    status, _ = kkt.solve()
    kkt._qp_layer_key, kkt._qp_layer_converged = key, status == 1


def _solve(sn, arrays, shared, objective_scale, key):
    sn.set_qp(*arrays, objective_scale=objective_scale, shared=shared)
    sn.initialize(np.zeros((sn.batch, sn.nx)))
    res, _ = sn.solve()
    sn._qp_layer_key, sn._qp_layer_status = key, res


def __getattr__(name):
    if name in __all__:
        if name not in _cls:
            _cls.update(_build())
        return _cls[name]
    raise AttributeError(name)
