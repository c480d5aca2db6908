"""calipso.jl_amd._marshal — the index layouts between numpy arrays in the user's shapes and the flat buffers of the C ABI, once: plain numpy, no ctypes, no torch,
no handle.  Solver.vjp (lead = ()), Group.vjp (lead = (count,)), SmallNewtonBatch.vjp / vjp_device (lead = (batch,)) and the layers of torch_layer read them.

The C side stores, per item of `lead` and per cotangent column j < k, one block per array — a vector as it is, a matrix r x c column-major — with k outermost in
the item; Python shows lead + shape [+ (k,)]."""
import numpy as np

QP_NAMES = "PqAbGh"


def qp_shapes(nx, ne, nc):
    """the arrays of the QP  min c x'Px + q'x  s.t. Ax = b, h - Gx >= 0  by name (qp_attach / set_qp)"""
    return dict(P=(nx, nx), q=(nx,), A=(ne, nx), b=(ne,), G=(nc, nx), h=(nc,))


def qp_names(qp):
    """True / None or False / names -> the validated names"""
    names = QP_NAMES if qp is True else (qp or "")
    if any(c not in QP_NAMES for c in names):
        raise ValueError("qp must be True or a string of names out of 'PqAbGh'")
    return names


def pack_cotangent(v, lead, N, message, also=None):
    """v of shape lead + (N,) or lead + (N, k) -> (flat buffer: per item column-major N x k, k, squeeze = v had no k axis).  also: a second admissible row count,
    the leading rows alone, the others zero.  message: the ValueError text of the caller"""
    v = np.asarray(v, dtype=np.float64)
    lead = tuple(lead)
    squeeze = v.ndim == len(lead) + 1
    if squeeze:
        v = v[..., None]
    if v.ndim != len(lead) + 2 or v.shape[:-2] != lead or v.shape[-2] not in (N, also):
        raise ValueError(message)
    k = v.shape[-1]
    if v.shape[-2] != N:
        w = np.zeros(lead + (N, k))
        w[..., :also, :] = v
        v = w
    return np.ascontiguousarray(np.swapaxes(v, -1, -2)).ravel(), k, squeeze


def unpack_columns(flat, lead, k, shape, squeeze):
    """the inverse for an output array: the first prod(lead) * k * prod(shape) doubles of `flat` -> lead + shape [+ (k,) unless squeeze], a copy.  shape: (n,) for a
    vector, (r, c) for a matrix stored column-major per column"""
    lead, shape = tuple(lead), tuple(shape)
    a = np.ravel(flat)[:int(np.prod(lead + (k,) + shape))].reshape(lead + (k,) + shape[::-1])
    nl = len(lead)
    a = np.transpose(a, tuple(range(nl)) + tuple(range(nl + len(shape), nl, -1)) + (nl,)).copy()
    return a[..., 0] if squeeze else a


def dual_rows(nx, ne, nc):
    """where the equality duals y and the cone duals z start in a point w = (x, r, s, y, z, t)"""
    oy, oz = nx + ne + nc, nx + 2 * ne + nc
    return oy, oz


def cotangent_from_parts(gx, gy, gz, lead, nx, ne, nc):
    """the cotangent lead + (N,) of a loss that sees x, the equality duals y and the cone duals z only (None: not at all), zeros in the other rows"""
    oy, oz = dual_rows(nx, ne, nc)
    v = np.zeros(tuple(lead) + (nx + 2 * ne + 3 * nc,))
    for g, at, n in ((gx, 0, nx), (gy, oy, ne), (gz, oz, nc)):
        if g is not None and n:
            v[..., at:at + n] = g
    return v
