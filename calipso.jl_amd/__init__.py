"""calipso.jl_amd — MI355X (gfx950) implementation of CALIPSO's Newton/KKT hot path behind the reference's
Solver / initialize! / solve! surface (thowell/CALIPSO.jl, src/CALIPSO.jl:48-50).

This Python module is the host-side mirror used where Julia is unavailable (the Julia `ccall` module with the same
surface is in julia/CalipsoHIP.jl).  It keeps the reference's names: `Solver`, `Options`, `initialize_b` (= initialize!),
`solve_b` (= solve!), and the field names of `solver.solution`, `solver.data`, `solver.problem`.  All arithmetic of the hot
path runs in libcalipso_hip.so (hand-written HIP); this module only moves user-evaluated data across the C ABI.
"""
import ctypes as C

import numpy as np

from ._lib import CALLBACK_FN, EVAL_FN, CalipsoHipError, lib
from ._marshal import QP_NAMES, pack_cotangent, qp_names, qp_shapes, unpack_columns

__all__ = ["Solver", "Group", "LDLSolver", "SmallBatch", "SparseKKT", "SparseKKTGroup", "SparseConicQP", "SparseConicQPGroup", "Comm", "ordering", "symbolic", "Options", "initialize_b", "solve_b", "CalipsoHipError", "FLAGS", "splitmix_uniform",
           "mfma_f64_peak"]

# evaluate! flags (include/calipso_hip.h)
FLAGS = dict(
    objective=1 << 0, objective_gradient_variables=1 << 1, objective_jacobian_variables_variables=1 << 2,
    equality_constraint=1 << 3, equality_jacobian_variables=1 << 4, equality_dual_jacobian_variables=1 << 5,
    equality_dual_jacobian_variables_variables=1 << 6, cone_constraint=1 << 7, cone_jacobian_variables=1 << 8,
    cone_dual_jacobian_variables=1 << 9, cone_dual_jacobian_variables_variables=1 << 10,
    objective_jacobian_variables_parameters=1 << 11, equality_jacobian_parameters=1 << 12,
    equality_dual_jacobian_variables_parameters=1 << 13, cone_jacobian_parameters=1 << 14,
    cone_dual_jacobian_variables_parameters=1 << 15)
CONE_BARRIER, CONE_BARRIER_GRADIENT, CONE_PRODUCT, CONE_JACOBIAN, CONE_TARGET = 1, 2, 4, 8, 16

STATUS_TEXT = {-1: "inertia correction failure", -2: "cone search failure", -3: "evaluation callback failed",
               -4: "bad argument", -5: "HIP error", -6: "cone layout not supported"}


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _opt(a):
    return _pd(a) if a is not None else None


class _Handle:
    """what the classes around a handle of the library share: the status check and the release.  Class attributes name the attribute that holds the handle, the
    library's last_error and destroy entries for it and the text of the error; nothing here needs an __init__"""
    _handle, _last_error, _destroy, _message = "_h", "calipso_hip_last_error", "calipso_hip_destroy", "%(what)s failed (%(rc)d): %(text)s"
    _STATUS_MESSAGE = "%(what)s: %(status)s (%(rc)d): %(text)s"      # the classes whose statuses are the CALIPSO_ERR_* of STATUS_TEXT

    def _error_text(self):
        return getattr(self._L, self._last_error)(getattr(self, self._handle)).decode()

    def _check(self, rc, what):
        if rc < 0:
            raise CalipsoHipError(self._message % dict(what=what, status=STATUS_TEXT.get(rc, "error"), rc=rc, text=self._error_text()))
        return rc

    def close(self):
        h = getattr(self, self._handle, None)
        if h is not None and h.value:
            getattr(self._L, self._destroy)(h)
            setattr(self, self._handle, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _vjp(handle, lead, cotangent, adjoint, theta, qp, message, call):
    """the body of Solver.vjp (lead = ()) and Group.vjp (lead = (count,)) for a `handle` with nx, ne, nc, np, N: pack the cotangent, size the buffers, call(k,
    cotangent, adjoint, theta, the six QP pointers) — the C entry —, and unpack what it wrote into lead + shape [+ (k,)]"""
    vc, k, squeeze = (None, 1, True) if cotangent is None else pack_cotangent(cotangent, lead, handle.N, message)
    if theta is None:
        theta = handle.np > 0
    names = qp_names(qp)
    shape = qp_shapes(handle.nx, handle.ne, handle.nc)
    columns = int(np.prod(lead, dtype=np.int64)) * max(k, 1)
    adj = np.zeros(columns * handle.N) if adjoint else None
    gth = np.zeros(max(columns * handle.np, 1)) if theta else None
    arrays = {c: np.zeros(max(columns * int(np.prod(shape[c])), 1)) for c in names}
    ptrs = (C.POINTER(C.c_double) * 6)(*[_pd(arrays[c]) if c in arrays else None for c in QP_NAMES]) if names else None
    call(int(k), _opt(vc), _opt(adj), _opt(gth), ptrs)
    out = {}
    if adjoint:
        out["adjoint"] = unpack_columns(adj, lead, k, (handle.N,), squeeze)
    if theta:
        out["theta"] = unpack_columns(gth, lead, k, (handle.np,), squeeze)
    for c in names:
        out[c] = unpack_columns(arrays[c], lead, k, shape[c], squeeze)
    return out


def splitmix_uniform(problem_id, stream_id, lo, hi, count):
    """SplitMix64 uniform stream of the synthetic benchmark problems (host function of the library)."""
    out = np.empty(int(count), dtype=np.float64)
    lib().calipso_hip_splitmix_uniform(problem_id, stream_id, lo, hi, int(count), _pd(out))
    return out


class Options(dict):
    """Options(...) of src/solver/options.jl:6-59 — keyword arguments override the reference defaults held by the library."""

    def __init__(self, **kw):
        super().__init__(**kw)


class _Point:
    """read-only snapshot of a Point (src/solver/point.jl:1-22)"""

    def __init__(self, w, nx, ne, nc):
        o = np.cumsum([0, nx, ne, nc, ne, nc, nc])
        self.all = w
        self.variables = w[o[0]:o[1]]
        self.equality_slack = w[o[1]:o[2]]
        self.cone_slack = w[o[2]:o[3]]
        self.equality_dual = w[o[3]:o[4]]
        self.cone_dual = w[o[4]:o[5]]
        self.cone_slack_dual = w[o[5]:o[6]]
        self.primals = w[:o[3]]


class _Dims:
    pass


class Solver(_Handle):
    """Solver(methods, num_variables, num_parameters, num_equality, num_cone; parameters, nonnegative_indices,
    second_order_indices, options)  — src/solver/solver.jl:46-150.

    `methods` stands in for ProblemMethods (src/solver/methods.jl): an object with
    evaluate(flags, x, y, z, theta, out) writing the requested ProblemData fields through out(name)."""
    _message = _Handle._STATUS_MESSAGE

    def __init__(self, methods, num_variables, num_parameters, num_equality, num_cone, parameters=None,
                 nonnegative_indices=None, second_order_indices=None, options=None, device=0, structure=None):
        """structure = dict(row_first, row_last, hessian_block_start) (1-based) makes a STRUCTURED handle (calipso_hip_create_structured): only the
        stage blocks live on the device"""
        L = lib()
        self._L = L
        nx, npar, ne, nc = int(num_variables), int(num_parameters), int(num_equality), int(num_cone)
        if nonnegative_indices is None:
            nonnegative_indices = list(range(1, nc + 1))
        if second_order_indices is None:
            second_order_indices = [[]]
        nn = np.asarray(list(nonnegative_indices), dtype=np.int64)
        ptr = np.zeros(len(second_order_indices) + 1, dtype=np.int64)
        flat = []
        for k, c in enumerate(second_order_indices):
            flat.extend(c)
            ptr[k + 1] = len(flat)
        flat = np.asarray(flat, dtype=np.int64)
        h = C.c_void_p()
        self.structure = structure
        if structure is not None:
            rf = np.ascontiguousarray(structure["row_first"], dtype=np.int64); rl = np.ascontiguousarray(structure["row_last"], dtype=np.int64)
            hb = np.ascontiguousarray(structure["hessian_block_start"], dtype=np.int64)
            assert rf.size == ne + nc and rl.size == ne + nc
            rc = L.calipso_hip_create_structured(nx, npar, ne, nc, len(nn), _pi(nn), len(second_order_indices), _pi(ptr), _pi(flat), device, _pi(rf), _pi(rl),
                                                 hb.size, _pi(hb), C.byref(h))
        else:
            rc = L.calipso_hip_create(nx, npar, ne, nc, len(nn), _pi(nn), len(second_order_indices), _pi(ptr), _pi(flat), device, C.byref(h))
        if rc != 0:
            msg = L.calipso_hip_last_error(h if h.value else None).decode()
            if h.value:
                L.calipso_hip_destroy(h)
            raise CalipsoHipError("calipso_hip_create failed (%d): %s" % (rc, msg))
        self._h = h
        self.methods = methods
        self.dimensions = _Dims()
        d = self.dimensions
        d.variables, d.parameters, d.equality_slack, d.cone_slack = nx, npar, ne, nc
        d.equality_dual, d.cone_dual, d.cone_slack_dual = ne, nc, nc
        d.symmetric = d.primal = nx + ne + nc
        d.total = nx + 2 * ne + 3 * nc
        self.nx, self.np, self.ne, self.nc, self.n, self.N = nx, npar, ne, nc, d.symmetric, d.total
        self.indices = {k: self.index(k) for k in ("variables", "equality_slack", "cone_slack", "equality_dual", "cone_dual",
                                                    "cone_slack_dual", "symmetric_equality", "symmetric_cone", "primals", "duals",
                                                    "violation_equality", "violation_cone", "parameters", "cone_nonnegative",
                                                    "cone_second_order", "cone_second_order_ptr")}
        # host ProblemData (problem_data.jl:33-100) that the user functions fill
        z = np.zeros
        self.problem = dict(
            objective=z(1), objective_gradient_variables=z(nx), objective_jacobian_variables_variables=z(nx * nx),
            objective_jacobian_variables_parameters=z(nx * npar), equality_constraint=z(ne), equality_jacobian_variables=z(ne * nx),
            equality_jacobian_parameters=z(ne * npar), equality_dual_jacobian_variables=z(nx),
            equality_dual_jacobian_variables_variables=z(nx * nx), equality_dual_jacobian_variables_parameters=z(nx * npar),
            cone_constraint=z(nc), cone_jacobian_variables=z(nc * nx), cone_jacobian_parameters=z(nc * npar),
            cone_dual_jacobian_variables=z(nx), cone_dual_jacobian_variables_variables=z(nx * nx),
            cone_dual_jacobian_variables_parameters=z(nx * npar))
        self.parameters = np.zeros(npar) if parameters is None else np.asarray(parameters, dtype=np.float64).copy()
        if npar:
            self.set("parameters", self.parameters)
        self.options = {}
        for k, v in (options or {}).items():
            self.set_option(k, v)
        self._cb = EVAL_FN(self._evaluate_callback)

    # ---- plumbing ---------------------------------------------------------------------------------------------
    def set(self, name, arr):
        a = np.ascontiguousarray(np.asarray(arr, dtype=np.float64).reshape(-1))
        self._check(self._L.calipso_hip_set_field(self._h, name.encode(), _pd(a), a.size), "set_field(%s)" % name)

    def get(self, name, length):
        out = np.zeros(int(length), dtype=np.float64)
        self._check(self._L.calipso_hip_get_field(self._h, name.encode(), _pd(out), out.size), "get_field(%s)" % name)
        return out

    def scalar(self, name):
        return float(self.get(name, 1)[0])

    def set_option(self, name, value):
        self.options[name] = value
        self.set("opt." + name, [float(value)])

    def index(self, name):
        n = self._L.calipso_hip_get_index(self._h, name.encode(), None, 0)
        if n < 0:
            raise KeyError(name)
        out = np.zeros(max(int(n), 1), dtype=np.int64)
        self._L.calipso_hip_get_index(self._h, name.encode(), _pi(out), n)
        return out[:n]

    def _out(self, name):
        return self.problem[name]

    _UPLOAD = [("objective", "objective"), ("objective_gradient_variables", "objective_gradient_variables"),
               ("equality_constraint", "equality_constraint"), ("equality_jacobian_variables", "equality_jacobian_variables"),
               ("equality_dual_jacobian_variables", "equality_dual_jacobian_variables"), ("cone_constraint", "cone_constraint"),
               ("cone_jacobian_variables", "cone_jacobian_variables"), ("cone_dual_jacobian_variables", "cone_dual_jacobian_variables"),
               ("equality_jacobian_parameters", "equality_jacobian_parameters"), ("cone_jacobian_parameters", "cone_jacobian_parameters")]

    # ---- sparse scatter of evaluate! (evaluate.jl:37-121): value caches + registered index lists instead of dense blocks ---------------
    def set_sparsity(self, field, rows, cols):
        """methods.<field>_sparsity: 1-based (row, col) lists in cache order; duplicates allowed (the last writer wins)"""
        r = np.ascontiguousarray(rows, dtype=np.int64); c = np.ascontiguousarray(cols, dtype=np.int64)
        self._check(self._L.calipso_hip_set_sparsity(self._h, field.encode(), r.size, _pi(r), _pi(c)), "set_sparsity(%s)" % field)

    def scatter_field(self, field, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        self._check(self._L.calipso_hip_scatter_field(self._h, field.encode(), _pd(v), v.size), "scatter_field(%s)" % field)

    def scatter_hessian(self, objective=None, equality_dual=None, cone_dual=None):
        a = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (objective, equality_dual, cone_dual)]
        args = []
        for v in a:
            args += [_pd(v) if v is not None else None, 0 if v is None else v.size]
        self._check(self._L.calipso_hip_scatter_hessian(self._h, *args), "scatter_hessian")

    def upload(self, flags):
        """hand the flagged ProblemData fields to the device (the tail of evaluate!, src/solver/evaluate.jl:37-121)"""
        p = self.problem
        for key, field in self._UPLOAD:
            if flags & FLAGS[key] and p[key].size:
                self.set(field, p[key])
        hess = FLAGS["objective_jacobian_variables_variables"] | FLAGS["equality_dual_jacobian_variables_variables"] | FLAGS["cone_dual_jacobian_variables_variables"]
        if flags & hess:
            # Lxx = fxx + (g'y)xx + (h'z)xx  (residual_jacobian_variables.jl:10-16; tensor terms iff options.constraint_tensor)
            L = p["objective_jacobian_variables_variables"].copy()
            if self.options.get("constraint_tensor", 1.0):
                L += p["equality_dual_jacobian_variables_variables"]
                L += p["cone_dual_jacobian_variables_variables"]
            self.set("lagrangian_hessian", L)
        par = (FLAGS["objective_jacobian_variables_parameters"] | FLAGS["equality_dual_jacobian_variables_parameters"] |
               FLAGS["cone_dual_jacobian_variables_parameters"])
        if flags & par and self.np:
            G = p["objective_jacobian_variables_parameters"].copy()     # residual_jacobian_parameters.jl:8-14
            G += p["equality_dual_jacobian_variables_parameters"]
            G += p["cone_dual_jacobian_variables_parameters"]
            self.set("lagrangian_gradient_parameters", G)

    def _evaluate_callback(self, user, flags, px, py, pz, pth):
        try:
            as_arr = np.ctypeslib.as_array
            x = as_arr(px, shape=(self.nx,))
            y = as_arr(py, shape=(self.ne,)) if self.ne else np.zeros(0)
            z = as_arr(pz, shape=(self.nc,)) if self.nc else np.zeros(0)
            th = as_arr(pth, shape=(self.np,)) if self.np else np.zeros(0)
            self.methods.evaluate(flags, x, y, z, th, self._out)
            self.upload(flags)
            return 0
        except Exception:   # pragma: no cover
            import traceback
            traceback.print_exc()
            return 1

    def evaluate(self, flags, which=0):
        """evaluate!(problem, methods, idx, point, parameters; <flags>) at the solution (0) or candidate (1) point"""
        w = self.get("solution" if which == 0 else "candidate", self.N)
        pt = _Point(w, self.nx, self.ne, self.nc)
        self.methods.evaluate(flags, pt.variables, pt.equality_dual, pt.cone_dual, self.parameters, self._out)
        self.upload(flags)

    # ---- reference-style views -----------------------------------------------------------------------------------
    @property
    def solution(self):
        return _Point(self.get("solution", self.N), self.nx, self.ne, self.nc)

    @property
    def candidate(self):
        return _Point(self.get("candidate", self.N), self.nx, self.ne, self.nc)

    def data(self, name):
        """solver.data.<name> (solver_data.jl): residual, step, residual_symmetric, step_symmetric, merit_gradient, solution_sensitivity"""
        sizes = dict(residual=self.N, residual_error=self.N, step=self.N, step_correction=self.N, residual_symmetric=self.n,
                     step_symmetric=self.n, merit_gradient=self.n, solution_sensitivity=self.N * self.np,
                     jacobian_parameters=self.N * self.np)
        v = self.get(name, sizes[name])
        if name in ("solution_sensitivity", "jacobian_parameters"):
            return v.reshape(self.np, self.N).T
        if name in ("residual", "residual_error", "step", "step_correction"):
            return _Point(v, self.nx, self.ne, self.nc)
        return v

    def jacobian_variables_symmetric(self):
        self._check(self._L.calipso_hip_residual_jacobian_variables_symmetric(self._h), "residual_jacobian_variables_symmetric")
        return self.get("jacobian_variables_symmetric", self.n * self.n).reshape(self.n, self.n).T

    # ---- hot-path entry points (one per reference function) ---------------------------------------------------------
    def cone(self, which=0, barrier=False, barrier_gradient=False, product=False, jacobian=False, target=False):
        fl = (CONE_BARRIER * barrier) | (CONE_BARRIER_GRADIENT * barrier_gradient) | (CONE_PRODUCT * product) | (CONE_JACOBIAN * jacobian) | (CONE_TARGET * target)
        self._check(self._L.calipso_hip_cone(self._h, which, int(fl)), "cone")

    def residual(self):
        self._check(self._L.calipso_hip_residual(self._h), "residual")

    def violations(self):
        out = np.zeros(5)
        self._check(self._L.calipso_hip_violations(self._h, _pd(out)), "violations")
        return dict(residual_violation=out[0], optimality_violation=out[1], slack_violation=out[2], equality_violation=out[3],
                    cone_product_violation=out[4])

    def jacobian_variables_mul(self, v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        out = np.zeros(self.N)
        self._check(self._L.calipso_hip_jacobian_variables_mul(self._h, _pd(v), _pd(out)), "jacobian_variables_mul")
        return out

    def factorize(self):
        inertia = np.zeros(3, dtype=np.int64)
        rc = self._check(self._L.calipso_hip_factorize(self._h, _pi(inertia)), "factorize")
        return tuple(int(v) for v in inertia), rc

    def inertia_correction(self):
        nf = C.c_int64(0)
        self._check(self._L.calipso_hip_inertia_correction(self._h, C.byref(nf)), "inertia_correction")
        return int(nf.value)

    def residual_symmetric(self, which=0):
        self._check(self._L.calipso_hip_residual_symmetric(self._h, which), "residual_symmetric")

    def linear_solve(self):
        self._check(self._L.calipso_hip_linear_solve(self._h), "linear_solve")

    def search_direction_symmetric(self, which=0):
        self._check(self._L.calipso_hip_search_direction_symmetric(self._h, which), "search_direction_symmetric")

    def iterative_refinement(self):
        r = C.c_int32(0)
        nrm = C.c_double(0.0)
        rc = self._check(self._L.calipso_hip_iterative_refinement(self._h, C.byref(r), C.byref(nrm)), "iterative_refinement")
        return rc == 0, int(r.value), float(nrm.value)

    def search_direction(self):
        return self._check(self._L.calipso_hip_search_direction(self._h), "search_direction")

    def search_direction_nonsymmetric(self):
        """step = H \\ residual on the unreduced system (src/solver/search_direction.jl:106-119), the reference's fallback when refinement fails"""
        return self._check(self._L.calipso_hip_search_direction_nonsymmetric(self._h), "search_direction_nonsymmetric")

    def cone_search(self):
        a, b = C.c_double(0), C.c_double(0)
        self._check(self._L.calipso_hip_cone_search(self._h, C.byref(a), C.byref(b)), "cone_search")
        return float(a.value), float(b.value)

    def cone_violation(self, xhat, x, tau):
        xhat = np.ascontiguousarray(xhat, dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64)
        v = C.c_int32(0)
        self._check(self._L.calipso_hip_cone_violation(self._h, _pd(xhat), _pd(x), tau, C.byref(v)), "cone_violation")
        return bool(v.value)

    def make_candidate(self, step_size, with_cone_slack=False):
        self._check(self._L.calipso_hip_candidate(self._h, step_size, int(with_cone_slack)), "candidate")

    def merit(self, which=0):
        m = C.c_double(0)
        self._check(self._L.calipso_hip_merit(self._h, which, C.byref(m)), "merit")
        return float(m.value)

    def merit_gradient(self):
        self._check(self._L.calipso_hip_merit_gradient(self._h), "merit_gradient")

    def constraint_violation(self, which=0):
        t = C.c_double(0)
        self._check(self._L.calipso_hip_constraint_violation(self._h, which, C.byref(t)), "constraint_violation")
        return float(t.value)

    def differentiate(self):
        self._check(self._L.calipso_hip_differentiate(self._h, self._cb, None), "differentiate")

    def differentiate_info(self):
        """report of the last differentiate() (calipso_hip_differentiate_info; set_option("differentiate_refinement", 1) turns the correction rounds on):
        dict(columns, rounds (largest over the columns), failed_columns (did not meet the stopping test), final_norm (largest over the columns)); zeros when no round ran"""
        return self._column_report("differentiate_info")

    def _column_report(self, what):
        out = np.zeros(4)
        self._check(getattr(self._L, "calipso_hip_" + what)(self._h, _pd(out)), what)
        return dict(columns=int(out[0]), rounds=int(out[1]), failed_columns=int(out[2]), final_norm=float(out[3]))

    def vjp(self, cotangent, adjoint=True, theta=None, qp=None):
        """differentiate! in reverse mode on this handle (calipso_hip_differentiate_adjoint): for cotangents v = dLoss/dw at the resident point, lambda = M' v for the map
        M that differentiate() applies to a column, and the gradients S' v for the S = dw/dtheta that differentiate() would return — one condensed solve per cotangent
        instead of one per parameter.  cotangent: (N,) or (N, k).  theta: -R_theta' lambda (default: when the handle has parameters); qp: True, or a string of names out
        of "PqAbGh": the data gradients of the QP given to qp_attach.  Returns a dict: "adjoint" (N[, k]), "theta" (np[, k]) and one entry per requested QP array in
        qp_attach's shape ([, k]); the trailing k axis only when the cotangent had one.  set_option("differentiate_refinement", 1) turns the correction rounds on
        (vjp_info)."""
        call = lambda *args: self._check(self._L.calipso_hip_differentiate_adjoint(self._h, self._cb, None, *args), "differentiate_adjoint")
        return _vjp(self, (), cotangent, adjoint, theta, qp, "cotangent must be (N,) or (N, k)", call)

    def vjp_info(self):
        """report of the last vjp() (calipso_hip_differentiate_adjoint_info), as differentiate_info(): dict(columns, rounds, failed_columns, final_norm)"""
        return self._column_report("differentiate_adjoint_info")

    def vjp_times(self):
        """HIP-event times of the last vjp() in ms: dict(device = entry to last kernel, copy = the results to the host, gradients = of device, the QP data-gradient
        kernels alone)"""
        out = np.zeros(3)
        self._check(self._L.calipso_hip_differentiate_adjoint_times(self._h, _pd(out)), "differentiate_adjoint_times")
        return dict(device=float(out[0]), copy=float(out[1]), gradients=float(out[2]))

    def set_device_evaluator(self, fn_ptr, user=None):
        """install a device-side evaluator (calipso_device_eval_fn, include/calipso_hip.h): `fn_ptr` is the C function's address (e.g.
        ctypes.cast(lib.sym, c_void_p)), `user` its opaque pointer; solve_b / differentiate then never call back into Python"""
        self._check(self._L.calipso_hip_set_device_evaluator(self._h, fn_ptr, user), "set_device_evaluator")
        self._device_eval = fn_ptr is not None

    def set_device_block_evaluator(self, fn_ptr, user=None):
        """structured handles: install an evaluator that writes the packed blocks themselves (calipso_device_block_eval_fn): no dense scratch on the device"""
        self._check(self._L.calipso_hip_set_device_block_evaluator(self._h, fn_ptr, user), "set_device_block_evaluator")
        self._device_eval = fn_ptr is not None

    def device_evaluate(self, flags, which=0):
        self._check(self._L.calipso_hip_device_evaluate(self._h, which, int(flags)), "device_evaluate")

    def set_callbacks(self, inner=None, outer=None):
        """callback_inner(custom, solver) / callback_outer(custom, solver) (src/solver/solver.jl:183,193): python callables taking the Solver"""
        self._cbi = CALLBACK_FN(lambda u, h: inner(self)) if inner else None
        self._cbo = CALLBACK_FN(lambda u, h: outer(self)) if outer else None
        ci = C.cast(self._cbi, C.c_void_p) if self._cbi else None
        co = C.cast(self._cbo, C.c_void_p) if self._cbo else None
        self._check(self._L.calipso_hip_set_callbacks(self._h, ci, co, None), "set_callbacks")

    def stats(self):
        out = np.zeros(8, dtype=np.int64)
        self._L.calipso_hip_stats(self._h, _pi(out))
        return dict(total_iterations=int(out[0]), outer=int(out[1]), factorizations=int(out[2]), refinement_failures=int(out[3]),
                    max_refinement_rounds=int(out[4]), fallbacks=int(out[5]), last_refinement_rounds=int(out[6]), newton_steps=int(out[7]))

    # ---- device-resident QP (synthetic benchmark) -----------------------------------------------------------------------
    def qp_attach(self, P, q, A, b, G, h, objective_scale=0.5):
        f = lambda M: np.ascontiguousarray(np.asarray(M, dtype=np.float64).T).reshape(-1)   # column-major
        v = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        Pc, Ac, Gc = f(P), f(A) if self.ne else np.zeros(1), f(G) if self.nc else np.zeros(1)
        qv, bv, hv = v(q), v(b) if self.ne else np.zeros(1), v(h) if self.nc else np.zeros(1)
        self._check(self._L.calipso_hip_qp_attach(self._h, _pd(Pc), _pd(qv), _pd(Ac), _pd(bv), _pd(Gc), _pd(hv), objective_scale), "qp_attach")

    def qp_evaluate(self, flags, which=0):
        self._check(self._L.calipso_hip_qp_evaluate(self._h, which, int(flags)), "qp_evaluate")

    def newton_step(self, advance=False):
        info = np.zeros(6)
        rc = self._check(self._L.calipso_hip_newton_step(self._h, int(advance), _pd(info)), "newton_step")
        return dict(status=rc, step_size=info[0], step_size_cone_slack_dual=info[1], refinement_rounds=int(info[2]),
                    factorizations=int(info[3]), merit_candidate=info[4], violation_candidate=info[5])

    def newton_steps(self, count, advance=False):
        """`count` Newton steps in one call (calipso_hip_newton_steps): the list of the per-step dicts newton_step returns"""
        info = np.zeros(6 * max(int(count), 1))
        status = np.zeros(max(int(count), 1), dtype=np.int32)
        self._check(self._L.calipso_hip_newton_steps(self._h, int(count), int(advance), _pd(info), status.ctypes.data_as(C.POINTER(C.c_int32))), "newton_steps")
        I = info.reshape(-1, 6)
        return [dict(status=int(status[k]), step_size=I[k, 0], step_size_cone_slack_dual=I[k, 1], refinement_rounds=int(I[k, 2]), factorizations=int(I[k, 3]),
                     merit_candidate=I[k, 4], violation_candidate=I[k, 5]) for k in range(int(count))]

    def phase_times(self):
        out = np.zeros(9)
        self._L.calipso_hip_phase_times(self._h, _pd(out))
        return out

    def kernel_times(self):
        """[0] ms of the panel-step launches of the last LDL^T (the pivot chain), [1] their number, [2] NP, [3] bytes of the device slab"""
        out = np.zeros(8)
        self._L.calipso_hip_kernel_times(self._h, _pd(out))
        return out

    def structure_work(self):
        """work of one Newton step on a handle that exploits its stage structure: dict(schur_flops, packed_doubles, segment_pairs, factor_flops, factor_nnz, order, structured)"""
        out = np.zeros(8)
        self._check(self._L.calipso_hip_structure_work(self._h, _pd(out)), "structure_work")
        return dict(schur_flops=out[0], packed_doubles=out[1], segment_pairs=int(out[2]), factor_flops=out[3], factor_nnz=out[4], order=int(out[5]), structured=bool(out[6]))

    def schedule_info(self):
        """dict(prologue_ahead_steps: Newton steps so far whose prologue ran on the second stream beside the factorisation, last_prologue_mode: 0 main stream,
        1 forked at the start of the step, 2 handed over while the pivot chain runs, ahead_undone: factorisations queued ahead of an exit test that held after all)"""
        out = np.zeros(4)
        self._check(self._L.calipso_hip_schedule_info(self._h, _pd(out)), "schedule_info")
        return dict(prologue_ahead_steps=int(out[0]), last_prologue_mode=int(out[1]), ahead_undone=int(out[2]))

    def schur_cache_info(self):
        """the cache of the Schur complement's equality products on a handle with an attached QP (calipso_hip_schur_cache_info): dict(captures: factorisations that
        stored the products, hits: that started from the stored ones, bypasses: that could have used the cache and went without, bytes: of the buffer); zeros: no cache"""
        out = np.zeros(4)
        self._check(self._L.calipso_hip_schur_cache_info(self._h, _pd(out)), "schur_cache_info")
        return dict(captures=int(out[0]), hits=int(out[1]), bypasses=int(out[2]), bytes=int(out[3]))

    def padded_nx(self):
        return int(self.kernel_times()[2])

    def device_bytes(self):
        return int(self.kernel_times()[3])

    def analyze_structure(self):
        """stage-banded structure from the non-zero pattern of the blocks currently on the device (include/calipso_hip.h); returns
        dict(half_bandwidth, band_blocks (0 = dense treatment), equality_rows_per_group, cone_rows_per_group)"""
        out = np.zeros(4, dtype=np.int64)
        self._check(self._L.calipso_hip_analyze_structure(self._h, _pi(out)), "analyze_structure")
        return dict(half_bandwidth=int(out[0]), band_blocks=int(out[1]), equality_rows_per_group=int(out[2]), cone_rows_per_group=int(out[3]))

    def clear_structure(self):
        self._check(self._L.calipso_hip_clear_structure(self._h), "clear_structure")

    def set_stage_parallel(self, on=True, batch=1):
        """after analyze_structure: factor the Schur complement by the multifrontal sparse LDL^T over a nested dissection of its pattern (for a
        trajectory problem log2(stages) launches instead of the chain of nx pivots); batch >= the largest group this handle leads.
        Returns dict(levels, largest_front, nnz_upper)."""
        out = np.zeros(4, dtype=np.int64)
        self._check(self._L.calipso_hip_set_stage_parallel(self._h, 1 if on else 0, int(batch), _pi(out)), "set_stage_parallel")
        return dict(levels=int(out[0]), largest_front=int(out[1]), nnz_upper=int(out[2]))

    def set_stage_blocks(self, on=True):
        """after analyze_structure: pack the blocks of [gx; hx] and of the Lagrangian Hessian and run the mat-vecs / the Schur complement on them
        (csrc/blocks.hip).  Returns dict(z_blocks, hessian_blocks, segments, packed_doubles)."""
        out = np.zeros(4, dtype=np.int64)
        self._check(self._L.calipso_hip_set_stage_blocks(self._h, 1 if on else 0, _pi(out)), "set_stage_blocks")
        return dict(z_blocks=int(out[0]), hessian_blocks=int(out[1]), segments=int(out[2]), packed_doubles=int(out[3]))

    def synchronize(self):
        self._check(self._L.calipso_hip_synchronize(self._h), "synchronize")

    def streams_concurrent(self, other):
        """calipso_hip_streams_concurrent: (side by side?, short kernel behind self's long one [us], behind other's [us], the long kernel [us], one chain of short kernels alone [us], both chains at once [us])"""
        out = np.zeros(6)
        self._check(self._L.calipso_hip_streams_concurrent(self._h, other._h, _pd(out)), "streams_concurrent")
        return bool(out[0]), float(out[1]), float(out[2]), float(out[3]), float(out[4]), float(out[5])

    def rebind_stream(self, priority_class=-1):
        """calipso_hip_rebind_stream: a new HIP stream for this handle (another hardware queue)"""
        self._check(self._L.calipso_hip_rebind_stream(self._h, int(priority_class)), "rebind_stream")


class Group(_Handle):
    """Up to 128 Solver handles of one shape (same dimensions and cone layout, same device) stepped in lockstep: every kernel
    launch of a group step covers all members (include/calipso_hip.h, "groups").  The reference has no counterpart — its
    `Solver`s are independent objects; this is how BASELINE config C4 keeps many of them in flight on one GPU."""
    _handle, _destroy, _message = "_g", "calipso_hip_group_destroy", _Handle._STATUS_MESSAGE

    def __init__(self, solvers):
        self.solvers = list(solvers)
        self._L = self.solvers[0]._L
        arr = (C.c_void_p * len(self.solvers))(*[s._h for s in self.solvers])
        h = C.c_void_p()
        rc = self._L.calipso_hip_group_create(arr, len(self.solvers), C.byref(h))
        if rc != 0:
            raise CalipsoHipError("group_create failed (%d): %s" % (rc, self._L.calipso_hip_last_error(self.solvers[0]._h).decode()))
        self._g = h

    def _error_text(self):
        return self._L.calipso_hip_last_error(self.solvers[0]._h).decode()      # (the library keeps a group's errors on its first member)

    def _set_evaluators(self):
        self._evals = (EVAL_FN * len(self.solvers))(*[s._cb for s in self.solvers])       # host callbacks (used by members without a device evaluator)
        self._L.calipso_hip_group_set_evaluators(self._g, self._evals, None)

    def newton_step(self, advance=False):
        """calipso_hip_newton_step for every member; returns one info dict per member (same keys as Solver.newton_step)"""
        B = len(self.solvers)
        info = np.zeros(6 * B)
        status = (C.c_int32 * B)()
        self._check(self._L.calipso_hip_group_newton_step(self._g, int(advance), _pd(info), status), "group_newton_step")
        out = []
        for k in range(B):
            r = info[6 * k: 6 * k + 6]
            out.append(dict(status=int(status[k]), step_size=r[0], step_size_cone_slack_dual=r[1], refinement_rounds=int(r[2]),
                            factorizations=int(r[3]), merit_candidate=r[4], violation_candidate=r[5]))
        return out

    def solve(self):
        """solve!(solver) for every member in lockstep (device evaluators attached); returns the per-member results
        (1 converged, 0 iteration caps reached, negative = error code of that member)"""
        B = len(self.solvers)
        res = (C.c_int32 * B)()
        self._set_evaluators()
        self._check(self._L.calipso_hip_group_solve(self._g, res), "group_solve")
        return [int(v) for v in res]

    def differentiate(self, tile=0):
        """differentiate! for every member through the same launches (calipso_hip_group_differentiate): per member what Solver.differentiate gives on the handle alone
        with differentiate_refinement off (the parameter Jacobians of members without a device evaluator come through their host callbacks, as in solve()).  tile: columns
        per workgroup of the batched products, 0 = the library's choice, 16 or 64 (the same bits either way).  Returns dict(sensitivity (count, N, np) = dw/dtheta per
        member — what each member's data("solution_sensitivity") reads afterwards —, status (count,))."""
        s0 = self.solvers[0]
        B, N, npar = len(self.solvers), s0.N, s0.np
        sens = np.zeros(max(B * N * npar, 1))
        status = np.zeros(B, dtype=np.int32)
        ms = np.zeros(2)
        self._set_evaluators()
        self._check(self._L.calipso_hip_group_differentiate(self._g, _pd(sens), status.ctypes.data_as(C.POINTER(C.c_int32)), int(tile), _pd(ms)), "group_differentiate")
        self._differentiate_ms = (float(ms[0]), float(ms[1]))
        return dict(sensitivity=np.transpose(sens[:B * N * npar].reshape(B, npar, N), (0, 2, 1)).copy(), status=status)

    def differentiate_ms(self):
        """HIP-event times in ms of the last differentiate(): (from its first enqueue to its last kernel, of that the column pass alone)"""
        return getattr(self, "_differentiate_ms", (0.0, 0.0))

    def vjp(self, cotangent, adjoint=True, theta=None, qp=None):
        """differentiate! in reverse mode for every member through the same launches (calipso_hip_group_differentiate_adjoint): per member what Solver.vjp gives on the
        handle alone with differentiate_refinement off.  cotangent: (count, N) or (count, N, k), member i's cotangents at its resident point.  theta, qp: as for Solver.vjp
        (the parameter Jacobians of members without a device evaluator come through their host callbacks, as in solve()).  Returns a dict of arrays with a leading member
        axis: "adjoint" (count, N[, k]), "theta" (count, np[, k]), one entry per requested QP array in qp_attach's shape (count, ...[, k]), and "status" (count,); the
        trailing k axis only when the cotangent had one."""
        status = np.zeros(len(self.solvers), dtype=np.int32)
        ms = C.c_double(0.0)

        def call(*args):
            self._set_evaluators()
            self._check(self._L.calipso_hip_group_differentiate_adjoint(self._g, *args, status.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ms)), "group_differentiate_adjoint")

        out = _vjp(self.solvers[0], (len(self.solvers),), cotangent, adjoint, theta, qp, "cotangent must be (count, N) or (count, N, k)", call)
        self._vjp_ms = float(ms.value)
        out["status"] = status
        return out

    def vjp_ms(self):
        """HIP-event time in ms of the last vjp(), from its first enqueue to its last kernel"""
        return getattr(self, "_vjp_ms", 0.0)

    def phase_times(self):
        return self.solvers[0].phase_times()

    def synchronize(self):
        self.solvers[0].synchronize()


def _csc_1based(A):
    import scipy.sparse as sp
    A = sp.csc_matrix(A)
    A.sort_indices()
    return (A, np.ascontiguousarray(A.indptr, dtype=np.int64) + 1, np.ascontiguousarray(A.indices, dtype=np.int64) + 1,
            np.ascontiguousarray(A.data, dtype=np.float64))


ORDERINGS = dict(natural=0, rcm=1, minimum_degree=2, nested_dissection=4)
SPARSE_METHODS = dict(ORDERINGS, nested_dissection_columns=5)     # 5: nested-dissection order with the column-level numeric phase (no fronts)


def ordering(A, method="rcm"):
    """elimination order (1-based, perm[k] = vertex eliminated k-th) of the symmetric pattern of A: "natural", "rcm", "minimum_degree"
    (calipso_hip_ordering; the reference takes perm = amd(A), qdldl.jl:135).  Host function: needs no device."""
    A, colptr, rowval, _ = _csc_1based(A)
    n = A.shape[0]
    perm = np.zeros(n, dtype=np.int64)
    rc = lib().calipso_hip_ordering(n, _pi(colptr), _pi(rowval), ORDERINGS[method], _pi(perm))
    if rc != 0:
        raise CalipsoHipError("calipso_hip_ordering failed (%d)" % rc)
    return perm


def symbolic(A, perm=None):
    """permute_symmetric + QDLDL_etree! of triu(A) under perm (qdldl.jl:358-395,642-742): dict(Pp, Pi, AtoPAPt, etree, Lnz, nnzL, half_bandwidth)"""
    A, colptr, rowval, _ = _csc_1based(A)
    n, nnz = A.shape[0], A.nnz
    Pp, Pi, mp = np.zeros(n + 1, dtype=np.int64), np.zeros(max(nnz, 1), dtype=np.int64), np.zeros(max(nnz, 1), dtype=np.int64)
    et, lnz, info = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(2, dtype=np.int64)
    pp = None if perm is None else np.ascontiguousarray(perm, dtype=np.int64)
    tot = lib().calipso_hip_symbolic(n, _pi(colptr), _pi(rowval), _pi(pp) if pp is not None else None, _pi(Pp), _pi(Pi), _pi(mp), _pi(et), _pi(lnz), _pi(info))
    if tot < -1:
        raise CalipsoHipError("calipso_hip_symbolic failed (%d)" % tot)
    return dict(Pp=Pp, Pi=Pi[:int(info[1])], AtoPAPt=mp[:nnz], etree=et, Lnz=lnz, nnzL=int(tot), half_bandwidth=int(info[0]))


class LDLSolver(_Handle):
    """LDLSolver / ldl_solver(A) of src/solver/linear_solver.jl:1-60 on the device: factorize!(s, A), compute_inertia!(s),
    linear_solve!(s, x, A, b).  A is a scipy.sparse CSC matrix (or anything scipy can convert); only triu(A) is read."""
    _message = _Handle._STATUS_MESSAGE

    def __init__(self, n, device=0):
        self._L = lib()
        self.n = int(n)
        h = C.c_void_p()
        rc = self._L.calipso_hip_ldl_create(self.n, device, C.byref(h))
        if rc != 0:
            raise CalipsoHipError("calipso_hip_ldl_create failed (%d): %s" % (rc, self._L.calipso_hip_last_error(h if h.value else None).decode()))
        self._h = h
        self.inertia = (0, 0, 0)          # Inertia(positive, negative, zero)  inertia.jl:1-5

    def analyze(self, A, method="rcm", perm=None):
        """install the elimination order of the following factorisations ("natural", "rcm", "minimum_degree", or perm=<1-based order>);
        returns (perm, dict(half_bandwidth, band_blocks (0 = dense treatment), nnzL, nnz_upper))"""
        A, colptr, rowval, _ = _csc_1based(A)
        p = np.zeros(self.n, dtype=np.int64) if perm is None else np.ascontiguousarray(perm, dtype=np.int64).copy()
        info = np.zeros(4, dtype=np.int64)
        m = 3 if perm is not None else ORDERINGS[method]
        self._check(self._L.calipso_hip_ldl_analyze_csc(self._h, self.n, _pi(colptr), _pi(rowval), m, _pi(p), _pi(info)), "analyze")
        return p, dict(half_bandwidth=int(info[0]), band_blocks=int(info[1]), nnzL=int(info[2]), nnz_upper=int(info[3]))

    def factorize(self, A):
        """factorize!(s, A; update) + compute_inertia!(s); returns the warning status (1 = zero pivot met)"""
        A, colptr, rowval, nzval = _csc_1based(A)
        out = np.zeros(3, dtype=np.int64)
        rc = self._check(self._L.calipso_hip_ldl_factorize_csc(self._h, self.n, _pi(colptr), _pi(rowval), _pd(nzval), _pi(out)), "factorize!")
        self.inertia = tuple(int(v) for v in out)
        return rc

    def compute_inertia(self):
        out = np.zeros(3, dtype=np.int64)
        self._check(self._L.calipso_hip_ldl_inertia(self._h, _pi(out)), "compute_inertia!")
        self.inertia = tuple(int(v) for v in out)
        return self.inertia

    def linear_solve(self, b, A=None, fact=False):
        """linear_solve!(s, x, A, b; fact): b is a vector (n) or a matrix (n x nrhs); returns x"""
        if fact:
            self.factorize(A)
        b = np.asarray(b, dtype=np.float64)
        nrhs = 1 if b.ndim == 1 else b.shape[1]
        bf = np.ascontiguousarray(b.reshape(self.n, nrhs).T).reshape(-1)          # column-major
        x = np.zeros_like(bf)
        self._check(self._L.calipso_hip_ldl_solve(self._h, self.n, nrhs, _pd(bf), _pd(x)), "linear_solve!")
        return x if b.ndim == 1 else x.reshape(nrhs, self.n).T


class SparseLDL(_Handle):
    """Sparse LDL^T on the device (include/calipso_hip.h, "sparse LDL^T on the device"): qdldl(A; perm) / QDLDL_factor! / solve! of
    src/solver/qdldl.jl for a scipy.sparse matrix A (only triu(A) is read), memory O(nnz(L)), level-scheduled over the elimination tree.
    method: "natural", "rcm", "minimum_degree", "nested_dissection" (multifrontal over the dissection tree when every front fits one CU's LDS,
    else as "nested_dissection_columns": the same order with the column-level numeric phase), or perm=<1-based order>."""
    _last_error, _destroy = "calipso_hip_sparse_last_error", "calipso_hip_sparse_destroy"

    def __init__(self, A, method="nested_dissection", perm=None, device=0):
        self._L = lib()
        A, colptr, rowval, _ = _csc_1based(A)
        self.n, self.nnz = A.shape[0], A.nnz
        pp = None if perm is None else np.ascontiguousarray(perm, dtype=np.int64)
        h = C.c_void_p()
        rc = self._L.calipso_hip_sparse_create(self.n, _pi(colptr), _pi(rowval), 3 if pp is not None else SPARSE_METHODS[method], _pi(pp) if pp is not None else None,
                                               device, C.byref(h))
        if rc != 0:
            msg = self._L.calipso_hip_sparse_last_error(h if h.value else None).decode()
            if h.value:
                self._L.calipso_hip_sparse_destroy(h)
            raise CalipsoHipError("calipso_hip_sparse_create failed (%d): %s" % (rc, msg))
        self._h = h
        info = np.zeros(8, dtype=np.int64)
        self._check(self._L.calipso_hip_sparse_info(self._h, _pi(info)), "sparse_info")
        self.info = dict(n=int(info[0]), nnz_upper=int(info[1]), nnzL=int(info[2]), levels=int(info[3]), launches=int(info[4]), widest_level=int(info[5]),
                         multiply_adds=int(info[6]), lds_accumulator=int(info[7]) == 1,
                         numeric={0: "columns_global_accumulator", 1: "columns_lds_accumulator", 2: "multifrontal"}[int(info[7])])
        self.inertia = (0, 0, 0)

    def set_batch(self, batch):
        """treat `batch` matrices of the analysed pattern per factorize / solve call (values (batch, nnz), right-hand sides (batch, n[, nrhs]))"""
        self._check(self._L.calipso_hip_sparse_set_batch(self._h, int(batch)), "sparse_set_batch")
        self.batch = int(batch)

    def factorize(self, A):
        """numeric factorisation of A (same pattern as analysed; a scipy.sparse matrix, or the nnz values in CSC order — (batch, nnz) after
        set_batch); returns the warning status (1 = an exact zero pivot was met, inertia[0] = -1 for that matrix)"""
        B = getattr(self, "batch", 1)
        if hasattr(A, "shape") and len(getattr(A, "shape")) == 2 and not isinstance(A, np.ndarray):
            A, _, _, vals = _csc_1based(A)
            if A.nnz != self.nnz:
                raise CalipsoHipError("SparseLDL.factorize: the pattern differs from the analysed one")
        else:
            vals = np.ascontiguousarray(A, dtype=np.float64).reshape(-1)
        if vals.size != B * self.nnz:
            raise CalipsoHipError("SparseLDL.factorize: expected %d x %d values" % (B, self.nnz))
        inr = np.zeros(3 * B, dtype=np.int64)
        rc = self._check(self._L.calipso_hip_sparse_factorize(self._h, _pd(vals), _pi(inr)), "sparse_factorize")
        self.inertia = tuple(int(v) for v in inr[:3])
        self.inertia_all = inr.reshape(B, 3)
        return rc

    def solve(self, b):
        """x = A^-1 b for a vector or an (n, nrhs) matrix; after set_batch: b of shape (batch, n) or (batch, n, nrhs)"""
        b = np.asarray(b, dtype=np.float64)
        B = getattr(self, "batch", 1)
        if B > 1:
            b3 = b.reshape(B, self.n, -1)
            nrhs = b3.shape[2]
            flat = np.ascontiguousarray(np.transpose(b3, (0, 2, 1))).reshape(-1)     # per matrix column-major n x nrhs
            X = np.zeros_like(flat)
            self._check(self._L.calipso_hip_sparse_solve(self._h, nrhs, _pd(flat), _pd(X)), "sparse_solve")
            X = np.transpose(X.reshape(B, nrhs, self.n), (0, 2, 1))
            return X[:, :, 0].copy() if b.ndim == 2 else X.copy()
        one = b.ndim == 1
        Bm = np.ascontiguousarray(b.reshape(self.n, -1).T).reshape(-1)          # column-major n x nrhs
        nrhs = Bm.size // self.n
        X = np.zeros_like(Bm)
        self._check(self._L.calipso_hip_sparse_solve(self._h, nrhs, _pd(Bm), _pd(X)), "sparse_solve")
        X = X.reshape(nrhs, self.n).T
        return X[:, 0].copy() if one else X.copy()

    def factorize_device(self, values):
        """factorize with the values already on the device: a float64 CUDA/HIP torch tensor of batch x nnz entries (CSC order)"""
        B = getattr(self, "batch", 1)
        assert values.is_cuda and values.is_contiguous() and values.numel() == B * self.nnz and values.element_size() == 8
        inr = np.zeros(3 * B, dtype=np.int64)
        rc = self._check(self._L.calipso_hip_sparse_factorize_device(self._h, C.c_void_p(values.data_ptr()), _pi(inr)), "sparse_factorize_device")
        self.inertia = tuple(int(v) for v in inr[:3])
        self.inertia_all = inr.reshape(B, 3)
        return rc

    def solve_device(self, b, out=None):
        """solve with device-resident right-hand sides: float64 torch tensor laid out batch x nrhs x n (each right-hand side contiguous);
        returns a tensor of the same layout (or writes `out`)"""
        B = getattr(self, "batch", 1)
        assert b.is_cuda and b.is_contiguous() and b.element_size() == 8 and b.numel() % (B * self.n) == 0
        nrhs = b.numel() // (B * self.n)
        if out is None:
            out = b.new_empty(b.shape)
        self._check(self._L.calipso_hip_sparse_solve_device(self._h, nrhs, C.c_void_p(b.data_ptr()), C.c_void_p(out.data_ptr())), "sparse_solve_device")
        return out

    def select(self, instance):
        """which matrix of the batch factor() reads"""
        self._check(self._L.calipso_hip_sparse_select(self._h, int(instance)), "sparse_select")

    def factor(self):
        """(perm (1-based), L as a scipy.sparse CSC unit-lower matrix, D)"""
        import scipy.sparse as sp
        nl = self.info["nnzL"]
        perm, Lp, Li = np.zeros(self.n, dtype=np.int64), np.zeros(self.n + 1, dtype=np.int64), np.zeros(max(nl, 1), dtype=np.int64)
        Lx, D = np.zeros(max(nl, 1)), np.zeros(self.n)
        self._check(self._L.calipso_hip_sparse_get_factor(self._h, _pi(perm), _pi(Lp), _pi(Li), _pd(Lx), _pd(D)), "sparse_get_factor")
        Lm = sp.csc_matrix((Lx[:nl], Li[:nl] - 1, Lp - 1), shape=(self.n, self.n)) + sp.identity(self.n, format="csc")
        return perm, Lm, D

    def timing(self):
        """(device milliseconds of the last factorisation, of the last solve)"""
        ms = np.zeros(2)
        self._check(self._L.calipso_hip_sparse_timing(self._h, _pd(ms)), "sparse_timing")
        return float(ms[0]), float(ms[1])


class _Columns:
    """A block (N,) or (N, k) — a host array, or a CUDA tensor for the device route — on its way through an entry of SparseKKT that takes and gives k x rows buffers:
    k, whether the caller's shape has no k axis, the input's pointer, outputs on the same side and the way back into the caller's shape.  Without a block: outputs
    for k columns alone.  (A CPU tensor's pointer goes through to the library, which refuses it naming the argument.)"""

    def __init__(self, handle, message=None, block=None, name=None, k=0, device=False):
        self.device, self.k, self.squeeze, self.pointer = device or hasattr(block, "is_cuda"), k, False, None
        if self.device:
            import torch
            self._empty, self._where = torch.empty, dict(dtype=torch.float64, device=torch.device("cuda", handle.device))
        if block is None:
            return
        if self.device:
            if block.dim() not in (1, 2) or block.shape[0] != handle.N:
                raise ValueError(message)
            self.squeeze, self.k = block.dim() == 1, (1 if block.dim() == 1 else int(block.shape[1]))
            self._block = block.detach().reshape(handle.N, self.k).t().contiguous()
            self.pointer = handle._device_pointer(self._block, name, self.k * handle.N)
        else:
            self._block, self.k, self.squeeze = pack_cotangent(block, (), handle.N, message)
            self.pointer = _pd(self._block)

    def entry(self, L, name):
        return getattr(L, "calipso_hip_" + name + ("_device" if self.device else ""))

    def empty(self, rows):
        """a k x rows output"""
        return self._empty((self.k, rows), **self._where) if self.device else np.zeros((self.k, rows))

    def ptr(self, out):
        if out is None:
            return None
        if self.device:
            return C.c_void_p(out.data_ptr())
        return _pd(out) if out.size else None

    def back(self, out):
        """a k x rows output in the caller's shape: (rows,), or (rows, k)"""
        if self.device:
            return out[0] if self.squeeze else out.t()
        return unpack_columns(out, (), self.k, (out.shape[1],), self.squeeze)


class SparseKKT(_Handle):
    """search_direction! (src/solver/search_direction.jl:1-23) on sparse problem data resident on the device (include/calipso_hip.h, "search_direction! on
    sparse problem data"; csrc/sparse_kkt.hip): assembly of jacobian_variables_symmetric, inertia correction, the symmetric solve and iterative refinement
    without a dense block anywhere.  Lxx (nx x nx, the full Lagrangian Hessian with both triangles), gx (ne x nx), hx (nc x nx): scipy sparse matrices whose
    PATTERN is used as it is (stored zeros included; a CSC matrix is taken in its own non-zero order, which later raw value arrays follow).  Cones: the first
    n_nonnegative rows of hx nonnegative (default: all that the second-order cones leave), then contiguous second-order cones of second_order_dims.
    method / perm as SparseLDL.  By default there is no `H \\ residual` fallback: search_direction returns status 2 (CALIPSO_WARN_REFINEMENT) with the last refined step;
    with the option krylov_fallback = 1 it goes on to solve_nonsymmetric (preconditioned GMRES, csrc/sparse_krylov.hip) and still returns 2 (fallback_info()).
    With attach_qp the same handle runs the vector half of solve! and a whole solve! of the sparse conic QP (csrc/sparse_solve.hip): initialize, solve, and the steps of an
    iteration one by one — and differentiate! in both directions (csrc/sparse_differentiate.hip): solve_columns, differentiate, vjp with the data gradients on the
    stored patterns.  With set_evaluator instead of attach_qp the same entries solve NONLINEAR problems: a device evaluator (calipso_device_sparse_eval_fn) writes fx, g,
    h, the objective and the non-zeros of Lxx, gx, hx into the handle's resident arrays (set_parameters, evaluate; codegen.TrajectoryProblem.sparse_solver makes such a
    handle from stage functions)."""
    _last_error, _destroy = "calipso_hip_sparse_kkt_last_error", "calipso_hip_sparse_kkt_destroy"
    _message = _Handle._STATUS_MESSAGE

    def __init__(self, Lxx, gx, hx, n_nonnegative=None, second_order_dims=(), method="nested_dissection", perm=None, device=0, options=None):
        import scipy.sparse as sp
        self._L = lib()
        as_csc = lambda A: A if sp.isspmatrix_csc(A) else sp.csc_matrix(A)
        Lxx, gx, hx = as_csc(Lxx), as_csc(gx), as_csc(hx)
        self.nx, self.ne, self.nc = int(Lxx.shape[0]), int(gx.shape[0]), int(hx.shape[0])
        if Lxx.shape != (self.nx, self.nx) or gx.shape[1] != self.nx or hx.shape[1] != self.nx:
            raise ValueError("SparseKKT: Lxx is nx x nx, gx ne x nx, hx nc x nx")
        self.n, self.N = self.nx + self.ne + self.nc, self.nx + 2 * self.ne + 3 * self.nc
        self.nnz = (int(Lxx.indptr[-1]), int(gx.indptr[-1]), int(hx.indptr[-1]))
        dims = np.ascontiguousarray(list(second_order_dims), dtype=np.int64)
        if n_nonnegative is None:
            n_nonnegative = self.nc - int(dims.sum())
        one_based = lambda A: (np.ascontiguousarray(A.indptr, dtype=np.int64) + 1, np.ascontiguousarray(A.indices, dtype=np.int64) + 1)
        pats = [one_based(A) for A in (Lxx, gx, hx)]
        pp = None if perm is None else np.ascontiguousarray(perm, dtype=np.int64)
        h = C.c_void_p()
        rc = self._L.calipso_hip_sparse_kkt_create(self.nx, self.ne, self.nc, int(n_nonnegative), int(dims.size), _pi(dims) if dims.size else None,
                                                   _pi(pats[0][0]), _pi(pats[0][1]), _pi(pats[1][0]), _pi(pats[1][1]), _pi(pats[2][0]), _pi(pats[2][1]),
                                                   3 if pp is not None else SPARSE_METHODS[method], _pi(pp) if pp is not None else None, device, C.byref(h))
        if rc != 0:
            raise CalipsoHipError("calipso_hip_sparse_kkt_create failed (%d): %s" % (rc, self._L.calipso_hip_sparse_kkt_last_error(None).decode()))
        self._h = h
        self.device = int(device)
        info = np.zeros(8, dtype=np.int64)
        self._check(self._L.calipso_hip_sparse_kkt_info(self._h, _pi(info)), "sparse_kkt_info")
        self.info = dict(n=int(info[0]), nnz_upper=int(info[1]), nnzL=int(info[2]), levels=int(info[3]),
                         numeric={0: "columns_global_accumulator", 1: "columns_lds_accumulator", 2: "multifrontal"}[int(info[4])], assemble_launches=int(info[5]),
                         max_cone_dimension=int(info[6]), N=int(info[7]))
        self._colptr, self._rowval = np.zeros(self.n + 1, dtype=np.int64), np.zeros(max(self.info["nnz_upper"], 1), dtype=np.int64)
        self._check(self._L.calipso_hip_sparse_kkt_pattern(self._h, _pi(self._colptr), _pi(self._rowval)), "sparse_kkt_pattern")
        self.inertia = (0, 0, 0)
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, name, value):
        """the regularisation and refinement options of options.jl:6-59 by name; "central_path": the scalar IC-2 reads"""
        self._check(self._L.calipso_hip_sparse_kkt_set_option(self._h, name.encode(), float(value)), "sparse_kkt_set_option(%s)" % name)

    def _is_device(self, a):
        return a is not None and (hasattr(a, "is_cuda") or isinstance(a, C.c_void_p))

    def _device_pointer(self, a, name, count):
        """a float64 CUDA tensor of `count` entries on the handle's device, or a raw device pointer (ctypes.c_void_p): its pointer"""
        if a is None:
            return None
        if not hasattr(a, "is_cuda"):
            return a
        import torch
        if a.dtype != torch.float64 or a.numel() != count or not a.is_contiguous():
            raise ValueError("%s must be a contiguous float64 tensor of %d entries" % (name, count))
        if a.is_cuda and a.device.index != self.device:
            raise ValueError("%s is on %s, the handle on device %d" % (name, a.device, self.device))
        if a.is_cuda:
            torch.cuda.current_stream(a.device).synchronize()      # the handle works on its own stream
        return C.c_void_p(a.data_ptr())      # (a CPU tensor's pointer goes through: the library refuses it, naming the argument)

    def set_values(self, Lxx=None, gx=None, hx=None, w=None, penalty=None, central_path=None):
        """non-zeros of Lxx, gx, hx (sparse matrices of the analysed pattern, or the values in its order), the point w (N), the penalty rho; None keeps what
        is resident.  Host arrays, or — all that are given — float64 CUDA tensors / raw device pointers as ctypes.c_void_p (the device route: the penalty is then
        one double on the device too)."""
        given = [a for a in (Lxx, gx, hx, w, penalty) if a is not None]
        if central_path is not None:
            self.set_option("central_path", central_path)
        if given and all(self._is_device(a) for a in given):
            names, counts = ("Lxx", "gx", "hx", "w", "penalty"), self.nnz + (self.N, 1)
            ptrs = [self._device_pointer(a, nm, ct) for a, nm, ct in zip((Lxx, gx, hx, w, penalty), names, counts)]
            self._check(self._L.calipso_hip_sparse_kkt_set_values_device(self._h, *ptrs), "sparse_kkt_set_values_device")
            return
        def values(A, count, name):
            if A is None:
                return None
            if hasattr(A, "indptr"):
                A = A.data
            v = np.ascontiguousarray(A, dtype=np.float64).reshape(-1)
            if v.size != count:
                raise CalipsoHipError("SparseKKT.set_values: %s has %d values, the analysed pattern %d" % (name, v.size, count))
            return v
        arrs = [values(Lxx, self.nnz[0], "Lxx"), values(gx, self.nnz[1], "gx"), values(hx, self.nnz[2], "hx"), values(w, self.N, "w"),
                None if penalty is None else np.array([float(penalty)])]
        self._check(self._L.calipso_hip_sparse_kkt_set_values(self._h, *[_opt(a) for a in arrs]), "sparse_kkt_set_values")

    def factorize(self, ep, ed):
        """one assemble + factorisation at (ep, ed); sets .inertia; returns the warning status (1 = an exact zero pivot was met)"""
        out = np.zeros(3, dtype=np.int64)
        rc = self._check(self._L.calipso_hip_sparse_kkt_factorize(self._h, float(ep), float(ed), _pi(out)), "sparse_kkt_factorize")
        self.inertia = tuple(int(v) for v in out)
        return rc

    def matrix(self):
        """triu(jacobian_variables_symmetric) of the last assemble, scipy CSC"""
        import scipy.sparse as sp
        nz = np.zeros(max(self.info["nnz_upper"], 1))
        self._check(self._L.calipso_hip_sparse_kkt_get_matrix(self._h, _pd(nz)), "sparse_kkt_get_matrix")
        k = self.info["nnz_upper"]
        return sp.csc_matrix((nz[:k], self._rowval[:k] - 1, self._colptr - 1), shape=(self.n, self.n))

    def mul(self, v):
        """H v for the unreduced matrix at the regularisation of the last assemble"""
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        if v.size != self.N:
            raise CalipsoHipError("SparseKKT.mul: v has %d entries, N = %d" % (v.size, self.N))
        out = np.zeros(self.N)
        self._check(self._L.calipso_hip_sparse_kkt_mul(self._h, _pd(v), _pd(out)), "sparse_kkt_mul")
        return out

    def solve_symmetric(self, residual):
        """search_direction_symmetric! with the current factorisation"""
        r = np.ascontiguousarray(residual, dtype=np.float64).reshape(-1)
        if r.size != self.N:
            raise CalipsoHipError("SparseKKT.solve_symmetric: the residual has %d entries, N = %d" % (r.size, self.N))
        out = np.zeros(self.N)
        self._check(self._L.calipso_hip_sparse_kkt_solve_symmetric(self._h, _pd(r), _pd(out)), "sparse_kkt_solve_symmetric")
        return out

    def search_direction(self, residual, regularization=(0.0, 0.0, 0.0)):
        """search_direction! from regularization = (ep, ep_last, ed): returns (step, regularization, info, status) with info = dict(factorizations, refinement_rounds,
        residual_norm, fallback_iterations) and status 0 or 2 (refinement failed: the last refined step, or with krylov_fallback the GMRES step).  A CUDA tensor / device pointer as residual: the device route,
        the step comes back as a CUDA tensor."""
        reg, info = np.ascontiguousarray(regularization, dtype=np.float64).copy(), np.zeros(4)
        if reg.size != 3:
            raise CalipsoHipError("SparseKKT.search_direction: regularization is (ep, ep_last, ed)")
        if self._is_device(residual):
            import torch
            step = torch.empty(self.N, dtype=torch.float64, device=torch.device("cuda", self.device))
            rp = self._device_pointer(residual, "residual", self.N)
            rc = self._L.calipso_hip_sparse_kkt_search_direction_device(self._h, rp, C.c_void_p(step.data_ptr()), _pd(reg), _pd(info))
        else:
            r = np.ascontiguousarray(residual, dtype=np.float64).reshape(-1)
            if r.size != self.N:
                raise CalipsoHipError("SparseKKT.search_direction: the residual has %d entries, N = %d" % (r.size, self.N))
            step = np.zeros(self.N)
            rc = self._L.calipso_hip_sparse_kkt_search_direction(self._h, _pd(r), _pd(step), _pd(reg), _pd(info))
        self.regularization = tuple(float(v) for v in reg)      # (also after an error: where the inertia correction stopped)
        self._check(rc, "search_direction!")
        return step, self.regularization, dict(factorizations=int(info[0]), refinement_rounds=int(info[1]), residual_norm=float(info[2]),
                                               fallback_iterations=int(info[3])), rc

    def solve_nonsymmetric(self, residual):
        """search_direction_nonsymmetric! for this handle: `H \\ residual` by restarted right-preconditioned GMRES with the current factorisation
        (csrc/sparse_krylov.hip), whatever the option krylov_fallback says.  Returns the step; fallback_info() says whether it converged.  A CUDA tensor / device
        pointer as residual: the device route, the step comes back as a CUDA tensor."""
        if self._is_device(residual):
            import torch
            step = torch.empty(self.N, dtype=torch.float64, device=torch.device("cuda", self.device))
            rp = self._device_pointer(residual, "residual", self.N)
            self._check(self._L.calipso_hip_sparse_kkt_solve_nonsymmetric_device(self._h, rp, C.c_void_p(step.data_ptr())), "sparse_kkt_solve_nonsymmetric_device")
            return step
        r = np.ascontiguousarray(residual, dtype=np.float64).reshape(-1)
        if r.size != self.N:
            raise CalipsoHipError("SparseKKT.solve_nonsymmetric: the residual has %d entries, N = %d" % (r.size, self.N))
        step = np.zeros(self.N)
        self._check(self._L.calipso_hip_sparse_kkt_solve_nonsymmetric(self._h, _pd(r), _pd(step)), "sparse_kkt_solve_nonsymmetric")
        return step

    FALLBACK_INFO = ("taken", "iterations", "cycles", "residual_norm", "converged", "device_ms", "launches", "solve_fallbacks", "solve_iterations",
                     "solve_most_iterations", "solve_unconverged", "workspace_bytes")

    def fallback_info(self):
        """the `H \\ residual` fallback (options krylov_fallback, krylov_restart, krylov_max_cycles): of the last search_direction / solve_nonsymmetric taken,
        iterations, cycles, residual_norm (the true |residual - H step|_inf), converged, device_ms, launches (its own kernels); over the last solve
        solve_fallbacks, solve_iterations, solve_most_iterations, solve_unconverged; workspace_bytes"""
        out = np.zeros(12)
        self._check(self._L.calipso_hip_sparse_kkt_fallback_info(self._h, _pd(out)), "sparse_kkt_fallback_info")
        info = dict(zip(self.FALLBACK_INFO, (float(v) for v in out)))
        for k in self.FALLBACK_INFO:
            if k not in ("residual_norm", "device_ms"):
                info[k] = int(info[k])
        return info

    def timing(self):
        """device milliseconds of the last search_direction: dict(assemble, factorize, solve, refinement_solves, refinement_mul, wall); and of the last solve_columns /
        differentiate / vjp: columns_map (its first pre + multi-column solve + post), columns_rounds (its correction rounds, read-backs included) — their assemble and
        factorisation are added to the first two"""
        ms = np.zeros(8)
        self._check(self._L.calipso_hip_sparse_kkt_timing(self._h, _pd(ms)), "sparse_kkt_timing")
        return dict(zip(("assemble", "factorize", "solve", "refinement_solves", "refinement_mul", "wall", "columns_map", "columns_rounds"), (float(v) for v in ms)))

    # ---- solve! on the same handle (include/calipso_hip.h, "solve! on sparse problem data"; csrc/sparse_solve.hip) ----------------------------------------
    SOLVE_INFO = ("total_iterations", "outer_iterations", "accepted_iterates", "factorizations", "max_refinement_rounds", "refinement_failures", "worst_warning",
                  "host_waits", "line_search_trials", "central_path", "penalty", "primal_regularization_last", "vector_ms", "search_direction_ms", "wall_ms", "status")
    VECTORS = dict(solution="N", candidate="N", dual="ne", residual="N", merit_gradient="n", step="N", cone_product="nc", cone_target="nc", barrier_gradient="nc",
                   equality_constraint="ne", cone_constraint="nc", objective_gradient_variables="nx")

    def _host_vector(self, a, name, count):
        v = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        if v.size != count:
            raise CalipsoHipError("SparseKKT: %s has %d entries, not %d" % (name, v.size, count))
        return v

    def attach_qp(self, q=None, b=None, h=None, objective_constant=0.0):
        """the vectors of the conic QP besides Lxx = c (P + P'), gx = A, hx = -G: q (nx), b (ne), h (nc); None keeps what is resident.  Host arrays or — all that
        are given — float64 CUDA tensors / raw device pointers"""
        given = [a for a in (q, b, h) if a is not None]
        counts = (self.nx, self.ne, self.nc)
        if given and all(self._is_device(a) for a in given):
            ptrs = [self._device_pointer(a, nm, ct) for a, nm, ct in zip((q, b, h), ("q", "b", "h"), counts)]
            self._check(self._L.calipso_hip_sparse_kkt_qp_attach_device(self._h, *ptrs, float(objective_constant)), "sparse_kkt_qp_attach_device")
        else:
            arrs = [None if a is None else self._host_vector(a, nm, ct) for a, nm, ct in zip((q, b, h), ("q", "b", "h"), counts)]
            self._check(self._L.calipso_hip_sparse_kkt_qp_attach(self._h, *[_opt(a) for a in arrs], float(objective_constant)), "sparse_kkt_qp_attach")
        self._parameter_nnz = None              # (the attached QP replaced an evaluator and its parameter patterns)

    def initialize(self, x0):
        """initialize!(solver, x0): x <- x0, slacks and duals as initialize.jl:9-48 (x0: a host array, or a CUDA tensor / device pointer)"""
        if self._is_device(x0):
            self._check(self._L.calipso_hip_sparse_kkt_initialize_device(self._h, self._device_pointer(x0, "x0", self.nx)), "sparse_kkt_initialize_device")
        else:
            self._check(self._L.calipso_hip_sparse_kkt_initialize(self._h, _pd(self._host_vector(x0, "x0", self.nx))), "sparse_kkt_initialize")

    def solve(self):
        """solve!: (status, info) with status 1 solved, 0 iteration caps, -102 a refinement failure without the options krylov_fallback (the `H \\ residual` fallback by
        GMRES: fallback_info() counts them) or continue_after_refinement_failure (the point is the last accepted iterate); the reference's error()s and refused
        arguments raise"""
        info = np.zeros(16)
        rc = self._L.calipso_hip_sparse_kkt_solve(self._h, _pd(info))
        out = dict(zip(self.SOLVE_INFO, (float(v) for v in info)))
        for k in self.SOLVE_INFO[:9] + ("status",):
            out[k] = int(out[k])
        self.solve_info = out
        if rc != -102:
            self._check(rc, "solve!")
        return rc, out

    def step_prologue(self):
        """the prologue of a Newton step at the resident point: dict(objective, barrier, merit, constraint_violation, residual_violation, optimality_error,
        slack_violation, norms = the eight norms behind them)"""
        sc = np.zeros(16)
        self._check(self._L.calipso_hip_sparse_kkt_step_prologue(self._h, 0, _pd(sc)), "sparse_kkt_step_prologue")
        out = dict(zip(("objective", "barrier", "merit", "constraint_violation", "residual_violation", "optimality_error", "slack_violation"), (float(v) for v in sc[:7])))
        out["norms"] = sc[8:].copy()
        return out

    def cone_search(self):
        """the cone search on the resident step: the step sizes (cone slacks, their duals)"""
        a = np.zeros(2)
        self._check(self._L.calipso_hip_sparse_kkt_cone_search(self._h, _pd(a)), "sparse_kkt_cone_search")
        return float(a[0]), float(a[1])

    def candidate(self, a_s, a_t):
        """the candidate at the two step sizes: (merit, constraint violation, merit_gradient . step.primals)"""
        out = np.zeros(3)
        self._check(self._L.calipso_hip_sparse_kkt_candidate(self._h, float(a_s), float(a_t), _pd(out)), "sparse_kkt_candidate")
        return tuple(float(v) for v in out)

    def accept(self, step_size):
        """the candidate becomes the solution: (|g|_inf, |s o t|_inf)"""
        out = np.zeros(2)
        self._check(self._L.calipso_hip_sparse_kkt_accept(self._h, float(step_size), _pd(out)), "sparse_kkt_accept")
        return float(out[0]), float(out[1])

    def outer_update(self):
        self._check(self._L.calipso_hip_sparse_kkt_outer_update(self._h), "sparse_kkt_outer_update")

    # ---- nonlinear problems: a device evaluator instead of the QP (include/calipso_hip.h, "solve! on sparse data with an evaluator") ------------------------------
    def set_evaluator(self, fn_ptr, user=None, num_parameters=0):
        """a calipso_device_sparse_eval_fn (a ctypes function pointer or c_void_p from a loaded library) and its user object; replaces attach_qp, and attach_qp
        replaces it; None removes it.  The caller keeps the library and the user object alive while the handle may call them"""
        fn = None if fn_ptr is None else C.cast(fn_ptr, C.c_void_p)
        self._check(self._L.calipso_hip_sparse_kkt_set_evaluator(self._h, fn, user, int(num_parameters)), "sparse_kkt_set_evaluator")
        self.num_parameters = int(num_parameters) if fn_ptr is not None else 0
        self._parameter_nnz = None

    def set_parameters(self, theta):
        """theta of the evaluator (num_parameters entries), resident on the handle: a host array, or a CUDA tensor / device pointer"""
        count = getattr(self, "num_parameters", 0)
        if self._is_device(theta):
            self._check(self._L.calipso_hip_sparse_kkt_set_parameters_device(self._h, self._device_pointer(theta, "theta", count)), "sparse_kkt_set_parameters_device")
        else:
            self._check(self._L.calipso_hip_sparse_kkt_set_parameters(self._h, _opt(self._host_vector(theta, "theta", count))), "sparse_kkt_set_parameters")

    def evaluate(self, flags, which=0):
        """the evaluator at the solution (which = 0) or at the candidate (1), synchronised: CALIPSO_EVAL_* bits without the dual gradients and the parameter Jacobians"""
        self._check(self._L.calipso_hip_sparse_kkt_evaluate(self._h, int(which), int(flags)), "sparse_kkt_evaluate")

    PARAMETER_ARRAYS = ("lagrangian_gradient_parameters", "equality_jacobian_parameters", "cone_jacobian_parameters")

    def set_parameter_patterns(self, Lp, gp, hp):
        """the stored patterns of dR/dtheta's three non-zero blocks, each with num_parameters columns: Lp (nx rows, the Lagrangian's theta-gradient), gp (ne rows), hp (nc
        rows) — scipy sparse matrices (their patterns, CSC) or 0-based (colptr, rowval) pairs with rows ascending within a column.  The evaluator then writes the values
        (evaluate_parameters, get(name)) and differentiate() / vjp(theta=True) take dR/dtheta from it; nothing of size N x num_parameters exists.  set_evaluator and
        attach_qp drop the patterns"""
        arrs = []
        for M in (Lp, gp, hp):
            if hasattr(M, "tocsc"):
                M = M.tocsc()
                M.sort_indices()
                colptr, rowval = M.indptr, M.indices
            else:
                colptr, rowval = M
            arrs += [np.ascontiguousarray(colptr, dtype=np.int64).reshape(-1) + 1, np.ascontiguousarray(rowval, dtype=np.int64).reshape(-1) + 1]
        count = getattr(self, "num_parameters", 0)
        for name, colptr, rowval in zip(("Lp", "gp", "hp"), arrs[0::2], arrs[1::2]):      # (the library reads colptr[num_parameters] and that many rows)
            if colptr.size != count + 1 or colptr[-1] - 1 != rowval.size:
                raise CalipsoHipError("SparseKKT.set_parameter_patterns: %s has %d column pointers and %d rows; the evaluator takes %d parameters" % (name, colptr.size, rowval.size, count))
        self._check(self._L.calipso_hip_sparse_kkt_set_parameter_patterns(self._h, *[_pi(a) if a.size else None for a in arrs]), "sparse_kkt_set_parameter_patterns")
        self._parameter_nnz = tuple(int(a.size) for a in arrs[1::2])

    def evaluate_parameters(self):
        """the evaluator's five parameter bits at the resident x, y, z, theta into the three resident arrays of set_parameter_patterns, synchronised"""
        self._check(self._L.calipso_hip_sparse_kkt_evaluate_parameters(self._h), "sparse_kkt_evaluate_parameters")

    def _has_parameter_patterns(self):
        return getattr(self, "_parameter_nnz", None) is not None and getattr(self, "num_parameters", 0) > 0

    # ---- differentiate! on the same handle (include/calipso_hip.h, "differentiate! on sparse problem data"; csrc/sparse_differentiate.hip) -------------------
    GRADIENTS = "LqgbHh"      # the data gradients of vjp by letter: Lxx, q, gx, b, hx, hvec — the matrices as the values on their stored patterns
    _QP_LETTERS = dict(P="L", A="g", G="H")      # a handle from SparseConicQP also answers for P, A, G

    def solve_columns(self, B, transposed=False):
        """X = M B for the condensed solve's map M of solve_symmetric (transposed: M' B) with the CURRENT factorisation, all columns of B (N,) or (N, k) through the
        launches of one; no refinement.  A CUDA tensor takes the device route and comes back as one"""
        cols = _Columns(self, "SparseKKT.solve_columns: B must be (N,) or (N, k)", B, "sparse_kkt_solve_columns")
        out = cols.empty(self.N)
        self._check(cols.entry(self._L, "sparse_kkt_solve_columns")(self._h, cols.k, 1 if transposed else 0, cols.pointer, cols.ptr(out)), "sparse_kkt_solve_columns")
        return cols.back(out)

    def differentiate(self, J=None, columns=None, device=False):
        """forward differentiate! for the caller's dR/dtheta J (N,) or (N, k): one factorisation at the (ep, ed) the handle holds, then S = -M J (with the correction rounds
        under set_option("differentiate_refinement", 1): differentiate_info).  J=None: the evaluator's own dR/dtheta on the stored patterns of set_parameter_patterns,
        evaluated at the resident point and theta — all num_parameters columns, or those of `columns` (0-based parameter indices, repeats allowed); the result is
        (N, k), bit for bit what differentiate(J) gives for the same block; device=True returns it as a CUDA tensor"""
        if J is None:
            if columns is None:
                k, cp = getattr(self, "num_parameters", 0), None
            else:
                selected = np.ascontiguousarray(columns, dtype=np.int64).reshape(-1) + 1
                k, cp = int(selected.size), _pi(selected)
            cols, name = _Columns(self, k=max(k, 1), device=device), "sparse_kkt_differentiate_parameters"      # (one column at least: the library refuses k = 0 by name)
            out = cols.empty(self.N)
            self._check(cols.entry(self._L, name)(self._h, k, cp, cols.ptr(out)), name + ("_device" if device else ""))
            return cols.back(out)[:, :k]
        if columns is not None:
            raise ValueError("SparseKKT.differentiate: columns selects parameters of the evaluator's dR/dtheta (J=None); a J of the caller's is taken whole")
        cols = _Columns(self, "SparseKKT.differentiate: J must be (N,) or (N, k)", J, "sparse_kkt_differentiate")
        out = cols.empty(self.N)
        self._check(cols.entry(self._L, "sparse_kkt_differentiate")(self._h, cols.k, cols.pointer, cols.ptr(out)), "sparse_kkt_differentiate")
        return cols.back(out)

    def vjp(self, V, adjoint=True, qp="", theta=None):
        """reverse differentiate! for cotangents V = dLoss/dw (N,) or (N, k): the same factorisation, lambda = M' V, and the gradients of the loss with respect to the data
        named in qp, letters out of "LqgbHh" = Lxx, q, gx, b, hx, hvec: vectors as they are, matrices as the values ON THEIR STORED PATTERNS in the handle's non-zero
        order.  A handle from SparseConicQP also takes "P", "A", "G": gradients on the stored patterns of the P, A, G it was given (grad_P = c (gLxx(i, j) + gLxx(j, i)),
        grad_A = g_gx, grad_G = -g_hx).  Returns a dict: "adjoint" (unless adjoint=False) and one entry per letter, each with a trailing k axis only when V had one.
        A CUDA tensor takes the device route and everything comes back as CUDA tensors.
        theta (default: True on a handle with set_parameter_patterns, else False): additionally "theta" = dLoss/dtheta = -R_theta' lambda (num_parameters,) or
        (num_parameters, k), from the evaluator's dR/dtheta on its stored patterns at the resident point and theta — no host evaluation, no dense array"""
        qp = qp or ""
        if theta is None:
            theta = self._has_parameter_patterns()
        if theta and qp:
            raise ValueError("SparseKKT.vjp: theta belongs to a handle with an evaluator, qp to one with an attached QP")
        if any(c not in self.GRADIENTS + "PAG" for c in qp):
            raise ValueError("SparseKKT.vjp: qp is a string of letters out of 'LqgbHh' (and 'PAG' on a handle from SparseConicQP)")
        if any(c in "PAG" for c in qp) and not hasattr(self, "_conic_qp"):
            raise ValueError("SparseKKT.vjp: P, A, G are the data of a handle from SparseConicQP; this handle answers for 'LqgbHh'")
        cols = _Columns(self, "SparseKKT.vjp: V must be (N,) or (N, k)", V, "V")
        adj = cols.empty(self.N) if adjoint else None
        out = {}
        if theta:                                # the two entries differ only in which gradient arrays follow the adjoint
            npar, name = getattr(self, "num_parameters", 0), "sparse_kkt_differentiate_adjoint_parameters"
            grad = cols.empty(max(npar, 1))
            self._check(cols.entry(self._L, name)(self._h, cols.k, cols.pointer, cols.ptr(adj), cols.ptr(grad)), name + ("_device" if cols.device else ""))
            out["theta"] = cols.back(grad[:, :npar])
        else:
            sizes = dict(zip(self.GRADIENTS, (self.nnz[0], self.nx, self.nnz[1], self.ne, self.nnz[2], self.nc)))
            grads = {c: cols.empty(sizes[c]) for c in set(self._QP_LETTERS.get(c, c) for c in qp)}
            ptrs = ((C.c_void_p if cols.device else C.POINTER(C.c_double)) * 6)(*[cols.ptr(grads.get(c)) for c in self.GRADIENTS]) if grads else None
            name = "sparse_kkt_differentiate_adjoint"
            self._check(cols.entry(self._L, name)(self._h, cols.k, cols.pointer, cols.ptr(adj), ptrs), name + ("_device" if cols.device else ""))
            for c in qp:
                g = grads[self._QP_LETTERS.get(c, c)]
                if c == "P":
                    ij, ji, scale = self._conic_qp_positions(cols.device)
                    g = scale * (g[:, ij] + g[:, ji])
                elif c == "G":
                    g = -g
                out[c] = cols.back(g)
        if adjoint:
            out = dict(adjoint=cols.back(adj), **out)
        return out

    def _conic_qp_positions(self, device):
        """for each stored entry (i, j) of the P given to SparseConicQP: where (i, j) and (j, i) lie in Lxx's non-zero order, and the objective scale"""
        ij, ji, scale = self._conic_qp
        if (ij < 0).any() or (ji < 0).any():
            raise CalipsoHipError("SparseKKT.vjp: an entry of P's pattern is not in the pattern of c (P + P') (the sum cancelled it): its gradient is not on Lxx's pattern")
        if device:
            import torch
            if not hasattr(self, "_conic_qp_device"):
                self._conic_qp_device = tuple(torch.as_tensor(a, device=torch.device("cuda", self.device)) for a in (ij, ji))
            return self._conic_qp_device + (scale,)
        return ij, ji, scale

    def _column_report(self, what):
        out = np.zeros(4)
        self._check(getattr(self._L, "calipso_hip_sparse_kkt_" + what)(self._h, _pd(out)), what)
        return dict(columns=int(out[0]), rounds=int(out[1]), failed_columns=int(out[2]), final_norm=float(out[3]))

    def differentiate_info(self):
        """report of the last differentiate(): dict(columns, rounds (largest over the columns), failed_columns, final_norm); zeros when no round ran"""
        return self._column_report("differentiate_info")

    def vjp_info(self):
        """report of the last vjp(), as differentiate_info()"""
        return self._column_report("differentiate_adjoint_info")

    def vjp_times(self):
        """HIP-event times of the last vjp() in ms: dict(device = entry to last kernel, copy = the results to the caller, gradients = of device, the gradient kernel alone)"""
        out = np.zeros(3)
        self._check(self._L.calipso_hip_sparse_kkt_differentiate_adjoint_times(self._h, _pd(out)), "sparse_kkt_differentiate_adjoint_times")
        return dict(device=float(out[0]), copy=float(out[1]), gradients=float(out[2]))

    def differentiate_bytes(self):
        """the device bytes solve_columns / differentiate / vjp hold for their columns: grown on demand, kept (a call that repeats its shapes allocates nothing)"""
        out = np.zeros(1, dtype=np.int64)
        self._check(self._L.calipso_hip_sparse_kkt_differentiate_bytes(self._h, _pi(out)), "sparse_kkt_differentiate_bytes")
        return int(out[0])

    def _vector_length(self, name):
        if name == "differentiate_slacks":      # (not a vector of the reference's solver: the s, then the t that differentiate! forms the cone blocks at)
            return 2 * self.nc
        extra = dict(objective=1, lagrangian_hessian=self.nnz[0], equality_jacobian_variables=self.nnz[1], cone_jacobian_variables=self.nnz[2])
        if name in self.PARAMETER_ARRAYS:       # the resident values of dR/dtheta's three blocks on their stored patterns (set_parameter_patterns)
            return (getattr(self, "_parameter_nnz", None) or (0, 0, 0))[self.PARAMETER_ARRAYS.index(name)]
        if name in extra:                       # the evaluator's objective at the solution; the three resident non-zero arrays on their stored patterns
            return extra[name]
        return getattr(self, self.VECTORS[name]) if name in self.VECTORS else 0

    def get(self, name):
        out = np.zeros(self._vector_length(name))
        self._check(self._L.calipso_hip_sparse_kkt_get(self._h, name.encode(), _pd(out), out.size), "sparse_kkt_get(%s)" % name)
        return out

    def set(self, name, v):
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        self._check(self._L.calipso_hip_sparse_kkt_set(self._h, name.encode(), _pd(v), v.size), "sparse_kkt_set(%s)" % name)

    def solution_device(self):
        """the resident point as a CUDA tensor of its own (a device-side copy of the N doubles on the handle's device)"""
        import torch
        p = C.c_void_p()
        self._check(self._L.calipso_hip_sparse_kkt_solution_device(self._h, C.byref(p)), "sparse_kkt_solution_device")

        class View:      # (the CUDA array interface: torch wraps the device memory without a copy)
            __cuda_array_interface__ = dict(shape=(self.N,), typestr="<f8", data=(p.value, False), version=2)
        return torch.as_tensor(View(), device=torch.device("cuda", self.device)).clone()

    def keep_trace(self, rows):
        self._check(self._L.calipso_hip_sparse_kkt_keep_trace(self._h, int(rows)), "sparse_kkt_keep_trace")
        self._trace_rows = int(rows)

    def trace(self):
        """solution.all after each accepted iterate of the last solve (the first keep_trace rows of them)"""
        cap = getattr(self, "_trace_rows", 0)
        out, accepted = np.zeros((max(cap, 1), self.N)), C.c_int64()
        rows = self._check(self._L.calipso_hip_sparse_kkt_trace(self._h, _pd(out), cap, C.byref(accepted)), "sparse_kkt_trace")
        return out[:rows]


class SparseKKTGroup(_Handle):
    """search_direction! for a GROUP of `members` (1 .. 128) same-pattern sparse problems in lockstep (include/calipso_hip.h, "search_direction! on sparse data, for
    GROUPS"; csrc/sparse_kkt_group.hip): one analysis, one multifrontal plan, the members through the same launches.  Lxx, gx, hx, the cones, method, perm, device as
    SparseKKT — only the PATTERNS are taken here; every value array is members x count, member-major: a (members, count) array, or a sequence of `members` sparse
    matrices / vectors.  Member m's results are bit for bit those of a SparseKKT on the same data.  Options are shared; central_path (kappa) and the penalty are per
    member.  There is no `H \\ residual` fallback in a group: a member whose refinement fails gets status 2 and its last refined step."""
    _last_error, _destroy = "calipso_hip_sparse_kkt_group_last_error", "calipso_hip_sparse_kkt_group_destroy"
    _message = _Handle._STATUS_MESSAGE
    REPORT = ("factorization_rounds", "refinement_rounds", "host_waits", "launches", "device_ms", "wall_ms", "last_factorization_active", "last_refinement_active")

    def __init__(self, Lxx, gx, hx, members, n_nonnegative=None, second_order_dims=(), method="nested_dissection", perm=None, device=0, options=None):
        import scipy.sparse as sp
        self._L = lib()
        as_csc = lambda A: A if sp.isspmatrix_csc(A) else sp.csc_matrix(A)
        Lxx, gx, hx = as_csc(Lxx), as_csc(gx), as_csc(hx)
        self.nx, self.ne, self.nc = int(Lxx.shape[0]), int(gx.shape[0]), int(hx.shape[0])
        if Lxx.shape != (self.nx, self.nx) or gx.shape[1] != self.nx or hx.shape[1] != self.nx:
            raise ValueError("SparseKKTGroup: Lxx is nx x nx, gx ne x nx, hx nc x nx")
        self.n, self.N = self.nx + self.ne + self.nc, self.nx + 2 * self.ne + 3 * self.nc
        self.nnz = (int(Lxx.indptr[-1]), int(gx.indptr[-1]), int(hx.indptr[-1]))
        self.members = int(members)
        dims = np.ascontiguousarray(list(second_order_dims), dtype=np.int64)
        if n_nonnegative is None:
            n_nonnegative = self.nc - int(dims.sum())
        one_based = lambda A: (np.ascontiguousarray(A.indptr, dtype=np.int64) + 1, np.ascontiguousarray(A.indices, dtype=np.int64) + 1)
        pats = [one_based(A) for A in (Lxx, gx, hx)]
        pp = None if perm is None else np.ascontiguousarray(perm, dtype=np.int64)
        h = C.c_void_p()
        rc = self._L.calipso_hip_sparse_kkt_group_create(self.nx, self.ne, self.nc, int(n_nonnegative), int(dims.size), _pi(dims) if dims.size else None,
                                                         _pi(pats[0][0]), _pi(pats[0][1]), _pi(pats[1][0]), _pi(pats[1][1]), _pi(pats[2][0]), _pi(pats[2][1]),
                                                         3 if pp is not None else SPARSE_METHODS[method], _pi(pp) if pp is not None else None, device, self.members, C.byref(h))
        if rc != 0:
            raise CalipsoHipError("calipso_hip_sparse_kkt_group_create failed (%d): %s" % (rc, self._L.calipso_hip_sparse_kkt_group_last_error(None).decode()))
        self._h = h
        self.device = int(device)
        info = np.zeros(9, dtype=np.int64)
        self._check(self._L.calipso_hip_sparse_kkt_group_info(self._h, _pi(info)), "sparse_kkt_group_info")
        self.info = dict(n=int(info[0]), nnz_upper=int(info[1]), nnzL=int(info[2]), levels=int(info[3]),
                         numeric={0: "columns_global_accumulator", 1: "columns_lds_accumulator", 2: "multifrontal"}[int(info[4])], assemble_launches=int(info[5]),
                         max_cone_dimension=int(info[6]), N=int(info[7]), members=int(info[8]))
        self._colptr, self._rowval = np.zeros(self.n + 1, dtype=np.int64), np.zeros(max(self.info["nnz_upper"], 1), dtype=np.int64)
        self._check(self._L.calipso_hip_sparse_kkt_group_pattern(self._h, _pi(self._colptr), _pi(self._rowval)), "sparse_kkt_group_pattern")
        self.inertia = [(0, 0, 0)] * self.members
        self.status = 0
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, name, value):
        """the regularisation and refinement options by name, shared by the group; "central_path": every member's kappa.  krylov_fallback = 1 is refused"""
        self._check(self._L.calipso_hip_sparse_kkt_group_set_option(self._h, name.encode(), float(value)), "sparse_kkt_group_set_option(%s)" % name)

    def _is_device(self, a):
        return a is not None and hasattr(a, "is_cuda")

    def _device_pointer(self, a, name, count):
        if a is None:
            return None
        import torch
        if a.dtype != torch.float64 or a.numel() != self.members * count or not a.is_contiguous():
            raise ValueError("%s must be a contiguous float64 tensor of %d x %d entries" % (name, self.members, count))
        if a.is_cuda and a.device.index != self.device:
            raise ValueError("%s is on %s, the group on device %d" % (name, a.device, self.device))
        if a.is_cuda:
            torch.cuda.current_stream(a.device).synchronize()      # the group works on its own stream
        return C.c_void_p(a.data_ptr())      # (a CPU tensor's pointer goes through: the library refuses it, naming the argument)

    def _host(self, a, name, count, what):
        """members x count doubles from a (members, count) array or a sequence of `members` sparse matrices / vectors"""
        if a is None:
            return None
        if not isinstance(a, np.ndarray):
            a = [np.asarray(m.data if hasattr(m, "indptr") else m, dtype=np.float64).reshape(-1) for m in a]
            if any(m.size != count for m in a):
                raise CalipsoHipError("SparseKKTGroup.%s: %s has %s values per member, not %d" % (what, name, sorted(set(m.size for m in a)), count))
        v = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        if v.size != self.members * count:
            raise CalipsoHipError("SparseKKTGroup.%s: %s has %d values, not %d x %d" % (what, name, v.size, self.members, count))
        return v

    def set_values(self, Lxx=None, gx=None, hx=None, w=None, penalty=None, central_path=None):
        """non-zeros of Lxx, gx, hx (per member: sparse matrices of the analysed pattern, or the values in its order), the points w (members x N), the penalties rho
        and central_path kappa (members each, or one number for all); None keeps what is resident.  Host data, or — all that are given of the first five — float64
        CUDA tensors of members x count entries (the device route; central_path stays a host value)."""
        kappa = None if central_path is None else np.ascontiguousarray(np.broadcast_to(np.asarray(central_path, dtype=np.float64).reshape(-1), (self.members,)))
        given = [a for a in (Lxx, gx, hx, w, penalty) if a is not None]
        names, counts = ("Lxx", "gx", "hx", "w", "penalty"), self.nnz + (self.N, 1)
        if given and all(self._is_device(a) for a in given):
            ptrs = [self._device_pointer(a, nm, ct) for a, nm, ct in zip((Lxx, gx, hx, w, penalty), names, counts)]
            self._check(self._L.calipso_hip_sparse_kkt_group_set_values_device(self._h, *(ptrs + [_opt(kappa)])), "sparse_kkt_group_set_values_device")
            return
        if penalty is not None:
            penalty = np.ascontiguousarray(np.broadcast_to(np.asarray(penalty, dtype=np.float64).reshape(-1), (self.members,)))
        arrs = [self._host(a, nm, ct, "set_values") for a, nm, ct in zip((Lxx, gx, hx, w, penalty), names, counts)]
        self._check(self._L.calipso_hip_sparse_kkt_group_set_values(self._h, *[_opt(a) for a in arrs + [kappa]]), "sparse_kkt_group_set_values")

    def factorize(self, ep, ed):
        """one assemble + one batched factorisation, member m at (ep[m], ed[m]) (numbers: the same for all); sets .inertia (a tuple per member); returns the warning
        status (1 = a member met an exact zero pivot)"""
        ep = np.ascontiguousarray(np.broadcast_to(np.asarray(ep, dtype=np.float64).reshape(-1), (self.members,)))
        ed = np.ascontiguousarray(np.broadcast_to(np.asarray(ed, dtype=np.float64).reshape(-1), (self.members,)))
        out = np.zeros(3 * self.members, dtype=np.int64)
        rc = self._check(self._L.calipso_hip_sparse_kkt_group_factorize(self._h, _pd(ep), _pd(ed), _pi(out)), "sparse_kkt_group_factorize")
        self.inertia = [tuple(int(v) for v in out[3 * m:3 * m + 3]) for m in range(self.members)]
        return rc

    def matrix(self, member):
        """triu(jacobian_variables_symmetric) of the member's last assemble, scipy CSC"""
        import scipy.sparse as sp
        nz = np.zeros(max(self.info["nnz_upper"], 1))
        self._check(self._L.calipso_hip_sparse_kkt_group_get_matrix(self._h, int(member), _pd(nz)), "sparse_kkt_group_get_matrix")
        k = self.info["nnz_upper"]
        return sp.csc_matrix((nz[:k], self._rowval[:k] - 1, self._colptr - 1), shape=(self.n, self.n))

    def mul(self, v):
        """H v per member (members x N) for the unreduced matrices at the regularisation of every member's last assemble"""
        v = self._host(v, "v", self.N, "mul")
        out = np.zeros(self.members * self.N)
        self._check(self._L.calipso_hip_sparse_kkt_group_mul(self._h, _pd(v), _pd(out)), "sparse_kkt_group_mul")
        return out.reshape(self.members, self.N)

    def solve_symmetric(self, residual):
        """search_direction_symmetric! per member (members x N) with the current factorisations"""
        r = self._host(residual, "the residual", self.N, "solve_symmetric")
        out = np.zeros(self.members * self.N)
        self._check(self._L.calipso_hip_sparse_kkt_group_solve_symmetric(self._h, _pd(r), _pd(out)), "sparse_kkt_group_solve_symmetric")
        return out.reshape(self.members, self.N)

    def search_direction(self, residual, regularization=(0.0, 0.0, 0.0)):
        """search_direction! of every member in lockstep from regularization = (ep, ep_last, ed) per member (members x 3, or one triple for all): returns
        (steps (members x N), regularizations (a triple per member), infos (a dict per member: factorizations, refinement_rounds, residual_norm), statuses (per member:
        0, 2 = refinement failed, -1 = inertia correction failed: that member's step is left as it was — zeros on the host route), report (dict of REPORT)).  .status
        is the worst member status.  A CUDA tensor as residual: the device route, the steps come back as a CUDA tensor."""
        reg = np.ascontiguousarray(np.broadcast_to(np.asarray(regularization, dtype=np.float64).reshape(-1, 3), (self.members, 3))).copy()
        info, status, report = np.zeros(4 * self.members), np.zeros(self.members, dtype=np.int32), np.zeros(8)
        if self._is_device(residual):
            import torch
            step = torch.zeros(self.members, self.N, dtype=torch.float64, device=torch.device("cuda", self.device))
            rp = self._device_pointer(residual, "residual", self.N)
            torch.cuda.current_stream(step.device).synchronize()
            rc = self._L.calipso_hip_sparse_kkt_group_search_direction_device(self._h, rp, C.c_void_p(step.data_ptr()), _pd(reg), _pd(info), status.ctypes.data_as(C.POINTER(C.c_int32)), _pd(report))
        else:
            r = self._host(residual, "the residual", self.N, "search_direction")
            step = np.zeros((self.members, self.N))
            rc = self._L.calipso_hip_sparse_kkt_group_search_direction(self._h, _pd(r), _pd(step), _pd(reg), _pd(info), status.ctypes.data_as(C.POINTER(C.c_int32)), _pd(report))
        if rc != -1:                                             # (CALIPSO_ERR_INERTIA is a member's status here: the others went on)
            self._check(rc, "search_direction! (group)")
        self.status = int(rc)
        self.regularization = [tuple(float(v) for v in reg[m]) for m in range(self.members)]
        infos = [dict(factorizations=int(info[4 * m]), refinement_rounds=int(info[4 * m + 1]), residual_norm=float(info[4 * m + 2])) for m in range(self.members)]
        rep = dict(zip(self.REPORT, (float(v) for v in report)))
        for k in self.REPORT:
            if not k.endswith("_ms"):
                rep[k] = int(rep[k])
        return step, self.regularization, infos, [int(v) for v in status], rep

    def timing(self):
        """device milliseconds of the last search_direction: dict(inertia_correction, solve, refinement, wall, device)"""
        ms = np.zeros(8)
        self._check(self._L.calipso_hip_sparse_kkt_group_timing(self._h, _pd(ms)), "sparse_kkt_group_timing")
        return dict(inertia_correction=float(ms[0]), solve=float(ms[1]), refinement=float(ms[2]), wall=float(ms[5]), device=float(ms[6]))

    # ---- solve! of every member in lockstep (include/calipso_hip.h, "solve! on sparse data, for GROUPS"; csrc/sparse_solve_group.hip) ----
    SOLVE_REPORT = REPORT + ("ticks", "outer_update_rounds", "line_search_trial_rounds", "solve_host_waits", "solve_launches", "vector_ms", "search_direction_ms", "solve_wall_ms")

    def attach_qp(self, q, b, h, objective_constants=None):
        """the vectors of every member's conic QP besides Lxx, gx, hx (set_values): q (members x nx), b (members x ne), h (members x nc) — (members, count) arrays or
        sequences of `members` vectors — and one objective constant per member (host values).  Host arrays or — all three — float64 CUDA tensors"""
        counts = (self.nx, self.ne, self.nc)
        const = None if objective_constants is None else np.ascontiguousarray(np.broadcast_to(np.asarray(objective_constants, dtype=np.float64).reshape(-1), (self.members,)))
        if all(self._is_device(a) for a in (q, b, h)):
            ptrs = [self._device_pointer(a, nm, ct) for a, nm, ct in zip((q, b, h), ("q", "b", "h"), counts)]
            self._check(self._L.calipso_hip_sparse_kkt_group_qp_attach_device(self._h, *(ptrs + [_opt(const)])), "sparse_kkt_group_qp_attach_device")
            return
        arrs = [self._host(a, nm, ct, "attach_qp") for a, nm, ct in zip((q, b, h), ("q", "b", "h"), counts)]
        self._check(self._L.calipso_hip_sparse_kkt_group_qp_attach(self._h, *[_opt(a) for a in arrs + [const]]), "sparse_kkt_group_qp_attach")

    def initialize(self, x0):
        """initialize!(solver, x0) of every member: x0 (members x nx) — a host array, or a CUDA tensor"""
        if self._is_device(x0):
            self._check(self._L.calipso_hip_sparse_kkt_group_initialize_device(self._h, self._device_pointer(x0, "x0", self.nx)), "sparse_kkt_group_initialize_device")
        else:
            self._check(self._L.calipso_hip_sparse_kkt_group_initialize(self._h, _opt(self._host(x0, "x0", self.nx, "initialize"))), "sparse_kkt_group_initialize")

    def solve(self):
        """solve! of every member in lockstep: (statuses (per member: 1 solved, 0 iteration caps, -102 a refinement failure without continue_after_refinement_failure
        — the point is the last accepted iterate —, -1 / -2 the reference's inertia / cone search error()s), infos (a dict per member, SparseKKT.SOLVE_INFO),
        report (dict of SOLVE_REPORT)).  .status is the worst member status; refused arguments raise.  Member m's results are bit for bit SparseKKT.solve's."""
        status, info, report = np.zeros(self.members, dtype=np.int32), np.zeros(16 * self.members), np.zeros(16)
        rc = self._L.calipso_hip_sparse_kkt_group_solve(self._h, status.ctypes.data_as(C.POINTER(C.c_int32)), _pd(info), _pd(report))
        if rc < 0 and not any(int(v) == rc for v in status):         # (a member's error status is that member's: the others went on)
            self._check(rc, "solve! (group)")
        self.status = int(rc)
        infos = []
        for m in range(self.members):
            out = dict(zip(SparseKKT.SOLVE_INFO, (float(v) for v in info[16 * m:16 * m + 16])))
            for k in SparseKKT.SOLVE_INFO[:9] + ("status",):
                out[k] = int(out[k])
            infos.append(out)
        rep = dict(zip(self.SOLVE_REPORT, (float(v) for v in report)))
        for k in self.SOLVE_REPORT:
            if not k.endswith("_ms"):
                rep[k] = int(rep[k])
        self.solve_info, self.solve_report = infos, rep
        return [int(v) for v in status], infos, rep

    def get(self, name, member):
        """a resident vector of `member` by SparseKKT's names (SparseKKT.VECTORS)"""
        out = np.zeros(getattr(self, SparseKKT.VECTORS[name]) if name in SparseKKT.VECTORS else 0)
        self._check(self._L.calipso_hip_sparse_kkt_group_get(self._h, name.encode(), int(member), _pd(out), out.size), "sparse_kkt_group_get(%s)" % name)
        return out

    def solution_device(self):
        """the members' resident points as a CUDA tensor of its own (members x N)"""
        import torch
        p = C.c_void_p()
        self._check(self._L.calipso_hip_sparse_kkt_group_solution_device(self._h, C.byref(p)), "sparse_kkt_group_solution_device")

        class View:      # (the CUDA array interface: torch wraps the device memory without a copy)
            __cuda_array_interface__ = dict(shape=(self.members, self.N), typestr="<f8", data=(p.value, False), version=2)
        return torch.as_tensor(View(), device=torch.device("cuda", self.device)).clone()

    def keep_trace(self, rows):
        self._check(self._L.calipso_hip_sparse_kkt_group_keep_trace(self._h, int(rows)), "sparse_kkt_group_keep_trace")
        self._trace_rows = int(rows)

    def trace(self, member):
        """solution.all after each accepted iterate of `member` in the last solve (the first keep_trace rows of them)"""
        cap = getattr(self, "_trace_rows", 0)
        out, accepted = np.zeros((max(cap, 1), self.N)), C.c_int64()
        rows = self._check(self._L.calipso_hip_sparse_kkt_group_trace(self._h, int(member), _pd(out), cap, C.byref(accepted)), "sparse_kkt_group_trace")
        return out[:rows]


def SparseConicQPGroup(problems, n_nonnegative=None, second_order_dims=(), objective_scale=0.5, **kw):
    """a list of (P, q, A, b, G, h) — min c x'Px + q'x  s.t.  Ax - b = 0,  h - Gx in K per member, as SparseConicQP takes them — as a SparseKKTGroup ready for
    initialize / solve: Lxx = c (P + P'), gx = A, hx = -G as CSC, every member's values and q, b, h resident.  Every member must have the first one's patterns:
    another pattern is refused with a message naming the member.  **kw goes to SparseKKTGroup"""
    import scipy.sparse as sp
    mats, vecs = [], []
    for m, (P, q, A, b, G, h) in enumerate(problems):
        P, A, G = (sp.csc_matrix(M) for M in (P, A, G))
        trio = [sp.csc_matrix(objective_scale * (P + P.T)), sp.csc_matrix(A), sp.csc_matrix(-G)]
        for M in trio:
            M.sort_indices()
        if mats:
            for name, M, first in zip(("P + P'", "A", "G"), trio, mats[0]):
                if M.shape != first.shape or not np.array_equal(M.indptr, first.indptr) or not np.array_equal(M.indices, first.indices):
                    raise CalipsoHipError("SparseConicQPGroup: member %d: the pattern of %s is not member 0's (a group shares one analysis; same-pattern problems only)" % (m, name))
        mats.append(trio); vecs.append((q, b, h))
    if not mats:
        raise CalipsoHipError("SparseConicQPGroup: no members")
    g = SparseKKTGroup(mats[0][0], mats[0][1], mats[0][2], len(mats), n_nonnegative=n_nonnegative, second_order_dims=second_order_dims, **kw)
    g.set_values([t[0] for t in mats], [t[1] for t in mats], [t[2] for t in mats])
    g.attach_qp([v[0] for v in vecs], [v[1] for v in vecs], [v[2] for v in vecs])
    return g


def SparseConicQP(P, q, A, b, G, h, n_nonnegative=None, second_order_dims=(), objective_scale=0.5, **kw):
    """min c x'Px + q'x  s.t.  Ax - b = 0,  h - Gx in K  (c = objective_scale) as a SparseKKT ready for initialize / solve: Lxx = c (P + P'), gx = A, hx = -G as CSC,
    values and q, b, h resident.  P, A, G: scipy sparse matrices (or dense arrays); the cones as SparseKKT takes them; **kw goes to SparseKKT.  The handle's vjp then
    also answers for "P", "A", "G": gradients on the stored patterns of P, A, G as given here (CSC order)"""
    import scipy.sparse as sp
    P, A, G = (sp.csc_matrix(M) for M in (P, A, G))
    Lxx, gx, hx = sp.csc_matrix(objective_scale * (P + P.T)), A, sp.csc_matrix(-G)
    for M in (Lxx, gx, hx):
        M.sort_indices()
    s = SparseKKT(Lxx, gx, hx, n_nonnegative=n_nonnegative, second_order_dims=second_order_dims, **kw)
    s.set_values(Lxx, gx, hx)
    s.attach_qp(q, b, h)
    # for SparseKKT.vjp(qp="P..."): where the stored entries (i, j) of P and their mirrors (j, i) lie in Lxx's non-zero order (-1: not in its pattern)
    nx = s.nx
    keys = np.repeat(np.arange(nx, dtype=np.int64), np.diff(Lxx.indptr)) * nx + Lxx.indices      # column-major keys of a sorted CSC pattern: ascending
    def position(rows, cols):
        want = cols.astype(np.int64) * nx + rows
        at = np.minimum(np.searchsorted(keys, want), max(keys.size - 1, 0))
        return np.where(keys[at] == want, at, -1) if keys.size else np.full(want.shape, -1, dtype=np.int64)
    P_csc = sp.csc_matrix(P)
    rows, cols = P_csc.indices, np.repeat(np.arange(nx), np.diff(P_csc.indptr))
    s._conic_qp = (position(rows, cols), position(cols, rows), float(objective_scale))
    return s


class SmallBatch(_Handle):
    """`batch` independent small systems (n <= 128) factored and solved for `nrhs` right-hand sides each in ONE launch, every system
    resident in the LDS of one workgroup (include/calipso_hip.h, "batched small systems"): the sensitivity solves of differentiate!
    (src/solver/differentiate.jl:29-58) for many MPC steps at once."""
    _last_error, _destroy = "calipso_hip_small_last_error", "calipso_hip_small_destroy"

    def __init__(self, n, nrhs, batch, device=0):
        self._L = lib()
        self.n, self.nrhs, self.batch = int(n), int(nrhs), int(batch)
        h = C.c_void_p()
        rc = self._L.calipso_hip_small_create(self.n, self.nrhs, self.batch, device, C.byref(h))
        if rc != 0:
            msg = self._L.calipso_hip_small_last_error(h if h.value else None).decode()
            if h.value:
                self._L.calipso_hip_small_destroy(h)
            raise CalipsoHipError("calipso_hip_small_create failed (%d): %s" % (rc, msg))
        self._h = h

    def set(self, K=None, B=None):
        """K: (batch, n, n) matrices (only the upper triangles are read); B: (batch, n, nrhs) right-hand sides"""
        kk = bb = None
        if K is not None:
            kk = np.ascontiguousarray(np.transpose(np.asarray(K, dtype=np.float64).reshape(self.batch, self.n, self.n), (0, 2, 1))).reshape(-1)
        if B is not None:
            bb = np.ascontiguousarray(np.transpose(np.asarray(B, dtype=np.float64).reshape(self.batch, self.n, self.nrhs), (0, 2, 1))).reshape(-1)
        self._check(self._L.calipso_hip_small_set(self._h, _pd(kk) if kk is not None else None, _pd(bb) if bb is not None else None), "small_set")

    def solve(self):
        """factor + solve every instance (one launch); returns the launch duration in milliseconds"""
        ms = C.c_double(0.0)
        self._check(self._L.calipso_hip_small_solve(self._h, C.byref(ms)), "small_solve")
        return float(ms.value)

    def get(self):
        """(X (batch, n, nrhs), inertia (batch, 3), number of instances that met an exact zero pivot)"""
        x = np.zeros(self.batch * self.n * self.nrhs)
        inr = np.zeros(3 * self.batch, dtype=np.int64)
        bad = self._check(self._L.calipso_hip_small_get(self._h, _pd(x), _pi(inr)), "small_get")
        return np.transpose(x.reshape(self.batch, self.nrhs, self.n), (0, 2, 1)), inr.reshape(self.batch, 3), bad


class SmallNewtonBatch(_Handle):
    """Solver / initialize! / solve! (src/solver/solver.jl:46-150, initialize.jl:9-48, solve.jl:8-377) for `batch` independent small conic QPs of one shape in ONE
    kernel launch: a workgroup per instance, everything in LDS, every decision of solve! on the device (include/calipso_hip.h, "solve! for a batch of SMALL conic QPs";
    csrc/smallnewton.hip).  QP data as qp_attach: min c x'Px + q'x s.t. Ax = b, h - Gx >= 0 (nonnegative cones).  options={...} go to set_option: the reference's
    options by name, "threads" (0, 64, 128, 256) and "lu_fallback" (0 or 1: where iterative refinement fails, take the reference's H \\ residual inside the kernel
    instead of stopping the instance with -102; costs batch x N^2 doubles of device memory).  Nonlinear problems: set_evaluator with a device evaluator compiled
    into a HIP library of the caller's (include/calipso_smallnewton.hpp), set_parameters, differentiate() with dR/dtheta from the evaluator.  vjp(): the
    reverse mode — gradients of a loss with respect to theta or the QP's data with one solve per cotangent (torch_layer.QPLayer builds on it)."""
    _last_error, _destroy = "calipso_hip_smallnewton_last_error", "calipso_hip_smallnewton_destroy"

    def __init__(self, nx, ne, nc, batch, device=0, options=None):
        self._L = lib()
        self.nx, self.ne, self.nc, self.batch = int(nx), int(ne), int(nc), int(batch)
        self.N = self.nx + 2 * self.ne + 3 * self.nc
        h = C.c_void_p()
        rc = self._L.calipso_hip_smallnewton_create(self.nx, self.ne, self.nc, self.batch, device, C.byref(h))
        if rc != 0:
            msg = self._L.calipso_hip_smallnewton_last_error(h if h.value else None).decode()
            if h.value:
                self._L.calipso_hip_smallnewton_destroy(h)
            raise CalipsoHipError("calipso_hip_smallnewton_create failed (%d): %s" % (rc, msg))
        self._h = h
        self.device = int(device)
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, name, value):
        self._check(self._L.calipso_hip_smallnewton_set_option(self._h, name.encode(), float(value)), "smallnewton_set_option(%s)" % name)

    def set_cones(self, n_nonnegative, second_order_dims=()):
        """cone layout: the first n_nonnegative cone entries nonnegative, then second-order cones of the given dimensions (contiguous)"""
        dims = np.ascontiguousarray(list(second_order_dims), dtype=np.int64)
        self._check(self._L.calipso_hip_smallnewton_set_cones(self._h, int(n_nonnegative), int(dims.size), _pi(dims) if dims.size else None), "smallnewton_set_cones")

    def set_qp(self, P, q, A, b, G, h, objective_scale=0.5, shared=None):
        """arrays of ONE problem (P (nx, nx), q (nx), A (ne, nx), ...) shared by all instances, or stacked along a leading batch axis"""
        P = np.asarray(P, dtype=np.float64)
        if shared is None:
            shared = P.ndim == 2
        K = 1 if shared else self.batch
        cm = lambda M, r, c: np.ascontiguousarray(np.transpose(np.asarray(M, dtype=np.float64).reshape(K, r, c), (0, 2, 1))).reshape(-1) if r * c else np.zeros(1)
        vv = lambda a, n: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(K, n)).reshape(-1) if n else np.zeros(1)
        Pc, Ac, Gc = cm(P, self.nx, self.nx), cm(A, self.ne, self.nx), cm(G, self.nc, self.nx)
        qv, bv, hv = vv(q, self.nx), vv(b, self.ne), vv(h, self.nc)
        self._check(self._L.calipso_hip_smallnewton_set_qp(self._h, _pd(Pc), _pd(qv), _pd(Ac), _pd(bv), _pd(Gc), _pd(hv), float(objective_scale), int(bool(shared))), "smallnewton_set_qp")
        self._evaluator = False

    def set_evaluator(self, cdll, symbol, n_parameters=0):
        """a device evaluator instead of the QP: `symbol` is the entry that CALIPSO_SMALLNEWTON_EVALUATOR (include/calipso_smallnewton.hpp) emitted into the HIP shared
        library `cdll` (a ctypes.CDLL, or its path); n_parameters = the length of theta per instance (set_parameters)"""
        if not isinstance(cdll, C.CDLL):
            cdll = C.CDLL(str(cdll))
        self._evlib = cdll                                                      # (the entry's code must outlive the handle's use of it)
        fn = C.cast(getattr(cdll, symbol), C.c_void_p)
        self.n_parameters = int(n_parameters)
        self._check(self._L.calipso_hip_smallnewton_set_evaluator(self._h, fn, self.n_parameters), "smallnewton_set_evaluator(%s)" % symbol)
        self._evaluator = True

    def set_parameters(self, theta):
        """theta (batch, n_parameters) per instance, or (n_parameters,) shared by all"""
        th = np.asarray(theta, dtype=np.float64)
        shared = th.ndim == 1
        if th.shape[-1] != getattr(self, "n_parameters", -1) or (not shared and th.shape != (self.batch, self.n_parameters)):
            raise ValueError("theta must be (batch, n_parameters) or (n_parameters,)")
        th = np.ascontiguousarray(th).reshape(-1)
        self._check(self._L.calipso_hip_smallnewton_set_parameters(self._h, _pd(th), int(shared)), "smallnewton_set_parameters")

    def set_state(self, w=None, dual=None, scalars=None):
        """w: (batch, N) points; dual: (batch, ne) multiplier estimates; scalars: (batch, 3) [central_path, fraction_to_boundary, penalty]"""
        f = lambda a, n: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(self.batch, n)).reshape(-1)
        ww, ll, ss = f(w, self.N), f(dual, max(self.ne, 1)) if (dual is not None and self.ne) else None, f(scalars, 3)
        self._check(self._L.calipso_hip_smallnewton_set_state(self._h, _pd(ww) if ww is not None else None, _pd(ll) if ll is not None else None, _pd(ss) if ss is not None else None), "smallnewton_set_state")

    def initialize(self, x0):
        """initialize!(solver, guess) for every instance: x0 (batch, nx) or one guess for all"""
        x0 = np.asarray(x0, dtype=np.float64)
        w = np.zeros((self.batch, self.N))
        w[:, :self.nx] = x0.reshape(-1, self.nx)
        self.set_state(w=w)

    def get_state(self):
        w = np.zeros(self.batch * self.N); lam = np.zeros(self.batch * max(self.ne, 1)); sc = np.zeros(self.batch * 6); cn = np.zeros(self.batch * 8, dtype=np.int64)
        self._check(self._L.calipso_hip_smallnewton_get_state(self._h, _pd(w), _pd(lam), _pd(sc), _pi(cn)), "smallnewton_get_state")
        names = ("total_iterations", "outer", "factorizations", "refinement_failures", "max_refinement_rounds", "last_refinement_rounds", "newton_steps", "accepted_iterates")
        return dict(solution=w.reshape(self.batch, self.N), dual=lam.reshape(self.batch, -1)[:, :self.ne], scalars=sc.reshape(self.batch, 6),
                    counters={n: cn.reshape(self.batch, 8)[:, i].copy() for i, n in enumerate(names)})

    def keep_trace(self, rows):
        self._trace_rows = int(rows)
        self._check(self._L.calipso_hip_smallnewton_trace(self._h, int(rows), None), "smallnewton_trace")

    def trace(self, rows=None):
        rows = int(rows if rows is not None else self._trace_rows)
        out = np.zeros(self.batch * rows * self.N)
        self._check(self._L.calipso_hip_smallnewton_trace(self._h, rows, _pd(out)), "smallnewton_trace")
        return out.reshape(self.batch, rows, self.N)

    def solve(self):
        """solve! of every instance, one launch: (result (batch,) int32 — 1 converged, 0 caps reached, < 0 see include/calipso_hip.h —, launch milliseconds)"""
        res = np.zeros(self.batch, dtype=np.int32); ms = C.c_double(0.0)
        self._check(self._L.calipso_hip_smallnewton_solve(self._h, res.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ms)), "smallnewton_solve")
        return res, float(ms.value)

    def steps(self, count, advance=False):
        """`count` Newton steps of every instance in one launch: (info (batch, 8), status (batch,), launch milliseconds)"""
        info = np.zeros(self.batch * 8); st = np.zeros(self.batch, dtype=np.int32); ms = C.c_double(0.0)
        self._check(self._L.calipso_hip_smallnewton_steps(self._h, int(count), int(bool(advance)), _pd(info), st.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ms)), "smallnewton_steps")
        return info.reshape(self.batch, 8), st, float(ms.value)

    def differentiate(self, jacobian_parameters=None):
        """differentiate! of every instance at its resident point, one launch (differentiate.jl:1-61): jacobian_parameters (batch, N, p) = dR/dtheta per instance, or
        (N, p) = one matrix for all instances, or None = the evaluator's dR/dtheta at the resident points (p = n_parameters); returns (sensitivity (batch, N, p) =
        dw/dtheta, status (batch,) — 1: the factorisation's inertia is not (nx, ne + nc, 0) —, launch milliseconds)"""
        N = self.nx + 2 * self.ne + 3 * self.nc
        if jacobian_parameters is None:
            p = getattr(self, "n_parameters", 0)
            out = np.zeros(self.batch * N * max(p, 1)); st = np.zeros(self.batch, dtype=np.int32); ms = C.c_double(0.0)
            self._check(self._L.calipso_hip_smallnewton_differentiate_parameters(self._h, _pd(out), st.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ms)), "smallnewton_differentiate_parameters")
            return np.transpose(out.reshape(self.batch, p, N), (0, 2, 1)).copy(), st, float(ms.value)
        J = np.asarray(jacobian_parameters, dtype=np.float64)
        shared = J.ndim == 2
        if shared:
            J = J[None]
        if J.ndim != 3 or J.shape[0] != (1 if shared else self.batch) or J.shape[1] != N:
            raise ValueError("jacobian_parameters must be (batch, N, p) or (N, p)")
        p = J.shape[2]
        Jc = np.ascontiguousarray(np.transpose(J, (0, 2, 1))).ravel()          # per instance column-major N x p
        out = np.zeros(self.batch * N * p); st = np.zeros(self.batch, dtype=np.int32); ms = C.c_double(0.0)
        self._check(self._L.calipso_hip_smallnewton_differentiate(self._h, int(p), int(shared), _pd(Jc), _pd(out), st.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ms)), "smallnewton_differentiate")
        return np.transpose(out.reshape(self.batch, p, N), (0, 2, 1)).copy(), st, float(ms.value)

    def vjp(self, cotangent, adjoint=True, theta=None, qp=None):
        """differentiate! in reverse mode, one launch (calipso_hip_smallnewton_differentiate_adjoint): for cotangents v = dLoss/dw at the resident points,
        lambda = M' v and the gradients v'S for the S = dw/dtheta that differentiate() would return.  cotangent: (batch, N) or (batch, N, k), or (batch, nx) /
        (batch, nx, k) for x alone (the other rows zero).  theta: -R_theta' lambda with the evaluator's dR/dtheta (default: when an evaluator with parameters is
        set); qp: the built-in QP's data gradients (default: when the QP is set).  Returns a dict: "adjoint" (batch, N[, k]), "theta" (batch, n_parameters[, k]),
        "P", "q", "A", "b", "G", "h" in set_qp's shapes (per instance, [, k]), "status" (batch,) as differentiate() and "ms"; the trailing k axis only when the
        cotangent had one"""
        message = "cotangent must be (batch, N), (batch, N, k), (batch, nx) or (batch, nx, k)"
        lead = (self.batch,)
        vc, k, squeeze = pack_cotangent(cotangent, lead, self.N, message, also=self.nx)
        if k < 1:
            raise ValueError(message)
        p, theta, qp = self._vjp_defaults(theta, qp)
        shape = qp_shapes(self.nx, self.ne, self.nc)
        nqp = sum(int(np.prod(s)) for s in shape.values())
        adj = np.zeros(self.batch * self.N * k) if adjoint else None
        gth = np.zeros(self.batch * k * max(p, 1)) if theta else None
        gqp = np.zeros(self.batch * k * nqp) if qp else None
        st = np.zeros(self.batch, dtype=np.int32); ms = C.c_double(0.0)
        self._check(self._L.calipso_hip_smallnewton_differentiate_adjoint(self._h, int(k), _pd(vc), _opt(adj), _opt(gth), _opt(gqp), st.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                           C.byref(ms)), "smallnewton_differentiate_adjoint")
        out = dict(status=st, ms=float(ms.value))
        if adjoint:
            out["adjoint"] = unpack_columns(adj, lead, k, (self.N,), squeeze)
        if theta:
            out["theta"] = unpack_columns(gth, lead, k, (p,), squeeze)
        if qp:      # ONE buffer: per instance and column the six arrays one after the other
            g = gqp.reshape(self.batch, k, nqp)
            at = 0
            for name, sh in shape.items():
                n = int(np.prod(sh))
                out[name] = unpack_columns(g[:, :, at:at + n], lead, k, sh, squeeze)
                at += n
        return out

    def _vjp_defaults(self, theta, qp):
        """(n_parameters in use, theta, qp) of vjp() / vjp_device(): theta by default when an evaluator with parameters is set, qp when the QP is"""
        evaluator = getattr(self, "_evaluator", False)
        p = getattr(self, "n_parameters", 0) if evaluator else 0
        return p, (evaluator and p > 0) if theta is None else theta, (not evaluator) if qp is None else qp

    # ---- the device-resident, stream-ordered entries (include/calipso_hip.h; csrc/smallnewton_io.hip): torch CUDA tensors in and out, nothing waits for the device ----
    def _qp_dims(self):
        return tuple(qp_shapes(self.nx, self.ne, self.nc).values())

    def _form(self, t, name, shapes, dtype="float64"):
        """a torch tensor of the dtype and one of the shapes, contiguous"""
        import torch
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a torch tensor" % name)
        if t.dtype != getattr(torch, dtype):
            raise ValueError("%s must be %s, not %s" % (name, dtype, t.dtype))
        if tuple(t.shape) not in [tuple(s) for s in shapes]:
            raise ValueError("%s must have shape %s, not %s" % (name, " or ".join(str(tuple(s)) for s in shapes), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)

    def _ptr(self, t, name):
        """a tensor on the handle's device: its device pointer (None for an empty tensor)"""
        if not t.is_cuda:
            raise ValueError("%s must be a CUDA tensor: the device entries take device memory only" % name)
        if t.device.index != getattr(self, "device", 0):
            raise ValueError("%s is on %s, the handle on device %d" % (name, t.device, getattr(self, "device", 0)))
        return C.c_void_p(t.data_ptr()) if t.numel() else None

    def _dev(self, t, name, shapes, dtype="float64"):
        """the checks every tensor passes before any C call: its form, then where it lives; returns its device pointer"""
        self._form(t, name, shapes, dtype)
        return self._ptr(t, name)

    def _empty(self, shape, dtype="float64"):
        import torch
        return torch.empty(shape, dtype=getattr(torch, dtype), device=torch.device("cuda", getattr(self, "device", 0)))

    def set_stream(self, stream=None):
        """all later work of the handle goes to `stream` — a torch.cuda.Stream (e.g. torch.cuda.current_stream()) or a raw hipStream_t as an int (0: the legacy
        default stream) —, or back to the handle's own stream (None).  The new stream waits on the device for what the old one holds; the handle does not own it."""
        if stream is None:
            self._check(self._L.calipso_hip_smallnewton_set_stream(self._h, None, 0), "smallnewton_set_stream")
        else:
            raw = int(getattr(stream, "cuda_stream", stream))
            self._check(self._L.calipso_hip_smallnewton_set_stream(self._h, C.c_void_p(raw), 1), "smallnewton_set_stream")

    def set_qp_device(self, P, q, A, b, G, h, objective_scale=0.5, row_major=True):
        """set_qp from float64 CUDA tensors, packed on the device.  Each array is ONE for all instances (P (nx, nx), q (nx,), A (ne, nx), ...) or stacked along a
        leading batch axis, independently of the others: a shared P is stored once.  row_major=False: the matrices are column-major, i.e. tensors of the transposed
        shape ([batch,] nx, rows).  Returns the mask of shared arrays (bit i: array i of P, q, A, b, G, h)."""
        data, mask = (P, q, A, b, G, h), 0
        for i, (name, t, dm) in enumerate(zip(QP_NAMES, data, self._qp_dims())):
            if len(dm) == 2 and not row_major:
                dm = (dm[1], dm[0])
            self._form(t, name, (dm, (self.batch,) + dm))
            if t.dim() == len(dm):
                mask |= 1 << i
        ptrs = [self._ptr(t, name) for name, t in zip(QP_NAMES, data)]
        self._check(self._L.calipso_hip_smallnewton_set_qp_device(self._h, *ptrs, float(objective_scale), mask, int(bool(row_major))), "smallnewton_set_qp_device")
        self._evaluator = False
        return mask

    def initialize_device(self, x0=None):
        """initialize!(solver, guess) for every instance: x0 (batch, nx) on the device, or None for zeros"""
        ptr = self._dev(x0, "x0", ((self.batch, self.nx),)) if x0 is not None else None
        self._check(self._L.calipso_hip_smallnewton_initialize_device(self._h, ptr), "smallnewton_initialize_device")

    def set_state_device(self, w=None, dual=None, scalars=None):
        """set_state from CUDA tensors: w (batch, N), dual (batch, ne), scalars (batch, 3) [central_path, fraction_to_boundary, penalty]"""
        pw = self._dev(w, "w", ((self.batch, self.N),)) if w is not None else None
        pl = self._dev(dual, "dual", ((self.batch, self.ne),)) if dual is not None else None
        ps = self._dev(scalars, "scalars", ((self.batch, 3),)) if scalars is not None else None
        self._check(self._L.calipso_hip_smallnewton_set_state_device(self._h, pw, pl, ps), "smallnewton_set_state_device")

    def set_parameters_device(self, theta):
        """theta (batch, n_parameters) per instance, or (n_parameters,) shared by all, on the device"""
        p = getattr(self, "n_parameters", -1)
        ptr = self._dev(theta, "theta", ((self.batch, p), (p,)))
        if ptr is not None:
            self._check(self._L.calipso_hip_smallnewton_set_parameters_device(self._h, ptr, int(theta.dim() == 1)), "smallnewton_set_parameters_device")

    def solve_device(self):
        """solve! of every instance, enqueued on the handle's stream: nothing comes back (solution_device, status_device)"""
        self._check(self._L.calipso_hip_smallnewton_solve_device(self._h), "smallnewton_solve_device")

    def solution_device(self, out=None, parts="xyz"):
        """x (batch, nx), y (batch, ne), z (batch, nc), w (batch, N) and status (batch,) int32 — the status of the last solve — gathered on the device: a dict
        with the keys named in `parts` (letters of "xyzw" and "s" for status) and those of `out`, a dict of tensors to write into (allocated with torch otherwise)"""
        shapes = dict(x=(self.batch, self.nx), y=(self.batch, self.ne), z=(self.batch, self.nc), w=(self.batch, self.N), status=(self.batch,))
        res = dict(out or {})
        for key in res:
            if key not in shapes:
                raise ValueError("solution_device: unknown output %r" % key)
        for letter in parts:
            key = "status" if letter == "s" else letter
            if key not in shapes:
                raise ValueError("solution_device: parts are letters of 'xyzws'")
        ptrs = {key: self._dev(t, key, (shapes[key],), "int32" if key == "status" else "float64") for key, t in res.items()}
        for letter in parts:
            key = "status" if letter == "s" else letter
            if key not in res:
                res[key] = self._empty(shapes[key], "int32" if key == "status" else "float64")
                ptrs[key] = C.c_void_p(res[key].data_ptr()) if res[key].numel() else None
        self._check(self._L.calipso_hip_smallnewton_get_solution_device(self._h, *[ptrs.get(key) for key in ("x", "y", "z", "w", "status")]), "smallnewton_get_solution_device")
        return res

    def status_device(self):
        """the solve status of every instance (1 converged, 0 caps reached, < 0: include/calipso_hip.h) of the last solve, as an int32 CUDA tensor: no read-back"""
        return self.solution_device(parts="s")["status"]

    def vjp_device(self, cotangent=None, x=None, y=None, z=None, adjoint=False, theta=None, qp=None, reduce="", out=None):
        """vjp() on the device (calipso_hip_smallnewton_differentiate_adjoint_device), CUDA tensors in and out.  The cotangent: `cotangent` (batch, N[, k]), or its
        parts x (batch, nx[, k]), y (batch, ne[, k]), z (batch, nc[, k]) — the rest zero.  theta / qp as vjp(); qp may also name the arrays wanted ("Pq").  reduce:
        names of the QP arrays whose gradient is summed over the batch on the device (deterministic: fixed chunks of 64 instances in order).  Gradients of an
        instance whose last SOLVE status is not 1 are NaN, before any sum.  Returns a dict as vjp() — "adjoint", "theta", "P" .. "h" in vjp()'s shapes (views of the
        buffers the kernels wrote; summed arrays without the batch axis) — and "status" (batch,) int32 as differentiate(), all on the device.  out: buffers to
        write into, in the kernels' layout: "adjoint" (batch, k, N), "theta" (batch, k, n_parameters), a QP array ([batch,] k) + its shape, "status" (batch,)."""
        B, N = self.batch, self.N
        mask = 0
        for n in (reduce or ""):
            if n not in QP_NAMES:
                raise ValueError("vjp_device: reduce names arrays of " + QP_NAMES)
            mask |= 1 << QP_NAMES.index(n)
        given = [(n, t) for n, t in (("cotangent", cotangent), ("x", x), ("y", y), ("z", z)) if t is not None]
        if not given or (cotangent is not None and len(given) > 1):
            raise ValueError("vjp_device: the cotangent as `cotangent` (batch, N[, k]) or as parts x, y, z")
        nd = given[0][1].dim() if hasattr(given[0][1], "dim") else -1
        k = given[0][1].shape[2] if nd == 3 else 1
        squeeze = nd != 3
        if k < 1:
            raise ValueError("vjp_device: k >= 1 cotangent columns")
        widths = dict(cotangent=N, x=self.nx, y=self.ne, z=self.nc)
        for n, t in given:
            self._form(t, n, [(B, widths[n]) + ((k,) if nd == 3 else ())])
        ptrs, keep = {}, []      # (keep: the permuted copies, alive until the call is enqueued)
        for n, t in given:
            ptrs[n] = self._ptr(t, n)
            if nd == 3 and k > 1 and t.numel():      # (batch, n, k) -> the kernel's column-major n x k per instance
                t = t.permute(0, 2, 1).contiguous()
                ptrs[n] = C.c_void_p(t.data_ptr())
            keep.append(t)
        p, theta, qp = self._vjp_defaults(theta, qp)
        names = qp_names(qp)
        out = dict(out or {})
        bufs = {}

        def buffer(key, shape, dtype="float64"):
            if key in out:
                self._dev(out[key], key, (shape,), dtype)
                bufs[key] = out[key]
            else:
                bufs[key] = self._empty(shape, dtype)
            return C.c_void_p(bufs[key].data_ptr()) if bufs[key].numel() else None

        p_adj = buffer("adjoint", (B, k, N)) if adjoint else None
        p_th = buffer("theta", (B, k, max(p, 1))) if theta else None
        p_st = buffer("status", (B,), "int32")
        gq = (C.c_void_p * 6)()
        for i, (n, dm) in enumerate(zip(QP_NAMES, self._qp_dims())):
            if n in names:
                ptr = buffer(n, ((k,) if (mask >> i) & 1 else (B, k)) + dm)
                gq[i] = ptr.value if ptr is not None else None
        self._check(self._L.calipso_hip_smallnewton_differentiate_adjoint_device(
            self._h, int(k), ptrs.get("cotangent"), ptrs.get("x"), ptrs.get("y"), ptrs.get("z"), p_adj, p_th, gq if names else None, mask, 1, p_st), "smallnewton_differentiate_adjoint_device")
        res = dict(status=bufs["status"])
        if adjoint:
            res["adjoint"] = bufs["adjoint"][:, 0] if squeeze else bufs["adjoint"].permute(0, 2, 1)
        if theta:
            res["theta"] = bufs["theta"][:, 0] if squeeze else bufs["theta"].permute(0, 2, 1)
        for i, (n, dm) in enumerate(zip(QP_NAMES, self._qp_dims())):
            if n in names:
                g = bufs[n]
                if (mask >> i) & 1:
                    res[n] = g[0] if squeeze else g.permute(*range(1, g.dim()), 0)
                else:
                    res[n] = g[:, 0] if squeeze else g.permute(0, *range(2, g.dim()), 1)
        return res


class Comm(_Handle):
    """RCCL communicator of the batched path (include/calipso_hip.h, "multi-GPU exchange"): one process per GPU; the only
    collectives are the post-round all-gather of per-problem status rows and the all-reduce of counters."""
    _handle, _last_error, _destroy = "_c", "calipso_hip_comm_last_error", "calipso_hip_comm_destroy"

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        rc = lib().calipso_hip_comm_unique_id(buf)
        if rc != 0:
            raise CalipsoHipError("comm_unique_id failed (%d): %s" % (rc, lib().calipso_hip_comm_last_error(None).decode()))
        return bytes(buf)

    def __init__(self, rank, nranks, unique_id, device=0):
        self._L = lib()
        self.rank, self.nranks = int(rank), int(nranks)
        buf = (C.c_uint8 * 128)(*unique_id)
        h = C.c_void_p()
        rc = self._L.calipso_hip_comm_init(self.rank, self.nranks, buf, device, C.byref(h))
        if rc != 0:
            raise CalipsoHipError("comm_init failed (%d): %s" % (rc, self._L.calipso_hip_comm_last_error(h if h.value else None).decode()))
        self._c = h

    def size(self):
        """(ranks, own rank) as the communicator itself reports them (ncclCommCount / ncclCommUserRank)"""
        out = np.zeros(2, dtype=np.int32)
        self._check(self._L.calipso_hip_comm_size(self._c, out.ctypes.data_as(C.POINTER(C.c_int32))), "comm_size")
        return int(out[0]), int(out[1])

    def gather_status(self, rows, capacity):
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 4)
        out = np.zeros((int(capacity), 4), dtype=np.int32)
        counts = np.zeros(self.nranks, dtype=np.int64)
        p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        n = self._check(self._L.calipso_hip_comm_gather_status(self._c, p32(rows), rows.shape[0], p32(out), out.shape[0], _pi(counts)), "comm_gather_status")
        return out[:n], counts

    def allreduce_sum(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        self._check(self._L.calipso_hip_comm_allreduce_sum(self._c, _pd(v), v.size), "comm_allreduce_sum")
        return v

def mfma_f64_peak(device=0):
    """measured fp64 matrix-core ceiling of the device in TFLOP/s (calipso_hip_mfma_f64_peak)"""
    t = C.c_double(0.0)
    rc = lib().calipso_hip_mfma_f64_peak(device, C.byref(t))
    if rc != 0:
        raise CalipsoHipError("mfma_f64_peak failed (%d)" % rc)
    return float(t.value)


def initialize_b(solver, guess):
    """initialize!(solver, guess)  src/solver/initialize.jl:9-13"""
    g = np.ascontiguousarray(guess, dtype=np.float64)
    solver._check(solver._L.calipso_hip_initialize(solver._h, _pd(g)), "initialize!")


def solve_b(solver):
    """solve!(solver)::Bool  src/solver/solve.jl:8-377 (raises on the reference's error() cases)"""
    attached = getattr(solver, "_qp_attached", False)
    rc = solver._L.calipso_hip_solve(solver._h, solver._cb, None)
    solver._check(rc, "solve!")
    return rc == 1
