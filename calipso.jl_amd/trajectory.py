"""From per-stage functions to a device evaluator of a Solver handle: the step the reference's trajectory layer takes for its users,
Solver(objective, dynamics, num_states, num_actions; equality, nonnegative, second_order, parameters) (src/trajectory_optimization/solver.jl:1-86), for the general
(dense) path and for structured handles:

    TP = codegen.TrajectoryProblem(objective, dynamics, num_states, num_actions, equality=..., nonnegative=..., second_order=..., num_parameters=..., name="pendulum")
    s = TP.solver(parameters=theta)          # compiles (cached), makes the handle — structured when TP.structure() says so — and sets the generated evaluator
    TP.initialize_states(s, TP.linear_interpolation(x1, xT, T)); solve_b(s)

Every stage function is applied to sympy symbols once per TEMPLATE: stages whose functions have the same expressions and dimensions share one (what generate_methods
does with `unique`, solver.jl:129-176), so a horizon of 2048 stages with one dynamics function costs one derivation.  Per template: the value, the non-zeros of the
Jacobian with respect to the local [x; u; y], of the Hessian of lambda'c (or of the cost) and of their theta_t-derivatives.

How the generated library is shaped (template_source() = the per-template device functions; source() = the whole .hip: these, the problem's shape, then
include/calipso_trajectory.hpp — the kernels and the host code, the same for every problem — and CALIPSO_TRAJECTORY_EVALUATOR, which emits the entries; the blob's
checks and every address are plain C++ in include/calipso_trajectory_tables.hpp):
  * one evaluation kernel: a lane per stage instance of a template, 64-thread workgroups, different templates in different workgroup ranges of the same launch (every
    branch on the template is workgroup-uniform).  Index and address tables are stage-minor ([entry][stage]): the lanes of a wavefront read consecutive words;
  * an output with ONE writer (the values, the objective gradient, the Jacobians' non-zeros) is stored where the ADDRESS TABLE says: entry -> offset in the destination,
    built once per handle from the dense layout, from the host copy of the block descriptors or — a sparse handle — from the stored patterns of its three non-zero
    arrays, uploaded on the first call from pinned memory;
  * an output that sums contributions of several stages (the objective, (g'y)x where stages t and t + 1 meet, (h'z)x, the Lagrangian Hessian, the Lagrangian's
    theta-gradient) gets per-stage PARTIALS and one finishing pass that adds them in a fixed order: no atomics, the same bits every run.  Quirk B-11 of the reference
    (tests/problems.py: TrajectoryProblem — where two consecutive dynamics stages both emit a (x_t+1, x_t+1) entry of (g'y)xx the later stage's value alone survives) is
    resolved HERE, by leaving the earlier stage's partial out of the finishing pass's list (hessian="reference", the default; "exact" sums them);
  * asked for a Jacobian or the Hessian the evaluator first zero-fills it (one launch over the packed storage or the dense arrays), then scatters.
One call enqueues at most four operations (the table upload of the first call, the fill, the evaluation kernel, the finishing pass); <name>_debug_last_enqueued counts.
The text does not depend on the horizon: the tables come from Python through <name>_user_create.  evaluate() is the numpy twin through the same tables."""
import ctypes
import inspect

import numpy as np

from . import Solver, SparseKKT
from . import codegen as _cg

KINDS = ("cost", "dynamics", "equality", "nonnegative", "second_order")
# evaluate! flags (include/calipso_hip.h)
F_OBJ, F_OBJ_GRAD, F_OBJ_HESS, F_EQ, F_EQ_JAC, F_EQ_DGRAD, F_EQ_DHESS, F_CONE, F_CONE_JAC, F_CONE_DGRAD, F_CONE_DHESS = [1 << k for k in range(11)]
F_OBJ_PAR, F_EQ_JAC_PAR, F_EQ_DPAR, F_CONE_JAC_PAR, F_CONE_DPAR = [1 << k for k in range(11, 16)]
# destinations.  0 .. 6 have one writer per address, 7 .. 11 are summed by the finishing pass
D_FX, D_G, D_H, D_GX, D_HX, D_GP, D_HP, D_F, D_GYX, D_HZX, D_LXX, D_LGP = range(12)
# per kind class (0 objective, 1 equality, 2 cone): value, Jacobian, dual gradient, dual Hessian, Jacobian wrt theta, dual gradient wrt theta
_BITS = ((F_OBJ, 0, F_OBJ_GRAD, F_OBJ_HESS, 0, F_OBJ_PAR), (F_EQ, F_EQ_JAC, F_EQ_DGRAD, F_EQ_DHESS, F_EQ_JAC_PAR, F_EQ_DPAR),
         (F_CONE, F_CONE_JAC, F_CONE_DGRAD, F_CONE_DHESS, F_CONE_JAC_PAR, F_CONE_DPAR))
_CLASS = {"cost": 0, "dynamics": 1, "equality": 1, "nonnegative": 2, "second_order": 2}
MAGIC = 0x43545250


class Indices:
    """the index sets of the reference's trajectory layer (indices.jl:41-180), 0-based: states[t], actions[t] into the variables; dynamics[t], equality[t] into the
    equality rows; nonnegative[t], second_order[t][k] into the cone rows; parameters[t] into theta"""


class _Template:
    def __init__(self, kind, ns, na, ny, nth, exprs):
        self.kind, self.ns, self.na, self.ny, self.nth, self.exprs = kind, ns, na, ny, nth, exprs
        self.cls = _CLASS[kind]
        self.nv, self.m = ns + na + ny, (0 if kind == "cost" else len(exprs))
        self.stages = []          # (stage, first row) of every instance
        self.host = None


class TrajectoryProblem:
    """TrajectoryProblem(objective, dynamics, num_states, num_actions, equality=None, nonnegative=None, second_order=None, num_parameters=None,
    hessian="reference" | "exact", name="trajectory")

    Lists of per-stage functions as in the reference: cost (x, u[, theta_t]) -> scalar, dynamics d(y, x, u[, theta_t]) -> num_states[t + 1] expressions, constraints
    (x, u[, theta_t]) -> sequences; second_order[t] is a list of functions, one cone each; None entries and None lists are empty_constraint; the last stage has no
    action (u is empty); a function takes theta_t iff its signature has the extra argument.  Variables [x_1; u_1; ...; x_T], equality rows [dynamics 1..T-1; stage
    equalities 1..T], cone rows: the nonnegative rows of all stages, then the second-order cones stage by stage (methods.jl:46-50); theta = vcat(theta_t).

    .nx .np .ne .nc .T .indices .nonnegative_indices .second_order_indices (1-based, as Solver takes them); structure(); evaluate() (the host twin, the `methods`
    contract of Solver and of the oracle); template_source(), source(), stats(), compile(), solver(); sparse_patterns(), sparse_solver() (a SparseKKT whose
    evaluations run in the generated library: the route for implicit dynamics and long horizons); initialize_states, initialize_actions, get_trajectory,
    linear_interpolation."""

    def __init__(self, objective, dynamics, num_states, num_actions, equality=None, nonnegative=None, second_order=None, num_parameters=None, hessian="reference",
                 name="trajectory", **unsupported):
        import sympy as sp
        self._sp = sp
        if "equality_general" in unsupported:
            raise ValueError("equality_general is not supported by TrajectoryProblem: write the general equality as stage equalities, or use codegen.Problem")
        if unsupported:
            raise TypeError("TrajectoryProblem: unexpected keyword %s" % ", ".join(sorted(unsupported)))
        _cg.check_name(name)
        if hessian not in ("reference", "exact"):
            raise ValueError('hessian must be "reference" or "exact", got %r' % (hessian,))
        self.name, self.hessian = name, hessian
        num_states, num_actions = [int(n) for n in num_states], [int(n) for n in num_actions]
        T = len(num_states)
        if T < 2:
            raise ValueError("a trajectory has at least two stages, got num_states of length %d" % T)
        lists = dict(objective=objective, dynamics=dynamics, equality=equality, nonnegative=nonnegative, second_order=second_order, num_parameters=num_parameters)
        want = dict(objective=T, dynamics=T - 1, equality=T, nonnegative=T, second_order=T, num_parameters=T)       # solver.jl:15-21
        if len(num_actions) != T - 1:
            raise ValueError("num_actions has length %d, expected %d (the last stage has no action)" % (len(num_actions), T - 1))
        for key, n in want.items():
            if lists[key] is None:
                if key in ("objective", "dynamics"):
                    raise ValueError("%s is required: a list of length %d" % (key, n))
                lists[key] = [None] * n if key != "num_parameters" else [0] * n
            lists[key] = list(lists[key])
            if len(lists[key]) != n:
                raise ValueError("%s has length %d, expected %d" % (key, len(lists[key]), n))
        nth = [int(n) for n in lists["num_parameters"]]
        self.T, self.num_states, self.num_actions, self.num_parameters = T, num_states, num_actions, nth
        na = num_actions + [0]

        # ---- templates: a function is applied once per (function, dimensions); equal expressions share one template
        self._v = [sp.Symbol("v%04d" % i) for i in range(max(num_states[t] + na[t] + (num_states[t + 1] if t < T - 1 else 0) for t in range(T)))]
        self._p = [sp.Symbol("p%04d" % i) for i in range(max(nth))]
        self.templates, by_call, by_form = [], {}, {}
        self._applications = 0

        def template(kind, fn, t):
            if fn is None:
                return None
            ns, nu, ny = num_states[t], na[t], (num_states[t + 1] if kind == "dynamics" else 0)
            call = (id(fn), kind, ns, nu, ny, nth[t])
            if call not in by_call:
                exprs = self._apply(kind, fn, ns, nu, ny, nth[t], t)
                held = set().union(*[e.free_symbols for e in exprs]) if exprs else set()
                used = max([i + 1 for i, s in enumerate(self._p[:nth[t]]) if s in held], default=0)      # (a template reads the leading parameters it names)
                form = (kind, ns, nu, ny, used, tuple(exprs))
                if exprs and form not in by_form:
                    by_form[form] = _Template(kind, ns, nu, ny, used, exprs)
                    self.templates.append(by_form[form])
                by_call[call] = (by_form[form] if exprs else None, fn)       # (fn kept alive: its id stays its own)
            return by_call[call][0]

        ind = self.indices = Indices()
        ind.states, ind.actions, ind.parameters = [], [], []
        at = pt = 0
        for t in range(T):
            ind.states.append(np.arange(at, at + num_states[t])); at += num_states[t]
            ind.actions.append(np.arange(at, at + na[t])); at += na[t]
            ind.parameters.append(np.arange(pt, pt + nth[t])); pt += nth[t]
        ind.actions = ind.actions[:T - 1]
        self.nx, self.np = at, pt
        per_stage = dict(cost=[template("cost", lists["objective"][t], t) for t in range(T)],
                         dynamics=[template("dynamics", lists["dynamics"][t], t) for t in range(T - 1)],
                         equality=[template("equality", lists["equality"][t], t) for t in range(T)],
                         nonnegative=[template("nonnegative", lists["nonnegative"][t], t) for t in range(T)])
        socs = []
        for t in range(T):
            fns = lists["second_order"][t]
            fns = [] if fns is None else (list(fns) if isinstance(fns, (list, tuple)) else [fns])
            socs.append([tp for tp in (template("second_order", fn, t) for fn in fns) if tp is not None])
            for tp in socs[-1]:
                if tp.m < 2:
                    raise ValueError("second_order[%d]: a second-order cone has at least two entries, got a function of length %d" % (t, tp.m))
        for t in range(T - 1):
            tp = per_stage["dynamics"][t]
            if tp is None or tp.m != num_states[t + 1]:
                raise ValueError("dynamics[%d] returns %d expressions, num_states[%d] = %d" % (t, 0 if tp is None else tp.m, t + 1, num_states[t + 1]))
        for t in range(T):
            if per_stage["cost"][t] is None:
                raise ValueError("objective[%d] is None: every stage needs a cost (a constant 0 will do)" % t)
        # rows: [dynamics; equalities], [nonnegative of all stages; second-order cones stage by stage]
        row = 0
        ind.dynamics, ind.equality, ind.nonnegative, ind.second_order = [], [], [], []
        for key, into in (("dynamics", ind.dynamics), ("equality", ind.equality)):
            for t, tp in enumerate(per_stage[key]):
                m = tp.m if tp is not None else 0
                into.append(np.arange(row, row + m))
                if tp is not None:
                    tp.stages.append((t, row))
                row += m
        self.ne, row = row, 0
        for t, tp in enumerate(per_stage["nonnegative"]):
            m = tp.m if tp is not None else 0
            ind.nonnegative.append(np.arange(row, row + m))
            if tp is not None:
                tp.stages.append((t, row))
            row += m
        self.n_nonnegative = row
        for t in range(T):
            ind.second_order.append([])
            for tp in socs[t]:
                ind.second_order[-1].append(np.arange(row, row + tp.m))
                tp.stages.append((t, row))
                row += tp.m
        self.nc = row
        for t, tp in enumerate(per_stage["cost"]):
            tp.stages.append((t, 0))
        self.nonnegative_indices = list(range(1, self.n_nonnegative + 1))
        self.second_order_indices = [[int(i) + 1 for i in c] for st in ind.second_order for c in st] or [[]]
        self.N = self.nx + 2 * self.ne + 3 * self.nc
        self._dynamics_of_stage = per_stage["dynamics"]
        for tp in self.templates:
            self._derive(tp)
        self._tables()
        self._text = self._host_ready = None

    # ---- applying and deriving -------------------------------------------------------------------------------------------------------------------
    def _apply(self, kind, fn, ns, nu, ny, nth, t):
        sp = self._sp
        self._applications += 1
        x, u, y, th = self._v[:ns], self._v[ns:ns + nu], self._v[ns + nu:ns + nu + ny], self._p[:nth]
        base = [list(y), list(x), list(u)] if kind == "dynamics" else [list(x), list(u)]
        try:
            arity = len(inspect.signature(fn).parameters)
        except (TypeError, ValueError):
            arity = len(base) + (1 if nth else 0)
        if arity not in (len(base), len(base) + 1):
            raise ValueError("%s[%d] takes %d arguments, expected %s" % (kind, t, arity, "(y, x, u[, theta])" if kind == "dynamics" else "(x, u[, theta])"))
        raw = fn(*(base + ([list(th)] if arity > len(base) else [])))
        what = "%s[%d]" % (kind, t)
        exprs = [_cg.as_scalar(sp, raw, what)] if kind == "cost" else _cg.as_sequence(sp, raw, what)
        _cg.check_symbols(exprs, set(x) | set(u) | set(y) | set(th), "%s may depend on its arguments alone" % what)
        return exprs

    def _derive(self, tp):
        """the non-zeros of a template's derivatives, each only by the symbols an expression holds"""
        sp = self._sp
        v, p = self._v[:tp.nv], self._p[:tp.nth]
        vi, pi = {s: i for i, s in enumerate(v)}, {s: i for i, s in enumerate(p)}
        tp.lam = [sp.Symbol("l%04d" % r) for r in range(tp.m)]

        def grad(e, index):
            out = {}
            for s in sorted(e.free_symbols, key=lambda s: s.name):
                if s in index:
                    d = sp.diff(e, s)
                    if d != 0:
                        out[index[s]] = d
            return out

        rows = [grad(e, vi) for e in tp.exprs]
        if tp.kind == "cost":
            tp.jac, g = [], rows[0]
            tp.grad = [(j, g.get(j, sp.Integer(0))) for j in range(tp.nv)]           # the objective gradient has one writer: every entry, zeros included
        else:
            tp.jac = [(r, j, d) for r in range(tp.m) for j, d in sorted(rows[r].items())]
            g = {}
            for r in range(tp.m):
                for j, d in rows[r].items():
                    g[j] = g.get(j, sp.Integer(0)) + tp.lam[r] * d
            tp.grad = sorted(g.items())
        hess, gth = {}, []
        for j, e in sorted(g.items()):
            for i, d in grad(e, vi).items():
                if i <= j:
                    hess[(i, j)] = d
                    hess[(j, i)] = d
            gth += [(j, k, d) for k, d in sorted(grad(e, pi).items())]
        tp.hess = [(i, j, hess[(i, j)]) for (j, i) in sorted((j, i) for (i, j) in hess)]      # column-major, like findnz
        tp.gth = gth
        tp.cth = [] if tp.kind == "cost" else [(r, k, d) for r, e in enumerate(tp.exprs) for k, d in sorted(grad(e, pi).items())]
        # partial outputs (summed by the finishing pass) and direct entries (through the address table), in the order the generated code numbers them
        tp.n_value_partials = 1 if tp.kind == "cost" else 0
        tp.n_grad_partials = 0 if tp.kind == "cost" else len(tp.grad)
        tp.nq = tp.n_value_partials + tp.n_grad_partials + len(tp.hess) + len(tp.gth)
        tp.nd = len(tp.jac) + len(tp.cth)

    def _tables(self):
        """per template the stage-minor index tables and the coordinates of its outputs; then the finishing pass's lists"""
        ind, T = self.indices, self.T
        slot0, contributions, emitted = 0, [], {}        # (destination, i, j, order (stage, kind), slot, class)
        for k, tp in enumerate(self.templates):
            n = tp.n = len(tp.stages)
            st = np.array([s for s, _ in tp.stages], dtype=np.int64)
            r0 = np.array([r for _, r in tp.stages], dtype=np.int64)
            var = np.zeros((tp.nv, n), dtype=np.int64)
            for c, (t, _) in enumerate(tp.stages):
                loc = np.concatenate([ind.states[t], ind.actions[t] if t < T - 1 else np.zeros(0, dtype=np.int64)] + ([ind.states[t + 1]] if tp.kind == "dynamics" else []))
                var[:, c] = loc
            tp.vi = var
            tp.ri = r0[None, :] + np.arange(tp.m, dtype=np.int64)[:, None]
            p0 = np.array([ind.parameters[t][0] if len(ind.parameters[t]) else 0 for t, _ in tp.stages], dtype=np.int64)
            tp.pi = p0[None, :] + np.arange(tp.nth, dtype=np.int64)[:, None]
            cls = tp.cls
            # direct entries: the Jacobian's non-zeros, then those of dc/dtheta
            tp.d_field = np.array([D_GX if cls == 1 else D_HX] * len(tp.jac) + [D_GP if cls == 1 else D_HP] * len(tp.cth), dtype=np.int64)
            tp.d_i = np.zeros((tp.nd, n), dtype=np.int64); tp.d_j = np.zeros((tp.nd, n), dtype=np.int64)
            for e, (r, j, _) in enumerate(tp.jac):
                tp.d_i[e], tp.d_j[e] = tp.ri[r], var[j]
            for e, (r, kk, _) in enumerate(tp.cth):
                tp.d_i[len(tp.jac) + e], tp.d_j[len(tp.jac) + e] = tp.ri[r], tp.pi[kk]
            # partials
            tp.slot0 = slot0
            tp.p_field = np.zeros(tp.nq, dtype=np.int64); tp.p_i = np.zeros((tp.nq, n), dtype=np.int64); tp.p_j = np.zeros((tp.nq, n), dtype=np.int64)
            tp.p_keep = np.ones((tp.nq, n), dtype=bool)
            q = 0
            if tp.kind == "cost":
                tp.p_field[q] = D_F; q += 1
            else:
                for j, _ in tp.grad:
                    tp.p_field[q], tp.p_i[q] = (D_GYX if cls == 1 else D_HZX), var[j]; q += 1
            for i, j, _ in tp.hess:
                tp.p_field[q], tp.p_i[q], tp.p_j[q] = D_LXX, var[i], var[j]
                if self.hessian == "reference" and tp.kind == "dynamics" and i >= tp.ns + tp.na and j >= tp.ns + tp.na:
                    a, b = i - tp.ns - tp.na, j - tp.ns - tp.na
                    for c, (t, _) in enumerate(tp.stages):          # quirk B-11: the later dynamics stage writes the same entry last
                        later = self._dynamics_of_stage[t + 1] if t + 1 < T - 1 else None
                        if later is not None and (a, b) in emitted.setdefault(id(later), {(ii, jj) for ii, jj, _ in later.hess}):
                            tp.p_keep[q, c] = False
                q += 1
            for j, kk, _ in tp.gth:
                tp.p_field[q], tp.p_i[q], tp.p_j[q] = D_LGP, var[j], tp.pi[kk]; q += 1
            order = st * len(KINDS) + KINDS.index(tp.kind)
            for q in range(tp.nq):
                keep = tp.p_keep[q]
                slots = slot0 + q * n + np.arange(n)
                contributions.append(np.stack([np.full(n, tp.p_field[q]), tp.p_i[q], tp.p_j[q], order, slots, np.full(n, cls)], axis=1)[keep])
            slot0 += tp.nq * n
        self.n_partials = slot0
        if slot0 >= 1 << 29:
            raise ValueError("the problem has %d partial outputs; the finishing pass addresses fewer than 2^29" % slot0)
        C = np.concatenate(contributions) if contributions else np.zeros((0, 6), dtype=np.int64)
        obj = C[C[:, 0] == D_F]
        self.obj_slots = obj[np.argsort(obj[:, 3], kind="stable"), 4]
        # the summed outputs: every variable's (g'y)x and (h'z)x, the non-zeros of the Hessian and of the Lagrangian's theta-gradient
        C = C[C[:, 0] != D_F]
        every = np.concatenate([np.stack([np.full(self.nx, f), np.arange(self.nx), np.zeros(self.nx, dtype=np.int64), np.full(self.nx, -1), np.full(self.nx, -1),
                                          np.zeros(self.nx, dtype=np.int64)], axis=1) for f in (D_GYX, D_HZX)])
        C = np.concatenate([every, C])
        C = C[np.lexsort((C[:, 3], C[:, 1], C[:, 2], C[:, 0]))]           # by destination, column, row, then the fixed order of the sum
        key = C[:, :3]
        first = np.ones(len(C), dtype=bool)
        first[1:] = (key[1:] != key[:-1]).any(axis=1)
        gid = np.cumsum(first) - 1
        G = int(gid[-1]) + 1 if len(C) else 0
        self.g_field, self.g_i, self.g_j = C[first, 0], C[first, 1], C[first, 2]
        real = C[:, 4] >= 0
        pos = np.arange(len(C)) - np.flatnonzero(first)[gid] - 1           # (the placeholder of a variable sorts first: order -1)
        is_vec = np.isin(C[:, 0], (D_GYX, D_HZX))
        pos = np.where(is_vec, pos, pos + 1)
        W = int(pos[real].max()) + 1 if real.any() else 1
        self.g_slots = np.full((W, G), -1, dtype=np.int64)
        self.g_slots[pos[real], gid[real]] = C[real, 4] | (C[real, 5] << 29)
        self.G, self.W = G, W

    # ---- structure ---------------------------------------------------------------------------------------------------------------------------------
    def _patterns(self):
        Zp = np.zeros((self.ne + self.nc, self.nx), dtype=bool)
        Hp = np.zeros((self.nx, self.nx), dtype=bool)
        for tp in self.templates:
            for e in range(len(tp.jac)):
                Zp[tp.d_i[e] + (self.ne if tp.cls == 2 else 0), tp.d_j[e]] = True
            q0 = tp.n_value_partials + tp.n_grad_partials
            for q in range(q0, q0 + len(tp.hess)):
                Hp[tp.p_i[q], tp.p_j[q]] = True
        return Zp, Hp | Hp.T

    def sparse_patterns(self):
        """the stored patterns a sparse handle takes, CSC as (colptr, rowval) pairs, 0-based, rows ascending: Lxx (both triangles), gx, hx — the non-zeros of
        _patterns(), from the index tables by np.unique on (column, row) pairs: nothing of size nx x nx or (ne + nc) x nx is allocated, whatever the horizon"""
        rows = {D_LXX: self.nx, D_GX: self.ne, D_HX: self.nc}
        keys = {D_LXX: [], D_GX: [], D_HX: []}          # column * rows + row: sorting the keys sorts by column, then row
        for tp in self.templates:
            if len(tp.jac):
                f = D_GX if tp.cls == 1 else D_HX
                keys[f].append((tp.d_j[:len(tp.jac)] * rows[f] + tp.d_i[:len(tp.jac)]).reshape(-1))
            q0 = tp.n_value_partials + tp.n_grad_partials
            if len(tp.hess):
                i, j = tp.p_i[q0:q0 + len(tp.hess)].reshape(-1), tp.p_j[q0:q0 + len(tp.hess)].reshape(-1)
                keys[D_LXX] += [j * self.nx + i, i * self.nx + j]
        out = []
        for f in (D_LXX, D_GX, D_HX):
            key = np.unique(np.concatenate(keys[f])) if keys[f] else np.zeros(0, dtype=np.int64)
            col, row = (key // rows[f], key % rows[f]) if rows[f] else (key, key)
            colptr = np.zeros(self.nx + 1, dtype=np.int64)
            np.cumsum(np.bincount(col, minlength=self.nx), out=colptr[1:])
            out.append((colptr, np.ascontiguousarray(row, dtype=np.int64)))
        return tuple(out)

    def sparse_parameter_patterns(self):
        """the stored patterns of dR/dtheta's three blocks a sparse handle takes (SparseKKT.set_parameter_patterns), CSC as (colptr, rowval) pairs with np columns, 0-based,
        rows ascending: lagrangian_gradient_parameters (nx rows: the D_LGP partials of every template), equality_jacobian_parameters (ne rows), cone_jacobian_parameters
        (nc rows) — from the index tables by np.unique on (column, row) keys, like sparse_patterns(): nothing of size nx x np, ne x np or nc x np is allocated"""
        rows = {D_LGP: self.nx, D_GP: self.ne, D_HP: self.nc}
        keys = {D_LGP: [], D_GP: [], D_HP: []}
        for tp in self.templates:
            nj = len(tp.jac)
            if len(tp.cth):
                f = D_GP if tp.cls == 1 else D_HP
                keys[f].append((tp.d_j[nj:nj + len(tp.cth)] * rows[f] + tp.d_i[nj:nj + len(tp.cth)]).reshape(-1))
            q0 = tp.nq - len(tp.gth)
            if len(tp.gth):
                keys[D_LGP].append((tp.p_j[q0:] * self.nx + tp.p_i[q0:]).reshape(-1))
        out = []
        for f in (D_LGP, D_GP, D_HP):
            key = np.unique(np.concatenate(keys[f])) if keys[f] else np.zeros(0, dtype=np.int64)
            col, row = (key // rows[f], key % rows[f]) if rows[f] else (key, key)
            colptr = np.zeros(self.np + 1, dtype=np.int64)
            np.cumsum(np.bincount(col, minlength=self.np), out=colptr[1:])
            out.append((colptr, np.ascontiguousarray(row, dtype=np.int64)))
        return tuple(out)

    def structure(self):
        """dict(row_first, row_last, hessian_block_start) (1-based) for Solver(structure=...) when the Lagrangian Hessian falls into at least two diagonal blocks (it does
        when no stage function couples x_t with x_t+1 in its second derivatives: explicit dynamics), else None (implicit dynamics, the pendulum: a dense handle).
        The row ranges are those of the pattern (tests/problems.py: structure_from_pattern) while a structured handle takes that many; on long horizons the rows of
        one stage function share one range"""
        Zp, Hp = self._patterns()
        first = np.ones(Zp.shape[0], dtype=np.int64); last = np.zeros(Zp.shape[0], dtype=np.int64)
        for k in range(Zp.shape[0]):
            nz = np.nonzero(Zp[k])[0]
            if nz.size:
                first[k], last[k] = nz[0] + 1, nz[-1] + 1
        runs = lambda: sum(1 for k in range(len(first)) if k in (0, self.ne) or first[k] != first[k - 1] or last[k] != last[k - 1])
        if runs() > max(64, len(first) // 2):
            # more runs of rows with one column range than a structured handle takes (csrc/blocks.hip: blocks_plan): the rows of one stage function share the
            # union of their ranges — one block per stage instance, the zeros inside it are written as zeros
            for tp in self.templates:
                if tp.m:
                    rows = tp.ri + (self.ne if tp.cls == 2 else 0)
                    empty = first[rows] > last[rows]                # (a row without a non-zero takes no part in the union)
                    lo, hi = np.where(empty, self.nx + 1, first[rows]).min(axis=0), np.where(empty, 0, last[rows]).max(axis=0)
                    lo, hi = np.where(lo > hi, 1, lo), np.where(lo > hi, 0, hi)
                    first[rows], last[rows] = lo[None, :], hi[None, :]
        starts, reach = [1], -1
        for j in range(self.nx):
            if j > starts[-1] - 1 and reach < j:
                starts.append(j + 1)
            nz = np.nonzero(Hp[:, j])[0]
            reach = max(reach, j, int(nz.max()) if nz.size else j)
        stage = np.zeros(self.nx, dtype=np.int64)
        for t, idx in enumerate(self.indices.states):
            stage[idx] = t
        for t, idx in enumerate(self.indices.actions):
            stage[idx] = t
        i, j = np.nonzero(Hp)
        if len(starts) < 2 or (stage[i] != stage[j]).any():
            return None
        return dict(row_first=first, row_last=last, hessian_block_start=np.array(starts, dtype=np.int64))

    # ---- the host twin ----------------------------------------------------------------------------------------------------------------------------
    def _sections(self, tp):
        """[(flag bit, [(target, expression)])] of a template: what the generated function computes under each flag.  Targets: ("value", r), ("fx", j), ("direct", e),
        ("part", q)"""
        bits = _BITS[tp.cls]
        out = []
        if tp.kind == "cost":
            out.append((bits[0], [(("part", 0), tp.exprs[0])]))
            out.append((bits[2], [(("fx", j), e) for j, e in tp.grad]))
            q = 1
        else:
            out.append((bits[0], [(("value", r), e) for r, e in enumerate(tp.exprs)]))
            out.append((bits[1], [(("direct", e), d) for e, (_, _, d) in enumerate(tp.jac)]))
            out.append((bits[2], [(("part", q), e) for q, (_, e) in enumerate(tp.grad)]))
            q = len(tp.grad)
        out.append((bits[3], [(("part", q + e), d) for e, (_, _, d) in enumerate(tp.hess)]))
        q += len(tp.hess)
        out.append((bits[4], [(("direct", len(tp.jac) + e), d) for e, (_, _, d) in enumerate(tp.cth)]))
        out.append((bits[5], [(("part", q + e), d) for e, (_, _, d) in enumerate(tp.gth)]))
        return [(b, items) for b, items in out if b and items]

    def _host(self, tp):
        if tp.host is None:
            sp = self._sp
            args = self._v[:tp.nv] + tp.lam + self._p[:tp.nth]
            tp.host = [(bit, [t for t, _ in items], sp.lambdify(args, [e for _, e in items], "numpy", cse=True)) for bit, items in self._sections(tp)]
        return tp.host

    def evaluate(self, flags, x, y, z, theta, out):
        """the `methods` contract of Solver and of oracle.OracleSolver.solve in numpy: per template one vectorised call over its stages, scattered through the tables
        the device code uses"""
        x, y, z, theta = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, y, z, theta))
        nx, ne, nc, npar = self.nx, self.ne, self.nc, self.np
        want = lambda bit, size=1: (flags & bit) and size
        dense = {}

        def field(name, size, bit):
            if want(bit, size):
                dense[name] = np.zeros(size)
            return dense.get(name)

        names = {0: ("objective_jacobian_variables_variables", "objective_jacobian_variables_parameters"),
                 1: ("equality_dual_jacobian_variables_variables", "equality_dual_jacobian_variables_parameters"),
                 2: ("cone_dual_jacobian_variables_variables", "cone_dual_jacobian_variables_parameters")}
        f = field("objective", 1, F_OBJ); fx = field("objective_gradient_variables", nx, F_OBJ_GRAD)
        vals = {1: field("equality_constraint", ne, F_EQ), 2: field("cone_constraint", nc, F_CONE)}
        jac = {1: field("equality_jacobian_variables", ne * nx, F_EQ_JAC), 2: field("cone_jacobian_variables", nc * nx, F_CONE_JAC)}
        dgr = {1: field("equality_dual_jacobian_variables", nx, F_EQ_DGRAD), 2: field("cone_dual_jacobian_variables", nx, F_CONE_DGRAD)}
        hes = {c: field(names[c][0], nx * nx, _BITS[c][3]) for c in range(3)}
        jth = {1: field("equality_jacobian_parameters", ne * npar, F_EQ_JAC_PAR), 2: field("cone_jacobian_parameters", nc * npar, F_CONE_JAC_PAR)}
        gth = {c: field(names[c][1], nx * npar, _BITS[c][5]) for c in range(3)}
        rows = {1: ne, 2: nc}
        for tp in self.templates:
            lam = y if tp.cls == 1 else z
            a = [x[tp.vi[j]] for j in range(tp.nv)] + [lam[tp.ri[r]] for r in range(tp.m)] + [theta[tp.pi[k]] for k in range(tp.nth)]
            for bit, targets, fn in self._host(tp):
                if not flags & bit:
                    continue
                got = fn(*a)
                for (what, e), val in zip(targets, got):
                    val = np.broadcast_to(np.asarray(val, dtype=np.float64), (tp.n,))
                    if what == "value":
                        vals[tp.cls][tp.ri[e]] = val
                    elif what == "fx":
                        fx[tp.vi[e]] = val
                    elif what == "direct":
                        into = jac if tp.d_field[e] in (D_GX, D_HX) else jth
                        into[tp.cls][tp.d_i[e] + tp.d_j[e] * rows[tp.cls]] = val
                    else:
                        dest, keep = tp.p_field[e], tp.p_keep[e]
                        if dest == D_F:
                            f[0] += val.sum()
                        elif dest in (D_GYX, D_HZX):
                            np.add.at(dgr[tp.cls], tp.p_i[e], val)
                        else:
                            np.add.at((hes if dest == D_LXX else gth)[tp.cls], (tp.p_i[e] + tp.p_j[e] * nx)[keep], val[keep])
        for name, arr in dense.items():
            buf = out(name)
            if buf.size:
                buf[:] = arr

    # ---- conveniences of solver.jl:88-127, utilities.jl:10-19 -----------------------------------------------------------------------------------
    @staticmethod
    def linear_interpolation(x0, xf, T):
        x0, xf = np.asarray(x0, dtype=np.float64), np.asarray(xf, dtype=np.float64)
        return [x0 + (xf - x0) * (t / (T - 1)) for t in range(T)]

    def _guess(self, target):
        return target.setdefault("_trajectory_guess", np.zeros(self.nx)) if isinstance(target, dict) else target

    def initialize_states(self, guess, states):
        """write a state trajectory into a vector of the variables (the guess handed to initialize_b); returns it"""
        for idx, v in zip(self.indices.states, states):
            guess[idx] = v
        return guess

    def initialize_actions(self, guess, actions):
        for idx, v in zip(self.indices.actions, actions):
            guess[idx] = v
        return guess

    def get_trajectory(self, solver_or_variables):
        s = solver_or_variables
        w = s.solution.variables if hasattr(s, "solution") else s.get("solution")[:self.nx] if isinstance(s, SparseKKT) else np.asarray(s)
        return [w[idx].copy() for idx in self.indices.states], [w[idx].copy() for idx in self.indices.actions]

    # ---- printing ----------------------------------------------------------------------------------------------------------------------------------
    def _function(self, k, tp):
        names = {s: "v%d" % i for i, s in enumerate(self._v[:tp.nv])}
        names.update({s: "l%d" % i for i, s in enumerate(tp.lam)})
        names.update({s: "p%d" % i for i, s in enumerate(self._p[:tp.nth])})
        sections = self._sections(tp)
        mask = 0
        for bit, _ in sections:
            mask |= bit
        cls = tp.cls
        lines = ["// template %d: %s, %d instance rows, local [x; u%s] = %d + %d%s, %d parameters" % (k, tp.kind, tp.m, "; y" if tp.ny else "", tp.ns, tp.na,
                                                                                              " + %d" % tp.ny if tp.ny else "", tp.nth),
                 "__device__ inline void %s_t%d(unsigned flags, int s, int n, const double* x, const double* lam, const double* th, const int* vi, const int* ri, const int* pi,"
                 % (self.name, k),
                 "        const int* ad, double* const* base, double* part) {",
                 "    if (s >= n || !(flags & 0x%xu)) return;" % mask,
                 "    (void)x; (void)lam; (void)th; (void)vi; (void)ri; (void)pi; (void)ad; (void)base; (void)part;"]
        used = set()
        for _, items in sections:
            for _, e in items:
                used |= e.free_symbols
        for i, s in enumerate(self._v[:tp.nv]):
            if s in used:
                lines.append("    const double v%d = x[vi[%d * n + s]];" % (i, i))
        for i, s in enumerate(tp.lam):
            if s in used:
                lines.append("    const double l%d = lam[ri[%d * n + s]];" % (i, i))
        for i, s in enumerate(self._p[:tp.nth]):
            if s in used:
                lines.append("    const double p%d = th[pi[%d * n + s]];" % (i, i))
        ops = 0
        for bit, items in sections:
            declarations, texts, n = _cg.body(self._sp, [e for _, e in items], names, "        ", "c")
            lines.append("    if (flags & 0x%xu) {" % bit)
            lines += declarations
            for (what, e), text in zip([t for t, _ in items], texts):
                if what == "value":
                    lines.append("        base[%d][ri[%d * n + s]] = %s;" % (D_G if cls == 1 else D_H, e, text))
                elif what == "fx":
                    lines.append("        base[%d][vi[%d * n + s]] = %s;" % (D_FX, e, text))
                elif what == "direct":
                    lines.append("        base[%d][ad[%d * n + s]] = %s;" % (int(tp.d_field[e]), e, text))
                else:
                    lines.append("        part[%d * n + s] = %s;" % (e, text))
            lines.append("    }")
            ops += n
        lines.append("}")
        return lines, ops

    def _generate(self):
        if self._text is not None:
            return
        if len(self.templates) > 96:
            raise ValueError("%d templates: the evaluation kernel's argument block holds at most 96" % len(self.templates))
        out = ["// %s: %d templates — generated by calipso.jl_amd/trajectory.py; do not edit" % (self.name, len(self.templates))]
        ops = []
        for k, tp in enumerate(self.templates):
            lines, n = self._function(k, tp)
            out += lines
            ops.append(n)
        out += ["__device__ inline void %s_template(int k, unsigned flags, int s, int n, const double* x, const double* y, const double* z, const double* th, const int* vi,"
                % self.name,
                "        const int* ri, const int* pi, const int* ad, double* const* base, double* part) {",
                "    switch (k) {"]
        for k, tp in enumerate(self.templates):
            out.append("    case %d: %s_t%d(flags, s, n, x, %s, th, vi, ri, pi, ad, base, part); break;" % (k, self.name, k, ("x", "y", "z")[tp.cls]))
        out += ["    default: break;", "    }", "}", ""]
        self._text, self._ops = "\n".join(out), ops

    def template_source(self):
        """the per-template device functions and their dispatch <name>_template alone: they need <math.h> and a __device__ that the including file may define away"""
        self._generate()
        return self._text

    def source(self):
        """the whole translation unit: the template functions, the problem type (the shape of every template and the dispatch), include/calipso_trajectory.hpp — the
        kernels and the host code, the same for every problem — and the macro that emits the entries"""
        name, arrays = self.name, (("KIND", [KINDS.index(tp.kind) for tp in self.templates]),) + tuple(
            (key.upper(), [getattr(tp, key) for tp in self.templates]) for key in ("nv", "m", "nth", "nd", "nq"))
        lines = ["// %s_device_eval, %s_block_eval, %s_user_create, %s_user_destroy, %s_debug_last_enqueued: device evaluators of a trajectory problem for "
                 "libcalipso_hip.so — generated by calipso.jl_amd/trajectory.py; do not edit" % ((name,) * 5),
                 "namespace {", "", self.template_source(),
                 "struct %s_problem {" % name,
                 "    static constexpr int NT = %d;" % len(self.templates)]
        lines += ["    static constexpr int %s[NT] = {%s};" % (key, ", ".join(str(v) for v in vals)) for key, vals in arrays]
        lines += ["    __device__ static void call(int k, unsigned flags, int s, int n, const double* x, const double* y, const double* z, const double* th, const int* vi,",
                  "            const int* ri, const int* pi, const int* ad, double* const* base, double* part) {",
                  "        %s_template(k, flags, s, n, x, y, z, th, vi, ri, pi, ad, base, part);" % name,
                  "    }", "};", "", "}  // namespace", "",
                  '#include "calipso_trajectory.hpp"', "",
                  "CALIPSO_TRAJECTORY_EVALUATOR(%s_problem, %s)" % (name, name), ""]
        return "\n".join(lines)

    def stats(self):
        """dict(stages, templates: per kind the number of templates, instances: per template (kind, stages), applications: how often a stage function was applied to
        symbols, operations: per template sympy's count after CSE, partials, summed_outputs, sum_width)"""
        self._generate()
        return dict(stages=self.T, templates={kind: sum(1 for tp in self.templates if tp.kind == kind) for kind in KINDS},
                    instances=[(tp.kind, tp.n) for tp in self.templates], applications=self._applications, operations=list(self._ops),
                    partials=int(self.n_partials), summed_outputs=int(self.G), sum_width=int(self.W))

    # ---- compiling and the handle -----------------------------------------------------------------------------------------------------------------
    def _build(self, directory, arch, **build):
        return _cg.compile_cached(self.name, self.source(), [], ["calipso_hip.h", "calipso_trajectory.hpp", "calipso_trajectory_tables.hpp"], "", directory=directory,
                                  arch=arch, **build)

    def library_path(self, directory=None, arch="gfx950"):
        return self._build(directory, arch)[2]

    def compile(self, directory=None, hipcc=None, arch="gfx950"):
        """Write source() and build it into a shared library; returns a codegen.Compiled (.path, .cdll; .symbol = <name>_device_eval).  Cached like Problem.compile: the
        file name carries a hash of the text, of include/calipso_hip.h and the two calipso_trajectory headers, the arch and the flags.  Plain kernels: a build takes
        seconds."""
        return self._build(directory, arch, hipcc=hipcc, symbol=self.name + "_device_eval")

    def tables(self):
        """the int32 blob <name>_user_create takes: header, per template its shape, then its index tables and output coordinates, then the finishing pass's lists"""
        parts = [np.array([MAGIC, len(self.templates), self.G, self.W, len(self.obj_slots), self.n_partials, self.nx, self.ne, self.nc, self.np], dtype=np.int64)]
        for tp in self.templates:
            parts.append(np.array([KINDS.index(tp.kind), tp.n, tp.nv, tp.m, tp.nth, tp.nd, tp.nq, 0], dtype=np.int64))
        for tp in self.templates:
            parts += [tp.vi.reshape(-1), tp.ri.reshape(-1), tp.pi.reshape(-1), tp.d_field, tp.d_i.reshape(-1), tp.d_j.reshape(-1)]
        parts += [self.g_field, self.g_i, self.g_j, self.g_slots.reshape(-1), self.obj_slots]
        blob = np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1) for p in parts])
        assert blob.min() >= -1 and blob.max() < 1 << 31
        return np.ascontiguousarray(blob, dtype=np.int32)

    def solver(self, parameters=None, options=None, device=0, structured=None, methods=None, **compile_args):
        """an ordinary Solver whose evaluations run in the generated library: the block evaluator on a structured handle (structured=True, or None when structure()
        gives one), the dense-layout evaluator on a dense handle.  `methods` replaces the host twin as the handle's host callback (the device route never calls it).
        The Solver keeps the library and the evaluator's user object alive; close() frees them."""
        st = self.structure() if structured in (None, True) else None
        if structured and st is None:
            raise ValueError("structured=True, but the Lagrangian Hessian of %s couples consecutive stages: structure() is None, the problem takes a dense handle" % self.name)
        built = self.compile(**compile_args)
        L = built.cdll
        create, destroy = getattr(L, self.name + "_user_create"), getattr(L, self.name + "_user_destroy")
        create.restype, create.argtypes, destroy.argtypes = ctypes.c_void_p, [ctypes.POINTER(ctypes.c_int32), ctypes.c_int64], [ctypes.c_void_p]
        blob = self.tables()
        user = create(blob.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), blob.size)
        if not user:
            raise RuntimeError("%s_user_create refused the tables" % self.name)
        try:
            s = TrajectorySolver(self if methods is None else methods, self.nx, self.np, self.ne, self.nc, parameters=parameters, nonnegative_indices=self.nonnegative_indices,
                                  second_order_indices=self.second_order_indices, options=options, device=device, structure=st)
        except Exception:
            destroy(user)
            raise
        s._trajectory, s._library, s._user, s._user_destroy = self, L, user, destroy
        entry = ctypes.cast(getattr(L, self.name + ("_block_eval" if st is not None else "_device_eval")), ctypes.c_void_p)
        (s.set_device_block_evaluator if st is not None else s.set_device_evaluator)(entry, user)
        return s

    def sparse_solver(self, parameters=None, options=None, device=0, method="nested_dissection", perm=None, **compile_args):
        """a SparseKKT on sparse_patterns() whose evaluations run in the generated library's <name>_sparse_eval: the route for problems whose Hessian couples
        consecutive stages (implicit dynamics: structure() is None) and for horizons a dense handle cannot hold.  The cone layout and theta (default: zeros) are set;
        every SparseKKT method works on it — initialize(x0), solve(), get("solution"), and get_trajectory(handle) here.  With parameters the patterns of
        sparse_parameter_patterns() are set too, so differentiate() and vjp(v, theta=True) take dR/dtheta from the evaluator.  The handle keeps the library and the
        evaluator's user object alive; close() frees them."""
        import scipy.sparse as sp
        built = self.compile(**compile_args)
        L = built.cdll
        create, destroy = getattr(L, self.name + "_user_create"), getattr(L, self.name + "_user_destroy")
        create.restype, create.argtypes, destroy.argtypes = ctypes.c_void_p, [ctypes.POINTER(ctypes.c_int32), ctypes.c_int64], [ctypes.c_void_p]
        blob = self.tables()
        user = create(blob.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), blob.size)
        if not user:
            raise RuntimeError("%s_user_create refused the tables" % self.name)
        try:
            mats = [sp.csc_matrix((np.ones(len(rowval)), rowval, colptr), shape=(rows, self.nx))
                    for (colptr, rowval), rows in zip(self.sparse_patterns(), (self.nx, self.ne, self.nc))]
            dims = [len(c) for st in self.indices.second_order for c in st]
            s = TrajectorySparseKKT(*mats, n_nonnegative=self.n_nonnegative, second_order_dims=dims, method=method, perm=perm, device=device, options=options)
        except Exception:
            destroy(user)
            raise
        s._trajectory, s._library, s._user, s._user_destroy = self, L, user, destroy
        s.set_evaluator(ctypes.cast(getattr(L, self.name + "_sparse_eval"), ctypes.c_void_p), user, self.np)
        if self.np > 0:                         # differentiate() / vjp(theta=True) take dR/dtheta from the evaluator, on these stored patterns
            s.set_parameter_patterns(*self.sparse_parameter_patterns())
        if parameters is not None:
            s.set_parameters(parameters)
        return s

    def enqueued(self, solver):
        """how many operations (copies, fills, kernels) the last evaluation call of `solver`'s evaluator enqueued"""
        fn = getattr(solver._library, self.name + "_debug_last_enqueued")
        fn.restype, fn.argtypes = ctypes.c_int32, [ctypes.c_void_p]
        return int(fn(solver._user))


class TrajectorySolver(Solver):
    """a Solver that owns the generated library's user object"""

    def close(self):
        h = getattr(self, "_h", None)
        live = h is not None and h.value
        if live:
            try:
                self.synchronize()          # (the user object's buffers outlive the kernels that read them)
            except Exception:
                pass
        Solver.close(self)
        user, self._user = getattr(self, "_user", None), None
        if user:
            self._user_destroy(user)


class TrajectorySparseKKT(SparseKKT):
    """a SparseKKT that owns the generated library's user object"""

    def close(self):
        h = getattr(self, "_h", None)
        user, self._user = getattr(self, "_user", None), None
        if h is not None and h.value and user:
            try:
                self.set_evaluator(None)    # synchronises the handle's stream: the user object's buffers outlive the kernels that read them
            except Exception:
                pass
        SparseKKT.close(self)
        if user:
            self._user_destroy(user)
