"""From per-stage functions to a device evaluator of a Solver handle: the step the reference's trajectory layer takes for its users,
Solver(objective, dynamics, num_states, num_actions; equality, nonnegative, second_order, parameters) (src/trajectory_optimization/solver.jl:1-86), for the general
(dense) path and for structured handles:

    TP = codegen.TrajectoryProblem(objective, dynamics, num_states, num_actions, equality=..., nonnegative=..., second_order=..., num_parameters=..., name="pendulum")
    s = TP.solver(parameters=theta)          # compiles (cached), makes the handle — structured when TP.structure() says so — and sets the generated evaluator
    TP.initialize_states(s, TP.linear_interpolation(x1, xT, T)); solve_b(s)

Every stage function is applied to sympy symbols once per TEMPLATE: stages whose functions have the same expressions and dimensions share one (what generate_methods
does with `unique`, solver.jl:129-176), so a horizon of 2048 stages with one dynamics function costs one derivation.  Per template: the value, the non-zeros of the
Jacobian with respect to the local [x; u; y], of the Hessian of lambda'c (or of the cost) and of their theta_t-derivatives.

How the generated library is shaped (template_source() = the per-template device functions, source() = the whole .hip):
  * one evaluation kernel: a lane per stage instance of a template, 64-thread workgroups, different templates in different workgroup ranges of the same launch (every
    branch on the template is workgroup-uniform).  Index and address tables are stage-minor ([entry][stage]): the lanes of a wavefront read consecutive words;
  * an output with ONE writer (the values, the objective gradient, the Jacobians' non-zeros) is stored where the ADDRESS TABLE says: entry -> offset in the destination,
    built once per handle from the dense layout or from the host copy of the block descriptors, uploaded on the first call from pinned memory;
  * an output that sums contributions of several stages (the objective, (g'y)x where stages t and t + 1 meet, (h'z)x, the Lagrangian Hessian, the Lagrangian's
    theta-gradient) gets per-stage PARTIALS and one finishing pass that adds them in a fixed order: no atomics, the same bits every run.  Quirk B-11 of the reference
    (tests/problems.py: TrajectoryProblem — where two consecutive dynamics stages both emit a (x_t+1, x_t+1) entry of (g'y)xx the later stage's value alone survives) is
    resolved HERE, by leaving the earlier stage's partial out of the finishing pass's list (hessian="reference", the default; "exact" sums them);
  * asked for a Jacobian or the Hessian the evaluator first zero-fills it (one launch over the packed storage or the dense arrays), then scatters.
One call enqueues at most four operations (the table upload of the first call, the fill, the evaluation kernel, the finishing pass); <name>_debug_last_enqueued counts.
The text does not depend on the horizon: the tables come from Python through <name>_user_create.  evaluate() is the numpy twin through the same tables."""
import ctypes
import hashlib
import inspect
import os
import re
import shutil
import subprocess

import numpy as np

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
    contract of Solver and of the oracle); template_source(), source(), stats(), compile(), solver(); initialize_states, initialize_actions, get_trajectory,
    linear_interpolation."""

    def __init__(self, objective, dynamics, num_states, num_actions, equality=None, nonnegative=None, second_order=None, num_parameters=None, hessian="reference",
                 name="trajectory", **unsupported):
        import sympy as sp
        self._sp = sp
        if "equality_general" in unsupported:
            raise ValueError("equality_general is not supported by TrajectoryProblem: write the general equality as stage equalities, or use codegen.Problem")
        if unsupported:
            raise TypeError("TrajectoryProblem: unexpected keyword %s" % ", ".join(sorted(unsupported)))
        if not re.fullmatch(r"[A-Za-z][A-Za-z0-9_]*", name):
            raise ValueError("name must be a C identifier, got %r" % (name,))
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
        if kind == "cost":
            try:
                f = sp.sympify(raw)
            except Exception:
                f = None
            if not isinstance(f, sp.Expr) or getattr(f, "is_Matrix", False):
                raise ValueError("%s must return one scalar expression, got %s" % (what, type(raw).__name__))
            exprs = [f]
        else:
            exprs = []
            for e in _cg.Problem._sequence(raw, what):
                try:
                    s = sp.sympify(e)
                except Exception:
                    s = None
                if not isinstance(s, sp.Expr) or getattr(s, "is_Matrix", False):
                    raise ValueError("%s must return a sequence of scalar expressions; one entry is a %s" % (what, type(e).__name__))
                exprs.append(s)
        known = set(x) | set(u) | set(y) | set(th)
        for e in exprs:
            extra = sorted(s.name for s in e.free_symbols if s not in known)
            if extra:
                raise ValueError("%s may depend on its arguments alone; found the symbols %s" % (what, ", ".join(extra)))
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
        w = solver_or_variables.solution.variables if hasattr(solver_or_variables, "solution") else np.asarray(solver_or_variables)
        return [w[idx].copy() for idx in self.indices.states], [w[idx].copy() for idx in self.indices.actions]

    # ---- printing ----------------------------------------------------------------------------------------------------------------------------------
    def _function(self, k, tp):
        sp = self._sp
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
            repl, reduced = sp.cse([e for _, e in items], symbols=sp.numbered_symbols("c"), order="canonical")
            nm = dict(names)
            for s_, _ in repl:
                nm[s_] = s_.name
            pr = _cg._Printer(sp, nm)
            lines.append("    if (flags & 0x%xu) {" % bit)
            lines += ["        const double %s = %s;" % (s_.name, pr(e)) for s_, e in repl]
            for (what, e), r in zip([t for t, _ in items], reduced):
                text = pr(r)
                if what == "value":
                    lines.append("        base[%d][ri[%d * n + s]] = %s;" % (D_G if cls == 1 else D_H, e, text))
                elif what == "fx":
                    lines.append("        base[%d][vi[%d * n + s]] = %s;" % (D_FX, e, text))
                elif what == "direct":
                    lines.append("        base[%d][ad[%d * n + s]] = %s;" % (int(tp.d_field[e]), e, text))
                else:
                    lines.append("        part[%d * n + s] = %s;" % (e, text))
            lines.append("    }")
            ops += sum(int(sp.count_ops(e)) for _, e in repl) + sum(int(sp.count_ops(e)) for e in reduced)
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
        """the whole translation unit: the template functions, the kernels and the four entries"""
        shape = "static const int T_KIND[NT] = {%s};\nstatic const int T_NV[NT] = {%s};\nstatic const int T_M[NT] = {%s};\nstatic const int T_NTH[NT] = {%s};\n" \
                "static const int T_ND[NT] = {%s};\nstatic const int T_NQ[NT] = {%s};\n" % tuple(
                    ", ".join(str(v) for v in vals) for vals in ([KINDS.index(tp.kind) for tp in self.templates], [tp.nv for tp in self.templates],
                                                                 [tp.m for tp in self.templates], [tp.nth for tp in self.templates],
                                                                 [tp.nd for tp in self.templates], [tp.nq for tp in self.templates]))
        return (_RUNTIME.replace("@TEMPLATES@", self.template_source()).replace("@SHAPE@", shape).replace("@NT@", str(len(self.templates)))
                .replace("@NAME@", self.name))

    def stats(self):
        """dict(stages, templates: per kind the number of templates, instances: per template (kind, stages), applications: how often a stage function was applied to
        symbols, operations: per template sympy's count after CSE, partials, summed_outputs, sum_width)"""
        self._generate()
        return dict(stages=self.T, templates={kind: sum(1 for tp in self.templates if tp.kind == kind) for kind in KINDS},
                    instances=[(tp.kind, tp.n) for tp in self.templates], applications=self._applications, operations=list(self._ops),
                    partials=int(self.n_partials), summed_outputs=int(self.G), sum_width=int(self.W))

    # ---- compiling and the handle -----------------------------------------------------------------------------------------------------------------
    def _plan_build(self, directory, arch):
        flags = _cg.FLAGS + ["--offload-arch=%s" % arch]
        h = hashlib.sha256()
        h.update(self.source().encode())
        with open(os.path.join(_cg.INCLUDE, "calipso_hip.h"), "rb") as fh:
            h.update(fh.read())
        h.update(("\0".join(flags) + "\0" + arch).encode())
        stem = "%s_%s" % (self.name, h.hexdigest()[:16])
        directory = os.path.abspath(directory or _cg.cache_directory())
        return flags, os.path.join(directory, stem + ".hip"), os.path.join(directory, "lib" + stem + ".so")

    def library_path(self, directory=None, arch="gfx950"):
        return self._plan_build(directory, arch)[2]

    def compile(self, directory=None, hipcc=None, arch="gfx950"):
        """Write source() and build it into a shared library; returns a codegen.Compiled (.path, .cdll; .symbol = <name>_device_eval).  Cached like Problem.compile: the
        file name carries a hash of the text, of include/calipso_hip.h, the arch and the flags.  Plain kernels: a build takes seconds."""
        flags, src, lib = self._plan_build(directory, arch)
        if not os.path.exists(lib):
            hipcc = hipcc or os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
            os.makedirs(os.path.dirname(lib), exist_ok=True)
            with open(src, "w") as fh:
                fh.write(self.source())
            tmp = "%s.%d.tmp" % (lib, os.getpid())
            run = subprocess.run([hipcc] + flags + ["-I" + _cg.INCLUDE, "-shared", src, "-o", tmp], capture_output=True, text=True)
            if run.returncode != 0:
                if os.path.exists(tmp):
                    os.remove(tmp)
                raise RuntimeError("%s failed (%d) on %s:\n%s" % (hipcc, run.returncode, src, run.stderr))
            os.replace(tmp, lib)
        return _cg.Compiled(lib, self.name + "_device_eval", src)

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
        from . import Solver
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
            s = _TrajectorySolver(self if methods is None else methods, self.nx, self.np, self.ne, self.nc, parameters=parameters, nonnegative_indices=self.nonnegative_indices,
                                  second_order_indices=self.second_order_indices, options=options, device=device, structure=st)
        except Exception:
            destroy(user)
            raise
        s._trajectory, s._library, s._user, s._user_destroy = self, L, user, destroy
        entry = ctypes.cast(getattr(L, self.name + ("_block_eval" if st is not None else "_device_eval")), ctypes.c_void_p)
        (s.set_device_block_evaluator if st is not None else s.set_device_evaluator)(entry, user)
        return s

    def enqueued(self, solver):
        """how many operations (copies, fills, kernels) the last evaluation call of `solver`'s evaluator enqueued"""
        fn = getattr(solver._library, self.name + "_debug_last_enqueued")
        fn.restype, fn.argtypes = ctypes.c_int32, [ctypes.c_void_p]
        return int(fn(solver._user))


def _make_solver_class():
    from . import Solver

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

    return TrajectorySolver


class _Lazy:
    """(the package imports codegen lazily; the Solver subclass is made on first use)"""
    cls = None

    def __call__(self, *a, **k):
        if _Lazy.cls is None:
            _Lazy.cls = _make_solver_class()
        return _Lazy.cls(*a, **k)


_TrajectorySolver = _Lazy()

_RUNTIME = r'''// @NAME@: device evaluators of a trajectory problem for libcalipso_hip.so — generated by calipso.jl_amd/trajectory.py; do not edit
//   @NAME@_device_eval   calipso_device_eval_fn        (dense layout)
//   @NAME@_block_eval    calipso_device_block_eval_fn  (the packed blocks of a structured handle)
// Both run the same kernels; they differ in the address table (entry -> offset in the destination), built once per handle on the first call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "calipso_hip.h"

namespace {

@TEMPLATES@
constexpr int NT = @NT@;
@SHAPE@
enum { D_FX, D_G, D_H, D_GX, D_HX, D_GP, D_HP, D_F, D_GYX, D_HZX, D_LXX, D_LGP, N_DEST };
constexpr uint32_t HESS = CALIPSO_EVAL_OBJECTIVE_HESSIAN | CALIPSO_EVAL_EQUALITY_DUAL_HESSIAN | CALIPSO_EVAL_CONE_DUAL_HESSIAN;
constexpr uint32_t LPAR = CALIPSO_EVAL_OBJECTIVE_JACOBIAN_PARAMETERS | CALIPSO_EVAL_EQUALITY_DUAL_JACOBIAN_PARAMETERS | CALIPSO_EVAL_CONE_DUAL_JACOBIAN_PARAMETERS;
constexpr int CHUNK = 1024;                    // elements one workgroup of the fill zeroes
constexpr int N_FILL = 6;                      // equality Jacobian, cone Jacobian, Hessian, dg/dtheta, dh/dtheta, the Lagrangian's theta-gradient
static const int FILL_DEST[N_FILL] = {D_GX, D_HX, D_LXX, D_GP, D_HP, D_LGP};
static const uint32_t FILL_FLAGS[N_FILL] = {CALIPSO_EVAL_EQUALITY_JACOBIAN, CALIPSO_EVAL_CONE_JACOBIAN, HESS, CALIPSO_EVAL_EQUALITY_JACOBIAN_PARAMETERS,
                                            CALIPSO_EVAL_CONE_JACOBIAN_PARAMETERS, LPAR};

struct EvalArgs {                              // (by value: a few hundred bytes)
    const double *x, *y, *z, *th;
    double* part;
    const int* tab;                            // the device tables
    double* base[N_DEST];
    uint32_t flags;
    int n[NT], wg0[NT + 1], part0[NT], vi[NT], ri[NT], pi[NT], ad[NT];      // per template: instances, first workgroup, first partial, offsets of its tables in tab
};
struct FinishArgs {
    const double* part;
    const int* tab;
    double* base[N_DEST];
    uint32_t flags;
    int G, W, n_obj, g_addr, g_field, g_slots, obj_slots;
};
struct FillArgs {
    const int* tab;
    double* base[N_FILL];
    int first[N_FILL], wg0[N_FILL + 1];        // per selected category: its first chunk in the chunk table, its first workgroup
    int count, c_off, c_len;
};

__global__ __launch_bounds__(64) void k_evaluate(EvalArgs a) {
    const int b = blockIdx.x;
    int k = 0;
    while (k + 1 < NT && b >= a.wg0[k + 1]) ++k;            // workgroup-uniform
    const int s = (b - a.wg0[k]) * 64 + threadIdx.x;
    @NAME@_template(k, a.flags, s, a.n[k], a.x, a.y, a.z, a.th, a.tab + a.vi[k], a.tab + a.ri[k], a.tab + a.pi[k], a.tab + a.ad[k], a.base, a.part + a.part0[k]);
}

// the sums: a lane per summed output adds its partials in the order of the list; the last workgroup adds the stage costs (lane l the costs l, l + 64, ..., then a
// fixed tree)
__global__ __launch_bounds__(64) void k_finish(FinishArgs a) {
    __shared__ double tree[64];
    if (blockIdx.x == gridDim.x - 1) {
        if (!(a.flags & CALIPSO_EVAL_OBJECTIVE)) return;
        double acc = 0.0;
        for (int i = threadIdx.x; i < a.n_obj; i += 64) acc += a.part[a.tab[a.obj_slots + i]];
        tree[threadIdx.x] = acc;
        __syncthreads();
        for (int w = 32; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) tree[threadIdx.x] += tree[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) a.base[D_F][0] = tree[0];
        return;
    }
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= a.G) return;
    const int f = a.tab[a.g_field + g];
    const uint32_t need = f == D_GYX ? CALIPSO_EVAL_EQUALITY_DUAL_GRADIENT : f == D_HZX ? CALIPSO_EVAL_CONE_DUAL_GRADIENT : f == D_LXX ? HESS : LPAR;
    if (!(a.flags & need)) return;
    double acc = 0.0;
    for (int w = 0; w < a.W; ++w) {
        const int word = a.tab[a.g_slots + w * a.G + g];
        if (word < 0) break;
        const int cls = word >> 29, slot = word & ((1 << 29) - 1);
        uint32_t bit = need;
        if (f == D_LXX) bit = cls == 0 ? CALIPSO_EVAL_OBJECTIVE_HESSIAN : cls == 1 ? CALIPSO_EVAL_EQUALITY_DUAL_HESSIAN : CALIPSO_EVAL_CONE_DUAL_HESSIAN;
        if (f == D_LGP) bit = cls == 0 ? CALIPSO_EVAL_OBJECTIVE_JACOBIAN_PARAMETERS : cls == 1 ? CALIPSO_EVAL_EQUALITY_DUAL_JACOBIAN_PARAMETERS : CALIPSO_EVAL_CONE_DUAL_JACOBIAN_PARAMETERS;
        if (a.flags & bit) acc += a.part[slot];
    }
    a.base[f][a.tab[a.g_addr + g]] = acc;
}

__global__ __launch_bounds__(256) void k_fill(FillArgs a) {
    const int b = blockIdx.x;
    int c = 0;
    while (c + 1 < a.count && b >= a.wg0[c + 1]) ++c;
    const int chunk = a.first[c] + (b - a.wg0[c]);
    const int off = a.tab[a.c_off + chunk], len = a.tab[a.c_len + chunk];
    double* dst = a.base[c] + off;
    for (int i = threadIdx.x; i < len; i += 256) dst[i] = 0.0;
}

struct Route {                                 // one layout of the destinations: the tables on the device and where they came from
    bool ready = false;
    int* pinned = nullptr; int* device = nullptr; size_t words = 0;
    int vi[NT], ri[NT], pi[NT], ad[NT];
    int g_addr = 0, g_field = 0, g_slots = 0, obj_slots = 0, c_off = 0, c_len = 0;
    int fill_first[N_FILL] = {0}, fill_count[N_FILL] = {0};
    const void* key0 = nullptr; int64_t key1 = 0;      // the layout it was built for: (descriptor array, first block's values) or (nullptr, jacobian_ld)
    double* block_base = nullptr;
};

struct User {
    int G = 0, W = 0, n_obj = 0, nx = 0, ne = 0, nc = 0, np = 0;
    int64_t n_part = 0;
    int n[NT];
    std::vector<int32_t> vi[NT], ri[NT], pi[NT], d_field[NT], d_i[NT], d_j[NT];
    std::vector<int32_t> g_field, g_i, g_j, g_slots, obj_slots;
    double* part = nullptr;
    Route dense, block;
    int last_enqueued = 0;
};

struct Segment { int cat; int64_t off, len; };

// where (dest, i, j) lives: an offset from the destination's base, or -1
struct DenseLayout {
    int64_t ld, nx, ne, nc;
    int64_t operator()(int dest, int64_t i, int64_t j) const {
        switch (dest) {
        case D_GX: case D_HX: return i + j * ld;
        case D_LXX: return i + j * nx;
        case D_GP: return i + j * ne;
        case D_HP: return i + j * nc;
        case D_LGP: return i + j * nx;
        default: return -1;
        }
    }
};
struct BlockLayout {
    const calipso_device_block_data* o; double* base;
    std::vector<int> jrow, hcol;              // the block of every row of [equality; cone] and of every column of the Hessian (-1: none)
    explicit BlockLayout(const calipso_device_block_data* out) : o(out), base(nullptr) {
        jrow.assign((size_t)(o->ne + o->nc), -1); hcol.assign((size_t)o->nx, -1);
        for (int64_t b = 0; b < o->n_jacobian_blocks; ++b) {
            const calipso_device_block& k = o->jacobian_blocks[b];
            if (!base || k.values < base) base = k.values;
            for (int64_t r = k.row0; r < k.row0 + k.nrows; ++r) if (r >= 0 && r < o->ne + o->nc) jrow[(size_t)r] = (int)b;
        }
        for (int64_t b = 0; b < o->n_hessian_blocks; ++b) {
            const calipso_device_block& k = o->hessian_blocks[b];
            if (!base || k.values < base) base = k.values;
            for (int64_t c = k.col0; c < k.col0 + k.ncols; ++c) if (c >= 0 && c < o->nx) hcol[(size_t)c] = (int)b;
        }
    }
    int64_t in(const calipso_device_block& k, int64_t r, int64_t c) const {
        if (r < k.row0 || r >= k.row0 + k.nrows || c < k.col0 || c >= k.col0 + k.ncols) return -1;
        return (k.values - base) + (r - k.row0) + (c - k.col0) * k.ld;
    }
    int64_t operator()(int dest, int64_t i, int64_t j) const {
        switch (dest) {
        case D_GX: case D_HX: { const int64_t r = dest == D_GX ? i : i + o->ne; const int b = jrow[(size_t)r]; return b < 0 ? -1 : in(o->jacobian_blocks[b], r, j); }
        case D_LXX: { const int b = hcol[(size_t)j]; return b < 0 ? -1 : in(o->hessian_blocks[b], i, j); }
        case D_GP: return i + j * o->ne;
        case D_HP: return i + j * o->nc;
        case D_LGP: return i + j * o->nx;
        default: return -1;
        }
    }
};

void add_segment(std::vector<Segment>& segs, int cat, int64_t off, int64_t len) {
    if (len <= 0) return;
    if (!segs.empty() && segs.back().cat == cat && segs.back().off + segs.back().len == off) { segs.back().len += len; return; }
    segs.push_back({cat, off, len});
}

// the tables of a route: the index tables as they are, the address table and the finishing pass's addresses through `where`, the fill's chunks from `segs`
// (sorted by category); one pinned block, one device block, one copy
template <class Where>
int build_route(User* u, Route& r, const Where& where, const std::vector<Segment>& segs, hipStream_t stream) {
    std::vector<int32_t> t;
    auto put = [&](const std::vector<int32_t>& v) { const int at = (int)t.size(); t.insert(t.end(), v.begin(), v.end()); return at; };
    for (int k = 0; k < NT; ++k) {
        r.vi[k] = put(u->vi[k]); r.ri[k] = put(u->ri[k]); r.pi[k] = put(u->pi[k]);
        std::vector<int32_t> ad((size_t)T_ND[k] * u->n[k]);
        for (int e = 0; e < T_ND[k]; ++e)
            for (int s = 0; s < u->n[k]; ++s) {
                const size_t at = (size_t)e * u->n[k] + s;
                const int64_t off = where(u->d_field[k][e], u->d_i[k][at], u->d_j[k][at]);
                if (off < 0 || off > INT32_MAX) return 4;            // a non-zero outside the declared structure, or a destination beyond 2^31 entries
                ad[at] = (int32_t)off;
            }
        r.ad[k] = put(ad);
    }
    std::vector<int32_t> ga((size_t)u->G);
    for (int g = 0; g < u->G; ++g) {
        const int f = u->g_field[g];
        const int64_t off = (f == D_GYX || f == D_HZX) ? u->g_i[g] : where(f, u->g_i[g], u->g_j[g]);
        if (off < 0 || off > INT32_MAX) return 4;
        ga[g] = (int32_t)off;
    }
    r.g_addr = put(ga); r.g_field = put(u->g_field); r.g_slots = put(u->g_slots); r.obj_slots = put(u->obj_slots);
    std::vector<int32_t> c_off, c_len;
    int cat = -1;
    for (const Segment& sg : segs) {
        if (sg.cat < cat) return 5;
        while (cat < sg.cat) { ++cat; r.fill_first[cat] = (int)c_off.size(); r.fill_count[cat] = 0; }
        for (int64_t at = 0; at < sg.len; at += CHUNK) {
            if (sg.off + at > INT32_MAX) return 4;
            c_off.push_back((int32_t)(sg.off + at)); c_len.push_back((int32_t)(sg.len - at < CHUNK ? sg.len - at : CHUNK));
            ++r.fill_count[cat];
        }
    }
    while (cat < N_FILL - 1) { ++cat; r.fill_first[cat] = (int)c_off.size(); r.fill_count[cat] = 0; }
    r.c_off = put(c_off); r.c_len = put(c_len);
    r.words = t.size() ? t.size() : 1;
    if (hipHostMalloc((void**)&r.pinned, r.words * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) return 2;
    if (hipMalloc((void**)&r.device, r.words * sizeof(int32_t)) != hipSuccess) return 2;
    if (!t.empty()) memcpy(r.pinned, t.data(), t.size() * sizeof(int32_t));
    if (hipMemcpyAsync(r.device, r.pinned, r.words * sizeof(int32_t), hipMemcpyHostToDevice, stream) != hipSuccess) return 2;
    ++u->last_enqueued;
    r.ready = true;
    return 0;
}

// fill, evaluate, finish on the stream: at most three launches
int run(User* u, const Route& r, uint32_t flags, const double* x, const double* y, const double* z, const double* th, double* const* base, hipStream_t stream) {
    FillArgs fa;
    fa.tab = r.device; fa.count = 0; fa.c_off = r.c_off; fa.c_len = r.c_len; fa.wg0[0] = 0;
    for (int c = 0; c < N_FILL; ++c)
        if ((flags & FILL_FLAGS[c]) && r.fill_count[c] > 0 && base[FILL_DEST[c]]) {
            fa.base[fa.count] = base[FILL_DEST[c]]; fa.first[fa.count] = r.fill_first[c]; fa.wg0[fa.count + 1] = fa.wg0[fa.count] + r.fill_count[c]; ++fa.count;
        }
    if (fa.count > 0) { hipLaunchKernelGGL(k_fill, dim3(fa.wg0[fa.count]), dim3(256), 0, stream, fa); ++u->last_enqueued; }
    EvalArgs ea;
    ea.x = x; ea.y = y; ea.z = z; ea.th = th; ea.part = u->part; ea.tab = r.device; ea.flags = flags;
    for (int d = 0; d < N_DEST; ++d) ea.base[d] = base[d];
    int wg = 0; int64_t p0 = 0;
    for (int k = 0; k < NT; ++k) {
        ea.n[k] = u->n[k]; ea.wg0[k] = wg; ea.part0[k] = (int)p0; ea.vi[k] = r.vi[k]; ea.ri[k] = r.ri[k]; ea.pi[k] = r.pi[k]; ea.ad[k] = r.ad[k];
        wg += (u->n[k] + 63) / 64; p0 += (int64_t)T_NQ[k] * u->n[k];
    }
    ea.wg0[NT] = wg;
    if (wg > 0) { hipLaunchKernelGGL(k_evaluate, dim3(wg), dim3(64), 0, stream, ea); ++u->last_enqueued; }
    if (flags & (CALIPSO_EVAL_OBJECTIVE | CALIPSO_EVAL_EQUALITY_DUAL_GRADIENT | CALIPSO_EVAL_CONE_DUAL_GRADIENT | HESS | LPAR)) {
        FinishArgs fi;
        fi.part = u->part; fi.tab = r.device; fi.flags = flags; fi.G = u->G; fi.W = u->W; fi.n_obj = u->n_obj;
        for (int d = 0; d < N_DEST; ++d) fi.base[d] = base[d];
        fi.g_addr = r.g_addr; fi.g_field = r.g_field; fi.g_slots = r.g_slots; fi.obj_slots = r.obj_slots;
        hipLaunchKernelGGL(k_finish, dim3((u->G + 63) / 64 + 1), dim3(64), 0, stream, fi);
        ++u->last_enqueued;
    }
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

void free_route(Route& r) {
    if (r.device) (void)hipFree(r.device);
    if (r.pinned) (void)hipHostFree(r.pinned);
    r = Route();
}

}  // namespace

extern "C" {

// tables: the int32 blob of TrajectoryProblem.tables(); returns NULL when it does not fit this library or an index lies outside its range
void* @NAME@_user_create(const int32_t* blob, int64_t words) {
    if (!blob || words < 10 + 8 * (int64_t)NT || blob[0] != 0x43545250 || blob[1] != NT) return nullptr;
    User* u = new User();
    u->G = blob[2]; u->W = blob[3]; u->n_obj = blob[4]; u->n_part = blob[5]; u->nx = blob[6]; u->ne = blob[7]; u->nc = blob[8]; u->np = blob[9];
    int64_t at = 10, slots = 0;
    bool ok = u->G >= 0 && u->W >= 1 && u->n_obj >= 0 && u->n_part >= 0;
    for (int k = 0; k < NT && ok; ++k, at += 8) {
        const int32_t* h = blob + at;
        u->n[k] = h[1];
        ok = h[0] == T_KIND[k] && h[1] >= 0 && h[2] == T_NV[k] && h[3] == T_M[k] && h[4] == T_NTH[k] && h[5] == T_ND[k] && h[6] == T_NQ[k];
        slots += (int64_t)T_NQ[k] * h[1];
    }
    ok = ok && slots == u->n_part && slots < (1 << 29);
    auto take = [&](std::vector<int32_t>& v, int64_t count, int64_t lo, int64_t hi) {       // every entry in [lo, hi)
        if (!ok || count < 0 || at + count > words) { ok = false; return; }
        v.assign(blob + at, blob + at + count); at += count;
        for (int32_t e : v) if (e < lo || e >= hi) { ok = false; return; }
    };
    for (int k = 0; k < NT && ok; ++k) {
        const int64_t n = u->n[k], rows = (T_KIND[k] == 1 || T_KIND[k] == 2) ? u->ne : u->nc;
        take(u->vi[k], T_NV[k] * n, 0, u->nx); take(u->ri[k], T_M[k] * n, 0, rows); take(u->pi[k], T_NTH[k] * n, 0, u->np);
        take(u->d_field[k], T_ND[k], D_GX, D_HP + 1); take(u->d_i[k], T_ND[k] * n, 0, rows);
        take(u->d_j[k], T_ND[k] * n, 0, u->nx > u->np ? u->nx : u->np);
        for (int e = 0; e < T_ND[k] && ok; ++e) {
            const int f = u->d_field[k][e];
            const int64_t cols = (f == D_GX || f == D_HX) ? u->nx : u->np;
            for (int64_t s = 0; s < n; ++s) if (u->d_j[k][(size_t)(e * n + s)] >= cols) ok = false;
        }
    }
    take(u->g_field, u->G, D_GYX, D_LGP + 1); take(u->g_i, u->G, 0, u->nx); take(u->g_j, u->G, 0, u->nx > u->np ? u->nx : u->np);
    if (ok && at + (int64_t)u->W * u->G <= words) {
        u->g_slots.assign(blob + at, blob + at + (int64_t)u->W * u->G); at += (int64_t)u->W * u->G;
        for (int32_t w : u->g_slots) if (w != -1 && (w < 0 || (w & ((1 << 29) - 1)) >= slots || (w >> 29) > 2)) ok = false;
    } else ok = false;
    take(u->obj_slots, u->n_obj, 0, slots);
    for (int g = 0; g < u->G && ok; ++g) if (u->g_j[g] >= (u->g_field[g] == D_LGP ? u->np : u->nx)) ok = false;
    if (ok && at != words) ok = false;
    if (ok && hipMalloc((void**)&u->part, sizeof(double) * (size_t)(slots ? slots : 1)) != hipSuccess) ok = false;
    if (!ok) { delete u; return nullptr; }
    return u;
}

void @NAME@_user_destroy(void* p) {
    User* u = (User*)p;
    if (!u) return;
    free_route(u->dense); free_route(u->block);
    if (u->part) (void)hipFree(u->part);
    delete u;
}

int32_t @NAME@_debug_last_enqueued(void* p) { return p ? ((User*)p)->last_enqueued : -1; }

int32_t @NAME@_device_eval(void* user, uint32_t flags, const double* x, const double* y, const double* z, const double* theta,
                           const calipso_device_problem_data* out, void* hip_stream) {
    User* u = (User*)user;
    if (!u || !out || out->nx != u->nx || out->ne != u->ne || out->nc != u->nc || out->np != u->np) return 1;
    hipStream_t stream = (hipStream_t)hip_stream;
    u->last_enqueued = 0;
    Route& r = u->dense;
    if (r.ready && (r.key1 != out->jacobian_ld)) return 3;               // the layout changed under the handle
    if (!r.ready) {
        const DenseLayout where{out->jacobian_ld, u->nx, u->ne, u->nc};
        if (out->jacobian_ld < u->ne + u->nc) return 1;
        std::vector<Segment> segs;
        for (int64_t j = 0; j < u->nx; ++j) add_segment(segs, 0, j * out->jacobian_ld, u->ne);
        for (int64_t j = 0; j < u->nx; ++j) add_segment(segs, 1, j * out->jacobian_ld, u->nc);
        add_segment(segs, 2, 0, (int64_t)u->nx * u->nx);
        add_segment(segs, 3, 0, (int64_t)u->ne * u->np); add_segment(segs, 4, 0, (int64_t)u->nc * u->np); add_segment(segs, 5, 0, (int64_t)u->nx * u->np);
        r.key1 = out->jacobian_ld;
        if (int rc = build_route(u, r, where, segs, stream)) { free_route(r); return rc; }
    }
    double* base[N_DEST] = {out->objective_gradient_variables, out->equality_constraint, out->cone_constraint, out->equality_jacobian_variables,
                            out->cone_jacobian_variables, out->equality_jacobian_parameters, out->cone_jacobian_parameters, out->objective,
                            out->equality_dual_jacobian_variables, out->cone_dual_jacobian_variables, out->lagrangian_hessian, out->lagrangian_gradient_parameters};
    return run(u, r, flags, x, y, z, theta, base, stream);
}

int32_t @NAME@_block_eval(void* user, uint32_t flags, const double* x, const double* y, const double* z, const double* theta,
                          const calipso_device_block_data* out, void* hip_stream) {
    User* u = (User*)user;
    if (!u || !out || out->nx != u->nx || out->ne != u->ne || out->nc != u->nc || out->np != u->np) return 1;
    if (out->n_jacobian_blocks + out->n_hessian_blocks < 1 || (out->n_jacobian_blocks && !out->jacobian_blocks) || (out->n_hessian_blocks && !out->hessian_blocks)) return 1;
    hipStream_t stream = (hipStream_t)hip_stream;
    u->last_enqueued = 0;
    Route& r = u->block;
    const void* key0 = out->n_hessian_blocks ? (const void*)out->hessian_blocks : (const void*)out->jacobian_blocks;
    const int64_t key1 = (int64_t)(intptr_t)(out->n_hessian_blocks ? out->hessian_blocks[0].values : out->jacobian_blocks[0].values);
    if (r.ready && (r.key0 != key0 || r.key1 != key1)) return 3;
    if (!r.ready) {
        const BlockLayout where(out);
        std::vector<Segment> segs;
        for (int cat = 0; cat < 2; ++cat)                     // the equality rows of every Jacobian block, then the cone rows: column by column, merged where contiguous
            for (int64_t b = 0; b < out->n_jacobian_blocks; ++b) {
                const calipso_device_block& k = out->jacobian_blocks[b];
                const int64_t lo = cat == 0 ? k.row0 : (k.row0 > out->ne ? k.row0 : out->ne);
                const int64_t hi = cat == 0 ? (k.row0 + k.nrows < out->ne ? k.row0 + k.nrows : out->ne) : k.row0 + k.nrows;
                for (int64_t j = 0; j < k.ncols; ++j) add_segment(segs, cat, (k.values - where.base) + (lo - k.row0) + j * k.ld, hi - lo);
            }
        for (int64_t b = 0; b < out->n_hessian_blocks; ++b) {
            const calipso_device_block& k = out->hessian_blocks[b];
            for (int64_t j = 0; j < k.ncols; ++j) add_segment(segs, 2, (k.values - where.base) + j * k.ld, k.nrows);
        }
        add_segment(segs, 3, 0, (int64_t)u->ne * u->np); add_segment(segs, 4, 0, (int64_t)u->nc * u->np); add_segment(segs, 5, 0, (int64_t)u->nx * u->np);
        r.key0 = key0; r.key1 = key1; r.block_base = where.base;
        if (int rc = build_route(u, r, where, segs, stream)) { free_route(r); return rc; }
    }
    double* base[N_DEST] = {out->objective_gradient_variables, out->equality_constraint, out->cone_constraint, r.block_base, r.block_base,
                            out->equality_jacobian_parameters, out->cone_jacobian_parameters, out->objective, out->equality_dual_jacobian_variables,
                            out->cone_dual_jacobian_variables, r.block_base, out->lagrangian_gradient_parameters};
    return run(u, r, flags, x, y, z, theta, base, stream);
}

}  // extern "C"
'''
