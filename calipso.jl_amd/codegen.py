"""From f(x, theta), g(x, theta), h(x, theta) to a device evaluator of the one-launch batch kernel: the step the reference's Solver(objective, equality, cone,
num_variables; parameters, nonnegative_indices, second_order_indices) takes for its users (src/solver/solver.jl:152-173, methods.jl:43-67, codegen.jl:1-90), for
SmallNewtonBatch.  The functions are applied to sympy symbols; sympy derives fx, [gx; hx], the Lagrangian Hessian and dR/dtheta; this module prints them as a
workgroup-cooperative HIP evaluator against include/calipso_smallnewton.hpp, compiles it for gfx950 and hands back a ready SmallNewtonBatch:

    P = codegen.Problem(49, objective, equality, num_parameters=102, name="cartpole")
    sn = P.batch(4096)                      # compiles (cached), set_cones, set_evaluator
    sn.set_parameters(theta); sn.initialize(x0); sn.solve(); sn.differentiate()

How the generated hooks are shaped (every thread of the instance calls each hook; there is no barrier inside one):
  * an output array that must be written whole (out, fx, Z, Hw) gets ONE strided fill loop for its structural zeros — it skips, by a static bit mask, the entries
    something else writes, so that no address has two writers between barriers — and one strided loop over a static (index, value) table for its other constants;
  * the non-constant outputs are canonicalised: the symbols of each expression are renamed to placeholders in order of first appearance; outputs with equal canonical
    forms are one GROUP, emitted as one strided loop whose body (after sympy.cse) reads its placeholders through a static index table with a row per member.  Every
    lane runs the same instructions: the nine stages of a trajectory problem are nine lanes of one loop.  Equal canonical forms use the body derived from them, so
    grouping cannot produce a wrong value; a missed merge only costs speed;
  * groups of one member (singletons) are dealt round-robin over the instance's wavefronts: wavefront k mod W evaluates singleton k (a wave-uniform branch), its
    lane 0 stores;
  * the objective's top-level terms are grouped the same way, every thread accumulates its members, then one c.sum.
evaluator_source() depends only on the documented members of the context (c.tid, C::threads, c.d.ldz, c.theta, c.fx, c.Z, c.Hw, c.sum), <math.h> and a __device__
that the including file may define away: it compiles with a host compiler against a mock context (tests/test_codegen_cpu.py).

Compiling one evaluator takes about a minute (cross-compiling the three-variable nonlinear_cone fixture for every build of the kernels took 59.5 s): the entry
instantiates all of them.  compile() therefore caches by a hash of everything that goes into the build."""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(os.path.dirname(_PKG), "include")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]          # tests/device_eval_small/Makefile
LAYOUT_RULE = ("the batch kernel's cone layout is the nonnegative entries first (indices 1 .. q), then contiguous second-order cones of dimension 2 .. 16 "
               "(include/calipso_hip.h: calipso_hip_smallnewton_set_cones)")
_FUNCTIONS = {"sin": "sin", "cos": "cos", "tan": "tan", "asin": "asin", "acos": "acos", "atan": "atan", "sinh": "sinh", "cosh": "cosh", "tanh": "tanh",
              "asinh": "asinh", "acosh": "acosh", "atanh": "atanh", "exp": "exp", "log": "log", "Abs": "fabs", "atan2": "atan2", "erf": "erf"}


def cache_directory():
    """the per-user directory compile() uses by default: $CALIPSO_CACHE_DIR, else $XDG_CACHE_HOME/calipso_jl_amd, else ~/.cache/calipso_jl_amd"""
    d = os.environ.get("CALIPSO_CACHE_DIR")
    if not d:
        d = os.path.join(os.environ.get("XDG_CACHE_HOME") or os.path.join(os.path.expanduser("~"), ".cache"), "calipso_jl_amd")
    return os.path.join(d, "evaluators")


def literal(v):
    """a double literal with 17 significant digits"""
    s = "%.17g" % float(v)
    if "inf" in s or "nan" in s:
        raise ValueError("the expressions hold a non-finite number (%s)" % s)
    return s if ("." in s or "e" in s) else s + ".0"


class _Printer:
    """sympy expression -> C: integer powers up to 4 as products, the elementary functions by their <math.h> names, numbers as double literals; `names` maps a
    Symbol to its C text"""

    def __init__(self, sp, names):
        self.sp, self.names = sp, names

    def atom(self, e):
        """printed so that it can stand as a factor or a base"""
        s = self(e)
        return s if (e.is_Symbol or e.is_Function or (e.is_Number and e >= 0)) else "(" + s + ")"

    def __call__(self, e):
        sp = self.sp
        if e.is_Symbol:
            return self.names[e]
        if e.is_Number or e.is_NumberSymbol:
            return literal(e)
        if e.is_Add:
            out = ""
            for k, t in enumerate(e.args):
                c, _ = t.as_coeff_Mul()
                if c.is_negative:
                    out += (" - " if k else "-") + self.term(-t)
                else:
                    out += (" + " if k else "") + self.term(t)
            return out
        if e.is_Mul:
            return self.term(e)
        if e.is_Pow:
            return self.power(e.base, e.exp)
        if e.is_Function:
            name = type(e).__name__
            if name == "sign":
                a = self.atom(e.args[0])
                return "((%s > 0.0) - (%s < 0.0))" % (a, a)
            if name in ("Max", "Min"):
                out = self(e.args[0])
                for a in e.args[1:]:
                    out = "%s(%s, %s)" % ("fmax" if name == "Max" else "fmin", out, self(a))
                return out
            if _FUNCTIONS.get(name):
                return "%s(%s)" % (_FUNCTIONS[name], ", ".join(self(a) for a in e.args))
        raise ValueError("codegen cannot print %s (%s) as C" % (type(e).__name__, str(e)[:80]))

    def term(self, e):
        """a product: coefficient * numerator / denominator"""
        if not e.is_Mul:
            return self.atom(e) if e.is_Add else self(e)
        c, rest = e.as_coeff_Mul()
        num, den = [], []
        for f in (rest.args if rest.is_Mul else (rest,)):
            if f.is_Pow and f.exp.is_Number and f.exp.is_negative:
                den.append(self.power(f.base, -f.exp))
            else:
                num.append(self.atom(f) if not f.is_Pow else self.power(f.base, f.exp, factor=True))
        sign = "-" if c.is_negative else ""
        c = abs(c)
        if c != 1 or not num:
            num.insert(0, literal(c))
        out = sign + " * ".join(num)
        if den:
            out += " / " + (den[0] if len(den) == 1 else "(" + " * ".join(den) + ")")
        return out

    def power(self, base, exp, factor=False):
        sp = self.sp
        if exp.is_Integer and 1 <= int(exp) <= 4:
            b = self.atom(base)
            s = " * ".join([b] * int(exp))
            return s if (factor or int(exp) == 1) else "(" + s + ")"
        if exp.is_Number and exp.is_negative:
            return "(1.0 / %s)" % self.power(base, -exp)
        if exp == sp.Rational(1, 2):
            return "sqrt(%s)" % self(base)
        if exp == sp.Rational(3, 2):
            return "(%s * sqrt(%s))" % (self.atom(base), self(base))
        return "pow(%s, %s)" % (self(base), self(exp))


class _Array:
    """one output array of a hook: entries [(dest tuple, expression)], `dense` = its number of entries when every one must be written (else only nonzeros are),
    `at(i, j)` = the C lvalue for a dest given as C texts, `fill_at` = the lvalue for the linear entry `e` of the fill loop"""

    def __init__(self, name, entries, at, dense=0, fill_at=None, order=None):
        self.name, self.at, self.dense, self.fill_at = name, at, dense, fill_at
        self.entries = sorted(entries, key=(lambda en: order(en[0])) if order else (lambda en: en[0]))
        self.linear = order or (lambda d: d[0])


class Compiled:
    """what Problem.compile returns: .path of the shared library, .symbol of its entry, .cdll (loaded on first use)"""

    def __init__(self, path, symbol, source_path):
        self.path, self.symbol, self.source_path = path, symbol, source_path
        self._cdll = None

    @property
    def cdll(self):
        if self._cdll is None:
            self._cdll = ctypes.CDLL(self.path)
        return self._cdll


def compile_cached(stem, text, extra_flags, headers, key, directory=None, hipcc=None, arch="gfx950", symbol=None):
    """The one build-and-cache path of both generators.  The file name is `stem` and a hash of the text, of the named files of include/ (name and contents, in
    sorted order), of the flags, `key` and the arch; directory defaults to cache_directory().  Without `symbol`: (compiler flags, path of the .hip, path of the
    library), nothing is written.  With it: the text is written and compiled unless the library exists (a library appears under its name only whole), and a
    Compiled comes back; a failing compile raises RuntimeError with the compiler's stderr."""
    flags = FLAGS + ["--offload-arch=%s" % arch] + list(extra_flags)
    h = hashlib.sha256()
    h.update(text.encode())
    for name in sorted(headers):
        with open(os.path.join(INCLUDE, name), "rb") as fh:
            h.update(name.encode() + b"\0" + fh.read())
    h.update(("\0".join(flags) + key + "\0" + arch).encode())
    stem = "%s_%s" % (stem, h.hexdigest()[:16])
    directory = os.path.abspath(directory or cache_directory())
    src, lib = os.path.join(directory, stem + ".hip"), os.path.join(directory, "lib" + stem + ".so")
    if symbol is None:
        return flags, src, lib
    if not os.path.exists(lib):
        hipcc = hipcc or os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        os.makedirs(directory, exist_ok=True)
        with open(src, "w") as fh:
            fh.write(text)
        tmp = "%s.%d.tmp" % (lib, os.getpid())
        run = subprocess.run([hipcc] + flags + ["-I" + INCLUDE, "-shared", src, "-o", tmp], capture_output=True, text=True)
        if run.returncode != 0:
            if os.path.exists(tmp):
                os.remove(tmp)
            raise RuntimeError("%s failed (%d) on %s:\n%s" % (hipcc, run.returncode, src, run.stderr))
        os.replace(tmp, lib)
    return Compiled(lib, symbol, src)


def sweep(directory, prefixes, keep):
    """remove the .hip and .so files of `directory` whose names start with one of `prefixes` and are not among the Compiled in `keep`: what an earlier state of a
    generator or of the headers left behind"""
    current = {os.path.basename(p) for c in keep for p in (c.path, c.source_path)}
    for name in sorted(os.listdir(directory)):
        if name.startswith(tuple(prefixes)) and name.endswith((".hip", ".so")) and name not in current:
            os.remove(os.path.join(directory, name))


def check_name(name):
    if not re.fullmatch(r"[A-Za-z][A-Za-z0-9_]*", name):
        raise ValueError("name must be a C identifier, got %r" % (name,))


def as_scalar(sp, raw, what, entry=False):
    """`raw` as one scalar sympy expression: what `what` returned, or (entry) one entry of the sequence it returned"""
    try:
        s = sp.sympify(raw)
    except Exception:
        s = None
    if not isinstance(s, sp.Expr) or getattr(s, "is_Matrix", False):
        raise ValueError(("%s must return a sequence of scalar expressions; one entry is a %s" if entry else "%s must return one scalar expression, got %s")
                         % (what, type(raw).__name__))
    return s


def as_sequence(sp, v, what):
    """what `what` returned as a list of scalar sympy expressions"""
    if getattr(v, "is_Matrix", False) and min(v.shape) > 1:
        raise ValueError("%s must return a sequence of scalar expressions, got a %d x %d matrix" % (what, v.shape[0], v.shape[1]))
    try:
        v = list(v)
    except TypeError:
        raise ValueError("%s must return a sequence of scalar expressions, got %s" % (what, type(v).__name__))
    return [as_scalar(sp, e, what, entry=True) for e in v]


def check_symbols(exprs, known, what):
    """`what`: the sentence the error opens with, who may depend on what alone"""
    for e in exprs:
        extra = sorted(s.name for s in e.free_symbols if s not in known)
        if extra:
            raise ValueError("%s; found the symbols %s" % (what, ", ".join(extra)))


def body(sp, exprs, names, indent, prefix):
    """(lines declaring the common subexpressions, printed expressions, operation count) after sympy.cse, its symbols named `prefix`0, `prefix`1, ..."""
    repl, reduced = sp.cse(list(exprs), symbols=sp.numbered_symbols(prefix), order="canonical")
    names = dict(names)
    for s, _ in repl:
        names[s] = s.name
    pr = _Printer(sp, names)
    lines = ["%sconst double %s = %s;" % (indent, s.name, pr(e)) for s, e in repl]
    ops = sum(int(sp.count_ops(e)) for _, e in repl) + sum(int(sp.count_ops(e)) for e in reduced)
    return lines, [pr(e) for e in reduced], ops


class Problem:
    """Problem(num_variables, objective, equality=None, cone=None, num_parameters=0, nonnegative_indices=None, second_order_indices=None, name="problem")

    objective / equality / cone are called as f(x, theta) when num_parameters > 0 and as f(x) otherwise (codegen.jl:7,40), with lists of sympy symbols; equality and
    cone return sequences, whose lengths are ne and nc (methods.jl:45-46).  Cone indices are 1-based as in the reference; the defaults are the reference's: all of h
    nonnegative, no second-order cones.  The batch kernel wants the nonnegative entries first and then contiguous second-order cones of dimension 2 .. 16, and
    1 .. 128 variables: anything else is a ValueError, nothing is permuted.

    .nx .ne .nc .np .N; evaluator_source() = the evaluator type (with its static tables) alone; source() = the whole .hip; stats(); compile(); batch()."""

    def __init__(self, num_variables, objective, equality=None, cone=None, num_parameters=0, nonnegative_indices=None, second_order_indices=None, name="problem"):
        import sympy as sp
        self._sp = sp
        check_name(name)
        self.name = name
        self.type_name = "".join(p[:1].upper() + p[1:] for p in name.split("_") if p) + "Evaluator"
        self.symbol = name + "_kernels"
        nx, npar = int(num_variables), int(num_parameters)
        if not 1 <= nx <= 128:
            raise ValueError("num_variables = %d: the batch kernel solves problems of 1 .. 128 variables (include/calipso_hip.h)" % nx)
        if npar < 0:
            raise ValueError("num_parameters = %d" % npar)
        # (zero-padded names: sympy orders the arguments of a sum or product by name, so the stages of a trajectory print — and canonicalise — alike)
        x = [sp.Symbol("x%04d" % i) for i in range(nx)]
        th = [sp.Symbol("p%04d" % i) for i in range(npar)]
        call = (lambda fn: fn(list(x), list(th))) if npar else (lambda fn: fn(list(x)))
        f = as_scalar(sp, call(objective), "the objective")
        vec = lambda fn, what: as_sequence(sp, call(fn), what) if fn is not None else []
        g, h = vec(equality, "equality"), vec(cone, "cone")
        ne, nc = len(g), len(h)
        check_symbols([f] + g + h, set(x) | set(th), "the functions may depend on x and theta alone")
        self.nx, self.ne, self.nc, self.np = nx, ne, nc, npar
        self.N = nx + 2 * ne + 3 * nc
        self.n_nonnegative, self.second_order_dims = self._cone_layout(nc, nonnegative_indices, second_order_indices)
        y = [sp.Symbol("y%04d" % i) for i in range(ne)]
        z = [sp.Symbol("z%04d" % i) for i in range(nc)]
        oy, oz = nx + ne + nc, nx + 2 * ne + nc
        # where a symbol is read: ("w", index into the point [x; r; s; y; z; t]) or ("th", index into theta)
        self._where = {}
        for i, s in enumerate(x):
            self._where[s] = ("w", i)
        for i, s in enumerate(y):
            self._where[s] = ("w", oy + i)
        for i, s in enumerate(z):
            self._where[s] = ("w", oz + i)
        for i, s in enumerate(th):
            self._where[s] = ("th", i)
        self._derive(f, g, h, x, y, z, th)
        self._text = None

    # ---- the problem ------------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _cone_layout(nc, nonnegative, second_order):
        nonneg = list(range(1, nc + 1)) if nonnegative is None else [int(i) for i in nonnegative]
        socs = [[int(i) for i in c] for c in (second_order or []) if len(c)]
        said = "nonnegative_indices = %s, second_order_indices = %s, nc = %d" % (nonneg, socs, nc)
        q = len(nonneg)
        if nonneg != list(range(1, q + 1)):
            raise ValueError("%s; got %s" % (LAYOUT_RULE, said))
        at = q
        for c in socs:
            if c != list(range(at + 1, at + len(c) + 1)):
                raise ValueError("%s; got %s" % (LAYOUT_RULE, said))
            if not 2 <= len(c) <= 16:
                raise ValueError("%s; got a second-order cone of dimension %d" % (LAYOUT_RULE, len(c)))
            at += len(c)
        if at != nc:
            raise ValueError("%s, together all nc entries; got %s" % (LAYOUT_RULE, said))
        return q, [len(c) for c in socs]

    def _derive(self, f, g, h, x, y, z, th):
        """the hooks' outputs as sympy expressions (calipso_smallnewton.hpp:17-30): every derivative only by the symbols an expression holds"""
        sp = self._sp
        nx, ne, nc, N = self.nx, self.ne, self.nc, self.N
        m = ne + nc
        oy, oz = nx + ne + nc, nx + 2 * ne + nc
        xi = {s: i for i, s in enumerate(x)}
        ti = {s: i for i, s in enumerate(th)}

        # Derivatives are taken term by term and ONCE per canonical form of a term: the stages of a trajectory share theirs, so sympy differentiates the
        # cart-pole step once and not nine times (the same renaming as the grouping's; the derivative of the canonical form is renamed back)
        zero = sp.Integer(0)
        taken = {}

        def gradient(e, index):          # {position: derivative} over the symbols of `index` that e holds, by position
            out = {}
            for term in sp.Add.make_args(e):
                own = self._symbols_in_order(term)
                ren = {s: sp.Symbol("q%04d" % k) for k, s in enumerate(own)}
                canonical = term.xreplace(ren)
                if canonical not in taken:
                    taken[canonical] = [sp.diff(canonical, ren[s]) for s in own]
                back = {v: k for k, v in ren.items()}
                for s, d in zip(own, taken[canonical]):
                    if s in index and d != 0:
                        out[index[s]] = out.get(index[s], zero) + d.xreplace(back)
            return {k: out[k] for k in sorted(out) if out[k] != 0}

        gh = g + h
        yz = y + z
        fx = gradient(f, xi)
        rows = [gradient(e, xi) for e in gh]
        hess, lxt = {}, {}                  # fxx + (y'g)xx + (z'h)xx and fxθ + (y'g)xθ + (z'h)xθ, assembled from the rows of [gx; hx]
        for j in range(-1, m):              # (-1: the objective)
            for c_, e in (fx if j < 0 else rows[j]).items():
                for r, d in gradient(e, xi).items():
                    if r <= c_:             # one triangle, mirrored: the Hessian of a twice-differentiable function
                        hess[(r, c_)] = hess.get((r, c_), zero) + (d if j < 0 else yz[j] * d)
                for k, d in (gradient(e, ti) if self.np else {}).items():
                    lxt[(c_, k)] = lxt.get((c_, k), zero) + (d if j < 0 else yz[j] * d)
        for (r, c_), d in list(hess.items()):
            hess[(c_, r)] = d
        self._hooks = {
            "objective": [_Array("f", [((k,), t) for k, t in enumerate(sp.Add.make_args(f))], None)],
            "constraints": [_Array("out", [((r,), e) for r, e in enumerate(gh)], lambda i: "out[%s]" % i, dense=m, fill_at="out[e]")],
            "derivatives": [
                _Array("fx", [((i,), fx.get(i, zero)) for i in range(nx)], lambda i: "c.fx[%s]" % i, dense=nx, fill_at="c.fx[e]"),
                _Array("Z", [((r, c_), rows[r].get(c_, zero)) for c_ in range(nx) for r in range(m)], lambda r, c_: "c.Z[%s + %s * ldz]" % (r, c_), dense=m * nx,
                       fill_at="c.Z[e %% %d + e / %d * ldz]" % (max(m, 1), max(m, 1)), order=lambda d: d[0] + d[1] * m),
                _Array("Hw", [((r + c_ * nx,), hess.get((r, c_), zero)) for c_ in range(nx) for r in range(nx)], lambda i: "c.Hw[%s]" % i, dense=nx * nx, fill_at="c.Hw[e]"),
            ],
        }
        if self.np:
            J = [((i + k * N,), d) for (i, k), d in lxt.items() if d != 0]
            for r, e in enumerate(gh):
                at = (oy + r) if r < ne else (oz + r - ne)
                J += [((at + k * N,), d) for k, d in gradient(e, ti).items()]
            self._hooks["jacobian_parameters"] = [_Array("J", J, lambda i: "J[%s]" % i)]

    # ---- canonical forms and groups --------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _symbols_in_order(e):
        """the symbols of e in order of first appearance, walking arguments left to right (shared subexpressions once; `seen` is only asked, never iterated)"""
        seen, out, stack = set(), [], [e]
        while stack:
            n = stack.pop()
            if n in seen:
                continue
            seen.add(n)
            if n.is_Symbol:
                out.append(n)
            else:
                stack.extend(reversed(n.args))
        return out

    def _plan(self, array):
        """(zeros, constants [(dest, value)], groups [(canonical, n_w, n_th, members [(w indices, th indices, dest)])]) of an array, groups in order of their first member"""
        sp = self._sp
        zeros, constants, groups = [], [], {}
        for dest, e in array.entries:
            if not e.free_symbols:
                v = float(e.evalf(20)) if not e.is_Number else float(e)
                if v == 0.0:
                    zeros.append(dest)
                else:
                    constants.append((dest, v))
                continue
            syms = self._symbols_in_order(e)
            ws = [s for s in syms if self._where[s][0] == "w"]
            ts = [s for s in syms if self._where[s][0] == "th"]
            ren = {s: sp.Symbol("a%04d" % k) for k, s in enumerate(ws)}
            ren.update({s: sp.Symbol("b%04d" % k) for k, s in enumerate(ts)})
            canonical = e.xreplace(ren)
            key = (canonical, len(ws), len(ts))
            groups.setdefault(key, []).append(([self._where[s][1] for s in ws], [self._where[s][1] for s in ts], dest))
        return zeros, constants, [(k[0], k[1], k[2], members) for k, members in groups.items()]

    # ---- printing --------------------------------------------------------------------------------------------------------------------------------
    def _generate(self):
        if self._text is not None:
            return
        sp = self._sp
        T = self.type_name
        tables, hooks, stats = [], {}, {}
        for hook, arrays in self._hooks.items():
            lines, st, singles = [], dict(outputs=0, constant_outputs=0, groups=[], singletons=0, operations=0, arrays={}), 0
            accumulate = hook == "objective"
            for array in arrays:
                zeros, constants, groups = self._plan(array)
                ast = dict(outputs=len(array.entries), constant_outputs=len(zeros) + len(constants), groups=[len(g[3]) for g in groups if len(g[3]) > 1],
                           singletons=sum(1 for g in groups if len(g[3]) == 1), operations=0)
                base = "%s_%s_%s" % (T, hook, array.name)
                if accumulate:
                    total = sum(v for _, v in constants)
                    if total != 0.0:
                        lines.append("        if (c.tid == 0) acc += %s;" % literal(total))
                else:
                    if array.dense and zeros:
                        if len(zeros) == array.dense:
                            lines.append("        for (int e = c.tid; e < %d; e += C::threads) %s = 0.0;" % (array.dense, array.fill_at))
                        else:       # (bit e set: entry e belongs to another writer)
                            words = [0] * ((array.dense + 31) // 32)
                            zset = set(array.linear(d) for d in zeros)
                            for e in range(array.dense):
                                if e not in zset:
                                    words[e >> 5] |= 1 << (e & 31)
                            tables.append("static __device__ const unsigned %s_written[%d] = {%s};" % (base, len(words), ", ".join("0x%08xu" % w for w in words)))
                            lines.append("        for (int e = c.tid; e < %d; e += C::threads) if (!((%s_written[e >> 5] >> (e & 31)) & 1u)) %s = 0.0;" % (array.dense, base, array.fill_at))
                    if constants:
                        nd = len(constants[0][0])
                        tables.append("static __device__ const int %s_const_at[%d][%d] = {%s};" % (base, len(constants), nd, ", ".join("{" + ", ".join(str(i) for i in d) + "}" for d, _ in constants)))
                        tables.append("static __device__ const double %s_const[%d] = {%s};" % (base, len(constants), ", ".join(literal(v) for _, v in constants)))
                        lines.append("        for (int e = c.tid; e < %d; e += C::threads) %s = %s_const[e];" % (len(constants), array.at(*["%s_const_at[e][%d]" % (base, k) for k in range(nd)]), base))
                gid = 0
                for canonical, nw, nt, members in groups:
                    if len(members) == 1:
                        ws, ts, dest = members[0]
                        names = {sp.Symbol("a%04d" % k): "w[%d]" % i for k, i in enumerate(ws)}
                        names.update({sp.Symbol("b%04d" % k): "th[%d]" % i for k, i in enumerate(ts)})
                        decl, (text,), ops = body(sp, [canonical], names, "            ", "s")
                        lines.append("        if (wave == %d %% W) {" % singles)
                        lines += decl
                        lines.append("            if (lane == 0) acc += %s;" % text if accumulate else "            if (lane == 0) %s = %s;" % (array.at(*[str(i) for i in dest]), text))
                        lines.append("        }")
                        singles += 1
                    else:
                        nd = len(members[0][2])
                        tab = "%s_g%d" % (base, gid)
                        gid += 1
                        tables.append("static __device__ const int %s[%d][%d] = {%s};" % (tab, len(members), nw + nt + nd, ", ".join("{" + ", ".join(str(i) for i in ws + ts + list(dest)) + "}" for ws, ts, dest in members)))
                        names = {sp.Symbol("a%04d" % k): "a%d" % k for k in range(nw)}
                        names.update({sp.Symbol("b%04d" % k): "b%d" % k for k in range(nt)})
                        decl, (text,), ops = body(sp, [canonical], names, "            ", "s")
                        lines.append("        for (int e = c.tid; e < %d; e += C::threads) {" % len(members))
                        lines.append("            const int* t = %s[e];" % tab)
                        loads = ["a%d = w[t[%d]]" % (k, k) for k in range(nw)] + ["b%d = th[t[%d]]" % (k, nw + k) for k in range(nt)]
                        lines.append("            const double %s;" % ", ".join(loads))
                        lines += decl
                        lines.append("            acc += %s;" % text if accumulate else "            %s = %s;" % (array.at(*["t[%d]" % (nw + nt + k) for k in range(nd)]), text))
                        lines.append("        }")
                    ast["operations"] += ops
                st["arrays"][array.name] = ast
                for k in ("outputs", "constant_outputs", "singletons", "operations"):
                    st[k] += ast[k]
                st["groups"] += ast["groups"]
            head = ["        const double* th = c.theta; (void)th; (void)w;"]
            if singles:
                head.append("        constexpr int W = C::threads >= 64 ? C::threads / 64 : 1;")
                head.append("        const int wave = c.tid / 64, lane = c.tid % 64;")
            if hook == "derivatives":
                head.append("        const int ldz = c.d.ldz; (void)ldz;")
            hooks[hook] = head + lines
            stats[hook] = st
        out = ["// %s: nx = %d, ne = %d, nc = %d, np = %d — generated by calipso.jl_amd/codegen.py; do not edit" % (T, self.nx, self.ne, self.nc, self.np)]
        out += tables
        out += ["struct %s {" % T,
                "    static constexpr bool constant_derivatives = false;",
                "    static constexpr bool provides_jacobian_parameters = %s;" % ("true" if self.np else "false"),
                "    template <class C> __device__ static double objective(C& c, const double* w) {",
                "        double acc = 0.0;"] + hooks["objective"] + [
                "        double v[1] = {acc};",
                "        c.sum(v);",
                "        return v[0];",
                "    }",
                "    template <class C> __device__ static void constraints(C& c, const double* w, double* out) {"] + hooks["constraints"] + [
                "    }",
                "    template <class C> __device__ static void derivatives(C& c, const double* w) {"] + hooks["derivatives"] + [
                "    }"]
        if self.np:
            out += ["    template <class C> __device__ static void jacobian_parameters(C& c, const double* w, double* J) {"] + hooks["jacobian_parameters"] + ["    }"]
        out += ["};", ""]
        self._text, self._stats = "\n".join(out), stats

    def evaluator_source(self):
        """the evaluator type and the static tables its hooks read, nothing else: no #include, no entry"""
        self._generate()
        return self._text

    def source(self):
        """the whole translation unit: the header, the evaluator in an unnamed namespace, the entry `<name>_kernels`"""
        return ('#include "calipso_smallnewton.hpp"\n#include <math.h>\n\nnamespace {\n\n%s\n}  // namespace\n\nCALIPSO_SMALLNEWTON_EVALUATOR(%s, %s)\n'
                % (self.evaluator_source(), self.type_name, self.symbol))

    def stats(self):
        """per hook: outputs, constant_outputs (structural zeros included), groups (the member counts of the template groups), singletons, operations (sympy's
        count after CSE, every group's body once), and the same per output array under "arrays" (derivatives: fx, Z = [gx; hx], Hw)"""
        self._generate()
        return self._stats

    # ---- compiling ---------------------------------------------------------------------------------------------------------------------------------
    def _build(self, directory, arch, sn_jb, **build):
        # (the five headers named: the hash — and with it the name of a library already built — does not move when include/ gains a file the evaluator never sees)
        return compile_cached(self.name, self.source(), ["-DSN_JB=%d" % int(sn_jb)] if sn_jb is not None else [],
                              ["calipso_hip.h", "calipso_options.hpp", "calipso_smallnewton.hpp", "calipso_smallnewton_device.hpp", "calipso_wave.hpp"],
                              "\0SN_JB=%s" % sn_jb, directory=directory, arch=arch, **build)

    def library_path(self, directory=None, arch="gfx950", sn_jb=None):
        """where compile() with the same arguments puts (or finds) the shared library"""
        return self._build(directory, arch, sn_jb)[2]

    def compile(self, directory=None, hipcc=None, arch="gfx950", sn_jb=None):
        """Write source() and build it into a shared library; returns a Compiled (.path, .cdll, .symbol).  The file name carries a hash of the generated text, the
        contents of the headers of include/ it is built against, SN_JB (sn_jb: the panel width the library was built with when not the header's default), the arch
        and the flags: a second call with nothing changed loads the existing library and does not run hipcc.  directory defaults to cache_directory(), per user and
        outside the package.  Takes about a minute: the entry instantiates every build of the kernels (three-variable nonlinear_cone: 59.5 s cross-compiling).  A
        failing compile raises RuntimeError with the compiler's stderr."""
        return self._build(directory, arch, sn_jb, hipcc=hipcc, symbol=self.symbol)

    def batch(self, batch, device=0, options=None, **compile_args):
        """a SmallNewtonBatch of `batch` instances with this problem's cone layout and its compiled evaluator set: set_parameters, initialize, solve"""
        from . import SmallNewtonBatch
        built = self.compile(**compile_args)
        sn = SmallNewtonBatch(self.nx, self.ne, self.nc, batch, device=device, options=options)
        sn.set_cones(self.n_nonnegative, self.second_order_dims)
        sn.set_evaluator(built.cdll, built.symbol, self.np)
        return sn


def __getattr__(name):
    """codegen.TrajectoryProblem: the front end for per-stage functions and Solver handles lives in trajectory.py, which imports this module"""
    if name == "TrajectoryProblem":
        from .trajectory import TrajectoryProblem
        return TrajectoryProblem
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
