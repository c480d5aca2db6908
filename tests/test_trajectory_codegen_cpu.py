"""codegen.TrajectoryProblem (calipso.jl_amd/trajectory.py) without a GPU: its bookkeeping and its numpy twin against flat problems built from the same stage functions
and against the committed pendulum and cart-pole problems, both Hessian modes; one derivation per template whatever the horizon; the generated per-template device
functions compiled by the host C++ compiler against a mock (tests/trajectory_host/main.cpp, under the address and undefined-behaviour sanitizers, run as a child
process); the host tables of the generated libraries (include/calipso_trajectory_tables.hpp through tests/trajectory_host/tables_main.cpp, the same way): the address
tables of the dense and of the block layout and the fill chunks against numpy, the checks of the blob; its refusals; the oracle solving through TrajectoryProblem.evaluate."""
import functools
import importlib.util
import inspect
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import problems as pr
from helpers import ROOT

HOST = os.path.join(ROOT, "tests", "trajectory_host", "main.cpp")
TABLES_HOST = os.path.join(ROOT, "tests", "trajectory_host", "tables_main.cpp")
PROBLEMS = os.path.join(ROOT, "tests", "device_eval_trajectory", "problems.py")
ALL_FLAGS = (1 << 16) - 1


@functools.lru_cache(maxsize=1)
def tp():
    if "trajectory_problems" in sys.modules:
        return sys.modules["trajectory_problems"]
    spec = importlib.util.spec_from_file_location("trajectory_problems", PROBLEMS)
    m = importlib.util.module_from_spec(spec)
    sys.modules["trajectory_problems"] = m
    spec.loader.exec_module(m)
    return m


def sizes(p):
    nx, ne, nc, npar = p.nx, p.ne, p.nc, p.np
    return {"objective": 1, "objective_gradient_variables": nx, "objective_jacobian_variables_variables": nx * nx, "objective_jacobian_variables_parameters": nx * npar,
            "equality_constraint": ne, "equality_jacobian_variables": ne * nx, "equality_jacobian_parameters": ne * npar, "equality_dual_jacobian_variables": nx,
            "equality_dual_jacobian_variables_variables": nx * nx, "equality_dual_jacobian_variables_parameters": nx * npar, "cone_constraint": nc,
            "cone_jacobian_variables": nc * nx, "cone_jacobian_parameters": nc * npar, "cone_dual_jacobian_variables": nx,
            "cone_dual_jacobian_variables_variables": nx * nx, "cone_dual_jacobian_variables_parameters": nx * npar}


def fields(p, x, y, z, theta):
    """every ProblemData field of p at the point, all flags, the parameter flags included"""
    S, out = sizes(p), {}
    p.evaluate(ALL_FLAGS, x, y, z, theta, lambda name: out.setdefault(name, np.zeros(S[name])))
    return {name: out.get(name, np.zeros(n)) for name, n in S.items()}


def agree(TP, flat, theta, tol=1e-13, points=3):
    assert (TP.nx, TP.np, TP.ne, TP.nc) == (flat.nx, flat.np, flat.ne, flat.nc)
    rng = np.random.default_rng(3)
    for _ in range(points):
        x, y, z = rng.standard_normal(TP.nx), rng.standard_normal(TP.ne), rng.standard_normal(TP.nc)
        a, b = fields(TP, x, y, z, theta), fields(flat, x, y, z, theta)
        for name in b:
            if b[name].size:
                assert np.abs(a[name] - b[name]).max() <= tol * max(1.0, np.abs(b[name]).max()), name


def flat_problem(name):
    """the flat pr.SymbolicProblem of the stage functions of `name` in the reference's row and cone order: [dynamics; stage equalities], [nonnegative of all stages;
    second-order cones stage by stage], theta = vcat(theta_t)"""
    a = tp().functions(name)
    ns, na = a["num_states"], a["num_actions"] + [0]
    T = len(ns)
    nth = a.get("num_parameters") or [0] * T
    xo, po = np.cumsum([0] + [ns[t] + na[t] for t in range(T)]), np.cumsum([0] + list(nth))

    def call(fn, t, z, th, lead=()):
        X, U = z[xo[t]:xo[t] + ns[t]], z[xo[t] + ns[t]:xo[t] + ns[t] + na[t]]
        args = list(lead) + [X, U]
        if len(inspect.signature(fn).parameters) > len(args):
            args.append(th[po[t]:po[t + 1]])
        return fn(*args)

    lists = {k: (a.get(k) or [None] * T) for k in ("equality", "nonnegative", "second_order")}
    objective = lambda z, th=(): sum(call(a["objective"][t], t, z, th) for t in range(T))

    def equality(z, th=()):
        e = []
        for t in range(T - 1):
            e += list(call(a["dynamics"][t], t, z, th, lead=[z[xo[t + 1]:xo[t + 1] + ns[t + 1]]]))
        for t in range(T):
            if lists["equality"][t] is not None:
                e += list(call(lists["equality"][t], t, z, th))
        return e

    cones = []

    def cone(z, th=()):
        h = []
        for t in range(T):
            if lists["nonnegative"][t] is not None:
                h += list(call(lists["nonnegative"][t], t, z, th))
        q = len(h)
        del cones[:]
        for t in range(T):
            for fn in (lists["second_order"][t] or []):
                c = list(call(fn, t, z, th))
                cones.append(list(range(len(h) + 1, len(h) + len(c) + 1)))
                h += c
        cone.q = q
        return h

    npar = int(po[-1])
    wrap = (lambda f: f) if npar else (lambda f: (lambda z: f(z)))
    prob = pr.SymbolicProblem(int(xo[-1]), wrap(objective), wrap(equality), wrap(cone), np_=npar, name=name)
    prob.nonnegative_indices, prob.second_order_indices = list(range(1, cone.q + 1)), [list(c) for c in cones] or [[]]
    return prob


def test_bookkeeping_and_every_field_of_the_ragged_problem():
    TP = tp().trajectory("ragged", hessian="exact")
    flat = flat_problem("ragged")
    assert (TP.nx, TP.np, TP.ne, TP.nc, TP.T) == (10, 3, 8, 5, 3)
    ind = TP.indices
    assert [list(i) for i in ind.states] == [[0, 1], [3, 4, 5], [8, 9]] and [list(i) for i in ind.actions] == [[2], [6, 7]]
    assert [list(i) for i in ind.dynamics] == [[0, 1, 2], [3, 4]] and [list(i) for i in ind.equality] == [[5, 6], [], [7]]
    assert [list(i) for i in ind.nonnegative] == [[], [0, 1], []] and [[list(c) for c in st] for st in ind.second_order] == [[], [], [[2, 3, 4]]]
    assert [list(i) for i in ind.parameters] == [[0, 1], [], [2]]
    assert TP.nonnegative_indices == [1, 2] == flat.nonnegative_indices and TP.second_order_indices == [[3, 4, 5]] == flat.second_order_indices
    agree(TP, flat, tp().parameters("ragged"))
    agree(TP, flat, np.array([-0.3, 1.9, 0.45]), points=1)


def test_pendulum_both_hessian_modes_against_the_committed_problem():
    """test/examples/pendulum.jl's stage functions: "reference" reproduces the last-writer scatter of quirk B-11 entry by entry, "exact" the summed Hessian"""
    ref = tp().trajectory("pendulum")
    assert ref.hessian == "reference" and ref.structure() is None
    agree(ref, pr.pendulum(), np.zeros(0))
    agree(tp().trajectory("pendulum", hessian="exact"), pr.pendulum(hessian_mode="sum"), np.zeros(0))
    # the two modes differ, and only in (g'y)xx at the (x_t+1, x_t+1) entries two stages emit
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal(ref.nx), rng.standard_normal(ref.ne)
    a, b = fields(ref, x, y, np.zeros(0), np.zeros(0)), fields(tp().trajectory("pendulum", hessian="exact"), x, y, np.zeros(0), np.zeros(0))
    differ = [name for name in a if not np.array_equal(a[name], b[name])]
    assert differ == ["equality_dual_jacobian_variables_variables"]
    states, actions = ref.get_trajectory(ref.initialize_actions(ref.initialize_states(np.zeros(ref.nx), ref.linear_interpolation([0.0, 0.0], [np.pi, 0.0], 11)), [[0.5]] * 10))
    assert np.allclose(states[5], [np.pi / 2, 0.0]) and np.allclose(states[10], [np.pi, 0.0]) and all(u == [0.5] for u in actions)
    assert np.array_equal(ref.initialize_states(np.zeros(ref.nx), ref.linear_interpolation([0.0, 0.0], [np.pi, 0.0], 11)), pr.pendulum().x0)


def test_cartpole_mpc_against_the_committed_problem_and_its_structure():
    TP = tp().trajectory("cartpole_mpc")
    prob = pr.cartpole_mpc()
    agree(TP, prob, prob.parameters, points=2)
    agree(TP, prob, prob.parameters + np.random.default_rng(1).uniform(0.1, 0.5, prob.np), points=1)
    got, want = TP.structure(), pr.structure_from_pattern(prob)
    for key in ("row_first", "row_last", "hessian_block_start"):
        assert np.array_equal(got[key], want[key]), key
    assert len(got["hessian_block_start"]) >= 2


def test_one_derivation_per_template_whatever_the_horizon():
    import sympy as sp
    codegen = tp().load_codegen()
    calls = []

    def dyn(y, x, u):
        calls.append(1)
        return [y[0] - x[0] - 0.1 * x[1], y[1] - x[1] - 0.1 * (u[0] - sp.sin(x[0]) * sp.cos(x[1]) ** 2)]

    cost = lambda x, u: x[0] ** 2 + 0.1 * sp.cos(x[1]) + 0.01 * u[0] ** 2
    final = lambda x, u: x[0] ** 2 + x[1] ** 2

    def make(T):
        t0 = time.perf_counter()
        P = codegen.TrajectoryProblem([cost] * (T - 1) + [final], [dyn] * (T - 1), [2] * T, [1] * (T - 1), equality=[lambda x, u: [x[0], x[1]]] + [None] * (T - 1), name="long")
        return P, time.perf_counter() - t0

    small, _ = make(8)
    del calls[:]
    big, seconds = make(2048)
    st = big.stats()
    assert len(calls) == 1 and st["templates"]["dynamics"] == 1 and st["templates"]["cost"] == 2 and st["applications"] == 4
    assert ("dynamics", 2047) in st["instances"] and st["stages"] == 2048
    assert (big.nx, big.ne) == (3 * 2048 - 1, 2 * 2047 + 2)
    assert seconds < 30.0                                              # (one derivation and numpy tables: about a second)
    t0 = time.perf_counter()
    text = big.source()
    assert time.perf_counter() - t0 < 5.0
    assert text == small.source()                                       # the text does not depend on the horizon: the tables travel through user_create
    assert "long_device_eval" in text and "long_block_eval" in text and "long_user_create" in text and "long_user_destroy" in text and "atomic" not in text
    assert big.tables().dtype == np.int32
    # T = 2: one dynamics stage, no interior stage
    two, _ = make(2)
    assert two.stats()["instances"] == [("cost", 1), ("cost", 1), ("dynamics", 1), ("equality", 1)] and (two.nx, two.ne) == (5, 4)
    flat = pr.SymbolicProblem(5, lambda z: cost(z[0:2], z[2:3]) + final(z[3:5], []), lambda z: dyn(z[3:5], z[0:2], z[2:3]) + [z[0], z[1]])
    agree(two, flat, np.zeros(0))


def test_generated_device_functions_on_the_host(tmp_path):
    """the per-template functions with __device__ defined away, every instance of the ragged problem (and three lanes past the last): the lambdified values to 1e-13"""
    TP = tp().trajectory("ragged")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    inc = tmp_path / "templates.inc"
    inc.write_text(TP.template_source())
    exe = str(tmp_path / "host")
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtimes = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"] + static_runtimes +
                           ['-DTEMPLATES_FILE="%s"' % inc, "-DNAME_TEMPLATE=%s_template" % TP.name, HOST, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    rng = np.random.default_rng(11)
    x, y, z, theta = rng.standard_normal(TP.nx), rng.standard_normal(TP.ne), rng.standard_normal(TP.nc), rng.uniform(0.5, 1.5, TP.np)
    lines = ["%d %d %d %d %d" % (TP.nx, TP.ne, TP.nc, TP.np, len(TP.templates))] + [" ".join("%.17g" % v for v in a) for a in (x, y, z, theta)]
    for t in TP.templates:
        lines.append("%d %d %d %d %d %d" % (t.n, t.nv, t.m, t.nth, t.nd, t.nq))
        lines += [" ".join(str(int(v)) for v in a.reshape(-1)) for a in (t.vi, t.ri, t.pi)]
    (tmp_path / "input.txt").write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(tmp_path / "input.txt")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.endswith("done\n"), run.stdout[-2000:] + run.stderr[-4000:]
    got = {}
    for line in run.stdout.splitlines()[:-1]:
        f = line.split()
        got[(f[0], int(f[1]))] = np.array([float(v) for v in f[2:]])
    close = lambda a, b: np.abs(a - b).max() <= 1e-13 * max(1.0, np.abs(b).max()) if b.size else a.size == 0
    for k, t in enumerate(TP.templates):
        lam = y if t.cls == 1 else z
        args = [x[t.vi[j]] for j in range(t.nv)] + [lam[t.ri[r]] for r in range(t.m)] + [theta[t.pi[j]] for j in range(t.nth)]
        direct, part = np.full((t.nd, t.n), np.nan), np.full((t.nq, t.n), np.nan)
        for bit, targets, fn in TP._host(t):
            for (what, e), val in zip(targets, fn(*args)):
                if what in ("direct", "part"):
                    (direct if what == "direct" else part)[e] = np.broadcast_to(np.asarray(val, dtype=np.float64), (t.n,))
        assert not np.isnan(direct).any() and not np.isnan(part).any()                    # every entry has a section that computes it
        assert got[("direct", k)].shape == (t.nd * t.n,) and close(got[("direct", k)], direct.reshape(-1)), (k, t.kind)
        assert got[("part", k)].shape == (t.nq * t.n,) and close(got[("part", k)], part.reshape(-1)), (k, t.kind)
    want = fields(TP, x, y, z, theta)
    assert close(got[("fx", 0)], want["objective_gradient_variables"]) and close(got[("g", 0)], want["equality_constraint"]) and close(got[("h", 0)], want["cone_constraint"])


@pytest.fixture(scope="module")
def tables_host(tmp_path_factory):
    """tests/trajectory_host/tables_main.cpp against include/calipso_trajectory_tables.hpp, built once like the program above: the host compiler, both sanitizers"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("tables_host") / "tables")
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtimes = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"] + static_runtimes +
                           ["-I" + os.path.join(ROOT, "include"), TABLES_HOST, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def route(exe, tmp_path, TP, layout, blob=None):
    """(return code, {(table, template or category): words}) of the route the program assembles from TP's shape, `blob` (default TP.tables()) and the layout lines;
    (None, {}) when it refuses the blob"""
    kinds = sys.modules[type(TP).__module__].KINDS
    blob = TP.tables() if blob is None else blob
    shape = [[kinds.index(t.kind) for t in TP.templates]] + [[getattr(t, a) for t in TP.templates] for a in ("nv", "m", "nth", "nd", "nq")]
    lines = [str(len(TP.templates))] + [" ".join(str(v) for v in vals) for vals in shape] + [str(blob.size), " ".join(str(int(v)) for v in blob)] + list(layout)
    (tmp_path / "tables.txt").write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(tmp_path / "tables.txt")], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.endswith("done\n"), run.stdout[-2000:] + run.stderr[-4000:]
    out = run.stdout.splitlines()[:-1]
    if out == ["refused"]:
        return None, {}
    got = {(f[0], int(f[1])): np.array([int(v) for v in f[2:]], dtype=np.int64) for f in (line.split() for line in out[1:])}
    return int(out[0].split()[1]), got


def covered(chunks):
    """the elements the fill chunks (offset, length, offset, length, ...) zero; no element twice, no chunk empty or longer than a workgroup's 1024"""
    off, length = chunks[0::2], chunks[1::2]
    assert ((length >= 1) & (length <= 1024)).all()
    cells = np.concatenate([np.arange(o, o + n) for o, n in zip(off, length)]) if len(off) else np.zeros(0, dtype=np.int64)
    assert len(np.unique(cells)) == len(cells)
    return np.sort(cells)


def test_route_tables_of_the_ragged_problem_in_the_dense_layout(tables_host, tmp_path):
    """the address table, the finishing pass's addresses and the fill chunks against numpy on the same coordinates, exactly"""
    TP = tp().trajectory("ragged")
    tr = sys.modules[type(TP).__module__]
    nx, ne, nc, npar = TP.nx, TP.ne, TP.nc, TP.np
    for ld in (ne + nc, ne + nc + 3):
        rc, got = route(tables_host, tmp_path, TP, ["dense %d" % ld])
        assert rc == 0
        for k, t in enumerate(TP.templates):
            ld_of = {tr.D_GX: ld, tr.D_HX: ld, tr.D_GP: ne, tr.D_HP: nc}
            want = t.d_i + t.d_j * np.array([ld_of[int(f)] for f in t.d_field], dtype=np.int64)[:, None]
            assert np.array_equal(got[("ad", k)], want.reshape(-1)), (ld, k, t.kind)
            for name, table in (("vi", t.vi), ("ri", t.ri), ("pi", t.pi)):
                assert np.array_equal(got[(name, k)], table.reshape(-1)), (name, k)
        vector = np.isin(TP.g_field, (tr.D_GYX, tr.D_HZX))
        assert set(TP.g_field[~vector]) <= {tr.D_LXX, tr.D_LGP}
        assert np.array_equal(got[("g_addr", 0)], np.where(vector, TP.g_i, TP.g_i + TP.g_j * nx))       # (the Hessian and the theta-gradient: both i + j nx)
        assert np.array_equal(got[("g_field", 0)], TP.g_field) and np.array_equal(got[("g_slots", 0)], TP.g_slots.reshape(-1))
        assert np.array_equal(got[("obj_slots", 0)], TP.obj_slots)
        leading = lambda rows: (np.arange(rows)[:, None] + ld * np.arange(nx)[None, :]).T.reshape(-1)
        assert np.array_equal(covered(got[("fill", 0)]), leading(ne)) and np.array_equal(covered(got[("fill", 1)]), leading(nc))
        for c, size in ((2, nx * nx), (3, ne * npar), (4, nc * npar), (5, nx * npar)):
            assert np.array_equal(covered(got[("fill", c)]), np.arange(size)), c
    assert route(tables_host, tmp_path, TP, ["dense %d" % (ne + nc - 1)])[0] == 1


def test_route_tables_of_a_cone_problem_in_the_block_layout(tables_host, tmp_path):
    """blocks derived from structure(), laid out back to back: every address inside its block; a block that leaves a non-zero out is code 4"""
    TP = tp().trajectory("cone_3")
    tr = sys.modules[type(TP).__module__]
    st = TP.structure()
    nx, ne, nc = TP.nx, TP.ne, TP.nc
    first, last = st["row_first"] - 1, st["row_last"] - 1
    jac, at = [], 0                                    # [row0, nrows, col0, ncols, offset, ld]: one block per run of rows with one column range
    for r in range(ne + nc):
        if r not in (0, ne) and (first[r], last[r]) == (first[r - 1], last[r - 1]):
            jac[-1][1] += 1
        else:
            jac.append([r, 1, int(first[r]), int(last[r] - first[r] + 1), 0, 0])
    for b in jac:
        b[4], b[5] = at, b[1]
        at += b[1] * b[3]
    starts = [int(s) - 1 for s in st["hessian_block_start"]] + [nx]
    hes = []
    for s0, s1 in zip(starts[:-1], starts[1:]):
        hes.append([s0, s1 - s0, s0, s1 - s0, at, s1 - s0])
        at += (s1 - s0) ** 2
    layout = lambda J: ["block %d %d %d" % (len(J), len(hes), at)] + [" ".join(str(v) for v in b) for b in J + hes]
    rc, got = route(tables_host, tmp_path, TP, layout(jac))
    assert rc == 0

    def inside(blocks, key, r, c):
        """the offsets of (r, c) in the block whose rows (key 0) or columns (key 2) hold them; every one must lie in its block"""
        out = np.full(r.shape, -1, dtype=np.int64)
        for row0, nrows, col0, ncols, off, ld in blocks:
            lo, n = (row0, nrows) if key == 0 else (col0, ncols)
            mine = ((r if key == 0 else c) >= lo) & ((r if key == 0 else c) < lo + n)
            assert ((r[mine] >= row0) & (r[mine] < row0 + nrows) & (c[mine] >= col0) & (c[mine] < col0 + ncols)).all()
            out[mine] = off + (r[mine] - row0) + (c[mine] - col0) * ld
        assert (out >= 0).all()
        return out

    for k, t in enumerate(TP.templates):
        want = np.zeros((t.nd, t.n), dtype=np.int64)
        for e, f in enumerate(t.d_field):
            if f in (tr.D_GX, tr.D_HX):
                want[e] = inside(jac, 0, t.d_i[e] + (ne if f == tr.D_HX else 0), t.d_j[e])
            else:
                want[e] = t.d_i[e] + t.d_j[e] * (ne if f == tr.D_GP else nc)
        assert np.array_equal(got[("ad", k)], want.reshape(-1)), (k, t.kind)
    want = np.where(np.isin(TP.g_field, (tr.D_GYX, tr.D_HZX)), TP.g_i, TP.g_i + TP.g_j * nx)
    H = TP.g_field == tr.D_LXX
    assert H.any()
    want[H] = inside(hes, 2, TP.g_i[H], TP.g_j[H])
    assert np.array_equal(got[("g_addr", 0)], want)
    # the fill: the equality rows of the Jacobian blocks, their cone rows, the Hessian blocks — together the packed storage, once
    cells = lambda blocks, lo, hi: np.sort(np.concatenate([(off + np.arange(max(lo, row0), min(hi, row0 + nrows))[:, None] - row0 + ld * np.arange(ncols)[None, :]).reshape(-1)
                                                           for row0, nrows, col0, ncols, off, ld in blocks]))
    parts = [covered(got[("fill", c)]) for c in range(3)]
    assert np.array_equal(parts[0], cells(jac, 0, ne)) and np.array_equal(parts[1], cells(jac, ne, ne + nc)) and np.array_equal(parts[2], cells(hes, 0, nx))
    assert np.array_equal(np.sort(np.concatenate(parts)), np.arange(at))
    # the first block without its last column: the row range's last non-zero lies there
    narrow = [list(b) for b in jac]
    narrow[0][3] -= 1
    assert route(tables_host, tmp_path, TP, layout(narrow))[0] == 4


def test_the_tables_blob_is_checked_word_by_word(tables_host, tmp_path):
    TP = tp().trajectory("ragged")
    tr = sys.modules[type(TP).__module__]
    blob, nt = TP.tables(), len(TP.templates)
    dense = ["dense %d" % (TP.ne + TP.nc)]
    assert route(tables_host, tmp_path, TP, dense, blob)[0] == 0
    at, where = 10 + 8 * nt, {}                   # where each template's tables start in the blob
    for k, t in enumerate(TP.templates):
        where[k] = dict(vi=at, d_j=at + (t.nv + t.m + t.nth) * t.n + t.nd + t.nd * t.n)
        at = where[k]["d_j"] + t.nd * t.n
    k, e = next((k, e) for k, t in enumerate(TP.templates) for e, f in enumerate(t.d_field) if f in (tr.D_GP, tr.D_HP))
    assert blob[where[0]["vi"]] == TP.templates[0].vi[0, 0] and blob[where[k]["d_j"] + e * TP.templates[k].n] == TP.templates[k].d_j[e, 0] and TP.np < TP.nx
    assert blob[-1] == TP.obj_slots[-1]

    def changed(index, value):
        b = blob.copy()
        b[index] = value
        return b

    refused = {"magic": changed(0, blob[0] ^ 1), "NT off by one": changed(1, nt + 1), "one word short": blob[:-1], "one word long": np.append(blob, 0),
               "a variable index nx": changed(where[0]["vi"], TP.nx), "a partial slot past the last": changed(-1, TP.n_partials),
               "a parameter column np": changed(where[k]["d_j"] + e * TP.templates[k].n, TP.np)}
    for what, b in refused.items():
        assert route(tables_host, tmp_path, TP, dense, np.ascontiguousarray(b, dtype=np.int32))[0] is None, what


def test_refusals():
    codegen = tp().load_codegen()
    a = tp().functions("pendulum")
    with pytest.raises(ValueError, match="num_actions has length 11, expected 10"):
        codegen.TrajectoryProblem(a["objective"], a["dynamics"], a["num_states"], a["num_actions"] + [1])
    with pytest.raises(ValueError, match="dynamics has length 9, expected 10"):
        codegen.TrajectoryProblem(a["objective"], a["dynamics"][:-1], a["num_states"], a["num_actions"])
    with pytest.raises(ValueError, match="objective has length 10, expected 11"):
        codegen.TrajectoryProblem(a["objective"][:-1], a["dynamics"], a["num_states"], a["num_actions"])
    for key in ("equality", "nonnegative", "second_order", "num_parameters"):
        with pytest.raises(ValueError, match="%s has length 3, expected 11" % key):
            codegen.TrajectoryProblem(a["objective"], a["dynamics"], a["num_states"], a["num_actions"], **{key: [None if key != "num_parameters" else 0] * 3})
    with pytest.raises(ValueError, match="equality_general is not supported"):
        codegen.TrajectoryProblem(a["objective"], a["dynamics"], a["num_states"], a["num_actions"], equality_general=lambda z: [z[0]])
    with pytest.raises(ValueError, match="at least two entries, got a function of length 1"):
        codegen.TrajectoryProblem(a["objective"], a["dynamics"], a["num_states"], a["num_actions"], second_order=[[lambda x, u: [x[0] + 2.0]]] + [None] * 10)
    with pytest.raises(ValueError, match="dynamics\\[0\\] returns 1 expressions, num_states\\[1\\] = 2"):
        codegen.TrajectoryProblem(a["objective"], [lambda y, x, u: [y[0] - x[0]]] + a["dynamics"][1:], a["num_states"], a["num_actions"])
    with pytest.raises(ValueError, match='hessian must be "reference" or "exact"'):
        codegen.TrajectoryProblem(a["objective"], a["dynamics"], a["num_states"], a["num_actions"], hessian="sum")
    # structured=True for a problem whose Hessian couples consecutive stages: refused before anything is compiled or a handle made
    with pytest.raises(ValueError, match="structured=True, but the Lagrangian Hessian of trajectory_pendulum couples consecutive stages"):
        tp().trajectory("pendulum").solver(structured=True)


def oracle_solve(oracle_mod, p, theta, x0):
    o = oracle_mod.OracleSolver(p.nx, p.np, p.ne, p.nc, p.nonnegative_indices, p.second_order_indices)
    if p.np:
        o.buf("parameters")[:] = theta
    o.point()["x"][:] = x0
    return o, o.solve(p)


def test_the_oracle_solves_through_the_host_twin(oracle_mod):
    TP, prob = tp().trajectory("pendulum"), pr.pendulum(action_guess=np.zeros(10))
    x0 = TP.initialize_states(np.zeros(TP.nx), TP.linear_interpolation([0.0, 0.0], [np.pi, 0.0], TP.T))
    assert np.array_equal(x0, prob.x0)
    a, sa = oracle_solve(oracle_mod, TP, np.zeros(0), x0)
    b, sb = oracle_solve(oracle_mod, prob, np.zeros(0), prob.x0)
    assert sa == 1 and sb == 1 and a.stats()["total_iterations"] == b.stats()["total_iterations"]
    assert np.abs(a.point()["all"] - b.point()["all"]).max() <= 1e-10
    # the cone-bearing problem: nonnegative rows and second-order cones, from a cold start
    for name in ("cone_5", "cone_65"):
        C = tp().trajectory(name)
        assert C.structure() is not None and C.nc == 2 * C.T + 3 * (C.T - 1)
        o, status = oracle_solve(oracle_mod, C, tp().parameters(name), np.zeros(C.nx))
        assert status == 1 and o.stats()["refinement_failures"] == 0, (name, status, o.stats())
        states, actions = C.get_trajectory(o.point()["x"])
        assert np.abs(states[0] - [-1.0, 0.0]).max() <= 1e-4 and all(np.linalg.norm(u) <= 2.0 + 1e-6 for u in actions)
