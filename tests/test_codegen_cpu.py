"""calipso.jl_amd/codegen.py without a GPU and without hipcc: the generated evaluators of tests/device_eval_generated/problems.py compiled by the host C++ compiler
against a mock of the kernel's context (tests/codegen_host/main.cpp, under the address and undefined-behaviour sanitizers, run as a child process) and compared
with sympy's lambdify of derivatives taken here (tests/problems.py: SymbolicProblem, from the same callables); the grouping the generator reports; that its text
does not depend on PYTHONHASHSEED; its refusals."""
import functools
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT

HOST = os.path.join(ROOT, "tests", "codegen_host", "main.cpp")
PROBLEMS = os.path.join(ROOT, "tests", "device_eval_generated", "problems.py")
THREADS = (1, 64, 256)


@functools.lru_cache(maxsize=1)
def gp():
    spec = importlib.util.spec_from_file_location("generated_problems", PROBLEMS)
    m = importlib.util.module_from_spec(spec)
    sys.modules["generated_problems"] = m
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def generated(name):
    return gp().generated(name)


def reference(prob, w, theta):
    """out, fx, Z = [gx; hx], Hw = fxx + (y'g)xx + (z'h)xx and J = dR/dtheta (residual_jacobian_parameters.jl:1-40) of the oracle's twin at the point w"""
    nx, ne, nc, npar = prob.nx, prob.ne, prob.nc, prob.np
    N, oy, oz = nx + 2 * ne + 3 * nc, nx + ne + nc, nx + 2 * ne + nc
    a = (list(w[:nx]), list(w[oy:oy + ne]), list(w[oz:oz + nc]), list(theta))
    m = lambda fn, r, c: np.asarray(fn(*a), dtype=np.float64).reshape(r, c) if r * c and fn is not None else np.zeros((r, c))
    J = np.zeros((N, npar))
    if npar:
        J[:nx] = m(prob._fxp, nx, npar) + m(prob._gyxp, nx, npar) + m(prob._hzxp, nx, npar)
        J[oy:oy + ne] = m(prob._gp, ne, npar)
        J[oz:oz + nc] = m(prob._hp, nc, npar)
    cm = lambda M: M.T.reshape(-1)          # column-major
    return dict(objective=np.array([float(prob._f(*a))]), constraints=np.concatenate([m(prob._g, ne, 1), m(prob._h, nc, 1)]).reshape(-1), fx=m(prob._fx, nx, 1).reshape(-1),
                Z=cm(np.concatenate([m(prob._gx, ne, nx), m(prob._hx, nc, nx)])), Hw=cm(m(prob._fxx, nx, nx) + m(prob._gyxx, nx, nx) + m(prob._hzxx, nx, nx)), J=cm(J))


@pytest.mark.parametrize("name", ["nonlinear_cone", "friction_cone", "cartpole_mpc", "chain", "no_parameters"])
def test_generated_values_match_sympy_on_the_host(tmp_path, name):
    """every hook, for every thread id of 1, 64 and 256 threads, at two random points: 1e-12 of the largest entry of each array, nothing left NaN"""
    P = generated(name)
    prob = gp().symbolic(name)
    assert (P.nx, P.ne, P.nc, P.np) == (prob.nx, prob.ne, prob.nc, prob.np)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    inc = tmp_path / "evaluator.inc"
    inc.write_text(P.evaluator_source())
    exe = str(tmp_path / "host")
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtimes = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"] + static_runtimes +
                           ['-DEVALUATOR_FILE="%s"' % inc, "-DEVALUATOR=" + P.type_name, "-DNX=%d" % P.nx, "-DNE=%d" % P.ne, "-DNC=%d" % P.nc, "-DNP=%d" % P.np, HOST, "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    rng = np.random.default_rng(7)
    points = [(rng.uniform(-1, 1, P.N), rng.uniform(0.5, 1.5, P.np)) for _ in range(2)]
    (tmp_path / "points.txt").write_text("".join("%.17g\n" % v for w, th in points for v in list(w) + list(th)))
    run = subprocess.run([exe, str(tmp_path / "points.txt")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.endswith("done\n"), run.stdout[-2000:] + run.stderr[-4000:]
    got = {}
    for line in run.stdout.splitlines()[:-1]:
        f = line.split()
        got[(f[0], int(f[1]), int(f[2]))] = np.array([float(v) for v in f[3:]])
    for k, (w, th) in enumerate(points):
        ref = reference(prob, w, th)
        for array, want in ref.items():
            for T in THREADS:
                have = got[(array, T, k)]
                assert have.shape == want.shape, (array, T, k, have.shape, want.shape)
                assert not np.isnan(have).any(), (array, T, k, int(np.isnan(have).sum()))
                err = np.abs(have - want).max() / np.abs(want).max() if want.size and np.abs(want).max() > 0 else (np.abs(have).max() if have.size else 0.0)
                assert err <= 1e-12, (array, T, k, err)


def test_grouping_of_the_chain_and_of_the_cart_pole():
    """chain: the 234 non-constant entries of [gx; hx] lie on three diagonals of 78.  All three have the canonical form a0 * a1 (d/dx_j of x_j x_j+1 x_j+2), so the
    rule "equal canonical forms are one group" makes them ONE group of 3 x 78; three groups of 78 would satisfy the assertions too, singletons or groups that
    split a diagonal would not.  cartpole_mpc: every non-constant group of the dynamics' Jacobian has one member per stage pair, 9"""
    z = generated("chain").stats()["derivatives"]["arrays"]["Z"]
    assert z["outputs"] == 78 * 80 and z["singletons"] == 0
    assert 1 <= len(z["groups"]) <= 3 and all(n % 78 == 0 for n in z["groups"]) and sum(z["groups"]) == 3 * 78, z
    assert z["constant_outputs"] == 78 * 80 - 3 * 78
    z = generated("cartpole_mpc").stats()["derivatives"]["arrays"]["Z"]
    assert z["singletons"] == 0 and z["groups"] and all(n == 9 for n in z["groups"]), z
    # x_{t+1} - f(x_t, u_t): +1 on 36 entries, the 4 rows of x_1 - x_init, and what the dynamics leave constant; never a non-constant entry outside a group
    assert z["constant_outputs"] + sum(z["groups"]) == 40 * 49
    st = generated("cartpole_mpc").stats()
    assert set(st) == {"objective", "constraints", "derivatives", "jacobian_parameters"}
    assert st["objective"]["groups"] == [49] and st["jacobian_parameters"]["groups"] == [49, 49] and st["jacobian_parameters"]["constant_outputs"] == 4
    for hook in st.values():
        assert hook["operations"] >= 1 and hook["outputs"] == hook["constant_outputs"] + hook["singletons"] + sum(hook["groups"])


def test_source_is_the_same_under_any_hash_seed(tmp_path):
    script = tmp_path / "emit.py"
    script.write_text("import importlib.util, sys\nspec = importlib.util.spec_from_file_location('generated_problems', %r)\nm = importlib.util.module_from_spec(spec)\n"
                      "spec.loader.exec_module(m)\nsys.stdout.write(m.generated('cartpole_mpc').source())\n" % PROBLEMS)
    texts = []
    for seed in ("1", "2"):
        run = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, env=dict(os.environ, PYTHONHASHSEED=seed), timeout=300)
        assert run.returncode == 0, run.stderr[-4000:]
        texts.append(run.stdout)
    assert texts[0] == texts[1] and "CALIPSO_SMALLNEWTON_EVALUATOR(GeneratedCartpoleMpcEvaluator, generated_cartpole_mpc_kernels)" in texts[0]
    assert texts[0] == generated("cartpole_mpc").source()


def test_refusals():
    codegen = gp().load_codegen()
    f = lambda x: x[0] ** 2 + x[1] ** 2
    h = lambda n: (lambda x: [x[0] + k for k in range(n)])
    with pytest.raises(ValueError, match="dimension 17"):
        codegen.Problem(2, f, cone=h(17), nonnegative_indices=[], second_order_indices=[list(range(1, 18))])
    with pytest.raises(ValueError, match="nonnegative entries first"):
        codegen.Problem(2, f, cone=h(5), nonnegative_indices=[4, 5], second_order_indices=[[1, 2, 3]])       # a second-order cone before the nonnegative entries
    with pytest.raises(ValueError, match="contiguous second-order cones"):
        codegen.Problem(2, f, cone=h(5), nonnegative_indices=[1], second_order_indices=[[2, 4], [3, 5]])     # interleaved cones
    with pytest.raises(ValueError, match="nonnegative entries first"):
        codegen.Problem(2, f, cone=h(5), nonnegative_indices=[1, 2], second_order_indices=[[3, 4]])          # entry 5 in no cone
    with pytest.raises(ValueError, match="1 .. 128 variables"):
        codegen.Problem(129, lambda x: sum(v ** 2 for v in x))
    with pytest.raises(ValueError, match="one scalar expression"):
        codegen.Problem(2, lambda x: [x[0], x[1]])
    P = codegen.Problem(2, f, cone=h(5), nonnegative_indices=[1, 2], second_order_indices=[[3, 4, 5]])       # the layout the kernel takes
    assert (P.nx, P.ne, P.nc, P.np, P.n_nonnegative, P.second_order_dims) == (2, 0, 5, 0, 2, [3])
    assert "provides_jacobian_parameters = false" in P.evaluator_source() and "jacobian_parameters(C&" not in P.evaluator_source()


def test_compile_caches_by_content_and_reports_a_failing_compiler(tmp_path, monkeypatch):
    """with stand-ins for hipcc (no device code is compiled here): one compiler run per content, none for a repeat; another arch or panel width is another file;
    the compiler's stderr in the error; the default directory is the user's cache, outside the package"""
    codegen = gp().load_codegen()
    log = tmp_path / "calls.log"
    fake = tmp_path / "fake_hipcc"
    fake.write_text('#!/bin/sh\necho "$@" >> %s\nwhile [ $# -gt 1 ]; do if [ "$1" = "-o" ]; then : > "$2"; fi; shift; done\n' % log)
    fake.chmod(0o755)
    bad = tmp_path / "bad_hipcc"
    bad.write_text("#!/bin/sh\necho 'error: no such thing as a frobnicator' >&2\nexit 1\n")
    bad.chmod(0o755)
    P = codegen.Problem(2, lambda x, th: (x[0] - th[0]) ** 2 + x[1] ** 2, num_parameters=1, name="cached")
    d = tmp_path / "cache"
    a = P.compile(directory=str(d), hipcc=str(fake))
    b = P.compile(directory=str(d), hipcc=str(bad))                       # up to date: the compiler is not run
    assert a.path == b.path == P.library_path(directory=str(d)) and a.symbol == "cached_kernels" and os.path.exists(a.path)
    assert len(log.read_text().splitlines()) == 1
    call = log.read_text()
    assert "--offload-arch=gfx950" in call and "-O3" in call and "-std=c++17" in call and "-fPIC" in call and "-shared" in call
    assert open(a.source_path).read() == P.source()
    c = P.compile(directory=str(d), hipcc=str(fake), arch="gfx942")
    e = P.compile(directory=str(d), hipcc=str(fake), sn_jb=4)
    assert len({a.path, c.path, e.path}) == 3 and len(log.read_text().splitlines()) == 3 and "-DSN_JB=4" in log.read_text()
    Q = codegen.Problem(2, lambda x, th: (x[0] - th[0]) ** 2 + 2 * x[1] ** 2, num_parameters=1, name="cached")
    assert Q.library_path(directory=str(d)) != a.path
    with pytest.raises(RuntimeError, match="frobnicator"):
        Q.compile(directory=str(d), hipcc=str(bad))
    assert not os.path.exists(Q.library_path(directory=str(d)))
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path / "xdg"))
    monkeypatch.delenv("CALIPSO_CACHE_DIR", raising=False)
    default = P.library_path()
    assert default.startswith(str(tmp_path / "xdg")) and not default.startswith(os.path.join(ROOT, "calipso.jl_amd"))


def test_c_printing():
    """integer powers up to 4 as products, the elementary functions by their C names, numbers as double literals with 17 significant digits"""
    import sympy as sp
    codegen = gp().load_codegen()
    P = codegen.Problem(2, lambda x: x[0] ** 4 + sp.sin(x[1]) * sp.exp(x[0]) + sp.sqrt(x[1] ** 2 + 1) + sp.tanh(x[0]) / 3 + x[1] ** 7 + 0.1 * x[0])
    text = P.evaluator_source()
    body = text[text.index("objective(C&"):text.index("constraints(C&")]
    assert "w[0] * w[0] * w[0] * w[0]" in body and "pow(w[1], 7.0)" in body
    for fn in ("sin(w[1])", "exp(w[0])", "sqrt(", "tanh(w[0])"):
        assert fn in body, fn
    assert "0.10000000000000001" in body and "0.33333333333333331" in body
