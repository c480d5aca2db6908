"""The host's Newton-step decisions (calipso.jl_amd/csrc/step_decisions.hpp: the regularisation walk, the refinement verdict, the exit tests, the cone step sizes, the
line search, the outer updates) on the CPU: tests/step_decisions/main.cpp includes only that header, is built with the plain host compiler (no HIP include path)
under the address and undefined-behaviour sanitizers, and run as a child process.  Its expected values are worked out by hand from the reference's formulas."""
import os
import shutil
import subprocess

from helpers import ROOT


def test_step_decisions_against_hand_derived_values(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "step_decisions")
    # (gcc links the sanitizer runtimes dynamically unless told otherwise; clang links them statically by itself and does not know gcc's two flags)
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtimes = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"] +
                           static_runtimes + [os.path.join(ROOT, "tests", "step_decisions", "main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "step decisions ok" in run.stdout
