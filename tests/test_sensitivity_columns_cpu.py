"""The column bookkeeping of differentiate!'s correction rounds (calipso.jl_amd/csrc/sensitivity_columns.hpp: which parameter columns still take a round, their round
counts, when the loop ends) on the CPU: tests/sensitivity_columns/main.cpp includes only that header and step_decisions.hpp, is built with the plain host compiler (no
HIP include path) under the address and undefined-behaviour sanitizers, and run as a child process.  Its expected values are worked out by hand from the loop of
iterative_refinement.jl:14-51."""
import os
import shutil
import subprocess

from helpers import ROOT


def test_sensitivity_columns_against_hand_derived_cases(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "sensitivity_columns")
    # (gcc links the sanitizer runtimes dynamically unless told otherwise; clang links them statically by itself and does not know gcc's two flags)
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtimes = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"] +
                           static_runtimes + [os.path.join(ROOT, "tests", "sensitivity_columns", "main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "sensitivity columns ok" in run.stdout
