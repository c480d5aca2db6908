"""The workspace layout of differentiate!'s p-column passes (calipso.jl_amd/csrc/column_layout.hpp: where the condensed pipeline, the columns and the correction rounds'
buffers live, forward and transposed) on the CPU: tests/column_layout/main.cpp includes only that header, is built with the plain host compiler (no HIP include path)
under the address and undefined-behaviour sanitizers, and run as a child process.  It checks sizes, bounds, the two permitted aliases and the totals the solver
reserved before the layout function existed."""
import os
import shutil
import subprocess

from helpers import ROOT


def test_column_layout_regions_and_totals(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "column_layout")
    # (gcc links the sanitizer runtimes dynamically unless told otherwise; clang links them statically by itself and does not know gcc's two flags)
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtimes = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"] +
                           static_runtimes + [os.path.join(ROOT, "tests", "column_layout", "main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "column layout ok" in run.stdout
