"""The weight formula of the lattice velocity transfers of the A_uu V-cycle (csrc/mg_lattice.hpp) in a stand-alone program
(tests/cpp/mg_lattice_check.cpp): 1D prolongation rows against the quadratic Lagrange polynomials in long double for 1..9 coarse cells, the
restriction rows as their exact transpose, a kept axis, and the tensor product on 3 x 2 x 2 -> 6 x 4 x 4 cells against a brute-force table.
On a machine without a GPU the program is built with AddressSanitizer and UndefinedBehaviorSanitizer; a GPU machine runs the plain program
(sanitizers stay on CPU machines)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lattice_transfer_weights_stand_alone(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "openifem_amd", "csrc")
    exe = str(tmp_path / "mg_lattice_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "mg_lattice_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    import openifem_amd.capi as capi
    sanitized = capi.load().ifem_device_count() == 0
    if sanitized:
        b = subprocess.run(base + san, capture_output=True, text=True)
        if b.returncode != 0:
            pytest.skip("the sanitizer build failed (no sanitizer runtimes?): " + b.stderr[-300:])
    else:
        subprocess.run(base, check=True)
    print("build:", "AddressSanitizer + UndefinedBehaviorSanitizer" if sanitized else "plain (a GPU machine)")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout
