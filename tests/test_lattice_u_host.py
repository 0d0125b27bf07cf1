"""The host side of the B / B^T stencil products (csrc/lattice.cpp: the velocity lattice map and the position signatures of its points) in a
stand-alone program (tests/cpp/lattice_u_check.cpp): boxes in 2D / 3D, degree 1 and 2, axes of one cell, random node orders, and the inputs
the map must refuse (hole, duplicate node, non-uniform cell).  On a machine without a GPU the program is built with AddressSanitizer and
UndefinedBehaviorSanitizer; a GPU machine runs the plain program (sanitizers stay on CPU machines)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_velocity_lattice_map_and_axis_classes_stand_alone(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "openifem_amd", "csrc")
    exe = str(tmp_path / "lattice_u_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "lattice_u_check.cpp"), os.path.join(csrc, "lattice.cpp"), "-o", exe]
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
