"""The host side of the fast-diagonalisation S_m solve (csrc/sm_direct_host.cpp) in a stand-alone program (tests/cpp/sm_direct_host_check.cpp):
the 1D factors against closed-form entries, Q^T M~ Q = I and K Q = M~ Q Lambda to 1e-12 for 1 .. 40 and 128 cells under all mask
combinations, the refusals (rank-deficient M~, singular Lambda, over the cap) and the mask reader on product and non-product constraint
sets.  On a machine without a GPU the program is built with AddressSanitizer and UndefinedBehaviorSanitizer; a GPU machine runs the plain
program (sanitizers stay on CPU machines)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_factors_eigen_solver_refusals_and_mask_reader_stand_alone(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "openifem_amd", "csrc")
    exe = str(tmp_path / "sm_direct_host_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "sm_direct_host_check.cpp"), os.path.join(csrc, "sm_direct_host.cpp"), "-o", exe]
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
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout
