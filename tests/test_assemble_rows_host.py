"""The index arithmetic of the row-owner assembly of A_uu (csrc/assemble_rows.hpp) in a stand-alone program
(tests/cpp/assemble_rows_check.cpp) on 1x1x1, 1x2x3, 2x2x2, 3x3x3 and 5x4x3 cells: every (row node, cell) incidence of the mesh is produced
exactly once, every lattice node has one owner, every column of a pair lies inside the lattice and inside its row's stencil box, and the
(row, column) entries produced are the lattice pattern with the multiplicity of the cells that hold them.
On a machine without a GPU the program is built with AddressSanitizer and UndefinedBehaviorSanitizer; a GPU machine runs the plain program
(sanitizers stay on CPU machines)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_owner_index_arithmetic_stand_alone(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "openifem_amd", "csrc")
    exe = str(tmp_path / "assemble_rows_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "assemble_rows_check.cpp"), "-o", exe]
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
