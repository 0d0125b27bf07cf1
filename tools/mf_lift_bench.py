"""Time the inhomogeneous assembly -- ifem_ins_assemble(use_nonzero = 1) with inflow values on the x- face -- under
ifem_tuning::stored_uu = 0, split by ifem_kprof_* families, and report what it leaves allocated:

    python tools/mf_lift_bench.py [n [reps [warmup]]] [--json FILE]

One context on the n^3 Q2/Q1 channel box (no multigrid levels).  Wall time per assembly: median and min / max over `reps` timed
assemblies after `warmup` untimed ones (the first builds the geometry cache, and on a build without the matrix-free lift allocates the
block CSR); the family split is the mean of the same repetitions.  The script only uses ifem_uu_stored_bytes when the library has it,
so the same file runs on a build from before the lift for an A/B comparison on one machine."""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openifem_amd import capi, host  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
if out_json in args:
    args.remove(out_json)
n = int(args[0]) if len(args) > 0 else 64
reps = int(args[1]) if len(args) > 1 else 7
warmup = int(args[2]) if len(args) > 2 else 3

prm = host.channel_prm(3)
prm = prm.replace("  set Use hard-coded boundary values = 0\n  set Number of Dirichlet BCs = 4\n  set Dirichlet boundary id = 2, 3, 4, 5\n"
                  "  set Dirichlet boundary components = 7, 7, 4, 4\n  set Dirichlet boundary values = 0, 0, 0, 0, 0, 0, 0, 0\n",
                  "  set Use hard-coded boundary values = 1\n  set Number of Dirichlet BCs = 5\n  set Dirichlet boundary id = 0, 2, 3, 4, 5\n"
                  "  set Dirichlet boundary components = 7, 7, 7, 4, 4\n  set Dirichlet boundary values = 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0\n")
prm = prm.replace("  set Number of Neumann BCs = 1\n  set Neumann boundary id = 0\n  set Neumann boundary values = 10\n", "  set Number of Neumann BCs = 0\n")
assert "Dirichlet boundary id = 0, 2" in prm and "Number of Neumann BCs = 0" in prm
H = 0.2
s = host.InsIM(prm, (n, n, n), (0, 0, 0), (2.0, H, H))
s.add_hard_coded_boundary_condition(0, lambda p, c, t: 6.0 * p[1] * (H - p[1]) / H ** 2 if c == 0 else 0.0)
s.set_multigrid(False)
s.setup(0)
s.channel_state()
L, ctx = s.L, s.ctx
tun = capi.Tuning()
L.ifem_default_tuning(C.byref(tun))
tun.stored_uu = 0
assert L.ifem_set_tuning(ctx, C.byref(tun)) == 0


def free_bytes():
    """hipMemGetInfo of the runtime the library already runs on"""
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(name)
        except OSError:
            continue
        free, total = C.c_size_t(), C.c_size_t()
        if hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0:
            return int(free.value)
    return -1


def stored_bytes():
    if not hasattr(L, "ifem_uu_stored_bytes"):
        return None
    L.ifem_uu_stored_bytes.restype = C.c_int64
    L.ifem_uu_stored_bytes.argtypes = [C.c_void_p]
    return int(L.ifem_uu_stored_bytes(ctx))


for _ in range(warmup):
    s.assemble(True)
s.synchronize()
wall, fam = [], {}
for _ in range(reps):
    s.kprof_begin()
    s.synchronize()
    t0 = time.perf_counter()
    s.assemble(True)
    s.synchronize()
    wall.append((time.perf_counter() - t0) * 1e3)
    for k, v in s.kprof_end().items():
        fam.setdefault(k, []).append(v["ms"])
wall.sort()
res = {"n": n, "cells": n ** 3, "dofs": sum(s.sizes()[1:]), "reps": reps, "warmup": warmup,
       "assemble_ms_median": statistics.median(wall), "assemble_ms_min": wall[0], "assemble_ms_max": wall[-1],
       "families_ms_mean": {k: sum(v) / len(v) for k, v in sorted(fam.items()) if sum(v) > 0},
       "uu_stored_bytes": stored_bytes(), "free_device_bytes_after": free_bytes(),
       "nnz_uu_blocks": int(L.ifem_nnz(ctx, 0))}
print(f"n = {n}: ifem_ins_assemble(use_nonzero = 1), stored_uu = 0: median {res['assemble_ms_median']:.3f} ms "
      f"(min {wall[0]:.3f}, max {wall[-1]:.3f}, {reps} repetitions after {warmup} warm-up)")
for k, v in res["families_ms_mean"].items():
    print(f"  {k:24s} {v:9.3f} ms")
print(f"  ifem_uu_stored_bytes = {res['uu_stored_bytes']}   free device memory = {res['free_device_bytes_after'] / 2 ** 30:.2f} GiB")
print(json.dumps(res))
if out_json:
    with open(out_json, "w") as f:
        json.dump(res, f, indent=1)
s.close()
