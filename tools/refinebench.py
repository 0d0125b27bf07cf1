#!/usr/bin/env python3
"""Times the two device passes of FluidSolver::refine_mesh -- ifem_kelly_estimate and ifem_transfer_solution -- on a uniform n^3 Q2/Q1
box and on the same box with a slab of cells refined once (recorded, not gated: profiles/refine.txt).

Per entry: the median over `--reps` calls after `--warmup` calls of
  call ms    a host clock around the C entry, which ends in a stream synchronise (the transfer entry uploads its table every call)
  kernel ms  the device time between the event pair of the entry's launch scope (ifem_kprof_begin / _end, family "refine")
and the rate of the ALGORITHMIC bytes over the kernel time: the solution vector once, the cell tables, the face table (or the transfer
table) and the output -- the formulas stated next to the launches in csrc/kelly.hip and csrc/transfer.hip.

  python tools/refinebench.py [--n 64] [--slab 8] [--reps 20] [--warmup 3] [--out profiles/refine.txt] [--host-only]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def solver(host, n, band):
    s = host.InsIM(host.channel_prm(3), (n, n, n), (0, 0, 0), (1.0, 1.0, 1.0))
    s.set_multigrid(False)  # the levels play no part in either pass
    if band:
        s.refine_band(0, band[0], band[1])
    return s


def field(uc, pc):
    u = np.stack([np.sin(3 * uc[:, 0] + uc[:, 1] ** 2 - uc[:, 2]), np.cos(2 * uc[:, 0] * uc[:, 1]) + uc[:, 0] * uc[:, 2],
                  np.sin(uc[:, 0] - 2 * uc[:, 1] + 1.5 * uc[:, 2] ** 2)], axis=1)
    return np.concatenate([u.ravel(), 0.1 * pc[:, 0] - 0.2 * pc[:, 1]])


def timed(fn, sync, reps, warmup):
    for _ in range(warmup):
        fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--slab", type=int, default=8, help="layers of coarse cells (along x) refined once in the second mesh")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-only", action="store_true", help="build meshes and tables only (no device): a rehearsal of the host side")
    a = ap.parse_args()
    from openifem_amd import capi, host
    n = a.n
    lo = (n // 4) / n
    band = (lo, lo + a.slab / n)
    lines = [f"refinebench: {n}^3 Q2/Q1 box; second mesh: {a.slab} layers of coarse cells refined once; median of {a.reps} calls after {a.warmup}"]
    meshes = {}
    for name, b in (("uniform", None), ("slab", band)):
        t0 = time.perf_counter()
        s = solver(host, n, b)
        s.setup_host_only(0) if a.host_only else s.setup(0)
        faces = s.face_table()
        meshes[name] = (s, faces)
        n_cells, n_u, n_p = s.sizes()
        lines.append(f"  mesh {name}: {n_cells} cells, {n_u} + {n_p} dofs, {len(s.hanging_lines()[0])} hanging lines (host set-up {time.perf_counter() - t0:.1f} s)")
    table = host.transfer_table(meshes["uniform"][0], meshes["slab"][0])
    if a.host_only:
        print("\n".join(lines))
        print(f"  transfer table: {len(table[0])} + {len(table[2])} entries")
        return
    ctxs = {}
    for name, (s, faces) in meshes.items():
        n_cells, n_u, n_p = s.sizes()
        c = capi.Context.borrow(s.ctx, 3, 2, n_u // 3, n_p)
        c.vec_set(capi.VEC_PRESENT, field(*s.node_coords()))
        ctxs[name] = c
        c.kelly_estimate(capi.VEC_PRESENT, faces, host=False)  # uploads the table once
        wall = timed(lambda: c.kelly_estimate(capi.VEC_PRESENT, host=False), s.synchronize, a.reps, a.warmup)
        s.kprof_begin()
        for _ in range(a.reps):
            c.kelly_estimate(capi.VEC_PRESENT, host=False)
        k = s.kprof_end()["refine"]
        ms, gb = k["ms"] / k["scopes"], k["bytes"] / k["scopes"] / 1e9
        lines.append(f"  ifem_kelly_estimate {name:8s}: call {statistics.median(wall):8.3f} ms (min {min(wall):.3f}, max {max(wall):.3f}), "
                     f"kernel {ms:8.3f} ms, {gb:.3f} GB algorithmic -> {gb / ms:6.3f} TB/s")
    src, dst = ctxs["uniform"], ctxs["slab"]
    sd = meshes["slab"][0]
    wall = timed(lambda: dst.transfer_solution(src, capi.VEC_PRESENT, *table), sd.synchronize, a.reps, a.warmup)
    sd.kprof_begin()
    for _ in range(a.reps):
        dst.transfer_solution(src, capi.VEC_PRESENT, *table)
    k = sd.kprof_end()["refine"]
    ms, gb = k["ms"] / k["scopes"], k["bytes"] / k["scopes"] / 1e9
    lines.append(f"  ifem_transfer_solution uniform -> slab: call {statistics.median(wall):8.3f} ms (min {min(wall):.3f}, max {max(wall):.3f}; with the upload "
                 f"of the table), kernel {ms:8.3f} ms, {gb:.3f} GB algorithmic -> {gb / ms:6.3f} TB/s")
    lines.append("  (the project's streaming kernel families reach 4.7-6.3 TB/s on this device: README)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    for s, _ in meshes.values():
        s.close()


if __name__ == "__main__":
    main()
