"""The launches of the INS assembly driver (csrc/assemble.hip), mode by mode, as an ordered list of (kernel, grid, workgroup):

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/asm_trace.py
    python tools/asm_trace.py --list DIR [OUT.txt]

The first form drives a fixed list of assemblies -- no solves -- through capi.Context on the 3x2x2 distorted Q2/Q1 box of
tests/test_gpu_matrix_free_mode.py::_box; the second prints the kernel trace rocprofv3 left under DIR in enqueue (dispatch id) order, with its
length and SHA-256.  Two builds of the library that give the same list enqueue the same device work for every mode below
(A/B: swap the libraries the way tools/ab_libs.sh does and compare the two lists)."""
import csv
import glob
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def drive():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    from openifem_amd import capi
    from test_gpu_matrix_free_mode import _box, _kw

    m, dofs, vals, ev, pr, _ = _box(3, 2, 3)
    P = capi.make_params(**_kw(3))

    def context(**tuning):
        ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
        if tuning:
            ctx.set_tuning(**tuning)
        ctx.set_constraints(0, dofs, None)
        ctx.set_constraints(1, dofs, vals)
        ctx.vec_set(capi.VEC_PRESENT, pr)
        ctx.vec_set(capi.VEC_EVAL, ev)
        return ctx

    # stored A_uu, geo_cache = 1: first (unconstrained pass + masked copies), kept, kept with the kKeep release of the copies;
    # then a changed constrained-dof set twice: the copies are re-integrated once, the second change only masks them
    ctx = context(geo_cache=1)
    for _ in range(3):
        ctx.assemble(P, False)
    for drop in (7, 13):
        keep = np.arange(len(dofs)) % drop != 0
        ctx.set_constraints(1, dofs[keep], vals[keep])
        ctx.assemble(P, True)
    ctx.close()
    for gc in (0, 2):  # the cell kernel integrates the geometry blocks every time / masked copies every time
        ctx = context(geo_cache=gc)
        for _ in range(2):
            ctx.assemble(P, True)
        ctx.close()
    # stored_uu = 0: a homogeneous set; inflow values: the lift, the kKeep release with the re-integration the lift asks for, kept
    ctx = context(stored_uu=0)
    for _ in range(2):
        ctx.assemble(P, False)
    ctx.close()
    ctx = context(stored_uu=0)
    for _ in range(4):
        ctx.assemble(P, True)
    ctx.close()
    # InsIMEX: a full assembly, then the right-hand side only
    ctx = context()
    ctx.imex_assemble(P, True, True)
    ctx.imex_assemble(P, True, False)
    ctx.close()
    print("asm_trace: 20 assemblies driven")


def listing(trace_dir, out=None):
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit(f"no *kernel_trace.csv under {trace_dir}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    rows = [{k.lower(): v for k, v in r.items()} for r in rows]  # (the header's letter case differs between rocprofv3 writers)
    # enqueue order: start times of launches on different streams (set-up work of a context runs beside the context's stream) tie or
    # swap from run to run
    rows.sort(key=lambda r: int(r["dispatch_id"]))
    lines = []
    for r in rows:
        name = r["kernel_name"].replace(" [clone .kd]", "")
        name = name[:-3] if name.endswith(".kd") else name
        grid = "x".join(r[f"grid_size_{a}"] for a in "xyz")
        wg = "x".join(r[f"workgroup_size_{a}"] for a in "xyz")
        lines.append(f"{name} grid {grid} workgroup {wg}")
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as fh:
            fh.write(text)
    print(f"{len(lines)} launches, sha256 {hashlib.sha256(text.encode()).hexdigest()}")
    return lines


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--list":
        listing(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        drive()
