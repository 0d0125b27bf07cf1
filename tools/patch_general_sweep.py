"""Does the vertex-patch smoother with one inverse per patch (ifem_tuning::uu_smoother = 1 with uu_patch_levels = 1, csrc/patch.hip) pay on the
cylinder?  tests/fluid_cylinder_mpi through the host mirror (gamma rho / mu = 100) at 3 - 5 refinements, and its extruded 3D mesh at 1
refinement, node-block Jacobi (smoother 0) against the patches (1) on a fresh solver each: the first time step (run_one_step(True): the Newton
iterations from the zero state) with inner iterations per A~^-1 application, FGMRES iterations summed over the Newton iterations, ms per
Newton iteration (wall clock of the step with everything in it: assembly, eigenvalue bounds, the coarse levels' patch setup), the ms of
building the finest level's patch tables and inverses (the first ifem_test_uu_patch_info after an assembly: host topology + device inverses +
one host wait; made before the step, which then finds them) and the bytes of the inverse store per level.

    python tools/patch_general_sweep.py [2d refinements ...] [--no-3d]       (default 3 4 5 and the 3D mesh; output: profiles/patch_general.txt)"""
import ctypes as C
import os
import re
import sys
import time

here = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(here))
sys.path.insert(0, os.path.join(os.path.dirname(here), "tests"))
from openifem_amd import capi, host  # noqa: E402

PRM = os.path.join(os.path.dirname(here), "tests", "golden", "prm", "fluid_cylinder_mpi.prm")


def prm_2d(refinements):
    return re.sub(r"set Global refinements\s*=\s*\d+", f"set Global refinements = {refinements}", open(PRM).read())


def prm_3d(refinements):
    prm = open(PRM).read()
    for old, new in (("set Dimension = 2", "set Dimension = 3"), ("set Global refinements = 3, 0", f"set Global refinements = {refinements}, 0"),
                     ("set Gravity = 0.0, 0.0", "set Gravity = 0.0, 0.0, 0.0"), ("set Initial velocity = 0.0, 0.0", "set Initial velocity = 0.0, 0.0, 0.0"),
                     ("set Number of Dirichlet BCs = 4", "set Number of Dirichlet BCs = 6"),
                     ("set Dirichlet boundary id = 0, 2, 3, 4", "set Dirichlet boundary id = 0, 2, 3, 4, 5, 6"),
                     ("set Dirichlet boundary components = 3, 3, 3, 3", "set Dirichlet boundary components = 7, 7, 7, 7, 7, 7"),
                     ("set Dirichlet boundary values = 0.2, 0, 0, 0, 0, 0, 0, 0", "set Dirichlet boundary values = " + ", ".join(["0"] * 18))):
        assert old in prm, old
        prm = prm.replace(old, new)
    return prm


def set_tuning(s, **kw):
    tun = capi.Tuning()
    s.L.ifem_default_tuning(C.byref(tun))
    for k, v in kw.items():
        setattr(tun, k, v)
    for c in s.all_ctxs():
        if s.L.ifem_set_tuning(c, C.byref(tun)) != 0:
            raise RuntimeError(s.L.ifem_last_error().decode())


def level_info(s):
    out = []
    for c in s.all_ctxs():
        o = (C.c_int64 * 4)()
        if s.L.ifem_test_uu_patch_info(c, o) != 0:
            raise RuntimeError(s.L.ifem_last_error().decode())
        out.append(list(o))
    return out


def run(dim, refinements, knob):
    from cylmesh import inflow_bc_3d
    s = host.InsIM(prm_3d(refinements) if dim == 3 else prm_2d(refinements), mesh="cylinder")
    try:
        if dim == 3:
            s.add_hard_coded_boundary_condition(0, lambda p, c, t: inflow_bc_3d(p, c))
        else:
            s.add_hard_coded_boundary_condition(0, lambda p, c, t: 4 * 0.3 * p[1] * (0.41 - p[1]) / (0.41 * 0.41) if (c == 0 and abs(p[0]) < 1e-10) else 0.0)
        s.set_multigrid(True)
        s.setup(refinements)
        setup_ms, info = float("nan"), []
        if knob:
            set_tuning(s, uu_smoother=1, uu_patch_levels=1)
            s.assemble(True)
            s.synchronize()
            t0 = time.perf_counter()
            level_info(s)  # builds the finest level's tables and inverses (the coarser levels have no operator state yet)
            s.synchronize()
            setup_ms = (time.perf_counter() - t0) * 1e3
        s.synchronize()
        t0 = time.perf_counter()
        s.run_one_step(True)
        s.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        st = s.last_stats()
        newton, fgmres = s.last_newton()
        v, p = s.get_current_solution()
        n_cells, n_u, n_p = s.sizes()
        if knob:
            info = level_info(s)
        return dict(cells=n_cells, dofs=n_u + n_p, newton=newton, fgmres=fgmres, inner=st.inner_iters / max(st.precond_applies, 1), ms=ms / max(newton, 1),
                    vmax=v.max(), pmax=p.max(), setup_ms=setup_ms, info=info)
    finally:
        s.close()


def main():
    args = [a for a in sys.argv[1:] if a != "--no-3d"]
    cases = [(2, int(a)) for a in args] or [(2, r) for r in (3, 4, 5)]
    if "--no-3d" not in sys.argv:
        cases.append((3, 1))
    print(f"{'mesh':<8} {'cells':>8} {'dofs':>9} {'smoother':>8} {'newton':>6} {'FGMRES':>6} {'inner/apply (last solve)':>24} {'ms/newton':>10} {'vmax':>9} {'pmax':>9}", flush=True)
    for dim, r in cases:
        for knob in (0, 1):
            o = run(dim, r, knob)
            print(f"{dim}D r={r:<3} {o['cells']:>8} {o['dofs']:>9} {knob:>8} {o['newton']:>6} {o['fgmres']:>6} {o['inner']:>24.1f} {o['ms']:>10.1f} {o['vmax']:>9.5f} {o['pmax']:>9.4f}", flush=True)
            if knob:
                print(f"         built before the step: patch tables and inverses of the finest level {o['setup_ms']:.1f} ms; per level (eligible, patches, inverses, bytes): {o['info']}", flush=True)


if __name__ == "__main__":
    main()
