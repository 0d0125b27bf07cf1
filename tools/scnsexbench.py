"""Time step of Fluid::MPI::SCnsEX (csrc/scnsex.hip) beside the SCnsIM step of the same mesh: the reference's acoustic duct
(tests/acoustic_duct_wave_mpi_scnsex) scaled to an n^3 Q1/Q1 box [0,4]x[0,1]x[0,1], same material, dt = 1e-7, the Gaussian inlet pulse.

Both solvers are set up by the C++ host mirror and take `--warm` mirror steps with the inlet held at the pulse's value at its first
instant (6 exp(-(0.5 / 0.15)^2 / 2) = 0.023; only run() advances the field time), so that the state is not at rest and every shape has
been launched.  The timed steps go through the C ABI on the mirror's context with the constraints as last made -- the
Python callback of the hard-coded boundary values (n^2 calls per step) is host time of this tool, not of either solver.  A host clock
around calls that end in a device synchronise; `--rounds` alternating rounds (SCnsEX, SCnsIM, SCnsEX, ...), the median round is reported.
One further SCnsEX step is logged per kernel family (ifem_kprof_begin / ifem_kprof_end); that step is not part of the timing.
`--no-im` times SCnsEX alone (profiles/scnsex.txt: a Newton iteration of SCnsIM takes 2.8 s at 32^3; at 128^3 its steps take minutes).

  python tools/scnsexbench.py --n 32                      # both solvers
  python tools/scnsexbench.py --n 128 --no-im             # the 128^3 box, SCnsEX alone
"""
import argparse
import ctypes as C
import os
import re
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

DT = 1e-7


def pulse(p, component, t):
    if component == 0 and abs(p[0]) < 1e-10:
        return 6.0 * np.exp(-0.5 * ((t - 0.5e-4) / 0.15e-4) ** 2)
    return 0.0


def pulse_increment(p, component, t):
    """SCnsIM solves for increments: the boundary value of a step is the change of the pulse (tests/acoustic_duct_wave_mpi)"""
    return pulse(p, component, t) - (0.0 if t < 2 * DT else pulse(p, component, t - DT))


def prm_text(steps):
    prm = open(os.path.join(ROOT, "tests", "golden", "prm", "acoustic_duct_wave_mpi_scnsex.prm")).read()
    for old, new in ((r"set Dimension = 2", "set Dimension = 3"), (r"set Global refinements = 3, 0", "set Global refinements = 0, 0"),
                     (r"set End time = 1e-4", f"set End time = {steps * DT:.6e}"), (r"set Save interval = 1e-1", "set Save interval = 1e3"),
                     (r"set Gravity = 0.0, 0.0", "set Gravity = 0.0, 0.0, 0.0"), (r"set Initial velocity = 0.0, 0.0", "set Initial velocity = 0.0, 0.0, 0.0"),
                     (r"set Number of Dirichlet BCs = 4", "set Number of Dirichlet BCs = 6"),
                     (r"set Dirichlet boundary id = 0, 1, 2, 3", "set Dirichlet boundary id = 0, 1, 2, 3, 4, 5"),
                     (r"set Dirichlet boundary components = 1, 1, 2, 2", "set Dirichlet boundary components = 1, 1, 2, 2, 4, 4"),
                     (r"set Dirichlet boundary values = 6, 0, 0, 0", "set Dirichlet boundary values = 6, 0, 0, 0, 0, 0")):
        prm, n = re.subn(old, new, prm)
        assert n == 1, old
    return prm


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=128, help="cells per direction")
    ap.add_argument("--warm", type=int, default=3, help="mirror steps with the pulse before the timed window")
    ap.add_argument("--steps", type=int, default=5, help="timed SCnsEX steps per round")
    ap.add_argument("--im-steps", type=int, default=2, help="timed SCnsIM steps per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-im", action="store_true", help="skip the SCnsIM solver")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    from openifem_amd import capi, host
    L = capi.load()
    if L.ifem_device_count() <= 0:
        sys.exit("scnsexbench: no HIP device (there is no CPU fallback and no CPU timing)")
    n = a.n
    prm = prm_text(10 ** 6)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ex = host.SCnsEX(prm, (n, n, n), (0, 0, 0), (4, 1, 1))
    ex.add_hard_coded_boundary_condition(0, pulse)
    im = None if a.no_im else host.SCnsIM(prm, (n, n, n), (0, 0, 0), (4, 1, 1))
    t0 = time.perf_counter()
    ex.setup(0)
    t1 = time.perf_counter()
    if im:
        im.add_hard_coded_boundary_condition(0, pulse_increment)
        im.setup(0)
    t2 = time.perf_counter()
    n_cells, n_u, n_p = ex.sizes()
    say(f"# SCnsEX beside SCnsIM: {n}^3 Q1/Q1 cells of [0,4]x[0,1]x[0,1], {n_u + n_p} dofs, mu 1.8e-4, rho 1.3e-3, dt {DT:g}")
    say(f"# set-up (host mirror + context): SCnsEX {t1 - t0:.2f} s" + (f", SCnsIM {t2 - t1:.2f} s" if im else "; SCnsIM not run (--no-im)"))
    P = capi.make_scns_params(1.8e-4, 1.3e-3, DT)
    tol, maxit = 1e-6, 8
    for _ in range(a.warm):  # (the first step integrates the matrices of SCnsEX; SCnsIM assembles every Newton iteration)
        ex.make_constraints()
        ex.run_one_step(True)
        print(f"warm-up: SCnsEX step done ({ex.last_step().outer_iterations} outer iterations)", flush=True)
        if im:
            im.make_constraints()
            im.run_one_step(True)
            print("warm-up: SCnsIM step done", flush=True)

    def ex_round():
        outer, cg = 0, 0
        L.ifem_synchronize(ex.ctx)
        t = time.perf_counter()
        for _ in range(a.steps):
            st = capi.ScnsexStats()
            rc = L.ifem_scnsex_step(ex.ctx, C.byref(P), tol, maxit, C.byref(st))
            if rc < 0:
                raise capi.IfemError(rc, L.ifem_last_error().decode())
            outer += st.outer_iterations
            cg += st.vel_iters + st.pre_iters
        L.ifem_synchronize(ex.ctx)
        return (time.perf_counter() - t) * 1e3 / a.steps, outer / a.steps, cg

    def im_round():
        newton = 0
        log = np.zeros((maxit + 1, 4))
        L.ifem_synchronize(im.ctx)
        t = time.perf_counter()
        for _ in range(a.im_steps):
            rc = L.ifem_scns_newton_step(im.ctx, C.byref(P), C.byref(im.opts), 0, tol, maxit, log.ctypes.data_as(C.c_void_p))
            if rc < 0:
                raise capi.IfemError(rc, L.ifem_last_error().decode())
            newton += rc
        L.ifem_synchronize(im.ctx)
        return (time.perf_counter() - t) * 1e3 / a.im_steps, newton / a.im_steps

    rex, rim, im_error = [], [], None
    for r in range(a.rounds):
        rex.append(ex_round())
        print(f"round {r}: SCnsEX {rex[-1][0]:.3f} ms/step", flush=True)
        if im and im_error is None:
            try:
                rim.append(im_round())
            except capi.IfemError as e:  # the comparison is context; SCnsEX is what this tool is about
                im_error = str(e)
    say("# round  SCnsEX ms/step  outer/step  ms/outer  |  SCnsIM ms/step  Newton/step  ms/Newton")
    for r in range(a.rounds):
        e = rex[r]
        i = rim[r] if r < len(rim) else None
        say(f"  {r}      {e[0]:10.3f}  {e[1]:10.2f}  {e[0] / e[1]:8.3f}  |  " + (f"{i[0]:10.3f}  {i[1]:11.2f}  {i[0] / i[1]:9.3f}" if i else "        n/a"))
    me = statistics.median(x[0] for x in rex)
    mo = statistics.median(x[0] / x[1] for x in rex)
    say(f"median  SCnsEX {me:.3f} ms/step, {mo:.3f} ms/outer iteration" +
        (f"; SCnsIM {statistics.median(x[0] for x in rim):.3f} ms/step, {statistics.median(x[0] / x[1] for x in rim):.3f} ms/Newton iteration"
         if rim else ""))
    if im_error:
        say(f"# SCnsIM stopped: {im_error}")
    nnzb = L.ifem_nnz(ex.ctx, 0)
    say(f"# matrix values: SCnsEX 2 x {nnzb} doubles = {2 * nnzb * 8 / 2 ** 30:.2f} GiB (A_uu block CSR: {L.ifem_uu_stored_bytes(ex.ctx)} bytes)" +
        (f"; SCnsIM stores {L.ifem_uu_stored_bytes(im.ctx) / 2 ** 30:.2f} GiB of A_uu alone" if im else
         f"; the stored A_uu of this mesh would hold {nnzb * 9 * 8 / 2 ** 30:.2f} GiB"))
    ex.kprof_begin()
    st = capi.ScnsexStats()
    L.ifem_scnsex_step(ex.ctx, C.byref(P), tol, maxit, C.byref(st))
    fam = ex.kprof_end()
    say(f"# one SCnsEX step by kernel family ({st.outer_iterations} outer iterations, CG {st.vel_iters} / {st.pre_iters} in the last):")
    say("#   family               scopes        ms      GB/s (algorithmic)")
    for name, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms"]):
        rate = f"{v['bytes'] / v['ms'] / 1e6:10.0f}" if v["ms"] > 0 and v["bytes"] > 0 else "         -"
        say(f"    {name:20s} {v['scopes']:6d} {v['ms']:9.3f}  {rate}")
    ex.close()
    if im:
        im.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
