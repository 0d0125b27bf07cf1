"""Where does the vertex-patch smoother of the A_uu V-cycle (ifem_tuning::uu_smoother = 1, csrc/patch.hip) pay?  The 3D channel through the
host mirror at n^3 cells, two parameter sets (the bench's mu = 1, gamma = 0.1, dt = 1e-3 and fluid_cavity.prm's mu = 0.01, gamma = 1, dt = 1e-2),
node-block Jacobi (0) against vertex patches (1) on one context per (n, set): inner iterations per A~^-1 application, FGMRES iterations,
ms per solve (one warm-up solve per setting, then the median of the repeats) and ms of one B r on the finest level (median of 20 calls of the
test aid ifem_test_uu_patch_vmult: the 2^dim colour launches plus its two conversion passes and one host wait).

    python tools/patch_sweep.py [n ...]        (default 16 32 64; 128 needs ~100 GB of device memory with the stored A_uu)"""
import ctypes as C
import os
import statistics
import sys
import time

here = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(here))
from openifem_amd import capi, host  # noqa: E402

SETS = {"bench (mu 1, gamma 0.1, dt 1e-3)": (1.0, 0.1, 1e-3), "cavity (mu 0.01, gamma 1, dt 1e-2)": (0.01, 1.0, 1e-2)}
REPEATS = 3


def set_tuning(s, **kw):
    tun = capi.Tuning()
    s.L.ifem_default_tuning(C.byref(tun))
    for k, v in kw.items():
        setattr(tun, k, v)
    for c in s.all_ctxs():
        if s.L.ifem_set_tuning(c, C.byref(tun)) != 0:
            raise RuntimeError(s.L.ifem_last_error().decode())


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [16, 32, 64]
    print(f"{'n':>4} {'parameters':<36} {'smoother':>8} {'inner/apply':>11} {'inner':>6} {'FGMRES':>6} {'ms/solve':>9} {'ms/B r':>8} {'types':>6} {'residual':>9}", flush=True)
    for n in sizes:
        for name, (mu, gamma, dt) in SETS.items():
            prm = host.channel_prm(3, dt=dt)
            prm = prm.replace("set Dynamic viscosity = 1\n", f"set Dynamic viscosity = {mu}\n").replace("set Grad-Div stabilization = 0.1\n", f"set Grad-Div stabilization = {gamma}\n")
            s = host.InsIM(prm, (n, n, n), (0, 0, 0), (2.0, 0.2, 0.2), device=0, verbose=False)
            try:
                s.set_multigrid(True, 0)
                s.setup(0)
                s.channel_state()
                s.opts.ainv_kind = capi.AINV_MG
                s.assemble(False)
                info = np_info(s)
                t_b = float("nan")
                if info[0]:
                    ts = []
                    for _ in range(21):
                        t0 = time.perf_counter()
                        if s.L.ifem_test_uu_patch_vmult(s.ctx, capi.VEC_UPDATE, capi.VEC_TMP) != 0:
                            raise RuntimeError(s.L.ifem_last_error().decode())
                        ts.append((time.perf_counter() - t0) * 1e3)
                    t_b = statistics.median(ts[1:])
                for knob in (0, 1):
                    set_tuning(s, uu_smoother=knob)
                    s.solve(False)  # warm-up: eigenvalue bounds, patch tables, graph capture
                    s.solve(False)
                    ts, st = [], None
                    for _ in range(REPEATS):
                        s.synchronize()
                        t0 = time.perf_counter()
                        st = s.solve(False)
                        s.synchronize()
                        ts.append((time.perf_counter() - t0) * 1e3)
                    res, bn = s.true_residual()
                    print(f"{n:>4} {name:<36} {knob:>8} {st.inner_iters / max(st.precond_applies, 1):>11.1f} {st.inner_iters:>6} {st.fgmres_iters:>6} "
                          f"{statistics.median(ts):>9.2f} {t_b if knob else float('nan'):>8.3f} {info[2] if knob else 0:>6} {res / bn:>9.2e}", flush=True)
            finally:
                s.close()


def np_info(s):
    out = (C.c_int64 * 4)()
    if s.L.ifem_test_uu_patch_info(s.ctx, out) != 0:
        raise RuntimeError(s.L.ifem_last_error().decode())
    return list(out)


if __name__ == "__main__":
    main()
