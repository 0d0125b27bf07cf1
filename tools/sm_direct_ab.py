#!/usr/bin/env python
"""A/B of ifem_solver_opts::sm_mg = 1 (multigrid-preconditioned CG of S_m) against 2 (fast diagonalisation, csrc/sm_direct.hip) on the bench's
channel, built the way bench.py builds it (multigpu.make_channel_solver, InsIM and kind="InsIMEX").  bench.py has no flag for the option.

Every (solver, sm_mg) run is a fresh child process under its own time limit; 1 and 2 alternate, --runs each; the first child that ends
abnormally stops the whole run.  --cold adds the cold_step / new_constraint_set_step legs of bench.py (ifem_tuning::geo_cache = 0 / 2), three
steps each, so that a factor build paid on every step would show.

  python tools/sm_direct_ab.py --n 128                      # InsIM 20 steps after 5, InsIMEX 3 steps after its 2 assembling steps
  python tools/sm_direct_ab.py --n 128 --cold --solvers insim
One JSON line per child on stdout, then a summary."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(st):
    return {"fgmres": st.fgmres_iters, "inner": st.inner_iters, "cg_sm": st.cg_sm_iters, "cg_mp": st.cg_mp_iters, "sm_mg_levels": st.sm_mg_levels,
            "t_cg_sm_ms": st.t_cg_sm_ms, "t_ainv_ms": st.t_ainv_ms, "t_cg_mp_ms": st.t_cg_mp_ms, "t_solve_ms": st.t_total_ms}


def child(args):
    import numpy as np
    from openifem_amd import capi, multigpu
    kind = "InsIMEX" if args.solver == "insimex" else "InsIM"
    s, reps, _ = multigpu.make_channel_solver(args.n, 0, 1, 0, None, multigrid=True, kind=kind)
    _, n_u, n_p = s.sizes()
    s.opts.sm_mg = args.sm_mg
    s.opts.verbose = 1  # the first solve only: its lines say which path S_m took, the probe value and the host time of the factor build
    s.channel_state()
    out = {"solver": args.solver, "sm_mg": args.sm_mg, "n": args.n, "steps": args.steps, "warmup": args.warmup}
    if kind == "InsIMEX":
        assert s.L.ifem_vec_copy(s.ctx, capi.VEC_PRESENT, capi.VEC_EVAL) == 0
        s.run_one_step(True, True)
        s.opts.verbose = 0
        s.run_one_step(False, True)
        for _ in range(max(0, args.warmup - 2)):
            s.run_one_step(False, False)
        step = lambda: s.run_one_step(False, False)
        last = s.last_stats
    else:
        keep = {}

        def step():
            s.assemble(False)
            keep["st"] = s.solve(False)

        step()
        s.opts.verbose = 0
        for _ in range(max(0, args.warmup - 1)):
            step()
        last = lambda: keep["st"]
    if args.cold:
        tun = capi.Tuning()
        s.L.ifem_default_tuning(C.byref(tun))
        legs = {}
        for label, gc in (("cold_step", 0), ("new_constraint_set_step", 2)):
            tun.geo_cache = gc
            for c_ in s.all_ctxs():
                assert s.L.ifem_set_tuning(c_, C.byref(tun)) == 0
            step()
            s.synchronize()
            ms = []
            s.opts.verbose = 1  # (a factor build on any of these steps would say so)
            for _ in range(3):
                t0 = time.time()
                step()
                s.synchronize()
                ms.append((time.time() - t0) * 1e3)
            s.opts.verbose = 0
            legs[label] = {"ms": ms, **_stats(last())}
        out["legs"] = legs
    else:
        s.synchronize()
        t0 = time.time()
        for _ in range(args.steps):
            step()
        s.synchronize()
        out["ms_per_step"] = (time.time() - t0) / args.steps * 1e3
        out.update(_stats(last()))
        r, b = s.true_residual()
        out["true_rel_residual"] = r / b if b > 0 else None
    # the aid on the finest level: which path its S_m solve takes now, the probe value of its factors and their size
    ctx = capi.Context.borrow(s.ctx, 3, 2, n_u // 3, n_p)
    o = capi.SolverOpts.from_buffer_copy(s.opts)
    _, info = ctx.sm_solve(np.random.default_rng(1).standard_normal(n_p), o)
    out["aid"] = {"direct": int(info[0]), "cg_iters": int(info[1]), "probe": info[2] * 1e-18, "table_bytes": int(info[3])}
    print("SMDAB " + json.dumps(out), flush=True)
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--solvers", default="insim,insimex")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--cold", action="store_true")
    ap.add_argument("--limit", type=int, default=240, help="time limit of one child in seconds")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--solver", default="insim")
    ap.add_argument("--sm-mg", type=int, default=1)
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = []
    for solver in args.solvers.split(","):
        steps = args.steps if args.steps is not None else (20 if solver == "insim" else 3)
        warmup = args.warmup if args.warmup is not None else (5 if solver == "insim" else 2)
        for run in range(args.runs):
            for mode in (1, 2):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--solver", solver, "--sm-mg", str(mode), "--n", str(args.n), "--steps", str(steps),
                       "--warmup", str(warmup)] + (["--cold"] if args.cold else [])
                try:
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
                except subprocess.TimeoutExpired:
                    print(f"STOP: {solver} sm_mg {mode} run {run} exceeded its {args.limit} s", flush=True)
                    return 2
                line = [l for l in p.stdout.splitlines() if l.startswith("SMDAB ")]
                if p.returncode != 0 or not line:
                    print(f"STOP: {solver} sm_mg {mode} run {run} ended with status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
                    return 2
                rec = json.loads(line[0][6:])
                rec["run"] = run
                rec["sm_lines"] = [l for l in p.stderr.splitlines() if "S_m solve" in l]
                m = re.search(r"last build ([0-9.]+) ms host", "\n".join(rec["sm_lines"]))
                rec["factor_build_host_ms"] = float(m.group(1)) if m else None
                results.append(rec)
                print(json.dumps(rec), flush=True)
    if not args.cold:
        for solver in args.solvers.split(","):
            for key in ("ms_per_step", "t_cg_sm_ms", "t_ainv_ms"):
                a = [r[key] for r in results if r["solver"] == solver and r["sm_mg"] == 1]
                b = [r[key] for r in results if r["solver"] == solver and r["sm_mg"] == 2]
                if a and b:
                    print(f"{solver} {key}: sm_mg 1 {['%.3f' % v for v in a]} median {sorted(a)[len(a) // 2]:.3f} | sm_mg 2 {['%.3f' % v for v in b]} "
                          f"median {sorted(b)[len(b) // 2]:.3f} | every 2 below every 1: {max(b) < min(a)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
