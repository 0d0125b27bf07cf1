#!/usr/bin/env python3
"""A/B of two builds of libifem_hip.so on the solver path: same cases, every case in a fresh child process per library (selected through
capi.LIB_PATH), counts and result arrays written per case, then compared.  Made for host-side restructurings of csrc/solver.hip, which must
not change a launch: see profiles/r10_solver_refactor.txt and profiles/solver_scaffolding_ab.txt for what can and cannot be equal bit for bit.

    tools/ab_solver.py run LIB_A LIB_B [--out DIR] [--runs-a 3] [--runs-b 1] [--cases REGEX] [--jobs 2] [--timeout 120]
    tools/ab_solver.py compare [DIR]
    tools/ab_solver.py list

run: DIR/a0 .. a<runs-a - 1> hold the runs of LIB_A (the parent), DIR/b0 .. those of LIB_B, one <case>.npz each (arrays, and the counts as JSON).
Children are started with subprocess, each under its own timeout, at most --jobs (two) at a time; a case on two virtual ranks is still one process.
The first child that ends abnormally (non-zero status, signal, timeout) stops the run: nothing more is started.
compare: per case -- counts equal or not (A runs among themselves, every A run against every B run), the largest difference of every array
relative to its largest entry for A/A, B/B and A/B, whether the velocity part of the first ifem_precond_vmult result is byte-equal, and the
lambda_max lines of the verbose case.

Fixture of the single-rank cases: the 16^3 bench channel with its three levels (tests/test_gpu_inner_f32.py), a fresh context per case;
three ifem_precond_vmult applications (eager, capture, replay) and two ifem_solve."""
import argparse
import ctypes as C
import itertools
import json
import os
import re
import subprocess
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_KEYS = ("fgmres_iters", "inner_iters", "cg_mp_iters", "cg_sm_iters", "precond_applies", "sm_mg_levels")


def _cases():
    """name -> (kind, settings); the order is the order of the run"""
    c = {}
    for name, kind in (("bjacobi", 0), ("bjacobi_f32", 1), ("bjacobi_mf", 3)):
        c[name] = ("channel", dict(ainv=kind))
    for maxit, f32, sm, graph in itertools.product((0, -2, None), (0, 1), (0, 1), (0, None)):
        name = f"mg_maxit{'D' if maxit is None else maxit}_f32{f32}_sm{sm}_graph{'D' if graph is None else graph}"
        c[name] = ("channel", dict(ainv=4, inner_maxit=maxit, inner_f32=f32, uu_smoother=sm, vcycle_graph_cells=graph))
    for f32, sm in itertools.product((0, 1), (0, 1)):
        c[f"mg_restart_f32{f32}_sm{sm}"] = ("channel", dict(ainv=4, inner_f32=f32, uu_smoother=sm, restart=True))
    c["mg_smoother_flip"] = ("flip", {})
    c["scnsim_cylinder"] = ("scns", {})
    for overlap, ainv in itertools.product((0, 1), (0, 4)):
        c[f"ranks2_overlap{overlap}_ainv{ainv}"] = ("ranks", dict(overlap=overlap, ainv=ainv))
    c["ranks2_explicit_schur"] = ("schur", {})
    c["mg_cold_then_warm"] = ("coldwarm", {})
    return c


# ---------------------------------------------------------------------------------------------------------------- the child: one case
def _tuning(s, capi, **kw):
    tun = capi.Tuning()
    s.L.ifem_default_tuning(C.byref(tun))
    for k, v in kw.items():
        if v is not None:
            setattr(tun, k, v)
    for ctx in s.all_ctxs():
        assert s.L.ifem_set_tuning(ctx, C.byref(tun)) == 0


def _get(s, vec, n):
    x = np.zeros(n)
    assert s.L.ifem_vec_get(s.ctx, vec, x.ctypes.data_as(C.c_void_p)) == 0
    return x


def _stats(st):
    return {k: int(getattr(st, k)) for k in COUNT_KEYS}


def _test_vector(n):
    g = np.arange(n)
    return np.cos(0.37 * g) + 0.1 * np.sin(1.3 * g)


def _precond(s, capi, v):
    ip = capi.make_params(mu=1.0, rho=1.0, gamma=0.1, dt=1e-3)
    assert s.L.ifem_vec_set(s.ctx, capi.VEC_TMP, v.ctypes.data_as(C.c_void_p)) == 0
    rc = s.L.ifem_precond_vmult(s.ctx, C.byref(ip), C.byref(s.opts), capi.VEC_UPDATE, capi.VEC_TMP)
    assert rc == 0, s.L.ifem_last_error().decode()
    return _get(s, capi.VEC_UPDATE, len(v))


def _channel16(capi):
    from openifem_amd import multigpu
    s, _, _ = multigpu.make_channel_solver(16, 0, 1, 0, None, multigrid=True)
    assert len(s.all_ctxs()) == 3
    s.channel_state()
    return s


def _case_channel(capi, ainv, inner_maxit=None, inner_f32=None, uu_smoother=None, vcycle_graph_cells=None, restart=False):
    s = _channel16(capi)
    s.opts.ainv_kind = ainv
    if inner_maxit is not None:
        s.opts.inner_maxit = inner_maxit
    if restart:  # GMRES(2) to 1e-6: several restart cycles, the context's restart length grows
        s.opts.inner_restart, s.opts.inner_rel, s.opts.inner_rel_first = 2, 1e-6, 0.0
    _tuning(s, capi, inner_f32=inner_f32, uu_smoother=uu_smoother, vcycle_graph_cells=vcycle_graph_cells)
    s.assemble(False)
    _, n_u, n_p = s.sizes()
    v = _test_vector(n_u + n_p)
    arrays, counts = {"n_u": np.array([n_u])}, {}
    for k in range(3):
        arrays[f"pv{k}"] = _precond(s, capi, v)
    counts["restart_length"] = int(s.L.ifem_inner_restart_length(s.ctx))
    counts["graph_after_vmult"] = list(capi.vcycle_graph_stats(s.L, s.ctx))
    for k in range(2):
        counts[f"solve{k}"] = _stats(s.solve(False))
        arrays[f"x{k}"] = _get(s, capi.VEC_UPDATE, n_u + n_p)
    counts["restart_length_end"] = int(s.L.ifem_inner_restart_length(s.ctx))
    counts["graph_end"] = list(capi.vcycle_graph_stats(s.L, s.ctx))
    s.close()
    return arrays, counts


def _case_flip(capi):
    """uu_smoother 0, 1, 0, 1 in turn on one context (one V-cycle per application), three applications each"""
    s = _channel16(capi)
    s.opts.ainv_kind = capi.AINV_MG
    s.opts.inner_maxit = 0
    s.assemble(False)
    _, n_u, n_p = s.sizes()
    v = _test_vector(n_u + n_p)
    arrays, counts = {"n_u": np.array([n_u])}, {}
    for turn, sm in enumerate((0, 1, 0, 1)):
        _tuning(s, capi, uu_smoother=sm)
        for k in range(3):
            arrays[f"pv{turn}_{k}" if turn or k else "pv0"] = _precond(s, capi, v)
    counts["turn0_equals_turn2"] = bool(all((arrays["pv0" if k == 0 else f"pv0_{k}"] == arrays[f"pv2_{k}"]).all() for k in range(3)))
    counts["turn1_equals_turn3"] = bool(all((arrays[f"pv1_{k}"] == arrays[f"pv3_{k}"]).all() for k in range(3)))
    counts["graph_end"] = list(capi.vcycle_graph_stats(s.L, s.ctx))
    s.close()
    return arrays, counts


def _case_scns(capi):
    """the SCnsIM solve of tests/test_gpu_scnsim.py::test_scns_solve_reaches_reference_tolerance (left-preconditioned gmres)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from cylmesh import CylinderMesh
    m = CylinderMesh(1, kv=1)

    def inflow(p, c):
        return 4 * 4.5 * p[1] * (0.41 - p[1]) / (0.41 * 0.41) if (c == 0 and abs(p[0]) < 1e-10) else 0.0

    dofs, vals = m.dirichlet({0: (3, [0.2, 0]), 2: (3, [0, 0]), 3: (3, [0, 0]), 4: (3, [0, 0])}, {0: inflow})
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    ctx.set_constraints(0, dofs, None)
    ctx.set_constraints(1, dofs, vals)
    ctx.scns_assemble(capi.make_scns_params(mu=1.8e-4, rho=1.3e-3, dt=1e-2), True)
    st = ctx.scns_solve(True)
    arrays = {"x0": ctx.vec_get(capi.VEC_UPDATE), "n_u": np.array([m.dim * m.n_unodes])}
    counts = {"solve0": _stats(st)}
    ctx.close()
    return arrays, counts


def _on_ranks(P, work):
    """work(rank, world_handle) on prod(P) virtual ranks (host threads over the in-process local world); the results by rank"""
    from openifem_amd import capi
    L = capi.load()
    world = int(np.prod(P))
    w = C.c_void_p(L.ifem_local_world_create(world))
    out, errs = [None] * world, []

    def run(rank):
        try:
            out[rank] = work(rank, w)
        except Exception:  # noqa
            import traceback
            errs.append((rank, traceback.format_exc()))

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise RuntimeError(str(errs))
    L.ifem_local_world_destroy(w)
    return out


def _owned_global(t, dim=3):
    nuo, npo = t["n_unodes_owned"], t["n_pnodes_owned"]
    gu = (t["l2g_u"][:nuo, None] * dim + np.arange(dim)[None, :]).ravel()
    return np.concatenate([gu, dim * t["n_unodes_global"] + t["l2g_p"][:npo]])


def _case_ranks(capi, overlap, ainv):
    """the default-tolerance solve of tests/test_gpu_multirank_local.py (8 x 4 x 4 cells on 2 x 1 x 1 virtual ranks; no multigrid levels
    below a context of the local world: plain CG(S_m), and with IFEM_AINV_MG the one-level cycle)"""
    from openifem_amd import host
    L, P, reps = capi.load(), (2, 1, 1), (8, 4, 4)

    def work(rank, w):
        s = host.InsIM(host.channel_prm(3), reps, (0, 0, 0), (2.0, 0.2, 0.2))
        s.set_partition(P, rank, local_world=w)
        s.setup(0)
        s.channel_state()
        assert L.ifem_halo_exchange(s.ctx, capi.VEC_EVAL) == 0
        s.opts.ainv_kind = ainv
        tun = capi.Tuning()
        L.ifem_default_tuning(C.byref(tun))
        tun.halo_overlap = overlap
        for ctx in s.all_ctxs():
            assert L.ifem_set_tuning(ctx, C.byref(tun)) == 0
        s.assemble(False)
        st = s.solve(False)
        t = s.partition_tables()
        n = 3 * t["n_unodes_owned"] + t["n_pnodes_owned"]
        res = (_owned_global(t), _get(s, capi.VEC_RHS, n), _get(s, capi.VEC_UPDATE, n), _stats(st), int(L.ifem_mg_depth(s.ctx)),
               int(L.ifem_inner_restart_length(s.ctx)), 3 * t["n_unodes_global"])
        s.close()
        return res

    out = _on_ranks(P, work)
    n = sum(len(o[0]) for o in out)
    rhs, upd = np.full(n, np.nan), np.full(n, np.nan)
    for g, r, u, *_ in out:
        rhs[g], upd[g] = r, u
    assert not np.isnan(rhs).any() and not np.isnan(upd).any()
    counts = {f"solve0_rank{r}": o[3] for r, o in enumerate(out)}
    counts["mg_depth"] = [o[4] for o in out]
    counts["restart_length"] = [o[5] for o in out]
    return {"x0": upd, "rhs": rhs, "n_u": np.array([out[0][6]])}, counts


def _case_schur(capi):
    """ifem_precond_vmult with the distributed explicit S_m (2-deep pressure halo) on 2 x 1 x 1 virtual ranks: the mesh and options of
    tests/test_gpu_multirank_local.py::test_distributed_explicit_schur_matches_single_context, smallest parameters"""
    from openifem_amd import host
    L, P, reps = capi.load(), (2, 1, 1), (8, 4, 4)

    def work(rank, w):
        s = host.InsIM(host.channel_prm(3), reps, (0, 0, 0), (2.0, 0.2, 0.2))
        s.set_partition(P, rank, local_world=w)
        s.setup(0)
        s.channel_state()
        assert L.ifem_halo_exchange(s.ctx, capi.VEC_EVAL) == 0
        s.opts.mp_rel = s.opts.sm_rel = 1e-13
        s.opts.inner_rel = 1e-11
        s.opts.inner_maxit = 6000
        s.opts.explicit_schur = 1
        s.assemble(False)
        t = s.partition_tables()
        g = _owned_global(t)
        z = _precond(s, capi, np.cos(0.37 * g) + 0.1 * np.sin(1.3 * g))
        s.close()
        return g, z, 3 * t["n_unodes_global"]

    out = _on_ranks(P, work)
    z = np.full(sum(len(o[0]) for o in out), np.nan)
    for g, zr, _ in out:
        z[g] = zr
    assert not np.isnan(z).any()
    return {"pv0": z, "n_u": np.array([out[0][2]])}, {}


def _case_coldwarm(capi):
    """the eigenvalue bounds, verbose: one context solved for constraint set 0 (cold estimates), for set 1, and once more after the
    evaluation point has grown by half (the warm estimates of every level).  The parent process keeps the lambda_max lines of stderr."""
    s = _channel16(capi)
    s.opts.ainv_kind = capi.AINV_MG
    s.opts.verbose = 1
    _, n_u, n_p = s.sizes()
    arrays, counts = {"n_u": np.array([n_u])}, {}
    for k, nonzero in enumerate((False, True, False)):
        if k == 2:
            ev = 1.5 * _get(s, capi.VEC_EVAL, n_u + n_p)
            assert s.L.ifem_vec_set(s.ctx, capi.VEC_EVAL, ev.ctypes.data_as(C.c_void_p)) == 0
        s.assemble(nonzero)
        counts[f"solve{k}"] = _stats(s.solve(nonzero))
        arrays[f"x{k}"] = _get(s, capi.VEC_UPDATE, n_u + n_p)
    s.close()
    return arrays, counts


def child(lib, case, out):
    sys.path.insert(0, ROOT)
    from openifem_amd import capi
    capi.LIB_PATH = os.path.abspath(lib)
    kind, kw = _cases()[case]
    fn = {"channel": _case_channel, "flip": _case_flip, "scns": _case_scns, "ranks": _case_ranks, "schur": _case_schur, "coldwarm": _case_coldwarm}[kind]
    arrays, counts = fn(capi, **kw)
    np.savez(out, counts=np.array(json.dumps(counts)), **arrays)


# ------------------------------------------------------------------------------------------------------------------------ the parent
LAMBDA_LINE = re.compile(r"A_uu V-cycle level (\d+) .*lambda_max estimate (\S+) \((warm|cold)\)")


def run(lib_a, lib_b, out, runs_a, runs_b, pattern, jobs, timeout):
    todo = [(f"{tag}{k}", lib, case) for case in _cases() if re.search(pattern, case)
            for tag, lib, runs in (("a", lib_a, runs_a), ("b", lib_b, runs_b)) for k in range(runs)]
    for tag, _, _ in todo:
        os.makedirs(os.path.join(out, tag), exist_ok=True)
    running, failed = [], None

    def reap(block):
        nonlocal failed
        for item in list(running):
            p, tag, case, path = item
            try:
                _, err = p.communicate(timeout=timeout if block else 0.2)
                rc = p.returncode
            except subprocess.TimeoutExpired:
                if not block:
                    continue
                p.kill()
                _, err = p.communicate()
                rc = "timeout"
            running.remove(item)
            lam = LAMBDA_LINE.findall(err or "")
            if lam:
                with open(path[:-4] + ".lambda.json", "w") as f:
                    json.dump(lam, f)
            print(f"{tag} {case}: {'ok' if rc == 0 else rc}", flush=True)
            if rc != 0 and failed is None:
                failed = (tag, case, rc, (err or "")[-3000:])
            block = False  # one blocking wait per call

    for tag, lib, case in todo:
        while len(running) >= jobs and failed is None:
            reap(True)
        if failed is not None:
            break
        path = os.path.join(out, tag, case + ".npz")
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "_child", lib, case, path], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                             text=True, cwd=ROOT)
        running.append((p, tag, case, path))
    while running:
        reap(True)
    if failed is not None:
        print(f"STOPPED at the first child that ended abnormally: {failed[0]} {failed[1]}: {failed[2]}\n{failed[3]}", flush=True)
        return 1
    return 0


def _load(path):
    z = np.load(path)
    return json.loads(str(z["counts"])), {k: z[k] for k in z.files if k != "counts"}


def _reldiff(a, b):
    if a.shape != b.shape:
        return float("inf")
    m = np.abs(a).max()
    return float(np.abs(a - b).max() / m) if m > 0 else float(np.abs(a - b).max())


def compare(out):
    tags = sorted(d for d in os.listdir(out) if re.fullmatch(r"[ab]\d+", d))
    A, B = [t for t in tags if t[0] == "a"], [t for t in tags if t[0] == "b"]
    aa, bb, ab = list(itertools.combinations(A, 2)), list(itertools.combinations(B, 2)), list(itertools.product(A, B))
    print(f"runs of A: {A}, of B: {B}; pairs A/A {len(aa)}, B/B {len(bb)}, A/B {len(ab)}")
    bad = 0
    for case in _cases():
        have = {t: _load(os.path.join(out, t, case + ".npz")) for t in tags if os.path.exists(os.path.join(out, t, case + ".npz"))}
        if len(have) < len(tags):
            print(f"{case}: missing in {sorted(set(tags) - set(have))}")
            continue
        counts_aa = all(have[x][0] == have[y][0] for x, y in aa)
        counts_ab = all(have[x][0] == have[y][0] for x, y in ab)
        names = [k for k in have[A[0]][1] if k != "n_u"]
        n_u = int(have[A[0]][1]["n_u"][0])
        d_aa, d_bb, d_ab = ({k: max([_reldiff(have[x][1][k], have[y][1][k]) for x, y in pairs], default=0.0) for k in names} for pairs in (aa, bb, ab))
        line = f"{case}: counts A/A {'equal' if counts_aa else 'UNEQUAL'}, A/B {'equal' if counts_ab else 'UNEQUAL'}"
        if "pv0" in names:
            vel = lambda t: have[t][1]["pv0"][:n_u].tobytes()  # noqa: E731
            v_aa, v_ab = all(vel(x) == vel(y) for x, y in aa), all(vel(x) == vel(y) for x, y in ab)
            n_ab, n_bb = sum(vel(x) == vel(y) for x, y in ab), sum(vel(x) == vel(y) for x, y in bb)
            line += f"; velocity part of the first P v byte-equal A/A {v_aa}, A/B {v_ab} ({n_ab} of {len(ab)} pairs; B/B {n_bb} of {len(bb)})"
            if v_aa and not v_ab:
                bad += 1
                line += "  <-- B CHANGES BYTES THAT A REPRODUCES"
        if not counts_ab:
            bad += 1
            for x, y in ab:
                if have[x][0] != have[y][0]:
                    line += f"\n    {x}: {have[x][0]}\n    {y}: {have[y][0]}"
                    break
        print(line)
        print(f"    counts of {A[0]}: {json.dumps(have[A[0]][0], separators=(',', ':'))}")
        for k in names:
            flag = ""
            if d_ab[k] > 2.0 * d_aa[k] and d_ab[k] > 0:
                flag = "  <-- A/B above twice A/A"
                bad += 1
            print(f"    {k:8s} largest difference / largest entry: A/A {d_aa[k]:.3e}   B/B {d_bb[k]:.3e}   A/B {d_ab[k]:.3e}{flag}")
        lam = {}
        for t in tags:
            p = os.path.join(out, t, case + ".lambda.json")
            if os.path.exists(p):
                lam[t] = json.load(open(p))
        if lam:
            same_a, same_b = all(lam.get(x) == lam.get(A[0]) for x in A), all(lam.get(x) == lam.get(A[0]) for x in B)
            print(f"    lambda_max lines (level, estimate, kind) of {A[0]}: {lam.get(A[0])}")
            print(f"    ... equal to all printed digits among A: {same_a}; A/B: {same_b}")
            if not (same_a and same_b):
                for t in tags[1:]:
                    print(f"    {t}: {lam.get(t)}")
                bad += 1 if same_a else 0
    print(f"{bad} finding(s) to explain" if bad else "nothing to explain: B differs from A by what A differs from itself")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("lib_a")
    r.add_argument("lib_b")
    r.add_argument("--out", default=os.path.join(ROOT, "build", "ab_solver"))
    r.add_argument("--runs-a", type=int, default=3)
    r.add_argument("--runs-b", type=int, default=1)
    r.add_argument("--cases", default=".")
    r.add_argument("--jobs", type=int, default=2, choices=(1, 2))
    r.add_argument("--timeout", type=float, default=120.0)
    c = sub.add_parser("compare")
    c.add_argument("out", nargs="?", default=os.path.join(ROOT, "build", "ab_solver"))
    sub.add_parser("list")
    k = sub.add_parser("_child")
    for a in ("lib", "case", "out"):
        k.add_argument(a)
    a = ap.parse_args()
    if a.cmd == "_child":
        child(a.lib, a.case, a.out)
        return 0
    if a.cmd == "list":
        print("\n".join(_cases()))
        return 0
    if a.cmd == "run":
        return run(a.lib_a, a.lib_b, a.out, a.runs_a, a.runs_b, a.cases, a.jobs, a.timeout)
    return compare(a.out)


if __name__ == "__main__":
    sys.exit(main())
