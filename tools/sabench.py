"""What the Spalart-Allmaras kernels cost (csrc/sa.hip, csrc/sa_wall.hip): per-launch time of k_sa_assemble, of the wall-distance kernels with
the wall faces of a channel, of the moving-wall update beside the fixed-wall kernel at the same point count, and the per-iteration cost of one
S-A solve, each beside its algorithmic bytes and the resulting share of the HBM
rate.  Measurements to be written down (profiles/sa_model.txt, profiles/sa_wall_function.txt), not thresholds; needs a GPU.

    python tools/sabench.py --cells 64 --kv 2 --reps 5

The times come from the library's own event pairs (ifem_kprof_begin / ifem_kprof_end: one pair per launch wrapper on the context
stream) and, for the solve, from a host clock around the call, which ends in a stream synchronise."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 6.29e12  # measured streaming rate of an MI355X (float4 copy); the spec is 8.0e12


def _timed(capi, L, ctx, reps, call):
    call()  # warm-up
    assert L.ifem_kprof_begin(ctx.h) == 0
    for _ in range(reps):
        call()
    k = capi.kprof_end(L, ctx.h)
    return (k["other"]["ms"] if "other" in k else sum(v["ms"] for v in k.values())) / reps


def moving_wall_leg(capi, L, ctx, m, P, wall, nw, reps, kv):
    """ifem_sa_update_moving_wall_distance (csrc/sa_wall.hip::k_sa_moving_wall) with nw wall vertices, beside k_sa_wall_distance with the same
    number of points in the same job: on the 3D box a point cloud (the vertex loop: distance + the u_tau payload), and on a 2D box with about as
    many nodes a closed nw-gon (the edge loop with its division and square root, then the vertex loop)"""
    import sa_wall_ref
    from boxmesh import BoxMesh
    rng = np.random.default_rng(11)
    res = {"wall_vertices": nw}
    # 3D: a point cloud in the middle of the channel; one solid cell, which the point location of the FSI side wants
    pts = np.array([2.0, 0.5, 0.5]) + 0.3 * rng.uniform(-1, 1, (nw, 3))
    ctx.fsi_set_solid(pts, np.arange(8, dtype=np.int32)[None, :], None)
    ctx.sa_set_moving_wall(capi.SaWall.make(rng.permutation(nw).astype(np.int32), np.zeros((nw, 3)), None, 0.02, 0.1))
    ctx.sa_set_shear_velocities(0.05 + 0.01 * rng.uniform(size=nw))
    nn = m.n_unodes
    ms = _timed(capi, L, ctx, reps, lambda: L.ifem_sa_update_moving_wall_distance(ctx.h, P, None, None))
    ctx.sa_set_moving_wall(None)
    ms_fixed = _timed(capi, L, ctx, reps, lambda: ctx.sa_set_wall_points(pts))
    ctx.sa_set_wall_points(wall)  # the channel's walls again, for the legs that follow
    res["box3d"] = {"nodes": nn, "pairs": nn * nw, "ms": ms, "pairs_per_s": nn * nw / (ms * 1e-3),
                    "k_sa_wall_distance_ms": ms_fixed, "k_sa_wall_distance_pairs_per_s": nn * nw / (ms_fixed * 1e-3)}
    # 2D: (n1 - 1) / kv cells per direction give n1^2 ~ nn nodes
    n1 = int(round(nn ** 0.5))
    c = (n1 - 1) // kv
    m2 = BoxMesh((c, c), (0, 0), (1.2, 1.2), kv=kv)
    c2 = capi.Context(2, kv, m2.vcoords, m2.cell_unodes, m2.cell_pnodes, m2.cell_face_bid, m2.n_unodes, m2.n_pnodes)
    s = sa_wall_ref.polygon_solid(nw, centre=(0.5713, 0.6091))
    vertex, normal, edges = sa_wall_ref.polygon_wall(s, rng)
    ms_fixed = _timed(capi, L, c2, reps, lambda: c2.sa_set_wall_points(s.vertices[vertex]))
    c2.fsi_set_solid(s.vertices, s.cells, s.bfaces)
    c2.sa_set_moving_wall(capi.SaWall.make(vertex, normal, edges, 0.02, 0.1))
    c2.sa_set_shear_velocities(0.05 + 0.01 * rng.uniform(size=nw))
    ms = _timed(capi, L, c2, reps, lambda: L.ifem_sa_update_moving_wall_distance(c2.h, P, None, None))
    pairs = m2.n_unodes * 2 * nw  # every node meets nw edges and nw vertices
    res["box2d"] = {"nodes": m2.n_unodes, "pairs": pairs, "ms": ms, "pairs_per_s": pairs / (ms * 1e-3),
                    "k_sa_wall_distance_ms": ms_fixed, "k_sa_wall_distance_pairs_per_s": m2.n_unodes * nw / (ms_fixed * 1e-3)}
    c2.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=64, help="cells per direction of the box")
    ap.add_argument("--kv", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="timed launches of each kernel")
    ap.add_argument("--solve", type=int, default=1, help="0: skip the solve (exact ILU(0) substitution runs in one workgroup)")
    ap.add_argument("--wall-vertices", type=int, default=4096, help="wall vertices of the moving-wall leg (0: skip it)")
    args = ap.parse_args()
    from openifem_amd import capi
    from boxmesh import BoxMesh
    import sa_ref
    L = capi.load()
    if L.ifem_device_count() == 0:
        raise SystemExit("sabench needs a GPU: there is no CPU fallback")
    n = args.cells
    m = BoxMesh((n, n, n), (0, 0, 0), (4.0, 1.0, 1.0), kv=args.kv)
    nn = m.n_unodes
    H = 1.0
    y = m.unode_coords[:, 1]
    fluid = np.zeros(3 * nn + m.n_pnodes)
    fluid[0:3 * nn:3] = 4.0 * y * (H - y) / H ** 2
    mu, rho, dt = 1e-3, 1.0, 1e-2
    wall = sa_ref.boundary_vertices(m, (2, 3))  # the two walls of the channel
    nodes = np.unique(np.concatenate([sa_ref.boundary_nodes(m, b) for b in (0, 2, 3)])).astype(np.int32)
    on_inflow = np.isin(nodes, sa_ref.boundary_nodes(m, 0))
    vals = np.where(on_inflow, 5 * mu / rho, 0.0)
    nu0 = np.full(nn, 3 * mu / rho)
    nu0[nodes] = 0.0
    ctx = capi.Context(3, args.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, nn, m.n_pnodes)
    ctx.vec_set(capi.VEC_PRESENT, fluid)
    ctx.sa_set_constraints(0, nodes, None)
    ctx.sa_set_constraints(1, nodes, vals)
    ctx.sa_vec_set(capi.SA_PRESENT, nu0)
    ctx.sa_vec_set(capi.SA_EVAL, nu0)
    P = capi.SaParams(mu, rho, dt)
    nnz = int(L.ifem_nnz(ctx.h, 0))  # blocks of A_uu = entries of the scalar matrix
    out = {"cells": m.n_cells, "nodes": nn, "kv": args.kv, "nnz": nnz, "wall_points": len(wall)}

    print(f"[sabench] context ready: {m.n_cells} cells, {nn} nodes, {nnz} matrix entries", file=sys.stderr, flush=True)
    ctx.sa_set_wall_points(wall)  # warm-up of both paths
    ctx.sa_assemble(P, True)
    assert L.ifem_kprof_begin(ctx.h) == 0
    for _ in range(args.reps):
        ctx.sa_set_wall_points(wall)
    k = capi.kprof_end(L, ctx.h)
    ms = k["other"]["ms"] / args.reps if "other" in k else sum(v["ms"] for v in k.values()) / args.reps
    by = nn * (3 + 1) * 8 + len(wall) * 3 * 8  # node points read, distances written, wall points once per workgroup tile (L2)
    out["wall_distance"] = {"ms": ms, "bytes": by, "hbm_share": by / (ms * 1e-3) / HBM_BYTES_PER_S,
                            "pair_distances_per_s": nn * len(wall) / (ms * 1e-3), "families": k}

    assert L.ifem_kprof_begin(ctx.h) == 0
    for _ in range(args.reps):
        ctx.sa_assemble(P, True)
    k = capi.kprof_end(L, ctx.h)
    fam = {name.lower(): v for name, v in k.items()}
    asm = next(v for name, v in fam.items() if "assemble" in name)
    nu = (args.kv + 1) ** 3
    # values written (one 8-byte atomic per local entry lands in the nnz values) + tables read per cell: posUU, node ids, the
    # node data (fluid, two nu~, d, flag, inhomogeneity), vertices
    by = nnz * 8 + m.n_cells * (nu * nu * 2 + nu * (4 + 8 * 7) + 8 * 3 * 8)
    ms = asm["ms"] / args.reps
    out["k_sa_assemble"] = {"ms": ms, "bytes": by, "hbm_share": by / (ms * 1e-3) / HBM_BYTES_PER_S,
                            "atomics_per_s": m.n_cells * nu * nu / (ms * 1e-3), "families": k}

    if args.wall_vertices:
        out["moving_wall"] = moving_wall_leg(capi, L, ctx, m, P, wall, args.wall_vertices, args.reps, args.kv)
    print("[sabench] kernels timed", file=sys.stderr, flush=True)
    if args.solve:
        t0 = time.perf_counter()
        its, res = ctx.sa_solve(True)  # includes the ILU(0) analysis (host) and factorisation
        first = time.perf_counter() - t0
        print(f"[sabench] first solve {first:.1f} s, {its} iterations", file=sys.stderr, flush=True)
        ctx.sa_assemble(P, True)
        assert L.ifem_kprof_begin(ctx.h) == 0
        t0 = time.perf_counter()
        its, res = ctx.sa_solve(True)  # factorisation + iterations
        wall_s = time.perf_counter() - t0
        k = capi.kprof_end(L, ctx.h)
        # per iteration: the matrix once (values + 4-byte columns), the factors twice (L and U sweeps), ~2 (j + 1) basis vectors of
        # Gram-Schmidt with re-orthogonalisation at iteration j (taken at j = its / 2)
        by = nnz * 12 + 2 * nnz * 12 + (4 * (its / 2 + 1) + 6) * nn * 8
        out["solve"] = {"iterations": its, "residual": res, "first_call_s": first, "s": wall_s, "ms_per_iteration": wall_s * 1e3 / max(its, 1),
                        "bytes_per_iteration": by, "hbm_share": by / (wall_s / max(its, 1)) / HBM_BYTES_PER_S, "families": k}
    ctx.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
