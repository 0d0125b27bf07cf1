"""y = S_m x from lattice stencil tables on uniform box levels (csrc/sm_stencil.hip) through the test aid ifem_test_sm_apply, and through
ifem_solve with the captured V-cycle.

Reference: S = B diag(M_u)^-1 B^T from the CSR exports (which 0: B and B^T as assembled, which 1: diag(M_u)), scipy fp64, and path 0 of the
aid (the fp64 CSR product of the assembled S_m).  Bound for both comparisons: max|y - y_ref| <= 1e-12 max|S x|.  The table entries are
copies of assembled entries; rows of one class differ by the rounding of the assembly's atomic order (a few 1e-16 relative) and are held to
1e-12 of their class by the build, so the 5^dim-term sums agree to about 125 x 1e-12 / sqrt(125) of an entry times |x| at worst and to a few
1e-16 in practice.  The achieved value is printed.
Shapes: axes with fewer than five nodes (signature collisions, clipped stencils, tiles larger than the lattice), every axis longer than one
tile in turn, 2D, Q1 velocity, random and Morton node orders, anisotropic cells."""
import ctypes as C

import numpy as np
import pytest

from boxmesh import BoxMesh
from partmesh import partition_mesh, run_virtual_ranks

pytestmark = pytest.mark.gpu

KW = dict(mu=0.7, rho=1.3, gamma=0.2, dt=0.01)
BOUND = 1e-12
EXTENT = (2.0, 0.2, 0.2)


def _capi():
    from openifem_amd import capi
    return capi


def _bcs(dim, outflow=False):
    """the channel's constraint set: inflow face and walls, outflow free (outflow=True: every face)"""
    flag = 3 if dim == 2 else 7
    bcs = {0: (flag, [0.3, -0.2, 0.1][:dim]), 2: (flag, [0.0] * dim), 3: (flag, [0.0] * dim)}
    if dim == 3:
        bcs.update({4: (flag, [0.0] * dim), 5: (flag, [0.0] * dim)})
    if outflow:
        bcs[1] = (flag, [0.0] * dim)
    return bcs


def _set_and_assemble(ctx, m, dofs, vals, rng):
    capi = _capi()
    ctx.set_constraints(0, dofs, None)
    ctx.set_constraints(1, dofs, vals)
    ctx.vec_set(capi.VEC_PRESENT, rng.standard_normal(m.n_dofs))
    ctx.vec_set(capi.VEC_EVAL, rng.standard_normal(m.n_dofs))
    ctx.assemble(capi.make_params(**KW), False)


def _assembled(m, seed, cell_pnodes=None, hanging=False, dofs=None, vals=None):
    capi = _capi()
    rng = np.random.default_rng(seed)
    if dofs is None:
        dofs, vals = m.dirichlet(_bcs(m.dim))
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes if cell_pnodes is None else cell_pnodes, m.cell_face_bid,
                       m.n_unodes, m.n_pnodes)
    if hanging:
        ctx.set_hanging_constraints(m.hang_dof, m.hang_ptr, m.hang_master, m.hang_weight)
    _set_and_assemble(ctx, m, dofs, vals, rng)
    return ctx, rng


def _schur(ctx, n_u):
    """S = B diag(M_u)^-1 B^T of the context from the exports, scipy fp64"""
    A, M = ctx.export_csr(0), ctx.export_csr(1)
    B, Bt = A[n_u:, :n_u], A[:n_u, n_u:]
    d = M[:n_u, :n_u].diagonal()
    dinv = np.where(d != 0, 1.0 / np.where(d != 0, d, 1.0), 0.0)
    import scipy.sparse as sp
    return (B @ sp.diags(dinv) @ Bt).tocsr()


def _schur_from_rows(ctx, n_u, n_p):
    """the same from the pressure rows alone (a context that keeps no A_uu: B^T is the transpose of the masked B)"""
    import scipy.sparse as sp
    rp, col, val = ctx.export_rows(n_u, n_p, 0)
    B = sp.csr_matrix((val, col, rp), shape=(n_p, n_u + n_p))[:, :n_u]
    rp, col, val = ctx.export_rows(0, n_u, 1)
    d = sp.csr_matrix((val, col, rp), shape=(n_u, n_u + n_p))[:, :n_u].diagonal()
    dinv = np.where(d != 0, 1.0 / np.where(d != 0, d, 1.0), 0.0)
    return (B @ sp.diags(dinv) @ B.T).tocsr()


def _check(ctx, S, xs, tag, stencil=True, scale_by_terms=False):
    """both paths of the aid against the reference for every x; returns the info of the last default-path call.  scale_by_terms: S x
    vanishes (the constant vector under the singular S_m), the bound is taken against max_i sum_j |S_ij x_j|, what the rounding scales with"""
    info = None
    for name, x in xs:
        y1, info = ctx.sm_apply(1, x)
        y0, _ = ctx.sm_apply(0, x)
        ref = S @ x
        scale = (abs(S) @ np.abs(x)).max() if scale_by_terms else np.abs(ref).max()
        e_ref, e_csr = np.abs(y1 - ref).max() / scale, np.abs(y1 - y0).max() / scale
        print(f"{tag}, {name}: stencil {int(info[0])}, classes {int(info[1])}, irregular rows {int(info[2])}, table {int(info[3])} B, "
              f"max|y - S x| / max|S x| = {e_ref:.2e}, against the CSR product {e_csr:.2e}")
        assert bool(info[0]) == stencil
        assert e_ref <= BOUND and e_csr <= BOUND
        if not stencil:
            assert np.array_equal(y1, y0)
    return info


def _xs(rng, n, nodes=()):
    out = [("random", rng.standard_normal(n))]
    for k, nd in enumerate(nodes):
        e = np.zeros(n)
        e[nd] = 1.0
        out.append((f"unit vector {k}", e))
    return out


def _box_case(reps, p0, p1, kv, seed, tag, perm=False, units=False):
    m = BoxMesh(reps, p0, p1, kv=kv)
    rng = np.random.default_rng(2000 + seed)
    cp, node = None, np.arange(m.n_pnodes)
    if perm:
        node = rng.permutation(m.n_pnodes)
        cp = node[m.cell_pnodes].astype(np.int32)
    ctx, _ = _assembled(m, seed, cell_pnodes=cp)
    S = _schur(ctx, m.n_u)
    assert S.shape == (m.n_pnodes, m.n_pnodes)
    info = _check(ctx, S, _xs(rng, m.n_pnodes, (node[0], node[m.n_pnodes // 2], node[-1]) if units else ()), tag)
    assert info[2] == 0  # the channel's constraint set leaves no row outside its class
    assert 1 <= info[1] <= 5 ** m.dim and info[3] > 0
    ctx.close()


def test_three_counts_three_edges_and_an_origin_off_zero():
    _box_case((5, 3, 2), (0.3, -0.1, 0.2), (2.3, 0.2, 0.9), 2, 1, "5 x 3 x 2", units=True)


@pytest.mark.parametrize("reps", [(4, 1, 3), (1, 1, 1)])
def test_axes_of_two_nodes(reps):
    _box_case(reps, (0.3, -0.1, 0.2), (2.3, 0.2, 0.9), 2, 2, f"{reps}", units=True)


@pytest.mark.parametrize("reps", [(70, 2, 2), (2, 70, 2), (2, 2, 70)])
def test_more_than_one_tile_on_each_axis(reps):
    _box_case(reps, (0.0, 0.0, 0.0), tuple(0.05 * r for r in reps), 2, 3, f"{reps}")


@pytest.mark.parametrize("reps,kv", [((7, 4), 2), ((70, 3), 2), ((2, 3, 2), 1)])
def test_two_dimensions_and_q1_velocity(reps, kv):
    dim = len(reps)
    _box_case(reps, (0.1, -0.2, 0.3)[:dim], (1.5, 0.6, 1.1)[:dim], kv, 4, f"{dim}D Q{kv} {reps}", units=True)


def test_random_renumbering_of_the_pressure_nodes():
    _box_case((4, 3, 5), (0.3, -0.1, 0.2), (2.3, 0.2, 0.9), 2, 5, "4 x 3 x 5, pressure nodes renumbered", perm=True, units=True)


def test_anisotropic_cells():
    _box_case((6, 5, 9), (0.0, 0.0, 0.0), (3.0, 0.25, 1.8), 2, 6, "6 x 5 x 9, h = 0.5 x 0.05 x 0.2")


def test_morton_ordered_mirror_and_every_level_of_its_chain():
    """the 16 x 8 x 8 channel through the host mirror (Morton order, multigrid levels attached): after one solve every level has its S_m"""
    from openifem_amd import capi, host
    s = host.InsIM(host.channel_prm(3), (16, 8, 8), (0, 0, 0), EXTENT)
    s.setup(0)
    s.channel_state()
    s.assemble(False)
    s.solve(False)
    levels = [((16, 8, 8), s.ctx)] + s.mg_levels()
    assert len(levels) >= 2  # (the mirror stops coarsening this mesh at 16 x 4 x 4)
    rng = np.random.default_rng(7)
    for reps, h in levels:
        n_un, n_pn = int(np.prod([2 * r + 1 for r in reps])), int(np.prod([r + 1 for r in reps]))
        ctx = capi.Context.borrow(h, 3, 2, n_un, n_pn)
        info = _check(ctx, _schur_from_rows(ctx, 3 * n_un, n_pn), _xs(rng, n_pn), f"mirror level {tuple(reps)}")
        assert info[2] == 0
    s.close()


# ---- constraint sets

def _mesh654():
    return BoxMesh((6, 5, 4), (0.3, -0.1, 0.2), (2.3, 0.9, 1.0), kv=2)


def test_all_faces_dirichlet_singular_schur_block():
    m = _mesh654()
    dofs, vals = m.dirichlet(_bcs(3, outflow=True))
    ctx, rng = _assembled(m, 11, dofs=dofs, vals=vals)
    S = _schur(ctx, m.n_u)
    info = _check(ctx, S, _xs(rng, m.n_pnodes, (0,)), "every face Dirichlet")
    assert info[2] == 0
    one = np.ones(m.n_pnodes)
    assert np.abs(S @ one).max() <= 1e-12 * (abs(S) @ one).max()  # singular: the constants are its kernel
    _check(ctx, S, [("constant", one)], "every face Dirichlet", scale_by_terms=True)
    ctx.close()


def test_one_interior_velocity_node_constrained_gives_irregular_rows():
    m = _mesh654()
    dofs, vals = m.dirichlet(_bcs(3))
    nd = np.nonzero(np.all(m.unode_lattice == np.array((5, 5, 4)), axis=1))[0]
    assert len(nd) == 1
    extra = 3 * int(nd[0]) + np.arange(3)
    assert not set(extra) & set(dofs)
    dofs, vals = np.concatenate([dofs, extra]).astype(np.int32), np.concatenate([vals, np.zeros(3)])
    ctx, rng = _assembled(m, 12, dofs=dofs, vals=vals)
    info = _check(ctx, _schur(ctx, m.n_u), _xs(rng, m.n_pnodes), "one interior velocity node constrained")
    assert 0 < info[2] <= 27  # at most the pressure nodes of the cells around the node
    ctx.close()


def test_random_constrained_dofs_beyond_the_cap_keep_the_csr_product():
    m = _mesh654()
    rng0 = np.random.default_rng(13)
    dofs = np.nonzero(rng0.random(m.n_u) < 0.3)[0].astype(np.int32)
    ctx, rng = _assembled(m, 13, dofs=dofs, vals=np.zeros(len(dofs)))
    info = _check(ctx, _schur(ctx, m.n_u), _xs(rng, m.n_pnodes), "30 % random constrained dofs", stencil=False)
    assert not info.any()
    ctx.close()


def test_reformed_schur_block_rebuilds_the_tables():
    m = _mesh654()
    ctx, rng = _assembled(m, 14)
    x = rng.standard_normal(m.n_pnodes)
    S0 = _schur(ctx, m.n_u)
    _check(ctx, S0, [("channel set", x)], "before the change")
    dofs, vals = m.dirichlet(_bcs(3, outflow=True))
    _set_and_assemble(ctx, m, dofs, vals, rng)
    S1 = _schur(ctx, m.n_u)
    assert np.abs((S1 - S0) @ x).max() > 1e-3 * np.abs(S0 @ x).max()  # the matrix did change
    _check(ctx, S1, [("every face", x)], "after the change")
    ctx.close()


def test_switching_the_path_off_and_on():
    m = _mesh654()
    ctx, rng = _assembled(m, 15)
    S = _schur(ctx, m.n_u)
    xs = _xs(rng, m.n_pnodes)
    _check(ctx, S, xs, "default")
    _, info = ctx.sm_apply(2)
    assert not info.any()
    _check(ctx, S, xs, "switched off", stencil=False)
    _, info = ctx.sm_apply(3)
    _check(ctx, S, xs, "switched on again")
    ctx.close()


# ---- not eligible: the CSR product as before

def test_moved_vertex_keeps_the_csr_product():
    m = BoxMesh((3, 2, 2), (0, 0, 0), EXTENT, kv=2)
    h = np.array(EXTENT) / np.array((3, 2, 2))
    m.vcoords = m.vcoords.copy()
    hit = np.all(np.abs(m.vcoords - h) < 1e-9 * h, axis=2)
    assert hit.sum() == 8
    m.vcoords[hit] += 1e-6 * h
    ctx, rng = _assembled(m, 16)
    assert not ctx.mf_uniform()[0]
    _check(ctx, _schur(ctx, m.n_u), _xs(rng, m.n_pnodes), "one vertex moved by 1e-6 h", stencil=False)
    ctx.close()


def test_hanging_node_mesh_keeps_the_csr_product():
    from hangmesh import HangingMesh
    m = HangingMesh((2, 2, 2), (0, 0, 0), (1.0, 0.8, 0.6), {(0, 0, 0)}, kv=2)
    capi = _capi()
    rng = np.random.default_rng(17)
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    ctx.set_hanging_constraints(m.hang_dof, m.hang_ptr, m.hang_master, m.hang_weight)
    ctx.vec_set(capi.VEC_PRESENT, rng.standard_normal(m.n_dofs))
    ctx.vec_set(capi.VEC_EVAL, rng.standard_normal(m.n_dofs))
    ctx.assemble(capi.make_params(**KW), False)
    # (the exported B carries the hanging rows as the assembly treats them; the product the solves use is the assembled S_m's either way)
    x = rng.standard_normal(m.n_pnodes)
    y1, info = ctx.sm_apply(1, x)
    y0, _ = ctx.sm_apply(0, x)
    assert not info.any() and np.array_equal(y1, y0) and np.isfinite(y0).all() and np.abs(y0).max() > 0
    ctx.close()


def test_two_virtual_ranks_keep_the_csr_product():
    """two virtual ranks of the 4 x 2 x 2 box: the collective path 1 of the aid forms S_m as a solve on the ranks would (sm_ensure, sm_apply: the
    distributed product) and the gathered result is the S x of the whole mesh, within the bound of the single-rank cases; the stencil path is
    not in use on either rank, also after path 3"""
    capi = _capi()
    m = BoxMesh((4, 2, 2), (0, 0, 0), EXTENT, kv=2)
    rng = np.random.default_rng(18)
    dofs, vals = m.dirichlet(_bcs(3))
    ev, pr, x = rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_pnodes)
    from partmesh import local_dirichlet
    parts = partition_mesh(m, (m.vcoords.mean(axis=1)[:, 0] > 1.0).astype(int), 2)

    def work(rank, P, ctx):
        ld, lv = local_dirichlet(P, dofs, vals)
        ctx.set_constraints(0, ld, None)
        ctx.set_constraints(1, ld, lv)
        ctx.vec_set(capi.VEC_PRESENT, pr[P.ext_gdof])
        ctx.vec_set(capi.VEC_EVAL, ev[P.ext_gdof])
        ctx.assemble(capi.make_params(**KW), False)
        y, info = ctx.sm_apply(1, x[P.owned_p])
        with pytest.raises(capi.IfemError):
            ctx.sm_apply(0, x[P.owned_p])  # the CSR product of the aid is single-rank
        return y, info.copy(), ctx.sm_apply(3)[1].copy()

    out = run_virtual_ranks(capi, parts, work)
    one, _ = _assembled(m, 18)  # the same mesh on one rank: the reference S, and there the stencil path is taken
    S = _schur(one, m.n_u)
    _check(one, S, [("one rank", x)], "4 x 2 x 2 on one rank")
    one.close()
    ref, y = S @ x, np.full(m.n_pnodes, np.nan)
    for P, (yr, info, info3) in zip(parts, out):
        assert not info.any() and not info3.any()
        y[P.owned_p] = yr
    err = np.abs(y - ref).max() / np.abs(ref).max()
    print(f"two virtual ranks: max|y - S x| / max|S x| = {err:.2e}")
    assert err <= BOUND


# ---- through ifem_solve: the captured V-cycle

@pytest.mark.parametrize("fp64,bound", [(True, 1e-9), (False, 1e-6)])
def test_captured_cycle_on_the_mirror_hierarchy(capfd, fp64, bound):
    """16^3 mirror chain: the second solve replays the captured S_m V-cycle, the third runs with the stencil path switched off on every level.
    The three solves are made the same solve: ifem_solver_opts::inner_rel_first = 0 (with it the context remembers whether the tight first
    inner solve paid, and the second solve of a context differs from its first by 8.7e-4 of the largest entry on either path).
    fp64: stored A_uu and IFEM_AINV_GMRES_BJACOBI, the kind under which the CSR product of S_m streams its fp64 values -- both paths then differ
    by the order of their sums only and the updates must agree to 1e-9 (measured: 0 replayed, 4.8e-15 switched off).
    The mirror's defaults (IFEM_AINV_MG): the path switched off streams single-precision copies of the values, 6e-8 per product; the bound is
    the 1e-6 of the largest entry of the inner stopping rules (measured: 0 replayed, 7.5e-7 switched off)."""
    from openifem_amd import capi, multigpu
    s, _, _ = multigpu.make_channel_solver(16, 0, 1, 0, None, multigrid=True)
    if fp64:
        tun = capi.Tuning()
        s.L.ifem_default_tuning(C.byref(tun))
        tun.stored_uu = 1
        for c in s.all_ctxs():
            assert s.L.ifem_set_tuning(c, C.byref(tun)) == 0
        s.opts.ainv_kind = capi.AINV_GMRES_BJACOBI
    s.opts.inner_rel_first = 0.0
    s.channel_state()
    s.assemble(False)
    _, n_u, n_p = s.sizes()
    info = np.zeros(4, np.int64)

    def solve():
        st = s.solve(False)
        x = np.zeros(n_u + n_p)
        assert s.L.ifem_vec_get(s.ctx, capi.VEC_UPDATE, x.ctypes.data_as(C.c_void_p)) == 0
        return x, (st.cg_sm_iters, st.sm_mg_levels, st.fgmres_iters)

    def graph():
        return capi.vcycle_graph_stats(s.L, s.ctx)  # (captures, launches) of the context's captured cycles, the S_m V-cycle among them

    runs, g = [solve()], [graph()]
    runs.append(solve())
    g.append(graph())
    # the first solve armed and captured the S_m cycle (two CG iterations or more see the same key); the second one only replays
    assert g[0][0] >= 1 and g[1][0] == g[0][0] and g[1][1] > g[0][1]
    for c in s.all_ctxs():
        assert s.L.ifem_test_sm_apply(c, 3, None, None, info.ctypes.data_as(C.c_void_p)) == 0
        assert info[0] == 1 and info[2] == 0
        assert s.L.ifem_test_sm_apply(c, 2, None, None, info.ctypes.data_as(C.c_void_p)) == 0
        assert info[0] == 0
    runs.append(solve())
    g.append(graph())
    assert g[2][0] > g[1][0] and g[2][1] > g[1][1]  # another product: captured anew, and replayed
    scale = np.abs(runs[0][0]).max()
    d01, d02 = np.abs(runs[1][0] - runs[0][0]).max() / scale, np.abs(runs[2][0] - runs[0][0]).max() / scale
    with capfd.disabled():
        print(f"fp64 {fp64}: (cg_sm_iters, sm_mg_levels, fgmres_iters): {[r[1] for r in runs]}; updates against the first solve: replayed {d01:.3e}, "
              f"stencil path off {d02:.3e} of the largest entry")
    assert runs[0][1] == runs[1][1] == runs[2][1] and runs[0][1][0] > 0 and runs[0][1][1] >= 2
    assert d01 <= bound and d02 <= bound
    s.close()
