"""y = B x, y = B^T x and y += B^T x from lattice stencil tables on uniform box levels (csrc/bb_stencil.hip) through the test aid
ifem_test_b_apply, and through ifem_solve.

Reference: the exported blocks (ifem_export_csr: B and B^T as assembled) multiplied in numpy longdouble, and path 0 of the aid (the fp64 CSR
product of the assembled block).  Bound for all three products and both comparisons: max|y - y_ref| <= 1e-12 max|y|, the project's bound for
the S_m product.  The table entries are copies of assembled entries; rows of one class are held to 1e-12 of their class by the build, the sums
have at most 375 terms.  The achieved values are printed.
Shapes: axes of two pressure nodes (fewer than five velocity nodes: signature collisions, clipped windows, tiles larger than the lattice), every
axis longer than one tile of either kernel in turn, 2D, Q1 velocity (keeps the CSR products), random and Morton node orders, anisotropic cells."""
import ctypes as C

import numpy as np
import pytest

from boxmesh import BoxMesh
from partmesh import partition_mesh, run_virtual_ranks

pytestmark = pytest.mark.gpu

KW = dict(mu=0.7, rho=1.3, gamma=0.2, dt=0.01)
BOUND = 1e-12
EXTENT = (2.0, 0.2, 0.2)
NAMES = ("B x", "B^T x", "y + B^T x")


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


def _assembled(m, seed, dofs=None, vals=None, perm=False, tuning=None):
    """context of the mesh with the channel's constraint set (or dofs / vals), assembled; perm: velocity and pressure nodes renumbered at random"""
    capi = _capi()
    rng = np.random.default_rng(seed)
    if dofs is None:
        dofs, vals = m.dirichlet(_bcs(m.dim))
    cu, cp = m.cell_unodes, m.cell_pnodes
    if perm:
        pu, pp = rng.permutation(m.n_unodes), rng.permutation(m.n_pnodes)
        cu, cp = pu[cu].astype(np.int32), pp[cp].astype(np.int32)
        dofs = (m.dim * pu[dofs // m.dim] + dofs % m.dim).astype(np.int32)
    ctx = capi.Context(m.dim, m.kv, m.vcoords, cu, cp, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    if tuning:
        ctx.set_tuning(**tuning)
    _set_and_assemble(ctx, m, dofs, vals, rng)
    return ctx, rng


def _blocks(ctx, n_u):
    A = ctx.export_csr(0)
    return A[n_u:, :n_u].tocsr(), A[:n_u, n_u:].tocsr()


def _ld(M, x, y=None):
    """M x (+ y) in longdouble"""
    M = M.tocsr()
    prod = M.data.astype(np.longdouble) * np.asarray(x, np.longdouble)[M.indices]
    out = np.zeros(M.shape[0], np.longdouble) if y is None else np.asarray(y, np.longdouble).copy()
    np.add.at(out, np.repeat(np.arange(M.shape[0]), np.diff(M.indptr)), prod)
    return out


def _check(ctx, B, Bt, rng, tag, stencil=True):
    """the three products, both paths of the aid against the longdouble reference; returns the infos of the default-path calls [B, B^T, add]"""
    n_p, n_u = B.shape
    xu, xp, y_in = rng.standard_normal(n_u), rng.standard_normal(n_p), rng.standard_normal(n_u)
    infos = []
    for which, name in enumerate(NAMES):
        x, M = (xu, B) if which == 0 else (xp, Bt)
        yy = y_in if which == 2 else None
        y1, info = ctx.b_apply(which, 1, x, yy)
        y0, _ = ctx.b_apply(which, 0, x, yy)
        ref = _ld(M, x, yy)
        scale = float(np.abs(ref).max())
        e_ref, e_csr = float(np.abs(y1 - ref).max()) / scale, float(np.abs(y1 - y0).max()) / scale
        print(f"{tag}, {name}: stencil {int(info[0])}, classes {int(info[1])}, irregular rows {int(info[2])}, table {int(info[3])} B, "
              f"max|y - ref| / max|y| = {e_ref:.2e}, against the CSR product {e_csr:.2e}")
        assert bool(info[0]) == stencil
        assert e_ref <= BOUND and e_csr <= BOUND
        if not stencil:
            assert np.array_equal(y1, y0) and not info.any()
        infos.append(info.copy())
    return infos


def _box_case(reps, p0, p1, kv, seed, tag, perm=False, stencil=True):
    m = BoxMesh(reps, p0, p1, kv=kv)
    ctx, rng = _assembled(m, seed, perm=perm)
    B, Bt = _blocks(ctx, m.n_u)
    assert B.shape == (m.n_pnodes, m.n_u) and Bt.shape == (m.n_u, m.n_pnodes)
    infos = _check(ctx, B, Bt, rng, tag, stencil=stencil)
    if stencil:
        for info, cap in zip(infos, (5, 10, 10)):
            assert info[2] == 0  # the channel's constraint set leaves no row outside its class
            assert 1 <= info[1] <= cap ** m.dim and info[3] > 0
    ctx.close()


def test_three_counts_three_edges_and_an_origin_off_zero():
    _box_case((5, 3, 2), (0.3, -0.1, 0.2), (2.3, 0.2, 0.9), 2, 1, "5 x 3 x 2")


@pytest.mark.parametrize("reps", [(4, 1, 3), (1, 1, 1)])
def test_axes_of_two_pressure_nodes(reps):
    _box_case(reps, (0.3, -0.1, 0.2), (2.3, 0.2, 0.9), 2, 2, f"{reps}")


@pytest.mark.parametrize("reps", [(70, 2, 2), (2, 70, 2), (2, 2, 70)])
def test_more_than_one_tile_on_each_axis(reps):
    _box_case(reps, (0.0, 0.0, 0.0), tuple(0.05 * r for r in reps), 2, 3, f"{reps}")


@pytest.mark.parametrize("reps", [(7, 4), (70, 3)])
def test_two_dimensions(reps):
    _box_case(reps, (0.1, -0.2), (1.5, 0.6), 2, 4, f"2D Q2 {reps}")


def test_q1_velocity_keeps_the_csr_products():
    _box_case((2, 3, 2), (0.1, -0.2, 0.3), (1.5, 0.6, 1.1), 1, 4, "3D Q1 (2, 3, 2)", stencil=False)


def test_random_renumbering_of_velocity_and_pressure_nodes():
    _box_case((4, 3, 5), (0.3, -0.1, 0.2), (2.3, 0.2, 0.9), 2, 5, "4 x 3 x 5, both node sets renumbered", perm=True)


def test_anisotropic_cells():
    _box_case((6, 5, 9), (0.0, 0.0, 0.0), (3.0, 0.25, 1.8), 2, 6, "6 x 5 x 9, h = 0.5 x 0.05 x 0.2")


def test_morton_ordered_mirror():
    """the 16 x 8 x 8 channel through the host mirror (Morton order, multigrid levels attached).  The mirror keeps no A_uu, so only the pressure rows
    can be exported: B from them; B^T against the CSR product of the stored B^T and against the transpose of B, which the masked copies of the
    channel's set are.  The coarser levels never build the tables."""
    from openifem_amd import capi, host
    s = host.InsIM(host.channel_prm(3), (16, 8, 8), (0, 0, 0), EXTENT)
    s.setup(0)
    s.channel_state()
    s.assemble(False)
    s.solve(False)
    import scipy.sparse as sp
    n_un, n_pn = 33 * 17 * 17, 17 * 9 * 9
    ctx = capi.Context.borrow(s.ctx, 3, 2, n_un, n_pn)
    rp, col, val = ctx.export_rows(3 * n_un, n_pn, 0)
    B = sp.csr_matrix((val, col, rp), shape=(n_pn, 3 * n_un + n_pn))[:, :3 * n_un].tocsr()
    infos = _check(ctx, B, B.T.tocsr(), np.random.default_rng(7), "mirror 16 x 8 x 8")
    assert all(i[2] == 0 for i in infos)
    info = np.zeros(4, np.int64)
    for reps, h in s.mg_levels():
        for which in (0, 1):
            assert s.L.ifem_test_b_apply(h, which, 3, None, None, info.ctypes.data_as(C.c_void_p)) == 0
            assert not info.any()  # a level below the finest uses B only to form its S_m
    s.close()


# ---- constraint sets

def _mesh654():
    return BoxMesh((6, 5, 4), (0.3, -0.1, 0.2), (2.3, 0.9, 1.0), kv=2)


def test_all_faces_dirichlet():
    m = _mesh654()
    dofs, vals = m.dirichlet(_bcs(3, outflow=True))
    ctx, rng = _assembled(m, 11, dofs=dofs, vals=vals)
    infos = _check(ctx, *_blocks(ctx, m.n_u), rng, "every face Dirichlet")
    assert all(i[2] == 0 for i in infos)
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
    infos = _check(ctx, *_blocks(ctx, m.n_u), rng, "one interior velocity node constrained")
    assert 0 < infos[0][2] <= 27  # B: at most the pressure nodes of the cells around the node
    # B^T: the node's own row and no other -- velocity constraints mask rows of B^T, the pressure columns are free.  (Exactly one: the rows
    # that share a wave with it in the classification, 16 lanes each, stay regular.)
    assert infos[1][2] == 1 and infos[2][2] == 1
    ctx.close()


def test_random_constrained_dofs_beyond_the_cap_keep_the_csr_products():
    m = _mesh654()
    dofs = np.nonzero(np.random.default_rng(13).random(m.n_u) < 0.3)[0].astype(np.int32)
    ctx, rng = _assembled(m, 13, dofs=dofs, vals=np.zeros(len(dofs)))
    _check(ctx, *_blocks(ctx, m.n_u), rng, "30 % random constrained dofs", stencil=False)
    ctx.close()


# ---- state changes

@pytest.mark.parametrize("geo_cache", [0, 2])
def test_rewritten_blocks_rebuild_the_tables(geo_cache):
    """geo_cache = 0: every assembly re-integrates the blocks; 2: every assembly masks the unconstrained copies.  The tables are re-made after
    each, and the products follow the new values"""
    m = _mesh654()
    ctx, rng = _assembled(m, 14, tuning=dict(geo_cache=geo_cache))
    B0, Bt0 = _blocks(ctx, m.n_u)
    builds = _check(ctx, B0, Bt0, rng, f"geo_cache {geo_cache}, channel set")[0][0]
    assert builds >= 1
    dofs, vals = m.dirichlet(_bcs(3, outflow=True))
    _set_and_assemble(ctx, m, dofs, vals, rng)
    B1, Bt1 = _blocks(ctx, m.n_u)
    assert abs(B1 - B0).max() > 1e-3 * abs(B0).max() and abs(Bt1 - Bt0).max() > 1e-3 * abs(Bt0).max()  # the blocks did change
    assert _check(ctx, B1, Bt1, rng, f"geo_cache {geo_cache}, every face")[0][0] == builds + 1
    _set_and_assemble(ctx, m, dofs, vals, rng)  # the same set again: written again all the same
    assert _check(ctx, B1, Bt1, rng, f"geo_cache {geo_cache}, every face again")[0][0] == builds + 2
    ctx.close()


def test_an_assembly_that_keeps_the_blocks_does_not_rebuild():
    capi = _capi()
    m = _mesh654()
    ctx, rng = _assembled(m, 15)  # (geo_cache = 1, the default)
    B, Bt = _blocks(ctx, m.n_u)
    builds = _check(ctx, B, Bt, rng, "first assembly")[0][0]
    assert builds == 1
    dofs, vals = m.dirichlet(_bcs(3))
    for k in range(2):  # the same constrained-dof set: the blocks stay, A_uu and the right-hand side are new
        _set_and_assemble(ctx, m, dofs, vals, rng)
        ctx.solve(capi.make_params(**KW), False)
        assert _check(ctx, B, Bt, rng, f"kept blocks {k}")[0][0] == builds
    ctx.close()


def test_switching_the_path_off_and_on():
    m = _mesh654()
    ctx, rng = _assembled(m, 16)
    B, Bt = _blocks(ctx, m.n_u)
    _check(ctx, B, Bt, rng, "default")
    assert not ctx.b_apply(0, 2)[1].any()
    _check(ctx, B, Bt, rng, "switched off", stencil=False)
    assert ctx.b_apply(1, 3)[1][0] >= 1
    _check(ctx, B, Bt, rng, "switched on again")
    ctx.close()


def test_after_an_scnsim_assembly_the_products_are_csr():
    capi = _capi()
    m = _mesh654()
    ctx, rng = _assembled(m, 17)
    _check(ctx, *_blocks(ctx, m.n_u), rng, "INS blocks")
    ctx.set_tuning(stored_uu=1)
    ctx.scns_assemble(capi.make_scns_params(mu=0.7, rho=1.3, dt=0.01), False)
    _check(ctx, *_blocks(ctx, m.n_u), rng, "stabilised blocks of an SCnsIM assembly", stencil=False)
    ctx.close()


# ---- not eligible: the CSR products as before

def test_moved_vertex_keeps_the_csr_products():
    m = BoxMesh((3, 2, 2), (0, 0, 0), EXTENT, kv=2)
    h = np.array(EXTENT) / np.array((3, 2, 2))
    m.vcoords = m.vcoords.copy()
    hit = np.all(np.abs(m.vcoords - h) < 1e-9 * h, axis=2)
    assert hit.sum() == 8
    m.vcoords[hit] += 1e-6 * h
    ctx, rng = _assembled(m, 18)
    assert not ctx.mf_uniform()[0]
    _check(ctx, *_blocks(ctx, m.n_u), rng, "one vertex moved by 1e-6 h", stencil=False)
    ctx.close()


def test_hanging_node_mesh_keeps_the_csr_products():
    from hangmesh import HangingMesh
    m = HangingMesh((2, 2, 2), (0, 0, 0), (1.0, 0.8, 0.6), {(0, 0, 0)}, kv=2)
    capi = _capi()
    rng = np.random.default_rng(19)
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    ctx.set_hanging_constraints(m.hang_dof, m.hang_ptr, m.hang_master, m.hang_weight)
    ctx.vec_set(capi.VEC_PRESENT, rng.standard_normal(m.n_dofs))
    ctx.vec_set(capi.VEC_EVAL, rng.standard_normal(m.n_dofs))
    ctx.assemble(capi.make_params(**KW), False)
    _check(ctx, *_blocks(ctx, m.dim * m.n_unodes), rng, "hanging-node mesh", stencil=False)
    ctx.close()


def test_two_virtual_ranks_keep_the_csr_products():
    capi = _capi()
    m = BoxMesh((4, 2, 2), (0, 0, 0), EXTENT, kv=2)
    rng = np.random.default_rng(20)
    dofs, vals = m.dirichlet(_bcs(3))
    ev, pr = rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_dofs)
    from partmesh import local_dirichlet
    parts = partition_mesh(m, (m.vcoords.mean(axis=1)[:, 0] > 1.0).astype(int), 2)

    def work(rank, P, ctx):
        ld, lv = local_dirichlet(P, dofs, vals)
        ctx.set_constraints(0, ld, None)
        ctx.set_constraints(1, ld, lv)
        ctx.vec_set(capi.VEC_PRESENT, pr[P.ext_gdof])
        ctx.vec_set(capi.VEC_EVAL, ev[P.ext_gdof])
        ctx.assemble(capi.make_params(**KW), False)
        r = np.random.default_rng(21 + rank)
        n_pl, n_po = ctx.n_local - ctx.n_u, ctx.n_owned - 3 * ctx.n_unodes_owned
        out = []
        for which, x in enumerate((r.standard_normal(ctx.n_u), r.standard_normal(n_pl), r.standard_normal(n_pl))):
            yy = r.standard_normal(3 * ctx.n_unodes_owned) if which == 2 else None
            y1, info = ctx.b_apply(which, 1, x, yy)
            y0, _ = ctx.b_apply(which, 0, x, yy)
            assert len(y1) == (n_po if which == 0 else 3 * ctx.n_unodes_owned)
            out.append((np.array_equal(y1, y0) and np.isfinite(y0).all() and np.abs(y0).max() > 0, info.copy(), ctx.b_apply(which, 3)[1].copy()))
        return out

    for per_rank in run_virtual_ranks(capi, parts, work):
        for same, info, info3 in per_rank:
            assert same and not info.any() and not info3.any()


# ---- through ifem_solve

def test_one_linear_solve_with_the_path_on_and_off():
    """16^3 mirror chain, stored A_uu and IFEM_AINV_GMRES_BJACOBI (fp64 products throughout: the outer operator launches B, the B^T add behind
    the A_uu product, the preconditioner B^T): the same solve with the stencil products and with the CSR ones.  inner_rel_first = 0 makes the
    solves of one context the same solve.  Iteration counts identical, updates within 1e-9 of the largest entry."""
    from openifem_amd import capi, multigpu
    s, _, _ = multigpu.make_channel_solver(16, 0, 1, 0, None, multigrid=True)
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
        return x, (st.fgmres_iters, st.inner_iters, st.cg_sm_iters, st.cg_mp_iters)

    runs = [solve()]
    for which in (0, 1):
        assert s.L.ifem_test_b_apply(s.ctx, which, 3, None, None, info.ctypes.data_as(C.c_void_p)) == 0
        assert info[0] == 1 and info[2] == 0  # the solve's set-up built the tables, once
    assert s.L.ifem_test_b_apply(s.ctx, 0, 2, None, None, info.ctypes.data_as(C.c_void_p)) == 0 and info[0] == 0
    runs.append(solve())
    assert s.L.ifem_test_b_apply(s.ctx, 0, 3, None, None, info.ctypes.data_as(C.c_void_p)) == 0 and info[0] == 1
    runs.append(solve())
    scale = np.abs(runs[0][0]).max()
    d_off, d_on = np.abs(runs[1][0] - runs[0][0]).max() / scale, np.abs(runs[2][0] - runs[0][0]).max() / scale
    print(f"(fgmres, inner, cg_sm, cg_mp) iterations: {[r[1] for r in runs]}; updates against the first solve: path off {d_off:.3e}, on again "
          f"{d_on:.3e} of the largest entry")
    assert runs[0][1] == runs[1][1] == runs[2][1] and runs[0][1][0] > 0
    assert d_off <= 1e-9 and d_on <= 1e-9
    s.close()
