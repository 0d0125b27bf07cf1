"""Constant-geometry variants of the matrix-free A_uu kernels (apply_mf.hip::k_apply_uu_mf2<..., UNI>, mg.hip::k_uu_diag<..., UNI>) on
contexts whose cells are all the same axis-aligned box (ifem_ctx::mf_uniform, decided at ifem_ctx_create; ifem_tuning::mf_uniform = 0
forces the general kernels), through the C ABI.

The checker is the stored block CSR (ifem_uu_vmult variant IFEM_AINV_GMRES_BJACOBI: the assembly kernels, themselves tied to the
oracle in test_gpu_parity.py), never the kernels under test.  Shapes: anisotropic cells (a swapped axis shows), an odd cell count
(the last wave works on one cell), every dim / degree instantiation.  The same comparisons run on the general path of a mesh with one
vertex moved by 1e-6 h, which must be detected."""
import ctypes as C

import numpy as np
import pytest

import orc
from boxmesh import BoxMesh
from partmesh import gather_owned, local_dirichlet, partition_mesh, run_virtual_ranks

pytestmark = pytest.mark.gpu

EXTENT = (2.0, 0.2, 0.2)
SHAPES = [(3, 2, (3, 2, 2)), (3, 2, (4, 2, 2)), (3, 1, (3, 2, 2)), (2, 2, (4, 3)), (2, 1, (4, 3))]
KW = dict(mu=0.7, rho=1.3, gamma=0.2, dt=0.01)
STORED, MF64, MF32 = 0, 3, 4  # IFEM_AINV_GMRES_BJACOBI, _MF, IFEM_AINV_MG


def _capi():
    from openifem_amd import capi
    return capi


def _mesh(dim, kv, reps, bump=False):
    m = BoxMesh(reps, (0,) * dim, EXTENT[:dim], kv=kv)
    if bump:  # one interior vertex (the corner shared by the cells around lattice point (1, 1[, 1])) off by 1e-6 h
        h = np.array(EXTENT[:dim]) / np.array(reps)
        p = h.copy()
        m.vcoords = m.vcoords.copy()
        hit = np.all(np.abs(m.vcoords - p) < 1e-9 * h, axis=2)
        assert hit.sum() == 2 ** dim
        m.vcoords[hit] += 1e-6 * h
    return m


def _bcs(dim):
    """inflow (x-) and the walls (y-, y+, and z-, z+ in 3D)"""
    flag = 3 if dim == 2 else 7
    bcs = {0: (flag, [0.3, -0.2, 0.1][:dim]), 2: (flag, [0.0] * dim), 3: (flag, [0.0] * dim)}
    if dim == 3:
        bcs.update({4: (flag, [0.0] * dim), 5: (flag, [0.0] * dim)})
    return bcs


def _assembled(m, seed, imex=False):
    capi = _capi()
    rng = np.random.default_rng(seed)
    dofs, vals = m.dirichlet(_bcs(m.dim))
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    ctx.set_constraints(0, dofs, None)
    ctx.set_constraints(1, dofs, vals)
    ctx.vec_set(capi.VEC_PRESENT, rng.standard_normal(m.n_dofs))
    ctx.vec_set(capi.VEC_EVAL, rng.standard_normal(m.n_dofs))
    if imex:
        ctx.imex_assemble(capi.make_params(**KW), False, True)
    else:
        ctx.assemble(capi.make_params(**KW), False)
    return ctx, rng


def _compare_operators(ctx, m, rng, tag):
    """the three comparisons of the issue on one assembled context; the figures are printed before they are asserted"""
    n_u = m.dim * m.n_unodes
    x = rng.standard_normal(m.n_dofs)
    ys, y64, y32 = (ctx.uu_vmult(x, v)[:n_u] for v in (STORED, MF64, MF32))
    e64 = np.abs(y64 - ys).max() / np.abs(ys).max()
    e32 = np.abs(y32 - y64).max() / np.abs(y64).max()
    a, b = ctx.uu_block_diag(0), ctx.uu_block_diag(1)
    eb = np.abs(a - b).max() / np.abs(a).max()
    print(f"{tag}: fp64 matrix-free vs stored {e64:.2e}, fp32 vs fp64 operator {e32:.2e}, node blocks {eb:.2e}")
    assert e64 <= 1e-13
    assert e32 <= 3e-5   # test_single_precision_operator_matches_the_fp64_operator
    assert eb <= 5e-6    # test_matrix_free_block_diagonal_equals_the_assembled_one
    assert np.abs(ctx.uu_block_diag(0) - a).max() == 0.0


@pytest.mark.parametrize("dim,kv,reps", SHAPES)
def test_uniform_kernels_match_the_stored_matrix(dim, kv, reps):
    m = _mesh(dim, kv, reps)
    ctx, rng = _assembled(m, 3 + dim + kv)
    uni, h = ctx.mf_uniform()
    assert uni
    want = np.array(EXTENT[:dim]) / np.array(reps)
    assert np.abs(h[:dim] - want).max() <= 8 * np.finfo(float).eps * max(EXTENT) and np.all(h[dim:] == 0)  # the detection's own allowance
    _compare_operators(ctx, m, rng, f"uniform {dim}D Q{kv} {reps}")
    ctx.close()


@pytest.mark.parametrize("dim,kv,reps", [(3, 2, (3, 2, 2)), (2, 1, (4, 3))])
def test_imex_matrix_without_convective_terms(dim, kv, reps):
    """CONV = false instantiations"""
    m = _mesh(dim, kv, reps)
    ctx, rng = _assembled(m, 29, imex=True)
    assert ctx.mf_uniform()[0]
    _compare_operators(ctx, m, rng, f"uniform imex {dim}D Q{kv}")
    ctx.close()


def test_moved_vertex_is_detected_and_the_general_kernels_still_agree():
    m = _mesh(3, 2, (3, 2, 2), bump=True)
    ctx, rng = _assembled(m, 8)
    uni, h = ctx.mf_uniform()
    assert not uni and np.all(h == 0)
    _compare_operators(ctx, m, rng, "one vertex moved by 1e-6 h")
    ctx.close()


def test_locally_refined_box_is_not_uniform():
    from hangmesh import HangingMesh
    capi = _capi()
    for m in (HangingMesh((3, 2), (0, 0), (1.5, 0.8), {(0, 0), (2, 1)}, kv=2), HangingMesh((2, 2, 2), (0, 0, 0), (1.0, 0.8, 0.6), {(0, 0, 0)}, kv=2)):
        ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
        assert ctx.mf_uniform()[0] is False
        ctx.close()


def test_lift_of_inhomogeneous_inflow_values_on_the_uniform_path():
    """ifem_tuning::stored_uu = 0 with non-zero inflow values (the LIFT instantiation): right-hand side against the stored assembly's"""
    capi = _capi()
    m = _mesh(3, 2, (3, 2, 2))
    rng = np.random.default_rng(41)
    dofs, vals = m.dirichlet(_bcs(3), {0: lambda p, c: 0.3 + 0.5 * p[1] if c == 0 else 0.1 * p[1]})
    assert np.abs(vals).max() > 0
    ev, pr = 0.3 * rng.standard_normal(m.n_dofs), 0.3 * rng.standard_normal(m.n_dofs)
    rhs = []
    for stored in (1, 0):
        ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
        if not stored:
            ctx.set_tuning(stored_uu=0)
            ctx.opts.ainv_kind = capi.AINV_GMRES_BJACOBI_MF
        assert ctx.mf_uniform()[0]
        ctx.set_constraints(0, dofs, None)
        ctx.set_constraints(1, dofs, vals)
        ctx.vec_set(capi.VEC_PRESENT, pr)
        ctx.vec_set(capi.VEC_EVAL, ev)
        ctx.assemble(capi.make_params(**KW), True)
        rhs.append(ctx.vec_get(capi.VEC_RHS))
        assert stored or ctx.uu_stored_bytes() == 0
        ctx.close()
    free = np.ones(m.n_dofs, bool)
    free[dofs] = False
    err = np.abs(rhs[1][free] - rhs[0][free]).max() / np.abs(rhs[0]).max()
    print("lifted right-hand side vs the stored assembly's (free rows):", err)
    assert err <= 1e-11


def test_bench_mesh_and_every_attached_level_are_uniform():
    from openifem_amd import multigpu
    solver, reps, _ = multigpu.make_channel_solver(16, 0, 1, 0, None, multigrid=True)
    ctxs = list(solver.all_ctxs())
    assert len(ctxs) >= 3
    hs = []
    for c in ctxs:
        h = np.zeros(3)
        assert solver.L.ifem_test_mf_uniform(c, h.ctypes.data_as(C.c_void_p)) == 1
        hs.append(h)
    assert np.abs(hs[0] - np.array(EXTENT) / 16).max() <= 8 * np.finfo(float).eps * max(EXTENT)
    for a, b in zip(hs, hs[1:]):  # every coarser level doubles some edges and keeps the others
        r = b / a
        assert np.all((np.abs(r - 1) < 1e-12) | (np.abs(r - 2) < 1e-12)) and r.max() > 1.5
    solver.close()


def test_knob_switches_the_kernels_and_rebuilds_the_vcycle_graph():
    """16 x 8 x 8 with the captured V-cycle: the same solve with ifem_tuning::mf_uniform = 1, then 0 on every level"""
    from openifem_amd import capi, host
    s = host.InsIM(host.channel_prm(3), (16, 8, 8), (0, 0, 0), EXTENT)
    s.setup(0)
    s.channel_state()
    s.opts.inner_restart = 16
    s.opts.ainv_kind = capi.AINV_MG
    s.assemble(False)
    _, n_u, n_p = s.sizes()
    res = []
    for knob in (1, 0):
        tun = capi.Tuning()
        s.L.ifem_default_tuning(C.byref(tun))
        assert tun.mf_uniform == 1
        tun.mf_uniform = knob
        for c in s.all_ctxs():
            assert s.L.ifem_set_tuning(c, C.byref(tun)) == 0
            assert s.L.ifem_test_mf_uniform(c, None) == knob
        before = capi.vcycle_graph_stats(s.L, s.ctx)
        st = s.solve(False)
        after = capi.vcycle_graph_stats(s.L, s.ctx)
        assert after[0] > before[0] and after[1] > before[1], (before, after)  # captured anew, and replayed
        x = np.zeros(n_u + n_p)
        assert s.L.ifem_vec_get(s.ctx, capi.VEC_UPDATE, x.ctypes.data_as(C.c_void_p)) == 0
        res.append((st.fgmres_iters, st.inner_iters, x))
    s.close()
    err = np.abs(res[0][2] - res[1][2]).max() / np.abs(res[1][2]).max()
    print("iterations (uniform, general):", res[0][:2], res[1][:2], "update difference", err)
    assert res[0][:2] == res[1][:2]
    assert err <= 1e-6


def test_two_virtual_ranks_match_the_single_context():
    capi = _capi()
    m = _mesh(3, 2, (4, 2, 2))
    rng = np.random.default_rng(19)
    dofs, vals = m.dirichlet(_bcs(3))
    ev, pr, x = rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_dofs)
    Pm = capi.make_params(**KW)

    def run(nranks):
        c = m.vcoords.mean(axis=1)
        cell_rank = (c[:, 0] > 1.0).astype(int) if nranks == 2 else np.zeros(m.n_cells, int)
        parts = partition_mesh(m, cell_rank, nranks)

        def work(rank, P, ctx):
            assert ctx.mf_uniform()[0]
            ld, lv = local_dirichlet(P, dofs, vals)
            ctx.set_constraints(0, ld, None)
            ctx.set_constraints(1, ld, lv)
            ctx.vec_set(capi.VEC_PRESENT, pr[P.ext_gdof])
            ctx.vec_set(capi.VEC_EVAL, ev[P.ext_gdof])
            ctx.assemble(Pm, False)
            return ctx.uu_vmult(x[P.own_gdof], MF64)

        return gather_owned(parts, run_virtual_ranks(capi, parts, work), m.n_dofs)[:3 * m.n_unodes]

    y1, y2 = run(1), run(2)
    err = np.abs(y2 - y1).max() / np.abs(y1).max()
    print("two ranks against one context, matrix-free fp64:", err)
    assert err <= 1e-13
