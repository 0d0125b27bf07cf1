"""The opt-in vertex-patch smoother of the A_uu V-cycle on uniform box levels (ifem_tuning::uu_smoother = 1; csrc/patch.hip, the wiring in
solver.hip::mg_uu_setup / mg_uu_smooth / mg_uu_vcycle), through the C ABI and the test aids ifem_test_uu_patch_vmult / _info.

The operator B = sum_v R_v^T A_v^-1 R_v is checked dof by dof against a host reference made from the oracle's matrix: the velocity block
of the oracle's system matrix at evaluation point 0 IS A0 = mu K + rho/dt M + gamma rho GradDiv with the assembly's elimination, and the
patches are built here from the mesh's cell -> node table (patches_by_definition), not from the library's table."""
import ctypes as C

import numpy as np
import pytest

from boxmesh import BoxMesh
from partmesh import local_dirichlet, partition_mesh, run_virtual_ranks
from test_gpu_inner_f32 import channel16  # noqa: F401  (fixture: the 16^3 bench channel with its three levels, assembled once for this module)

pytestmark = pytest.mark.gpu

CAVITY = dict(mu=0.01, rho=1.0, gamma=1.0, dt=1e-2)  # the regime of fluid_cavity.prm: gamma rho / mu = 100


def patches_by_definition(m):
    """[nodes of the patch of vertex v] from the cell tables alone: local node a of a cell belongs to the patch of the cell's corner
    vertex b when it lies within one node spacing of the corner along every axis (the +-1 lattice box around the vertex, clipped at the
    domain because there are no cells beyond it).  Every such node satisfies the covering rule -- each cell containing it also contains
    the vertex -- which is asserted here; the rule alone would also admit the domain-boundary nodes of the cells next to the boundary,
    which the +-1 box leaves to the boundary vertices' own patches."""
    dim, n1 = m.dim, m.kv + 1
    nu, nv = n1 ** dim, 2 ** dim
    la = np.stack(np.unravel_index(np.arange(nu), (n1,) * dim), axis=-1)[:, ::-1]  # local lattice index of node a, x fastest
    lb = np.stack(np.unravel_index(np.arange(nv), (2,) * dim), axis=-1)[:, ::-1]   # corner b
    near = (np.abs(la[None, :, :] - m.kv * lb[:, None, :]) <= 1).all(-1)            # [corner][node]
    node_cells = [set() for _ in range(m.n_unodes)]
    vert_cells = [set() for _ in range(m.n_pnodes)]
    patch = [set() for _ in range(m.n_pnodes)]
    for c in range(m.n_cells):
        for n in m.cell_unodes[c]:
            node_cells[n].add(c)
        for b, v in enumerate(m.cell_pnodes[c]):
            vert_cells[v].add(c)
            patch[v].update(int(n) for n in m.cell_unodes[c][near[b]])
    for v in range(m.n_pnodes):
        assert all(node_cells[n] <= vert_cells[v] for n in patch[v])
    return [np.array(sorted(p), np.int64) for p in patch]


def reference_patch_vmult(m, A_uu, r):
    """every A_v inverted in fp64; the inverse and r rounded to float, the sum in fp64"""
    dim = m.dim
    rf = r.astype(np.float32).astype(np.float64)
    A = A_uu.tocsr()
    out = np.zeros(m.n_u)
    sizes = {}
    for nodes in patches_by_definition(m):
        dofs = (dim * nodes[:, None] + np.arange(dim)[None, :]).ravel()
        Av = A[dofs][:, dofs].toarray()
        inv = np.linalg.inv(Av).astype(np.float32).astype(np.float64)
        out[dofs] += inv @ rf[dofs]
        sizes[len(nodes)] = sizes.get(len(nodes), 0) + 1
    return out, sizes


def _patch_case(m, bcs):
    """device B r and the host reference of one mesh / constraint set in the cavity regime"""
    import orc
    from openifem_amd import capi
    dofs, vals = m.dirichlet(bcs)
    rng = np.random.default_rng(7)
    present = rng.standard_normal(m.n_dofs)
    evalp = np.zeros(m.n_dofs)  # evaluation point 0: no convective term in the matrix
    r = np.zeros(m.n_dofs)
    r[:m.n_u] = rng.standard_normal(m.n_u) * (1.0 + 10.0 * (np.arange(m.n_u) % 7 == 0))  # rough, no two neighbours alike
    S = orc.System(m)
    S.set_constraints(0, dofs, None)
    S.set_constraints(1, dofs, vals)
    S.assemble(orc.make_params(**CAVITY), False, evalp, present)
    A_uu = S.csr("A")[:m.n_u, :m.n_u]
    ref, sizes = reference_patch_vmult(m, A_uu, r[:m.n_u])
    ctx = capi.Context(m.dim, 2, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    try:
        ctx.set_constraints(0, dofs, None)
        ctx.set_constraints(1, dofs, vals)
        ctx.vec_set(capi.VEC_PRESENT, present)
        ctx.vec_set(capi.VEC_EVAL, evalp)
        ctx.assemble(capi.make_params(**CAVITY), False)
        info = ctx.uu_patch_info()
        y = ctx.uu_patch_vmult(r)[:m.n_u]
    finally:
        ctx.close()
    return y, ref, sizes, info


def test_patch_operator_matches_the_host_reference_3d():
    """5 x 4 x 3 cells with unequal edges (swapped axes would show): 24 interior patches and every face, edge and corner class, so clipped
    patches and tile remainders are covered; Dirichlet on all components of three faces (flag 7), on one component of one face (flag 4),
    two faces free.  With identically rounded inputs the difference is the fp32 accumulation over <= 81 terms; an indexing error is O(1).
    Measured on one MI355X: 6.3e-8 of max |B r| (bound 1e-4)."""
    m = BoxMesh((5, 4, 3), (0, 0, 0), (1.0, 0.6, 0.75), kv=2)
    bcs = {2: (7, [0.0] * 3), 3: (7, [0.0] * 3), 0: (7, [0.3, -0.2, 0.1]), 4: (4, [0.0])}
    y, ref, sizes, info = _patch_case(m, bcs)
    assert sizes == {27: 24, 18: 52, 12: 36, 8: 8}
    eligible, n_patches, n_types, nbytes = info
    assert eligible and n_patches == m.n_pnodes == 120
    assert 1 <= n_types <= n_patches and nbytes == n_types * 81 * 81 * 4
    err = np.abs(y - ref).max() / np.abs(ref).max()
    print(f"3D vertex-patch B r against the host reference: {err:.3e} of max |B r| = {np.abs(ref).max():.3e}; {n_types} patch types")
    assert err <= 1e-4


def test_patch_operator_matches_the_host_reference_2d():
    """5 x 3 cells, Q2: measured on one MI355X 5.8e-8 of max |B r| (bound 1e-4)"""
    m = BoxMesh((5, 3), (0, 0), (1.0, 0.45), kv=2)
    bcs = {2: (3, [0.0] * 2), 0: (3, [0.3, -0.2]), 3: (2, [0.0])}
    y, ref, sizes, info = _patch_case(m, bcs)
    assert sizes == {9: 8, 6: 12, 4: 4}
    eligible, n_patches, n_types, nbytes = info
    assert eligible and n_patches == m.n_pnodes == 24
    assert nbytes == n_types * 18 * 18 * 4
    err = np.abs(y - ref).max() / np.abs(ref).max()
    print(f"2D vertex-patch B r against the host reference: {err:.3e} of max |B r| = {np.abs(ref).max():.3e}; {n_types} patch types")
    assert err <= 1e-4


def _set_tuning(s, **kw):
    from openifem_amd import capi
    tun = capi.Tuning()
    s.L.ifem_default_tuning(C.byref(tun))
    assert tun.uu_smoother == 0
    for k, v in kw.items():
        setattr(tun, k, v)
    for c in s.all_ctxs():
        assert s.L.ifem_set_tuning(c, C.byref(tun)) == 0, s.L.ifem_last_error().decode()


def _precond(s, ip, v):
    from openifem_amd import capi
    assert s.L.ifem_vec_set(s.ctx, capi.VEC_TMP, v.ctypes.data_as(C.c_void_p)) == 0
    rc = s.L.ifem_precond_vmult(s.ctx, C.byref(ip), C.byref(s.opts), capi.VEC_UPDATE, capi.VEC_TMP)
    assert rc == 0, s.L.ifem_last_error().decode()
    x = np.zeros(len(v))
    assert s.L.ifem_vec_get(s.ctx, capi.VEC_UPDATE, x.ctypes.data_as(C.c_void_p)) == 0
    return x


def test_patch_vcycle_is_deterministic_and_replays_as_a_graph():
    """the 16^3 channel with its three levels, A~^-1 = one V-cycle: three applications through the captured graph (eager, capture, replay)
    and three eager ones are all the same bits; uu_smoother = 0 set explicitly is the context that never heard of the field"""
    from openifem_amd import capi, multigpu
    s, _, _ = multigpu.make_channel_solver(16, 0, 1, 0, None, multigrid=True)
    try:
        assert len(list(s.all_ctxs())) == 3
        s.channel_state()
        s.opts.ainv_kind = capi.AINV_MG
        s.opts.inner_maxit = 0
        s.assemble(False)
        _, n_u, n_p = s.sizes()
        g = np.arange(n_u + n_p)
        v = np.cos(0.37 * g) + 0.1 * np.sin(1.3 * g)
        ip = capi.make_params(mu=1.0, rho=1.0, gamma=0.1, dt=1e-3)
        untouched = [_precond(s, ip, v) for _ in range(3)]  # no ifem_set_tuning yet
        for c in s.all_ctxs():  # every level of this chain is a uniform box of Q2 cells on one rank
            out = np.zeros(4, np.int64)
            assert s.L.ifem_test_uu_patch_info(c, out.ctypes.data_as(C.c_void_p)) == 0 and out[0] == 1 and out[1] > 0
        z = {}
        for cells in (262144, 0):
            _set_tuning(s, uu_smoother=1, vcycle_graph_cells=cells)
            before = capi.vcycle_graph_stats(s.L, s.ctx)
            z[cells] = [_precond(s, ip, v) for _ in range(3)]
            after = capi.vcycle_graph_stats(s.L, s.ctx)
            print(f"uu_smoother = 1, vcycle_graph_cells = {cells}: hipGraph captures {after[0] - before[0]}, launches {after[1] - before[1]}")
            if cells:
                assert after[0] - before[0] >= 1 and after[1] - before[1] >= 2  # the graphs were captured and replayed
            else:
                assert after[1] == before[1]
        assert np.isfinite(z[0][0]).all() and np.abs(z[0][0][:n_u]).max() > 0
        for a in z[262144] + z[0]:
            assert np.array_equal(a, z[0][0])
        assert not np.array_equal(z[0][0][:n_u], untouched[0][:n_u])  # it is another smoother
        _set_tuning(s, uu_smoother=0)
        back = [_precond(s, ip, v) for _ in range(3)]
        for a, b in zip(untouched, back):
            assert np.array_equal(a, b)
    finally:
        s.close()


def test_each_smoother_kind_keeps_its_bound_and_graph_across_a_switch(channel16):
    """ifem_precond_vmult (IFEM_AINV_MG, default options) with uu_smoother = 0, 1, 0, 1 in turn on one context, three applications each
    (eager, capture, replay): a kind that comes back finds its own Chebyshev bound again (ifem_ctx::uu_bound[kind]) and its graph is
    captured anew for the tuning epoch -- the first and third settings are the same bits, and so are the second and fourth"""
    from openifem_amd import capi
    s, n_u, n_p, v, defaults = channel16
    for k, val in defaults.items():
        setattr(s.opts, k, val)
    ip = capi.make_params(mu=1.0, rho=1.0, gamma=0.1, dt=1e-3)
    z = []
    for knob in (0, 1, 0, 1):
        _set_tuning(s, uu_smoother=knob)
        z.append([_precond(s, ip, v) for _ in range(3)])
    _set_tuning(s)
    assert all(np.isfinite(a).all() for zs in z for a in zs) and np.abs(z[0][0][:n_u]).max() > 0
    assert not np.array_equal(z[0][0][:n_u], z[1][0][:n_u])  # it is another smoother
    for first, again in ((z[0], z[2]), (z[1], z[3])):
        for a in first + again:
            assert np.array_equal(a, first[0])


def test_patch_smoother_needs_fewer_inner_iterations_in_the_cavity_regime():
    """16^3 channel at gamma rho / mu = 100 (viscosity 0.01, grad-div 1.0, dt 1e-2), product default options: the solve converges and the
    inner iteration count is strictly below the node-block Jacobi smoother's (a fresh context each).
    Measured on one MI355X: 28 inner iterations with node-block Jacobi, 14 with the vertex patches, 3 FGMRES iterations with both
    (profiles/patch_smoother.txt)"""
    from openifem_amd import capi, host
    prm = host.channel_prm(3, dt=1e-2)
    assert "set Dynamic viscosity = 1\n" in prm and "set Grad-Div stabilization = 0.1\n" in prm
    prm = prm.replace("set Dynamic viscosity = 1\n", "set Dynamic viscosity = 0.01\n").replace("set Grad-Div stabilization = 0.1\n", "set Grad-Div stabilization = 1.0\n")
    counts = {}
    for knob in (0, 1):
        s = host.InsIM(prm, (16, 16, 16), (0, 0, 0), (2.0, 0.2, 0.2), device=0, verbose=False)
        try:
            s.set_multigrid(True, 0)
            s.setup(0)
            s.channel_state()
            s.opts.ainv_kind = capi.AINV_MG
            if knob:
                _set_tuning(s, uu_smoother=knob)
            s.assemble(False)
            st = s.solve(False)
            res, bn = s.true_residual()
            counts[knob] = (st.inner_iters, st.fgmres_iters, st.precond_applies, res / bn)
        finally:
            s.close()
    for knob in (0, 1):
        print(f"uu_smoother = {knob}: inner iterations {counts[knob][0]}, FGMRES iterations {counts[knob][1]}, "
              f"preconditioner applications {counts[knob][2]}, true residual / ||b|| {counts[knob][3]:.3e}")
    assert counts[1][3] <= 1.05e-4
    assert counts[1][0] < counts[0][0]


def test_levels_that_are_not_eligible_keep_the_node_blocks():
    """two virtual ranks of the (4, 2, 2) box: a partitioned level is not eligible, uu_smoother = 1 changes nothing there (same bits from
    the same assembly), and any value but 0 / 1 is refused"""
    from openifem_amd import capi
    m = BoxMesh((4, 2, 2), (0, 0, 0), (2.0, 0.2, 0.2), kv=2)
    rng = np.random.default_rng(19)
    bcs = {0: (7, [0.3, -0.2, 0.1]), 2: (7, [0.0] * 3), 3: (7, [0.0] * 3), 4: (7, [0.0] * 3), 5: (7, [0.0] * 3)}
    dofs, vals = m.dirichlet(bcs)
    ev, pr, x = rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_dofs)
    Pm = capi.make_params(mu=0.7, rho=1.3, gamma=0.2, dt=0.01)
    cell_rank = (m.vcoords.mean(axis=1)[:, 0] > 1.0).astype(int)
    parts = partition_mesh(m, cell_rank, 2)

    def work(rank, P, ctx):
        ld, lv = local_dirichlet(P, dofs, vals)
        ctx.set_constraints(0, ld, None)
        ctx.set_constraints(1, ld, lv)
        ctx.vec_set(capi.VEC_PRESENT, pr[P.ext_gdof])
        ctx.vec_set(capi.VEC_EVAL, ev[P.ext_gdof])
        ctx.opts.ainv_kind = capi.AINV_MG
        ctx.assemble(Pm, False)
        info = ctx.uu_patch_info()
        out = {}
        for knob in (0, 1):
            ctx.set_tuning(uu_smoother=knob)
            out[knob] = ctx.precond_vmult(Pm, x[P.own_gdof])
        with pytest.raises(capi.IfemError) as e:
            ctx.set_tuning(uu_smoother=2)
        ctx._tuning = None
        return info, out, e.value.code

    for info, out, code in run_virtual_ranks(capi, parts, work):
        assert info == (False, 0, 0, 0)
        assert np.isfinite(out[0]).all() and np.abs(out[0]).max() > 0
        assert np.array_equal(out[0], out[1])
        assert code == capi.E_BADPARAM
