"""The vertex-patch smoother of the A_uu V-cycle on levels whose cells differ (ifem_tuning::uu_smoother = 1 with uu_patch_levels = 1: one stored
inverse per patch; the general form at the end of csrc/patch.hip), through the C ABI and the test aids ifem_test_uu_patch_vmult / _info.

The operator B = sum_v R_v^T A_v^-1 R_v is checked dof by dof against the host reference of test_gpu_patch_smoother.py: the velocity block of the
oracle's matrix at evaluation point 0 in the cavity regime, every A_v inverted in fp64 by numpy, the patches taken from the mesh's cell -> node
table by definition (patches_by_definition), not from the library's tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from boxmesh import BoxMesh
from cylmesh import CylinderMesh, CylinderMesh3D, inflow_bc, inflow_bc_3d
from partmesh import local_dirichlet, partition_mesh, run_virtual_ranks
from test_gpu_patch_smoother import CAVITY, reference_patch_vmult

pytestmark = pytest.mark.gpu

GENERAL = dict(uu_patch_levels=1)


def _rough(m):
    """the right-hand side of test_gpu_patch_smoother._patch_case: rough, no two neighbours alike"""
    rng = np.random.default_rng(7)
    present = rng.standard_normal(m.n_dofs)
    r = np.zeros(m.n_dofs)
    r[:m.n_u] = rng.standard_normal(m.n_u) * (1.0 + 10.0 * (np.arange(m.n_u) % 7 == 0))
    return present, r


def _host_reference(m, dofs, vals):
    import orc
    present, r = _rough(m)
    evalp = np.zeros(m.n_dofs)  # evaluation point 0: no convective term in the matrix
    S = orc.System(m)
    S.set_constraints(0, dofs, None)
    S.set_constraints(1, dofs, vals)
    S.assemble(orc.make_params(**CAVITY), False, evalp, present)
    return reference_patch_vmult(m, S.csr("A")[:m.n_u, :m.n_u], r[:m.n_u])


def _device(m, dofs, vals, tuning, vmult=True):
    """(B r or the refusal, info) of one context with `tuning` set before the assembly"""
    from openifem_amd import capi
    present, r = _rough(m)
    ctx = capi.Context(m.dim, 2, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    try:
        if tuning:
            ctx.set_tuning(**tuning)
        ctx.set_constraints(0, dofs, None)
        ctx.set_constraints(1, dofs, vals)
        ctx.vec_set(capi.VEC_PRESENT, present)
        ctx.vec_set(capi.VEC_EVAL, np.zeros(m.n_dofs))
        ctx.assemble(capi.make_params(**CAVITY), False)
        info = ctx.uu_patch_info()
        y = None
        if vmult:
            y = ctx.uu_patch_vmult(r)[:m.n_u]
            info2 = ctx.uu_patch_info()
            assert tuple(info2) == tuple(info)  # the product found the tables the query made
    finally:
        ctx.close()
    return y, tuple(info)


def _cyl2d_bcs(m):
    return m.dirichlet({0: (3, [0.0, 0.0]), 2: (3, [0.0] * 2), 3: (3, [0.0] * 2), 4: (3, [0.0] * 2)}, fields={0: inflow_bc})


def test_general_patch_operator_matches_the_host_reference_2d():
    """CylinderMesh(0): 92 cells, 122 patches of 4 / 6 / 9 / 11 nodes (vertices of valence 1, 2, 4, 5), the curved ring cells; inflow values on
    id 0, zero on the walls and the cylinder, outflow free.  One inverse per patch, stored as full squares.  With identically rounded inputs
    the difference is the fp32 accumulation over <= 22 terms and the fp64 inversion on the device; an indexing error is O(1).
    Measured on one MI355X: 4.9e-8 of max |B r| (bound 1e-4)."""
    m = CylinderMesh(0)
    assert m.n_cells == 92
    dofs, vals = _cyl2d_bcs(m)
    ref, sizes = _host_reference(m, dofs, vals)
    assert sizes == {4: 4, 6: 56, 9: 58, 11: 4}
    y, info = _device(m, dofs, vals, GENERAL)
    eligible, n_patches, n_inverses, nbytes = info
    assert eligible and n_patches == m.n_pnodes == 122 and n_inverses == 122
    assert 4 * sum(cnt * (2 * n) ** 2 for n, cnt in sizes.items()) <= nbytes <= 122 * 26 ** 2 * 4
    err = np.abs(y - ref).max() / np.abs(ref).max()
    print(f"2D cylinder, per-patch inverses: B r against the host reference: {err:.3e} of max |B r| = {np.abs(ref).max():.3e}; {nbytes} bytes of inverses")
    assert err <= 1e-4


def test_general_patch_operator_matches_the_host_reference_3d():
    """CylinderMesh3D(0): 832 cells, 1233 patches of 8 / 12 / 18 / 22 / 27 / 33 nodes (up to 99 dofs: two rows per lane, a packed 99 x 100 / 2
    triangle in the setup kernel).  Inflow values on id 0, zero on the y walls and the cylinder, only the z component on the z = 0 face (partially
    constrained patches), the z = 0.41 face and the outflow free.  Measured on one MI355X: 2.2e-7 of max |B r| (bound 1e-4)."""
    m = CylinderMesh3D(0)
    assert m.n_cells == 832
    bcs = {0: (7, [0.0] * 3), 2: (7, [0.0] * 3), 3: (7, [0.0] * 3), 6: (7, [0.0] * 3), 4: (4, [0.0])}
    dofs, vals = m.dirichlet(bcs, fields={0: inflow_bc_3d})
    ref, sizes = _host_reference(m, dofs, vals)
    assert sizes == {8: 8, 12: 152, 18: 568, 22: 8, 27: 469, 33: 28}
    y, info = _device(m, dofs, vals, GENERAL)
    eligible, n_patches, n_inverses, nbytes = info
    assert eligible and n_patches == m.n_pnodes == 1233 and n_inverses == 1233
    assert 4 * sum(cnt * (3 * n) ** 2 for n, cnt in sizes.items()) <= nbytes <= 1233 * 117 ** 2 * 4
    err = np.abs(y - ref).max() / np.abs(ref).max()
    print(f"3D cylinder, per-patch inverses: B r against the host reference: {err:.3e} of max |B r| = {np.abs(ref).max():.3e}; {nbytes} bytes of inverses")
    assert err <= 1e-4


def test_general_form_equals_the_shared_type_form_on_a_box():
    """the 5 x 4 x 3 box of test_gpu_patch_smoother with mf_uniform = 0 and uu_patch_levels = 1: the general kernels on a uniform mesh.  B r
    agrees with the host reference and with the default tuning's shared-type result, both to 1e-4 of max |B r|.
    Measured on one MI355X: 7.2e-8 against the reference, 1.1e-7 against the shared-type form."""
    m = BoxMesh((5, 4, 3), (0, 0, 0), (1.0, 0.6, 0.75), kv=2)
    bcs = {2: (7, [0.0] * 3), 3: (7, [0.0] * 3), 0: (7, [0.3, -0.2, 0.1]), 4: (4, [0.0])}
    dofs, vals = m.dirichlet(bcs)
    ref, sizes = _host_reference(m, dofs, vals)
    assert sizes == {27: 24, 18: 52, 12: 36, 8: 8}
    y_gen, info_gen = _device(m, dofs, vals, dict(mf_uniform=0, uu_patch_levels=1))
    y_box, info_box = _device(m, dofs, vals, None)
    assert info_gen[:3] == (True, 120, 120) and info_gen[3] == 4 * sum(cnt * (3 * n) ** 2 for n, cnt in sizes.items())
    assert info_box[0] and info_box[1] == 120 and info_box[3] == info_box[2] * 81 * 81 * 4  # (the shared-type tables: one 81 x 81 per type)
    scale = np.abs(ref).max()
    e_ref, e_box = np.abs(y_gen - ref).max() / scale, np.abs(y_gen - y_box).max() / np.abs(y_box).max()
    print(f"box, per-patch inverses: {e_ref:.3e} against the host reference, {e_box:.3e} against the shared-type form")
    assert e_ref <= 1e-4 and e_box <= 1e-4
    # without the switch a box whose uniform kernels are off takes no patches at all
    _, info_off = _device(m, dofs, vals, dict(mf_uniform=0), vmult=False)
    assert info_off == (False, 0, 0, 0)


def _cylinder_prm(refinements):
    prm = open(os.path.join(os.path.dirname(__file__), "golden", "prm", "fluid_cylinder_mpi.prm")).read()
    return re.sub(r"set Global refinements\s*=\s*\d+", f"set Global refinements = {refinements}", prm)


def _cylinder_flow(refinements):
    """the mirror's InsIM on tests/fluid_cylinder_mpi with the levels of its refinement history (test_gpu_multigrid._cylinder_run)"""
    from openifem_amd import host
    flow = host.InsIM(_cylinder_prm(refinements), mesh="cylinder")
    flow.add_hard_coded_boundary_condition(0, lambda p, c, t: 4 * 0.3 * p[1] * (0.41 - p[1]) / (0.41 * 0.41) if (c == 0 and abs(p[0]) < 1e-10) else 0.0)
    flow.set_multigrid(True)
    flow.setup(refinements)
    return flow


def _set_tuning(s, **kw):
    from openifem_amd import capi
    tun = capi.Tuning()
    s.L.ifem_default_tuning(C.byref(tun))
    assert tun.uu_smoother == 0 and tun.uu_patch_levels == 0
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


def _level_info(s):
    out = []
    for c in s.all_ctxs():
        o = np.zeros(4, np.int64)
        assert s.L.ifem_test_uu_patch_info(c, o.ctypes.data_as(C.c_void_p)) == 0, s.L.ifem_last_error().decode()
        out.append(tuple(int(x) for x in o))
    return out


CYL = dict(mu=0.001, rho=1.0, gamma=0.1, dt=1e-2)  # fluid_cylinder_mpi.prm: gamma rho / mu = 100


def test_off_means_off():
    """uu_patch_levels = 0 (the default): the cylinder is not eligible and the test aid refuses it; uu_smoother = 1 then changes nothing on the
    mirror's cylinder at 2 refinements (one V-cycle of IFEM_AINV_MG, same bits as uu_smoother = 0); any value but 0 / 1 is refused"""
    from openifem_amd import capi
    m = CylinderMesh(0)
    dofs, vals = _cyl2d_bcs(m)
    present, r = _rough(m)
    ctx = capi.Context(2, 2, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    try:
        ctx.set_constraints(0, dofs, None)
        ctx.set_constraints(1, dofs, vals)
        ctx.vec_set(capi.VEC_PRESENT, present)
        ctx.vec_set(capi.VEC_EVAL, np.zeros(m.n_dofs))
        ctx.assemble(capi.make_params(**CAVITY), False)
        for tuning in (None, dict(uu_smoother=1), dict(uu_smoother=1, uu_patch_levels=0)):
            if tuning:
                ctx.set_tuning(**tuning)
            assert tuple(ctx.uu_patch_info()) == (False, 0, 0, 0)
            with pytest.raises(capi.IfemError) as e:
                ctx.uu_patch_vmult(r)
            assert e.value.code == capi.E_BADPARAM
        with pytest.raises(capi.IfemError) as e:
            ctx.set_tuning(uu_patch_levels=2)
        assert e.value.code == capi.E_BADPARAM
        ctx._tuning = None
        with pytest.raises(capi.IfemError) as e:
            ctx.set_tuning(uu_patch_levels=-1)
        assert e.value.code == capi.E_BADPARAM
    finally:
        ctx.close()
    s = _cylinder_flow(2)
    try:
        assert len(s.all_ctxs()) == 3  # refinements 2, 1, 0
        s.opts.inner_maxit = 0
        s.assemble(False)
        _, n_u, n_p = s.sizes()
        g = np.arange(n_u + n_p)
        v = np.cos(0.37 * g) + 0.1 * np.sin(1.3 * g)
        ip = capi.make_params(**CYL)
        z = {}
        for name, tuning in (("untouched", None), ("off", dict(uu_smoother=0)), ("smoother only", dict(uu_smoother=1, uu_patch_levels=0)),
                             ("levels only", dict(uu_smoother=0, uu_patch_levels=1))):
            if tuning is not None:
                _set_tuning(s, **tuning)
            z[name] = [_precond(s, ip, v) for _ in range(3)]
            if name == "smoother only":
                assert all(i == (0, 0, 0, 0) for i in _level_info(s))
        assert np.isfinite(z["off"][0]).all() and np.abs(z["off"][0][:n_u]).max() > 0
        for zs in z.values():
            for a in zs:
                assert np.array_equal(a, z["untouched"][0])
    finally:
        s.close()


def test_general_patch_vcycle_on_the_cylinder_is_deterministic_replays_and_converges():
    """the mirror's cylinder at 3 refinements (7424 cells, four levels down to the 116 coarse cells, none of them a box) with uu_smoother = 1, uu_patch_levels = 1: every
    level takes the patches; three eager applications of the V-cycle and three through the captured graph (eager, capture, replay: each level's
    own number of colour launches) are the same bits and differ from the node-block result; the first time step then reaches the reference's
    constants 0.374235 / 46.5226 within 1e-3 (the bound of test_cylinder_level_chain_from_the_refinement_history)"""
    from openifem_amd import capi
    s = _cylinder_flow(3)
    try:
        assert len(s.all_ctxs()) == 4 and s.opts.ainv_kind == capi.AINV_MG  # refinements 3 .. 0
        maxit = s.opts.inner_maxit
        s.opts.inner_maxit = 0
        s.assemble(False)
        _, n_u, n_p = s.sizes()
        g = np.arange(n_u + n_p)
        v = np.cos(0.37 * g) + 0.1 * np.sin(1.3 * g)
        ip = capi.make_params(**CYL)
        blocks = _precond(s, ip, v)
        z = {}
        for cells in (262144, 0):
            _set_tuning(s, uu_smoother=1, uu_patch_levels=1, vcycle_graph_cells=cells)
            before = capi.vcycle_graph_stats(s.L, s.ctx)
            z[cells] = [_precond(s, ip, v) for _ in range(3)]
            after = capi.vcycle_graph_stats(s.L, s.ctx)
            print(f"cylinder, per-patch inverses, vcycle_graph_cells = {cells}: hipGraph captures {after[0] - before[0]}, launches {after[1] - before[1]}")
            if cells:
                assert after[0] - before[0] >= 1 and after[1] - before[1] >= 2  # the graphs were captured and replayed
            else:
                assert after[1] == before[1]
        info = _level_info(s)
        print("cylinder levels (eligible, patches, inverses, bytes):", info)
        assert all(i[0] == 1 and i[1] > 0 and i[2] == i[1] and i[3] > 0 for i in info)
        assert np.isfinite(z[0][0]).all() and np.abs(z[0][0][:n_u]).max() > 0
        for a in z[262144] + z[0]:
            assert np.array_equal(a, z[0][0])
        assert not np.array_equal(z[0][0][:n_u], blocks[:n_u])  # it is another smoother
        s.opts.inner_maxit = maxit
        _set_tuning(s, uu_smoother=1, uu_patch_levels=1)
        s.run_one_step(True)
        vel, p = s.get_current_solution()
        st = s.last_stats()
        print(f"cylinder, per-patch inverses: vmax {vel.max():.6f}, pmax {p.max():.4f}, FGMRES {st.fgmres_iters}, inner {st.inner_iters} in {st.precond_applies} applications")
        assert abs(vel.max() - 0.374235) / 0.374235 < 1e-3 and abs(p.max() - 46.5226) / 46.5226 < 1e-3
    finally:
        s.close()


def test_general_patches_need_no_more_inner_iterations_on_the_cylinder():
    """the mirror's cylinder at 4 refinements, zero state (no convective term: the operator is A0 at gamma rho / mu = 100), product default
    options, a fresh context per smoother: assemble(False) + solve(False) converges to 1.05e-4 ||b|| and the vertex patches need no more inner
    iterations than the node blocks.  At the zero state the zero-constraint right-hand side has nothing but rounding in it, so the same is asked
    of assemble(True) + solve(True) on the same context, whose right-hand side carries the inflow profile (the operator is still A0).
    Measured on one MI355X (non-zero constraints): 37 inner iterations with the node blocks, 14 with the patches, 4 FGMRES iterations with
    both; with zero constraints ||b|| = 0 and neither solver iterates.  The table over 3 - 6 refinements: profiles/patch_general.txt"""
    counts = {}
    for knob in (0, 1):
        s = _cylinder_flow(4)
        try:
            if knob:
                _set_tuning(s, uu_smoother=1, uu_patch_levels=1)
            for nonzero in (False, True):
                s.assemble(nonzero)
                st = s.solve(nonzero)
                res, bn = s.true_residual()
                counts[knob, nonzero] = (st.inner_iters, st.fgmres_iters, st.precond_applies, res, bn)
            if knob:
                assert all(i[0] == 1 and i[2] == i[1] > 0 for i in _level_info(s))
        finally:
            s.close()
    for key, (inner, fg, app, res, bn) in sorted(counts.items()):
        print(f"uu_smoother = {key[0]}, non-zero constraints {key[1]}: inner iterations {inner}, FGMRES iterations {fg}, "
              f"preconditioner applications {app}, true residual {res:.3e}, ||b|| {bn:.3e}")
    for nonzero in (False, True):
        assert counts[1, nonzero][3] <= 1.05e-4 * counts[1, nonzero][4]
        assert counts[1, nonzero][0] <= counts[0, nonzero][0]
    assert counts[0, True][0] > 0 and counts[1, True][4] > 0


def test_a_partitioned_cylinder_level_keeps_the_node_blocks():
    """two virtual ranks of CylinderMesh(0), cut through the ring: a partitioned level is not eligible with both switches on, and the V-cycle
    gives the same bits as with them off (same assembly)"""
    from openifem_amd import capi
    m = CylinderMesh(0)
    rng = np.random.default_rng(19)
    dofs, vals = _cyl2d_bcs(m)
    ev, pr, x = rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_dofs)
    Pm = capi.make_params(mu=0.7, rho=1.3, gamma=0.2, dt=0.01)
    cell_rank = (m.vcoords.mean(axis=1)[:, 0] > 0.25).astype(int)
    assert 0 < cell_rank.sum() < m.n_cells
    parts = partition_mesh(m, cell_rank, 2)

    def work(rank, P, ctx):
        ld, lv = local_dirichlet(P, dofs, vals)
        ctx.set_constraints(0, ld, None)
        ctx.set_constraints(1, ld, lv)
        ctx.vec_set(capi.VEC_PRESENT, pr[P.ext_gdof])
        ctx.vec_set(capi.VEC_EVAL, ev[P.ext_gdof])
        ctx.opts.ainv_kind = capi.AINV_MG
        ctx.assemble(Pm, False)
        out, info = {}, {}
        for knob in (0, 1):
            ctx.set_tuning(uu_smoother=knob, uu_patch_levels=knob)
            info[knob] = tuple(ctx.uu_patch_info())
            out[knob] = ctx.precond_vmult(Pm, x[P.own_gdof])
        return info, out

    for info, out in run_virtual_ranks(capi, parts, work):
        assert info[0] == info[1] == (False, 0, 0, 0)
        assert np.isfinite(out[0]).all() and np.abs(out[0]).max() > 0
        assert np.array_equal(out[0], out[1])
