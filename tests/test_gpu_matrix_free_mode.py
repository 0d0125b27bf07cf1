"""ifem_tuning::stored_uu = 0 as a complete mode, through the C ABI: non-zero constraint values (either set) reach the right-hand
side through the matrix-free inhomogeneity lift (apply_mf.hip::uu_lift_mf) and hanging-node lines are condensed around the
matrix-free operator -- no assembly of the mode allocates A_uu values (ifem_uu_stored_bytes == 0).

The checker is the oracle: its literal distribute_local_to_global (orc_ins_assemble, orc_ins_assemble_affine_dense) gives the
right-hand side K g has been moved into; on constrained rows the oracle's diagonal is |Ke_rr| summed over the cells while this
mode applies the diagonal of its own node blocks (integrated in single precision by default), so those rows are checked for
CONSISTENCY of the two sides of the equation (rhs_r = d_r g_r with the d_r the operator applies), which is what makes the update
equal g_r there.  Reference: mpi_insim.cpp:343-355 (distribute_local_to_global), :390 (constraints.distribute)."""
import ctypes as C
import os

import numpy as np
import pytest

import orc
from boxmesh import BoxMesh
from hangmesh import HangingMesh
from partmesh import gather_owned, local_dirichlet, partition_mesh, run_virtual_ranks

pytestmark = pytest.mark.gpu

KW = dict(mu=0.7, rho=1.3, gamma=0.1, dt=0.05, neumann={1: 2.0})
INFLOW = {0: lambda p, c: 0.3 + 0.5 * p[1] if c == 0 else 0.1 * p[1]}


def _capi():
    from openifem_amd import capi
    return capi


def _kw(dim):
    return dict(KW, g=(0.2, -9.8, 0.4)[:dim])


def _bcs(dim):
    flag = 3 if dim == 2 else 7
    return {0: (flag, [0.3, -0.2, 0.1][:dim]), 2: (flag, [0.0] * dim)}


def _matrix_free(ctx, capi):
    ctx.set_tuning(stored_uu=0)
    ctx.opts.ainv_kind = capi.AINV_GMRES_BJACOBI_MF


# ---------------------------------------------------------------------------------------------------------------------
# 1. the lift against the oracle on conforming meshes

def _box(dim, kv, seed):
    reps = {(2, 2): (5, 3), (2, 1): (6, 4), (3, 2): (3, 2, 2), (3, 1): (3, 3, 2)}[(dim, kv)]
    rng = np.random.default_rng(seed)
    m = BoxMesh(reps, (0,) * dim, (1.0, 0.6, 0.4)[:dim], kv=kv)
    m.vcoords = m.vcoords.copy()
    m.vcoords += 0.02 * rng.standard_normal(m.vcoords.shape)  # d-linear distorted cells (general Jacobians)
    dofs, vals = m.dirichlet(_bcs(dim), INFLOW)
    assert np.abs(vals).max() > 0
    ev, pr = 0.3 * rng.standard_normal(m.n_dofs), 0.3 * rng.standard_normal(m.n_dofs)
    return m, dofs, vals, ev, pr, rng


def _conforming(dim, kv, use_nonzero, seed, values_in_set0=False):
    capi = _capi()
    m, dofs, vals, ev, pr, rng = _box(dim, kv, seed)
    S = orc.System(m)
    S.set_constraints(0, dofs, vals if values_in_set0 else None)
    S.set_constraints(1, dofs, vals)
    S.assemble(orc.make_params(**_kw(dim)), use_nonzero, ev, pr)
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    _matrix_free(ctx, capi)
    ctx.set_constraints(0, dofs, vals if values_in_set0 else None)
    ctx.set_constraints(1, dofs, vals)
    ctx.vec_set(capi.VEC_PRESENT, pr)
    ctx.vec_set(capi.VEC_EVAL, ev)
    ctx.assemble(capi.make_params(**_kw(dim)), use_nonzero)
    return m, ctx, capi, S, dofs, vals, rng


def _check_lifted_rhs(m, ctx, capi, S, dofs, g):
    b, bo = ctx.vec_get(capi.VEC_RHS), S.rhs()
    free = np.ones(m.n_dofs, bool)
    free[dofs] = False
    err = np.abs(b[free] - bo[free]).max() / np.abs(bo).max()
    print("free rows: |b - b_oracle| / max|b_oracle| =", err)
    assert err <= 1e-11
    # constrained rows: the same diagonal on both sides of the equation
    x = np.zeros(m.n_dofs)
    x[dofs] = g
    y = ctx.system_vmult(x)
    errc = np.abs(b[dofs] - y[dofs]).max() / np.abs(y[dofs]).max()
    print("constrained rows: |b_r - (A x_g)_r| / max =", errc)
    assert errc <= 1e-12
    nz = g != 0
    assert np.all(y[dofs][nz] / g[nz] > 0)
    assert ctx.uu_stored_bytes() == 0


@pytest.mark.parametrize("dim,kv", [(2, 2), (2, 1), (3, 2), (3, 1)])
def test_lifted_rhs_matches_the_oracle(dim, kv):
    m, ctx, capi, S, dofs, vals, _ = _conforming(dim, kv, True, 7 + dim + kv)
    _check_lifted_rhs(m, ctx, capi, S, dofs, vals)
    ctx.close()


def test_lift_serves_the_imex_matrix_too():
    # InsIMEX::assemble (no convective terms in the matrix: the CONV = false instantiation of the lift kernel)
    capi = _capi()
    m, dofs, vals, ev, pr, _ = _box(3, 2, 23)
    S = orc.System(m)
    S.set_constraints(0, dofs, None)
    S.set_constraints(1, dofs, vals)
    S.imex_assemble(orc.make_params(**_kw(3)), True, True, pr)
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    _matrix_free(ctx, capi)
    ctx.set_constraints(0, dofs, None)
    ctx.set_constraints(1, dofs, vals)
    ctx.vec_set(capi.VEC_PRESENT, pr)
    ctx.imex_assemble(capi.make_params(**_kw(3)), True, True)
    _check_lifted_rhs(m, ctx, capi, S, dofs, vals)
    ctx.close()


def test_values_in_constraint_set_0_are_lifted_as_well():
    # use_nonzero = False with non-zero values handed to set 0: the oracle (AffineConstraints) moves K g for whichever object
    # the assembly uses
    m, ctx, capi, S, dofs, vals, _ = _conforming(3, 2, False, 31, values_in_set0=True)
    _check_lifted_rhs(m, ctx, capi, S, dofs, vals)
    ctx.close()


def test_homogeneous_set_keeps_the_plain_matrix_free_assembly():
    m, ctx, capi, S, dofs, vals, _ = _conforming(2, 2, False, 37)
    b, bo = ctx.vec_get(capi.VEC_RHS), S.rhs()
    assert np.abs(b - bo).max() <= 1e-11 * np.abs(bo).max() and np.abs(b[dofs]).max() == 0
    assert ctx.uu_stored_bytes() == 0
    ctx.close()


def test_pressure_dofs_cannot_be_constrained_so_the_lift_has_no_bt_half():
    # the B^T half of the lift (b_u -= B0^T[:, constrained p] g_p) would serve constrained PRESSURE dofs: ifem_set_constraints
    # refuses those for every mode (api.hip: "pressure Dirichlet constraints are not supported"), so there is nothing to lift and
    # nothing to compare; the refusal itself is what is pinned here
    capi = _capi()
    m, dofs, vals, ev, pr, _ = _box(2, 2, 41)
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    _matrix_free(ctx, capi)
    with pytest.raises(capi.IfemError) as e:
        ctx.set_constraints(1, np.append(dofs, m.n_u + 1), np.append(vals, 0.7))
    assert "pressure" in str(e.value)
    ctx.close()


def test_repeated_inhomogeneous_assemblies_survive_the_release_of_the_unconstrained_blocks():
    # the geometry cache gives its unconstrained B / B^T back after a few assemblies with an unchanged set; the lift needs B and
    # has them re-integrated once
    m, ctx, capi, S, dofs, vals, _ = _conforming(3, 2, True, 43)
    for _ in range(4):
        ctx.assemble(capi.make_params(**_kw(3)), True)
        _check_lifted_rhs(m, ctx, capi, S, dofs, vals)
    ctx.close()


def test_refused_assembly_leaves_the_context_and_the_device_as_they_were():
    # stored_uu = 0 takes B / B^T from the geometry cache: with geo_cache = 0 the assembly is refused, and the refusal comes before
    # anything is zero-filled or recorded -- the next accepted assembly of the same set KEEPS the cached blocks, so it shows what
    # the refused one left behind.  (The sums are atomic-ordered: 1e-12 of the largest entry, not bitwise.)
    capi = _capi()
    m, dofs, vals, ev, pr, rng = _box(3, 2, 47)
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    _matrix_free(ctx, capi)
    ctx.set_constraints(0, dofs, None)
    ctx.set_constraints(1, dofs, vals)
    ctx.vec_set(capi.VEC_PRESENT, pr)
    ctx.vec_set(capi.VEC_EVAL, ev)
    P = capi.make_params(**_kw(3))
    ctx.assemble(P, True)
    x = rng.standard_normal(m.n_dofs)
    y0, b0 = ctx.system_vmult(x), ctx.vec_get(capi.VEC_RHS)
    assert ctx.uu_stored_bytes() == 0
    ctx.set_tuning(geo_cache=0)
    with pytest.raises(capi.IfemError) as e:
        ctx.assemble(P, True)
    assert e.value.code == capi.E_BADPARAM and "geo_cache" in str(e.value)
    assert ctx.uu_stored_bytes() == 0
    ctx.set_tuning(geo_cache=1)
    ctx.assemble(P, True)
    y1, b1 = ctx.system_vmult(x), ctx.vec_get(capi.VEC_RHS)
    ey, eb = np.abs(y1 - y0).max() / np.abs(y0).max(), np.abs(b1 - b0).max() / np.abs(b0).max()
    print("after the refusal: system_vmult", ey, "rhs", eb)
    assert ey <= 1e-12 and eb <= 1e-12
    assert ctx.uu_stored_bytes() == 0
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. Newton update

@pytest.mark.parametrize("dim,kv", [(2, 2), (3, 2)])
def test_newton_update_matches_the_dense_solve_of_the_oracles_system(dim, kv):
    m, ctx, capi, S, dofs, vals, _ = _conforming(dim, kv, True, 11 + dim + kv)
    ctx.opts.fgmres_rel = 1e-10
    ctx.opts.inner_rel = 1e-3
    st = ctx.solve(capi.make_params(**_kw(dim)), True)
    upd = ctx.vec_get(capi.VEC_UPDATE)
    xo = np.linalg.solve(S.csr("A").toarray(), S.rhs())
    assert np.abs(xo[dofs] - vals).max() <= 1e-12  # (constraints.distribute: the constrained entries are their values)
    assert st.fgmres_iters < 200
    err = np.abs(upd - xo).max() / np.abs(xo).max()
    print("update against the dense solve:", err)
    assert err <= 1e-6
    assert ctx.uu_stored_bytes() == 0
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. hanging nodes

def _hmesh(dim, kv):
    if dim == 2:
        return HangingMesh((3, 2), (0, 0), (1.5, 0.8), {(0, 0), (2, 1)}, kv=kv)
    return HangingMesh((2, 2, 2), (0, 0, 0), (1.0, 0.8, 0.6), {(0, 0, 0)}, kv=kv)


def _hanging(dim, kv, use_nonzero, seed, mf_f32=1):
    capi = _capi()
    m = _hmesh(dim, kv)
    assert len(m.hang_dof) > 0
    rng = np.random.default_rng(seed)
    # inflow profile on x- (some masters of hanging lines on the boundary carry a value), no-slip on y-
    dofs, vals = m.dirichlet(_bcs(dim), INFLOW)
    ev, pr = 0.3 * rng.standard_normal(m.n_dofs), 0.3 * rng.standard_normal(m.n_dofs)
    S = orc.System(m)
    S.set_constraints(0, dofs, None)
    S.set_constraints(1, dofs, vals)
    Ao, bo = S.assemble_affine_dense(orc.make_params(**_kw(dim)), use_nonzero, ev, pr, m)
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    _matrix_free(ctx, capi)
    ctx.set_tuning(mf_f32=mf_f32)
    ctx.set_constraints(0, dofs, None)
    ctx.set_constraints(1, dofs, vals)
    ctx.set_hanging_constraints(m.hang_dof, m.hang_ptr, m.hang_master, m.hang_weight)
    ctx.vec_set(capi.VEC_PRESENT, pr)
    ctx.vec_set(capi.VEC_EVAL, ev)
    ctx.assemble(capi.make_params(**_kw(dim)), use_nonzero)
    return m, ctx, capi, Ao, bo, dofs, vals, rng


@pytest.mark.parametrize("dim,kv", [(2, 2), (2, 1), (3, 2), (3, 1)])
@pytest.mark.parametrize("use_nonzero", [True, False])
@pytest.mark.parametrize("mf_f32", [1, 0])
def test_condensed_system_with_hanging_nodes_matches_distribute_local_to_global(dim, kv, use_nonzero, mf_f32):
    """mf_f32 = 1 (the default): the node blocks, and with them the diagonal d_r of the Dirichlet and hanging rows, are integrated in
    single precision -- those decoupled rows are checked for the consistency of d_r between operator and right-hand side.
    mf_f32 = 0: d_r is the fp64 sum of |Ke_rr| over the cells, the oracle's own definition, and EVERY regular row of the right-hand
    side and of the operator is compared literally."""
    m, ctx, capi, Ao, bo, dofs, vals, rng = _hanging(dim, kv, use_nonzero, 5 + dim + kv, mf_f32)
    assert ctx.uu_stored_bytes() == 0
    hang = m.hang_dof
    free = np.ones(m.n_dofs, bool)
    free[dofs] = False
    free[hang] = False  # regular rows that are not Dirichlet rows (those are checked for consistency in section 1)
    reg = np.setdiff1d(np.arange(m.n_dofs), hang)
    b = ctx.vec_get(capi.VEC_RHS)
    err = np.abs(b[free] - bo[free]).max() / np.abs(bo).max()
    print("condensed rhs, regular rows:", err)
    assert err <= 1e-11
    if not mf_f32:
        assert np.abs(b[reg] - bo[reg]).max() <= 1e-11 * np.abs(bo).max()
    hu = hang < m.n_u
    for _ in range(3):
        x = rng.standard_normal(m.n_dofs)
        y, yo = ctx.system_vmult(x), Ao @ x
        erro = np.abs(y[free] - yo[free]).max() / np.abs(yo).max()
        print("condensed operator, regular rows:", erro)
        assert erro <= 1e-11
        if not mf_f32:
            assert np.abs(y[reg] - yo[reg]).max() <= 1e-11 * np.abs(yo).max()
            assert np.abs(y[hang][hu] / x[hang][hu] - Ao[hang[hu], hang[hu]]).max() <= 1e-10 * np.abs(Ao.diagonal()).max()
        # Dirichlet rows: decoupled, positive diagonal, the same one the right-hand side carries
        dr = y[dofs] / x[dofs]
        assert np.all(dr > 0)
        g = vals if use_nonzero else 0 * vals
        assert np.abs(b[dofs] - dr * g).max() <= 1e-12 * max(np.abs(dr * g).max(), 1e-300) + 0.0
        # hanging rows: decoupled with a positive diagonal, and the equation d_h x_h = rhs_h has the oracle's solution
        d = y[hang] / x[hang]
        assert np.all(d > 0)
        x2 = x.copy()
        x2[reg] = 0
        assert np.abs(ctx.system_vmult(x2)[reg]).max() == 0  # no coupling from the hanging columns
        sol, solo = b[hang] / d, bo[hang] / Ao[hang, hang]
        errh = np.abs(sol[hu] - solo[hu]).max()
        print("hanging rows, rhs_h / d_h:", errh)
        assert errh <= 1e-10 * max(np.abs(solo).max(), 1.0)
    ctx.close()


@pytest.mark.parametrize("dim,kv", [(2, 2), (3, 2)])
def test_newton_update_with_hanging_nodes_matches_the_dense_solve(dim, kv):
    m, ctx, capi, Ao, bo, dofs, vals, rng = _hanging(dim, kv, True, 11 + dim + kv)
    ctx.opts.fgmres_rel = 1e-10
    ctx.opts.inner_rel = 1e-3
    st = ctx.solve(capi.make_params(**_kw(dim)), True)
    upd = ctx.vec_get(capi.VEC_UPDATE)
    xo = m.prolongation() @ np.linalg.solve(Ao, bo)
    assert st.fgmres_iters < 200
    err = np.abs(upd - xo).max() / np.abs(xo).max()
    print("update against the dense solve:", err)
    assert err <= 1e-6
    assert np.abs(upd - m.prolongation() @ upd).max() <= 1e-12 * np.abs(upd).max()
    assert ctx.uu_stored_bytes() == 0
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. Poiseuille on a hanging mesh

def test_poiseuille_on_a_hanging_node_mesh_without_a_stored_block():
    capi = _capi()
    m = HangingMesh((4, 2), (0, 0), (2.0, 0.2), {(1, 0), (2, 1)}, kv=2)
    dofs, vals = m.dirichlet({2: (3, [0, 0]), 3: (3, [0, 0])})
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    _matrix_free(ctx, capi)
    ctx.set_constraints(0, dofs, None)
    ctx.set_constraints(1, dofs, vals)
    ctx.set_hanging_constraints(m.hang_dof, m.hang_ptr, m.hang_master, m.hang_weight)
    ctx.opts.fgmres_rel = 1e-8
    P = capi.make_params(mu=1.0, rho=1.0, gamma=0.1, dt=1e-3, neumann={0: 10.0})
    ctx.vec_set(capi.VEC_PRESENT, np.zeros(m.n_dofs))
    for step in range(80):
        rc, _ = ctx.newton_step(P, step == 0)
        assert rc > 0
    v = ctx.vec_get(capi.VEC_PRESENT)[:m.n_u].reshape(-1, 2)
    y = m.unode_coords[:, 1]
    exact = 10.0 / (2 * 1.0 * 2.0) * y * (0.2 - y)
    assert abs(v[:, 0].max() - 2.5e-2) / 2.5e-2 < 1e-6
    assert np.abs(v[:, 0] - exact).max() < 1e-7 and np.abs(v[:, 1]).max() < 1e-7
    assert ctx.uu_stored_bytes() == 0
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. virtual ranks

def _cell_ranks(m, nranks):
    c = m.vcoords.mean(axis=1)
    mid = 0.5 * (c.min(axis=0) + c.max(axis=0))
    r = (c[:, 0] > mid[0]).astype(int)
    if nranks == 4:
        r += 2 * (c[:, 1] > mid[1]).astype(int)
    return r


def _run_ranks(m, nranks, dofs, vals, ev, pr, hanging, solve):
    capi = _capi()
    parts = partition_mesh(m, _cell_ranks(m, nranks) if nranks > 1 else np.zeros(m.n_cells, int), nranks)
    Pm = capi.make_params(**_kw(m.dim))

    def work(rank, P, ctx):
        _matrix_free(ctx, capi)
        ld, lv = local_dirichlet(P, dofs, vals)
        ctx.set_constraints(0, ld, None)
        ctx.set_constraints(1, ld, lv)
        if hanging:
            ctx.set_hanging_constraints(P.hang_dof, P.hang_ptr, P.hang_master, P.hang_weight)
        ctx.vec_set(capi.VEC_PRESENT, pr[P.ext_gdof])
        ctx.vec_set(capi.VEC_EVAL, ev[P.ext_gdof])
        ctx.opts.fgmres_rel = 1e-10
        ctx.opts.inner_rel = 1e-3
        ctx.assemble(Pm, True)
        out = {"rhs": ctx.vec_get(capi.VEC_RHS), "upd": np.zeros(P.n_owned)}
        if solve:
            ctx.solve(Pm, True)
            out["upd"] = ctx.vec_get(capi.VEC_UPDATE)
        out["bytes"] = ctx.uu_stored_bytes()
        return out

    res = run_virtual_ranks(capi, parts, work)
    assert all(r["bytes"] == 0 for r in res)
    return tuple(gather_owned(parts, [r[k] for r in res], m.n_dofs) for k in ("rhs", "upd"))


@pytest.mark.parametrize("nranks", [2, 4])
def test_conforming_box_with_inflow_values_on_virtual_ranks(nranks):
    rng = np.random.default_rng(51)
    m = BoxMesh((4, 4, 2), (0, 0, 0), (1.0, 0.6, 0.4), kv=2)
    dofs, vals = m.dirichlet(_bcs(3), INFLOW)
    ev, pr = 0.3 * rng.standard_normal(m.n_dofs), 0.3 * rng.standard_normal(m.n_dofs)
    b1, u1 = _run_ranks(m, 1, dofs, vals, ev, pr, False, True)
    bN, uN = _run_ranks(m, nranks, dofs, vals, ev, pr, False, True)
    S = orc.System(m)  # the single context of this mode is itself tied to the oracle
    S.set_constraints(1, dofs, vals)
    S.assemble(orc.make_params(**_kw(3)), True, ev, pr)
    free = np.ones(m.n_dofs, bool)
    free[dofs] = False
    assert np.abs(b1[free] - S.rhs()[free]).max() <= 1e-11 * np.abs(S.rhs()).max()
    eb, eu = np.abs(bN - b1).max() / np.abs(b1).max(), np.abs(uN - u1).max() / np.abs(u1).max()
    print("ranks against one context: rhs", eb, "update", eu)
    assert eb <= 1e-6 and eu <= 1e-6


@pytest.mark.parametrize("dim", [2, 3])
def test_hanging_meshes_on_two_virtual_ranks(dim):
    if dim == 2:
        m = HangingMesh((6, 4), (0, 0), (3.0, 1.6), {(1, 1), (2, 1), (2, 2), (4, 0), (3, 3)}, kv=2)
    else:
        m = HangingMesh((3, 2, 2), (0, 0, 0), (1.5, 0.8, 0.6), {(0, 0, 0), (2, 1, 1)}, kv=2)
    rng = np.random.default_rng(100 + dim)
    dofs, vals = m.dirichlet(_bcs(dim), INFLOW)
    ev, pr = 0.3 * rng.standard_normal(m.n_dofs), 0.3 * rng.standard_normal(m.n_dofs)
    b1, u1 = _run_ranks(m, 1, dofs, vals, ev, pr, True, True)
    bN, uN = _run_ranks(m, 2, dofs, vals, ev, pr, True, True)
    S = orc.System(m)
    S.set_constraints(0, dofs, None)
    S.set_constraints(1, dofs, vals)
    Ao, bo = S.assemble_affine_dense(orc.make_params(**_kw(dim)), True, ev, pr, m)
    free = np.ones(m.n_dofs, bool)
    free[dofs] = False
    free[m.hang_dof] = False
    assert np.abs(b1[free] - bo[free]).max() <= 1e-11 * np.abs(bo).max()
    xo = m.prolongation() @ np.linalg.solve(Ao, bo)
    assert np.abs(u1 - xo).max() <= 1e-6 * np.abs(xo).max()
    eb, eu = np.abs(bN - b1).max() / np.abs(b1).max(), np.abs(uN - u1).max() / np.abs(u1).max()
    print("ranks against one context: rhs", eb, "update", eu)
    assert eb <= 1e-6 and eu <= 1e-6
    Cm = m.prolongation()
    assert np.abs(uN - Cm @ uN).max() <= 1e-12 * np.abs(uN).max()


# ---------------------------------------------------------------------------------------------------------------------
# 6. cylinder time step

def test_cylinder_time_step_never_allocates_the_block():
    from openifem_amd import capi, host
    prm = open(os.path.join(os.path.dirname(__file__), "golden", "prm", "fluid_cylinder_mpi.prm")).read()
    out = {}
    for stored in (1, 0):
        flow = host.InsIM(prm, mesh="cylinder")
        flow.add_hard_coded_boundary_condition(0, lambda p, c, t: 4 * 0.3 * p[1] * (0.41 - p[1]) / (0.41 * 0.41) if (c == 0 and abs(p[0]) < 1e-10) else 0.0)
        flow.setup(3)
        tun = capi.Tuning()
        flow.L.ifem_default_tuning(C.byref(tun))
        tun.stored_uu = stored
        for c_ in flow.all_ctxs():
            assert flow.L.ifem_set_tuning(c_, C.byref(tun)) == 0
        flow.run_one_step(True)
        v, p = flow.get_current_solution()
        out[stored] = (v.max(), p.max(), flow.last_newton()[0], [int(flow.L.ifem_uu_stored_bytes(c_)) for c_ in flow.all_ctxs()])
        flow.close()
    print(out)
    assert abs(out[0][0] - 0.374235) / 0.374235 < 1e-3 and abs(out[0][1] - 46.5226) / 46.5226 < 1e-3, out
    assert out[0][2] == out[1][2], out  # the same number of Newton iterations
    assert out[1][3][0] > 0
    assert all(b == 0 for b in out[0][3]), out  # after the whole loop, on every context of the hierarchy


# ---------------------------------------------------------------------------------------------------------------------
# 7. FSI caller

def test_fsi_step_on_the_locally_refined_leaflet_mesh():
    """One step of the fluid side of MPI::FSI::run on one context: moving solid -> indicator, Dirichlet lines v_solid - present
    merged into both constraint objects (fsi.hip marks set 1 inhomogeneous on every step: the caller the lift exists for),
    Newton loop with apply_nonzero_constraints.  The mirror's own leaflet case (tests/test_gpu_fsi_caller.py::
    mirror_loop_device_inputs) is SCnsIM<2> Q1/Q1, which has its own A_pp and always stores its blocks, so it cannot run in this
    mode; this is the same channel, the same refined band, the same moving solid and the same device-produced inputs with the
    InsIM Q2/Q1 fluid the mode serves."""
    capi = _capi()
    import test_gpu_fsi_caller as F
    reps = (int(F.L_ / F.HC), int(F.H_ / F.HC))
    refine = {(i, j) for i in range(reps[0]) for j in range(reps[1]) if F.L_ / 4 - 2 * F.A_ <= (i + 0.5) * F.HC <= F.L_ / 4 + 3 * F.A_}
    m = HangingMesh(reps, (0, 0), (F.L_, F.H_), refine, kv=2)
    assert len(m.hang_dof) > 0
    bdofs, bvals = m.dirichlet({0: (3, [0, 0]), 2: (3, [0, 0]), 3: (3, [0, 0])},
                               {0: lambda p, c: 6.0 * p[1] * (F.H_ - p[1]) / F.H_ ** 2 if c == 0 else 0.0})
    P = capi.make_params(mu=F.KW["mu"], rho=F.KW["rho"], gamma=0.1, dt=F.KW["dt"])
    out = {}
    for stored in (1, 0):
        ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
        ctx.set_tuning(stored_uu=stored)
        ctx.opts.ainv_kind = capi.AINV_GMRES_BJACOBI_MF
        ctx.opts.fgmres_rel = 1e-10
        ctx.set_hanging_constraints(m.hang_dof, m.hang_ptr, m.hang_master, m.hang_weight)
        ctx.vec_set(capi.VEC_PRESENT, np.zeros(m.n_dofs))
        s = F._meshed_solid(0)
        ctx.fsi_set_solid(s.vertices, s.cells, s.bfaces, s.velocity, s.acceleration, s.stress)
        ind, _ = ctx.fsi_update_indicator(m.n_cells)
        assert ind.sum() > 0
        ctx.set_constraints(1, bdofs, bvals)
        ctx.set_constraints(0, bdofs, None)
        st = ctx.fsi_find_fluid_bc(F.KW["dt"], True)
        assert st.n_not_found == 0
        flags, cv = ctx.get_constraints(1)
        assert flags.sum() > len(bdofs) and np.abs(cv).max() > 0
        rc, _ = ctx.newton_step(P, True, tol=1e-8, maxit=10)
        assert rc > 0
        out[stored] = (ctx.vec_get(capi.VEC_PRESENT), ctx.uu_stored_bytes())
        ctx.close()
    n_u = m.n_u
    ev = np.abs(out[0][0][:n_u] - out[1][0][:n_u]).max() / np.abs(out[1][0][:n_u]).max()
    ep = np.abs(out[0][0][n_u:] - out[1][0][n_u:]).max() / np.abs(out[1][0][n_u:]).max()
    print("present, matrix-free against the block CSR: velocity", ev, "pressure", ep)
    assert ev <= 1e-6 and ep <= 1e-6
    assert out[1][1] > 0 and out[0][1] == 0
