"""The M_p solve of the block preconditioner by tensor-product line solves (csrc/mp_direct.hip; ifem_solver_opts::mp_solver = 0) through the
test aid ifem_test_mp_solve, and through ifem_solve.

Reference of the correctness cases: M_p from the CSR export, dense, fp64, numpy.linalg.solve.  Bound max|x - x_ref| <= 1e-11 max|x_ref|:
kappa(M_d) <= 6 per axis, so kappa(M_p) <= 216; 216 x 2.2e-16 with a factor of about 200 for the two solves that are compared and the
rounding of the assembly's atomic order gives about 1e-11.  The achieved value is printed.
Shapes: three different counts and edges with an origin off zero, 2 x 2 one-dimensional matrices, lines longer than a wave / the 32-column
tile of the contiguous axis / the 16-entry batch of the strided axes on each axis in turn, 2D, Q1 velocity, Morton and random node orders.
The contexts that must keep CG (a moved vertex, hanging nodes, two ranks, mp_solver = 1) are checked against the stopping rule of that CG
on the exported matrix."""
import ctypes as C

import numpy as np
import pytest

from boxmesh import BoxMesh
from partmesh import partition_mesh, run_virtual_ranks

pytestmark = pytest.mark.gpu

KW = dict(mu=0.7, rho=1.3, gamma=0.2, dt=0.01)
BOUND = 1e-11
EXTENT = (2.0, 0.2, 0.2)


def _capi():
    from openifem_amd import capi
    return capi


def _bcs(dim):
    flag = 3 if dim == 2 else 7
    bcs = {0: (flag, [0.3, -0.2, 0.1][:dim]), 2: (flag, [0.0] * dim), 3: (flag, [0.0] * dim)}
    if dim == 3:
        bcs.update({4: (flag, [0.0] * dim), 5: (flag, [0.0] * dim)})
    return bcs


def _assembled(m, seed, cell_pnodes=None, hanging=False):
    capi = _capi()
    rng = np.random.default_rng(seed)
    dofs, vals = m.dirichlet(_bcs(m.dim))
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes if cell_pnodes is None else cell_pnodes, m.cell_face_bid,
                       m.n_unodes, m.n_pnodes)
    ctx.set_constraints(0, dofs, None)
    ctx.set_constraints(1, dofs, vals)
    if hanging:
        ctx.set_hanging_constraints(m.hang_dof, m.hang_ptr, m.hang_master, m.hang_weight)
    ctx.vec_set(capi.VEC_PRESENT, rng.standard_normal(m.n_dofs))
    ctx.vec_set(capi.VEC_EVAL, rng.standard_normal(m.n_dofs))
    ctx.assemble(capi.make_params(**KW), False)
    return ctx, rng


def _mass(ctx, n_u_owned, n_u_local):
    """M_p of the context (owned rows x local columns) from the mass export, dense"""
    return ctx.export_csr(1)[n_u_owned:, n_u_local:].toarray()


def _check_direct(ctx, Mp, rhs, tag):
    for name, b in rhs:
        x, direct, its = ctx.mp_solve(b)
        ref = np.linalg.solve(Mp, b)
        err = np.abs(x - ref).max() / np.abs(ref).max()
        print(f"{tag}, {name}: direct {direct}, CG iterations {its}, max|x - x_ref| / max|x_ref| = {err:.2e}")
        assert direct and its == 0
        assert err <= BOUND


def _rhs(rng, n, corner, interior):
    ec, ei = np.zeros(n), np.zeros(n)
    ec[corner], ei[interior] = 1.0, 1.0
    return [("random", rng.standard_normal(n)), ("unit vector at a corner node", ec), ("unit vector at an interior node", ei)]


def _box_case(reps, p0, p1, kv, seed, tag, all_rhs=False, perm=False):
    m = BoxMesh(reps, p0, p1, kv=kv)
    rng = np.random.default_rng(1000 + seed)
    cp = None
    node = np.arange(m.n_pnodes)
    if perm:  # a seeded random renumbering of the pressure nodes in the arrays handed to ifem_ctx_create
        node = rng.permutation(m.n_pnodes)
        cp = node[m.cell_pnodes].astype(np.int32)
    ctx, _ = _assembled(m, seed, cell_pnodes=cp)
    Mp = _mass(ctx, m.n_u, m.n_u)
    assert Mp.shape == (m.n_pnodes, m.n_pnodes)
    rhs = [("random", rng.standard_normal(m.n_pnodes))]
    if all_rhs:
        inner = np.nonzero(np.all((m.pnode_lattice > 0) & (m.pnode_lattice < np.array(m.np1) - 1), axis=1))[0]
        rhs = _rhs(rng, m.n_pnodes, node[0], node[inner[len(inner) // 2]])
    _check_direct(ctx, Mp, rhs, tag)
    ctx.close()


def test_three_counts_three_edges_and_an_origin_off_zero():
    _box_case((5, 3, 2), (0.3, -0.1, 0.2), (2.3, 0.2, 0.9), 2, 1, "5 x 3 x 2", all_rhs=True)


@pytest.mark.parametrize("reps", [(4, 1, 3), (1, 1, 1)])
def test_lines_of_two_nodes(reps):
    _box_case(reps, (0.3, -0.1, 0.2), (2.3, 0.2, 0.9), 2, 2, f"{reps}")


@pytest.mark.parametrize("reps", [(70, 2, 2), (2, 70, 2), (2, 2, 70)])
def test_lines_longer_than_a_wave_and_a_tile_on_each_axis(reps):
    _box_case(reps, (0.0, 0.0, 0.0), tuple(0.05 * r for r in reps), 2, 3, f"{reps}")


@pytest.mark.parametrize("reps,kv", [((7, 4), 2), ((70, 3), 2), ((2, 3, 2), 1)])
def test_two_dimensions_and_q1_velocity(reps, kv):
    dim = len(reps)
    _box_case(reps, (0.1, -0.2, 0.3)[:dim], (1.5, 0.6, 1.1)[:dim], kv, 4, f"{dim}D Q{kv} {reps}")


def test_random_renumbering_of_the_pressure_nodes():
    _box_case((4, 3, 5), (0.3, -0.1, 0.2), (2.3, 0.2, 0.9), 2, 5, "4 x 3 x 5, pressure nodes renumbered", all_rhs=True, perm=True)


def test_morton_ordered_mirror_and_every_level_of_its_chain():
    """the 16 x 8 x 8 channel through the host mirror (Morton order, multigrid levels attached): after one solve every level has its M_p"""
    from openifem_amd import capi, host
    s = host.InsIM(host.channel_prm(3), (16, 8, 8), (0, 0, 0), EXTENT)
    s.setup(0)
    s.channel_state()
    s.assemble(False)
    st = s.solve(False)
    assert st.cg_mp_iters == 0
    levels = [((16, 8, 8), s.ctx)] + s.mg_levels()
    assert len(levels) >= 2  # (the mirror stops coarsening this mesh at 16 x 4 x 4)
    rng = np.random.default_rng(6)
    for reps, h in levels:
        n_un, n_pn = int(np.prod([2 * r + 1 for r in reps])), int(np.prod([r + 1 for r in reps]))
        ctx = capi.Context.borrow(h, 3, 2, n_un, n_pn)
        Mp = _mass(ctx, 3 * n_un, 3 * n_un)
        assert Mp.shape == (n_pn, n_pn)
        _check_direct(ctx, Mp, [("random", rng.standard_normal(n_pn))], f"mirror level {reps}")
    s.close()


# ---- contexts that keep CG: the result obeys the stopping rule of that CG on the exported matrix

def _check_cg(x, direct, its, Mp, b, opts, tag):
    res, tol = np.linalg.norm(b - Mp @ x), max(opts.mp_abs, opts.mp_rel * np.linalg.norm(b))
    print(f"{tag}: direct {direct}, CG iterations {its}, ||b - M_p x|| = {res:.3e}, tolerance {tol:.3e}")
    assert not direct and its > 0
    assert res <= tol


def test_moved_vertex_keeps_cg():
    m = BoxMesh((3, 2, 2), (0, 0, 0), EXTENT, kv=2)
    h = np.array(EXTENT) / np.array((3, 2, 2))
    m.vcoords = m.vcoords.copy()
    hit = np.all(np.abs(m.vcoords - h) < 1e-9 * h, axis=2)
    assert hit.sum() == 8
    m.vcoords[hit] += 1e-6 * h
    ctx, rng = _assembled(m, 7)
    assert not ctx.mf_uniform()[0]
    b = rng.standard_normal(m.n_pnodes)
    _check_cg(*ctx.mp_solve(b), _mass(ctx, m.n_u, m.n_u), b, ctx.opts, "one vertex moved by 1e-6 h")
    ctx.close()


def test_hanging_node_mesh_keeps_cg():
    from hangmesh import HangingMesh
    m = HangingMesh((2, 2, 2), (0, 0, 0), (1.0, 0.8, 0.6), {(0, 0, 0)}, kv=2)
    ctx, rng = _assembled(m, 8, hanging=True)
    n_u = m.dim * m.n_unodes
    b = rng.standard_normal(m.n_pnodes)
    _check_cg(*ctx.mp_solve(b), _mass(ctx, n_u, n_u), b, ctx.opts, "hanging-node mesh")
    ctx.close()


def test_mp_solver_1_keeps_cg_on_an_eligible_box():
    m = BoxMesh((5, 3, 2), (0.3, -0.1, 0.2), (2.3, 0.2, 0.9), kv=2)
    ctx, rng = _assembled(m, 9)
    b = rng.standard_normal(m.n_pnodes)
    Mp = _mass(ctx, m.n_u, m.n_u)
    assert ctx.mp_solve(b)[1]
    ctx.opts.mp_solver = 1
    _check_cg(*ctx.mp_solve(b), Mp, b, ctx.opts, "mp_solver = 1")
    ctx.opts.mp_solver = 0
    assert ctx.mp_solve(b)[1]
    ctx.close()


def test_two_virtual_ranks_keep_cg():
    capi = _capi()
    m = BoxMesh((4, 2, 2), (0, 0, 0), EXTENT, kv=2)
    rng = np.random.default_rng(10)
    dofs, vals = m.dirichlet(_bcs(3))
    ev, pr, b = rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_pnodes)
    from partmesh import local_dirichlet
    parts = partition_mesh(m, (m.vcoords.mean(axis=1)[:, 0] > 1.0).astype(int), 2)
    opts = []

    def work(rank, P, ctx):
        ld, lv = local_dirichlet(P, dofs, vals)
        ctx.set_constraints(0, ld, None)
        ctx.set_constraints(1, ld, lv)
        ctx.vec_set(capi.VEC_PRESENT, pr[P.ext_gdof])
        ctx.vec_set(capi.VEC_EVAL, ev[P.ext_gdof])
        ctx.assemble(capi.make_params(**KW), False)
        opts.append(ctx.opts)
        return ctx.mp_solve(b[P.owned_p]), _mass(ctx, 3 * P.n_unodes_owned, 3 * P.n_unodes)

    out = run_virtual_ranks(capi, parts, work)
    Mp, x = np.zeros((m.n_pnodes, m.n_pnodes)), np.zeros(m.n_pnodes)
    for P, ((xr, direct, its), Mr) in zip(parts, out):
        assert not direct and its > 0
        Mp[np.ix_(P.owned_p, P.l2g_p)] = Mr
        x[P.owned_p] = xr
    _check_cg(x, False, out[0][0][2], Mp, b, opts[0], "two virtual ranks")


# ---- through ifem_solve

def test_through_the_solve_on_the_mirror_hierarchy(capfd):
    """16^3 channel, the mirror's default options: mp_solver 0 against 1, and a re-integrated M_p (geo_cache = 0) is probed again.
    One fresh solver per setting: the context remembers whether the tight first inner solve paid (ifem_solver_opts::inner_rel_first backs off
    after a miss), so a second solve on the same context is not the same solve."""
    from openifem_amd import capi, multigpu
    out, keep = {}, None
    for mode in (1, 0):
        s, _, _ = multigpu.make_channel_solver(16, 0, 1, 0, None, multigrid=True)
        s.channel_state()
        s.assemble(False)
        _, n_u, n_p = s.sizes()
        s.opts.mp_solver = mode
        st = s.solve(False)
        x = np.zeros(n_u + n_p)
        assert s.L.ifem_vec_get(s.ctx, capi.VEC_UPDATE, x.ctypes.data_as(C.c_void_p)) == 0
        res, rhs = s.true_residual()
        with capfd.disabled():
            print(f"mp_solver {mode}: fgmres {st.fgmres_iters}, inner {st.inner_iters}, cg_mp_iters {st.cg_mp_iters}, true residual / ||rhs|| = {res / rhs:.4e}")
        assert res <= 1.05e-4 * rhs
        out[mode] = (x, st.cg_mp_iters)
        if mode == 1:
            s.close()
    diff = np.abs(out[0][0] - out[1][0]).max() / np.abs(out[1][0]).max()
    with capfd.disabled():
        print(f"updates, direct against CG: {diff:.3e} of the largest entry")
    assert out[0][1] == 0 and out[1][1] > 0
    assert diff <= 1e-5
    # the same values again: no new probe; re-integrated values: probed again, and the path stays on
    s.opts.verbose = 1
    capfd.readouterr()
    assert s.solve(False).cg_mp_iters == 0
    assert "M_p: line solves" not in capfd.readouterr().err
    tun = capi.Tuning()
    s.L.ifem_default_tuning(C.byref(tun))
    tun.geo_cache = 0
    for c in s.all_ctxs():
        assert s.L.ifem_set_tuning(c, C.byref(tun)) == 0
    s.assemble(False)
    st = s.solve(False)
    err = capfd.readouterr().err
    s.opts.verbose = 0
    assert "M_p: line solves" in err and "miss the assembled matrix" not in err
    assert st.cg_mp_iters == 0
    s.close()
