"""x = S_m^-1 b by fast diagonalisation on uniform box levels (csrc/sm_direct.hip, ifem_solver_opts::sm_mg = 2) through the test aid
ifem_test_sm_solve, and through ifem_solve / run_one_step of the host mirror.

Reference: S = B diag(M_u)^-1 B^T from the CSR exports (as tests/test_gpu_sm_stencil.py::_schur builds it), dense, numpy.linalg.solve.
Direct path: max|S x - b| <= 1e-10 max|b|.  Every shape here has cond(Lambda) <= about 1e4; the numpy restatement of the same algorithm reaches
2e-14 .. 2e-13 on such shapes, a margin of 500.  The achieved value is printed.
CG path: ||S x - b||_2 <= max(sm_abs, sm_rel ||b||) and info[0] == 0.  The CG checks run under IFEM_AINV_GMRES_BJACOBI, the kind whose S_m
product streams the fp64 values, so that the recurrence residual CG stops on is the residual the test forms."""
import numpy as np
import pytest

from boxmesh import BoxMesh
from partmesh import partition_mesh, run_virtual_ranks
from test_gpu_sm_stencil import KW, EXTENT, _bcs, _assembled, _schur, _schur_from_rows, _set_and_assemble

pytestmark = pytest.mark.gpu

BOUND = 1e-10


def _capi():
    from openifem_amd import capi
    return capi


def _opts(ctx, sm_mg, verbose=0):
    capi = _capi()
    o = capi.SolverOpts.from_buffer_copy(ctx.opts)
    o.sm_mg, o.verbose = sm_mg, verbose
    o.ainv_kind = capi.AINV_GMRES_BJACOBI
    return o


def _rhs(rng, n, nodes=()):
    out = [("random", rng.standard_normal(n))]
    for k, nd in enumerate(nodes):
        e = np.zeros(n)
        e[nd] = 1.0
        out.append((f"unit vector {k}", e))
    return out


def _check_direct(ctx, S, bs, tag):
    """sm_mg = 2 takes the direct path and solves S x = b to the bound; returns the last info"""
    Sd = S.toarray()
    info = None
    for name, b in bs:
        x, info = ctx.sm_solve(b, _opts(ctx, 2))
        res = np.abs(Sd @ x - b).max() / np.abs(b).max()
        ref = np.linalg.solve(Sd, b)
        print(f"{tag}, {name}: direct {int(info[0])}, CG iterations {int(info[1])}, probe {info[2] * 1e-18:.2e}, tables {int(info[3])} B, "
              f"max|S x - b| / max|b| = {res:.2e}, max|x - x_ref| / max|x_ref| = {np.abs(x - ref).max() / np.abs(ref).max():.2e}")
        assert info[0] == 1 and info[1] == 0 and info[3] > 0
        assert 0 < info[2] * 1e-18 <= 1e-7
        assert res <= BOUND
    return info


def _check_cg(ctx, apply_s, b, tag, sm_mg=2):
    """the solve keeps CG and meets its stopping rule; apply_s: x -> S x in fp64"""
    o = _opts(ctx, sm_mg)
    x, info = ctx.sm_solve(b, o)
    r, tol = np.linalg.norm(apply_s(x) - b), max(o.sm_abs, o.sm_rel * np.linalg.norm(b))
    print(f"{tag}: direct {int(info[0])}, CG iterations {int(info[1])}, ||S x - b|| = {r:.3e}, bound {tol:.3e}")
    assert info[0] == 0 and info[2] == 0 and info[3] == 0 and info[1] > 0
    assert r <= tol
    return x, info


def _csr_product(ctx):
    return lambda x: ctx.sm_apply(0, x)[0]


def _box_case(reps, p0, p1, seed, tag, perm=False, units=False, dofs_of=None):
    m = BoxMesh(reps, p0, p1, kv=2)
    rng = np.random.default_rng(3000 + seed)
    cp, node = None, np.arange(m.n_pnodes)
    if perm:
        node = rng.permutation(m.n_pnodes)
        cp = node[m.cell_pnodes].astype(np.int32)
    dofs, vals = (None, None) if dofs_of is None else dofs_of(m)
    ctx, _ = _assembled(m, seed, cell_pnodes=cp, dofs=dofs, vals=vals)
    S = _schur(ctx, m.n_u)
    _check_direct(ctx, S, _rhs(rng, m.n_pnodes, (node[0], node[m.n_pnodes // 2], node[-1]) if units else ()), tag)
    ctx.close()


# ---- shapes that take the direct path

def test_three_counts_three_edges_and_an_origin_off_zero():
    _box_case((5, 3, 2), (0.3, -0.1, 0.2), (2.3, 0.2, 0.9), 1, "5 x 3 x 2", units=True)


def test_two_cells_per_axis():
    _box_case((2, 2, 2), (0.3, -0.1, 0.2), (2.3, 0.2, 0.9), 2, "2 x 2 x 2", units=True)


@pytest.mark.parametrize("reps", [(17, 2, 2), (2, 17, 2), (2, 2, 17)])
def test_more_than_one_mfma_tile_on_each_axis(reps):
    _box_case(reps, (0.0, 0.0, 0.0), tuple(0.05 * r for r in reps), 3, f"{reps}", units=True)


@pytest.mark.parametrize("reps", [(7, 4), (33, 3)])
def test_two_dimensions(reps):
    _box_case(reps, (0.1, -0.2), (1.5, 0.6), 4, f"2D {reps}", units=True)


def test_anisotropic_cells():
    _box_case((6, 5, 9), (0.0, 0.0, 0.0), (3.0, 0.25, 1.8), 6, "6 x 5 x 9, h = 0.5 x 0.05 x 0.2")


def test_random_renumbering_of_the_pressure_nodes():
    _box_case((4, 3, 5), (0.3, -0.1, 0.2), (2.3, 0.2, 0.9), 5, "4 x 3 x 5, pressure nodes renumbered", perm=True, units=True)


def test_slip_faces_with_the_normal_component_only():
    # inflow no-slip, outflow free, y faces constrain v only, z faces no-slip
    bcs = {0: (7, [0.3, -0.2, 0.1]), 2: (2, [0.0]), 3: (2, [0.0]), 4: (7, [0.0] * 3), 5: (7, [0.0] * 3)}
    _box_case((3, 3, 2), (0.3, -0.1, 0.2), (2.3, 0.8, 0.9), 7, "3 x 3 x 2, slip faces", units=True, dofs_of=lambda m: m.dirichlet(bcs))


def test_an_axis_of_one_cell_with_one_free_end():
    bcs = {0: (3, [0.3, -0.2]), 2: (3, [0.0, 0.0])}
    _box_case((6, 1), (0.1, -0.2), (1.5, 0.1), 8, "2D 6 x 1, faces 1 and 3 free", units=True, dofs_of=lambda m: m.dirichlet(bcs))


def test_morton_ordered_mirror_finest_level_direct_coarser_levels_build_nothing():
    """the 16 x 8 x 8 channel through the host mirror (Morton order, multigrid levels attached), solved with sm_mg = 2"""
    from openifem_amd import capi, host
    s = host.InsIM(host.channel_prm(3), (16, 8, 8), (0, 0, 0), EXTENT)
    s.setup(0)
    s.channel_state()
    s.assemble(False)
    st = s.solve(False)  # the default first: the V-cycle forms S_m on every level of the chain (the direct path never touches the coarser ones)
    assert st.sm_mg_levels >= 2
    s.opts.sm_mg = 2
    st = s.solve(False)
    assert st.sm_mg_levels == 0 and st.cg_sm_iters == 0 and st.precond_applies > 0
    r, b = s.true_residual()
    assert r <= 1.05e-4 * b
    levels = [((16, 8, 8), s.ctx)] + s.mg_levels()
    assert len(levels) >= 2
    rng = np.random.default_rng(9)
    for k, (reps, h) in enumerate(levels):
        n_un, n_pn = int(np.prod([2 * r + 1 for r in reps])), int(np.prod([r + 1 for r in reps]))
        ctx = capi.Context.borrow(h, 3, 2, n_un, n_pn)
        if k == 0:
            _check_direct(ctx, _schur_from_rows(ctx, 3 * n_un, n_pn), _rhs(rng, n_pn), "mirror 16 x 8 x 8")
        else:  # no coarser level builds factors: with the option set it keeps CG, and holds no table
            _check_cg(ctx, _csr_product(ctx), rng.standard_normal(n_pn), f"mirror level {tuple(reps)}")
    s.close()


# ---- shapes that keep CG

def _mesh654():
    return BoxMesh((6, 5, 4), (0.3, -0.1, 0.2), (2.3, 0.9, 1.0), kv=2)


def test_an_axis_of_one_cell_with_both_ends_dirichlet_keeps_cg():
    m = BoxMesh((4, 1, 3), (0.3, -0.1, 0.2), (2.3, 0.2, 0.9), kv=2)
    ctx, rng = _assembled(m, 21)
    _check_cg(ctx, _csr_product(ctx), rng.standard_normal(m.n_pnodes), "4 x 1 x 3, channel set")
    ctx.close()


def test_all_faces_dirichlet_singular_block_keeps_cg():
    m = _mesh654()
    dofs, vals = m.dirichlet(_bcs(3, outflow=True))
    ctx, rng = _assembled(m, 22, dofs=dofs, vals=vals)
    b = ctx.sm_apply(0, rng.standard_normal(m.n_pnodes))[0]  # in the range of the singular block
    _check_cg(ctx, _csr_product(ctx), b, "every face Dirichlet")
    ctx.close()


def test_a_face_with_one_tangential_component_keeps_cg():
    m = _mesh654()
    bcs = _bcs(3)
    bcs[3] = (1, [0.0])  # the y+ wall holds u only
    dofs, vals = m.dirichlet(bcs)
    ctx, rng = _assembled(m, 23, dofs=dofs, vals=vals)
    _check_cg(ctx, _csr_product(ctx), rng.standard_normal(m.n_pnodes), "a tangential-only face")
    ctx.close()


def test_one_interior_velocity_node_constrained_keeps_cg():
    m = _mesh654()
    dofs, vals = m.dirichlet(_bcs(3))
    nd = np.nonzero(np.all(m.unode_lattice == np.array((5, 5, 4)), axis=1))[0]
    extra = 3 * int(nd[0]) + np.arange(3)
    dofs, vals = np.concatenate([dofs, extra]).astype(np.int32), np.concatenate([vals, np.zeros(3)])
    ctx, rng = _assembled(m, 24, dofs=dofs, vals=vals)
    _check_cg(ctx, _csr_product(ctx), rng.standard_normal(m.n_pnodes), "one interior velocity node constrained")
    ctx.close()


def test_random_constrained_dofs_keep_cg():
    m = _mesh654()
    dofs = np.nonzero(np.random.default_rng(25).random(m.n_u) < 0.3)[0].astype(np.int32)
    ctx, rng = _assembled(m, 25, dofs=dofs, vals=np.zeros(len(dofs)))
    _check_cg(ctx, _csr_product(ctx), rng.standard_normal(m.n_pnodes), "30 % random constrained dofs")
    ctx.close()


def test_moved_vertex_keeps_cg():
    m = BoxMesh((3, 2, 2), (0, 0, 0), EXTENT, kv=2)
    h = np.array(EXTENT) / np.array((3, 2, 2))
    m.vcoords = m.vcoords.copy()
    hit = np.all(np.abs(m.vcoords - h) < 1e-9 * h, axis=2)
    assert hit.sum() == 8
    m.vcoords[hit] += 1e-6 * h
    ctx, rng = _assembled(m, 26)
    assert not ctx.mf_uniform()[0]
    _check_cg(ctx, _csr_product(ctx), rng.standard_normal(m.n_pnodes), "one vertex moved by 1e-6 h")
    ctx.close()


def test_hanging_node_mesh_keeps_cg():
    from hangmesh import HangingMesh
    m = HangingMesh((2, 2, 2), (0, 0, 0), (1.0, 0.8, 0.6), {(0, 0, 0)}, kv=2)
    capi = _capi()
    rng = np.random.default_rng(27)
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    ctx.set_hanging_constraints(m.hang_dof, m.hang_ptr, m.hang_master, m.hang_weight)
    ctx.vec_set(capi.VEC_PRESENT, rng.standard_normal(m.n_dofs))
    ctx.vec_set(capi.VEC_EVAL, rng.standard_normal(m.n_dofs))
    ctx.assemble(capi.make_params(**KW), False)
    b = ctx.sm_apply(0, rng.standard_normal(m.n_pnodes))[0]  # (nothing is constrained: the constants are in the kernel)
    _check_cg(ctx, _csr_product(ctx), b, "hanging-node mesh")
    ctx.close()


def test_two_virtual_ranks_keep_cg():
    capi = _capi()
    m = BoxMesh((4, 2, 2), (0, 0, 0), EXTENT, kv=2)
    rng = np.random.default_rng(28)
    dofs, vals = m.dirichlet(_bcs(3))
    ev, pr, b = rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_pnodes)
    from partmesh import local_dirichlet
    parts = partition_mesh(m, (m.vcoords.mean(axis=1)[:, 0] > 1.0).astype(int), 2)
    tol = []

    def work(rank, P, ctx):
        ld, lv = local_dirichlet(P, dofs, vals)
        ctx.set_constraints(0, ld, None)
        ctx.set_constraints(1, ld, lv)
        ctx.vec_set(capi.VEC_PRESENT, pr[P.ext_gdof])
        ctx.vec_set(capi.VEC_EVAL, ev[P.ext_gdof])
        ctx.assemble(capi.make_params(**KW), False)
        o = _opts(ctx, 2)
        tol.append(max(o.sm_abs, o.sm_rel * np.linalg.norm(b)))
        x, info = ctx.sm_solve(b[P.owned_p], o)
        return x, info.copy()

    out = run_virtual_ranks(capi, parts, work)
    one, _ = _assembled(m, 28)
    S = _schur(one, m.n_u)
    one.close()
    x = np.full(m.n_pnodes, np.nan)
    for P, (xr, info) in zip(parts, out):
        assert info[0] == 0 and info[2] == 0 and info[3] == 0 and info[1] > 0
        x[P.owned_p] = xr
    r = np.linalg.norm(S @ x - b)
    print(f"two virtual ranks: ||S x - b|| = {r:.3e}, bound {tol[0]:.3e}")
    assert r <= tol[0]


def test_after_an_scnsim_assembly_the_context_keeps_cg():
    """After a direct solve on the INS blocks an SCnsIM assembly writes its stabilised blocks into the same context: the factors must not be used
    again, the solve is the CG of sm_mg = 1 on the new S = B diag(M_u)^-1 B^T and meets its stopping rule.
    The right-hand side: the stabilised B and B^T are not transposes of each other, S is not symmetric (|S - S^T| = 0.06 |S|, negative definite,
    complex pairs among its eigenvalues), and CG is no solver for such a matrix: on a random right-hand side it runs to its cap with this
    option and without it (6 x 5 x 4 on an MI355X: 210 iterations, ||S x - b|| = 1.006e+01 against 1.381e-02, the same iterate under
    sm_mg = 0, 1 and 2; that figure is printed, the production SCnsIM solver never solves with S_m).  Where CG is defined on S it has to deliver:
    for b a real eigenvector of S the Krylov space is one-dimensional, x = b / lambda, whatever the symmetry.  The same b through the stale
    factors of the INS blocks would miss the rule by more than ||b|| (S0 is positive definite, lambda < 0), which is asserted as well."""
    capi = _capi()
    m = _mesh654()
    ctx, rng = _assembled(m, 29)
    b_rnd = rng.standard_normal(m.n_pnodes)
    S0 = _schur(ctx, m.n_u)
    _check_direct(ctx, S0, [("INS blocks", b_rnd)], "6 x 5 x 4")
    ctx.set_tuning(stored_uu=1)
    ctx.scns_assemble(capi.make_scns_params(mu=0.7, rho=1.3, dt=0.01), False)
    S = _schur(ctx, m.n_u).toarray()
    assert np.abs(S - S.T).max() > 1e-3 * np.abs(S).max()  # (the premise of the choice of b)
    ev, V = np.linalg.eig(S)
    real = np.nonzero(ev.imag == 0)[0]
    k = real[np.argmax(np.abs(ev[real].real))]
    b = V[:, k].real * (np.sqrt(m.n_pnodes) / np.linalg.norm(V[:, k].real))
    o = _opts(ctx, 2)
    x, info = ctx.sm_solve(b, o)
    r, tol = np.linalg.norm(S @ x - b), max(o.sm_abs, o.sm_rel * np.linalg.norm(b))
    print(f"stabilised blocks of an SCnsIM assembly, b an eigenvector (lambda = {ev[k].real:.4e}): direct {int(info[0])}, CG iterations {int(info[1])}, "
          f"||S x - b|| = {r:.3e}, bound {tol:.3e}; through the S_m of the INS blocks ||S0 x - b|| = {np.linalg.norm(S0 @ x - b):.3e}")
    assert info[0] == 0 and info[2] == 0 and info[3] == 0 and info[1] > 0
    assert r <= tol
    assert np.linalg.norm(S0 @ x - b) > np.linalg.norm(b)
    x1, info1 = ctx.sm_solve(b, _opts(ctx, 1))
    assert np.array_equal(x, x1) and np.array_equal(info, info1)  # exactly the behaviour of sm_mg = 1
    xr, info_r = ctx.sm_solve(b_rnd, o)
    print(f"the same context, random b: direct {int(info_r[0])}, CG iterations {int(info_r[1])}, ||S x - b|| = {np.linalg.norm(S @ xr - b_rnd):.3e} "
          f"(CG on a non-symmetric matrix; bound {max(o.sm_abs, o.sm_rel * np.linalg.norm(b_rnd)):.3e})")
    assert info_r[0] == 0 and info_r[2] == 0 and info_r[3] == 0
    ctx.close()


def test_q1_velocity_keeps_cg():
    m = BoxMesh((2, 3, 2), (0.1, -0.2, 0.3), (1.5, 0.6, 1.1), kv=1)
    ctx, rng = _assembled(m, 30)
    b = ctx.sm_apply(0, rng.standard_normal(m.n_pnodes))[0]  # (the equal-order pair has spurious pressure modes: the block is singular)
    _check_cg(ctx, _csr_product(ctx), b, "Q1 velocity")
    ctx.close()


@pytest.mark.parametrize("sm_mg", [1, 0])
def test_other_values_of_the_option_are_bit_equal_to_the_context_before_it_saw_the_option(sm_mg):
    """one context: the solve under sm_mg = 1 / 0 before the option was ever used, a direct solve (factors built, probe run), the first solve
    again.  (Two contexts cannot be compared bit by bit: the assembly's atomic order leaves their S_m values a few 1e-16 apart.)"""
    m = _mesh654()
    ctx, rng = _assembled(m, 31)
    b = rng.standard_normal(m.n_pnodes)
    x0, i0 = _check_cg(ctx, _csr_product(ctx), b, f"sm_mg = {sm_mg} on a context that never saw the option", sm_mg=sm_mg)
    _check_direct(ctx, _schur(ctx, m.n_u), [("option 2", b)], "6 x 5 x 4")
    x1, i1 = _check_cg(ctx, _csr_product(ctx), b, f"sm_mg = {sm_mg} after a direct solve", sm_mg=sm_mg)
    assert np.array_equal(x0, x1) and np.array_equal(i0, i1)
    ctx.close()


# ---- behaviour

def _eigen_solves(err):
    import re
    return [int(k) for k in re.findall(r"fast diagonalisation on the .* lattice, (\d+) axis eigen-solves so far", err)]


def test_a_new_constraint_set_builds_new_factors_and_the_solve_follows(capfd):
    """Two changes of the set on one context.  The outflow takes a Dirichlet value on its normal component: the x axis gets new factors, but
    with every normal component held the flow is enclosed and the block singular -- the refusal rule applies, CG follows the new S_m.  Then
    the outflow is free again and the y+ wall too: new factors on x and y, and the direct solve follows that S_m."""
    m = _mesh654()
    ctx, rng = _assembled(m, 32)
    b = rng.standard_normal(m.n_pnodes)
    S0 = _schur(ctx, m.n_u)
    x0, _ = ctx.sm_solve(b, _opts(ctx, 2, verbose=1))
    assert _eigen_solves(capfd.readouterr().err) == [3]
    bcs = _bcs(3)
    bcs[1] = (1, [0.0])  # the outflow now holds its normal component
    dofs, vals = m.dirichlet(bcs)
    _set_and_assemble(ctx, m, dofs, vals, rng)
    S1 = _schur(ctx, m.n_u)
    assert np.abs((S1 - S0) @ x0).max() > 1e-3 * np.abs(b).max()  # the matrix did change
    b1 = S1 @ rng.standard_normal(m.n_pnodes)
    o = _opts(ctx, 2, verbose=1)
    x1, info = ctx.sm_solve(b1, o)
    err = capfd.readouterr().err
    assert "singular" in err and info[0] == 0 and info[1] > 0
    assert np.linalg.norm(S1 @ x1 - b1) <= max(o.sm_abs, o.sm_rel * np.linalg.norm(b1))
    bcs = _bcs(3)
    del bcs[3]  # the y+ wall is free
    dofs, vals = m.dirichlet(bcs)
    _set_and_assemble(ctx, m, dofs, vals, rng)
    S2 = _schur(ctx, m.n_u)
    assert np.abs((S2 - S0) @ x0).max() > 1e-3 * np.abs(b).max()
    x2, info = ctx.sm_solve(b, _opts(ctx, 2, verbose=1))
    assert _eigen_solves(capfd.readouterr().err) == [6]  # x (built for the enclosed set meanwhile) and y have new keys, z keeps its factors
    res = np.abs(S2 @ x2 - b).max() / np.abs(b).max()
    with capfd.disabled():
        print(f"new constraint set: max|S2 x - b| / max|b| = {res:.2e}, probe {info[2] * 1e-18:.2e}")
    assert info[0] == 1 and res <= BOUND
    ctx.close()


def test_without_the_geometry_cache_the_factors_are_reused_and_the_probe_reruns(capfd):
    m = _mesh654()
    capi = _capi()
    rng = np.random.default_rng(33)
    dofs, vals = m.dirichlet(_bcs(3))
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    ctx.set_tuning(geo_cache=0)
    b = rng.standard_normal(m.n_pnodes)
    counts = []
    for k in range(3):
        _set_and_assemble(ctx, m, dofs, vals, rng)  # S_m is re-formed by every assembly
        x, info = ctx.sm_solve(b, _opts(ctx, 2, verbose=1))
        counts += _eigen_solves(capfd.readouterr().err)
        assert info[0] == 1 and np.abs(_schur(ctx, m.n_u) @ x - b).max() <= BOUND * np.abs(b).max()
    x, info = ctx.sm_solve(b, _opts(ctx, 2, verbose=1))  # nothing re-formed: no probe line
    counts += _eigen_solves(capfd.readouterr().err)
    assert counts == [3, 3, 3]  # three probes, one build
    ctx.close()


def test_linear_solve_and_one_step_of_the_mirror_with_the_option_1_2_1(capfd):
    """16^3 channel chain.  The updates of 1 and 2 are not compared beyond the outer tolerance: two different preconditioners.  The linear solves
    are held to 1.05e-4 ||rhs||; the last solve of a run_one_step Newton loop to the whole outer rule (its absolute arm decides there)."""
    from openifem_amd import capi, multigpu
    s, _, _ = multigpu.make_channel_solver(16, 0, 1, 0, None, multigrid=True)
    s.opts.inner_rel_first = 0.0  # (with it the context remembers whether the tight first inner solve paid: the third solve would differ from the first)
    s.channel_state()
    s.assemble(False)
    runs = []
    for mode in (1, 2, 1):
        s.opts.sm_mg = mode
        st = s.solve(False)
        r, b = s.true_residual()
        runs.append((st.fgmres_iters, st.inner_iters, st.cg_sm_iters, st.cg_mp_iters, st.sm_mg_levels))
        assert r <= 1.05e-4 * b
    steps = []
    for mode in (1, 2, 1):
        s.opts.sm_mg = mode
        s.channel_state()  # every step from the same perturbed state, so that its Newton loop has something to converge from
        assert s.L.ifem_vec_copy(s.ctx, capi.VEC_PRESENT, capi.VEC_EVAL) == 0
        s.run_one_step(True)
        st, (newton, fgmres_sum) = s.last_stats(), s.last_newton()
        r, b = s.true_residual()
        steps.append((st.fgmres_iters, st.inner_iters, st.cg_sm_iters, st.cg_mp_iters, st.sm_mg_levels, newton, fgmres_sum))
        assert newton >= 1 and fgmres_sum >= 1 and st.fgmres_iters >= 1
        # the outer rule is max(fgmres_abs, fgmres_rel ||rhs||): the last Newton solve of a converged step has ||rhs|| of a few 1e-12 and stops on
        # its absolute arm (sm_mg = 1 as well: 3.6e-13 of 3.6e-12 measured), the same 5 % allowed on either arm
        assert r <= 1.05 * max(s.opts.fgmres_rel * b, s.opts.fgmres_abs)
    with capfd.disabled():
        print(f"(fgmres, inner, cg_sm, cg_mp, sm_mg_levels): linear solves with sm_mg 1, 2, 1: {runs}; last solve of run_one_step, + (Newton iterations, summed FGMRES): {steps}")
    assert runs[0] == runs[2] and runs[0][2] > 0 and runs[0][4] >= 2
    assert runs[1][2] == 0 and runs[1][4] == 0
    assert steps[1][2] == 0 and steps[1][4] == 0 and steps[0][4] >= 2 and steps[2][4] >= 2
    s.close()
