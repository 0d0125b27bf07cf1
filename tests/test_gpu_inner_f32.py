"""The single-precision flexible inner solver of IFEM_AINV_MG and the trimmed A_uu V-cycle (ifem_tuning::inner_f32; krylov.hip::fgmres_f32,
solver.hip::mg_uu_vcycle(trim), mg.hip::k_vc_entry / k_vc_exit, the `first` flag and mode 1 of apply_mf.hip::k_mf_gather), through the C ABI.

inner_f32 = 0 is the path as it was before the knob existed (fp64 bases, conversion passes, zero fills, every smoothing step in full), so
one build is compared with itself.  What the trimmed cycle leaves out is never read: with inner_maxit = 0 (A~^-1 = one V-cycle) the two
settings must agree bit for bit.  With the Krylov iteration around it the stored basis columns are rounded to float: same iteration
counts, results equal to the rounding of the basis."""
import ctypes as C

import numpy as np
import pytest

from boxmesh import BoxMesh
from partmesh import gather_owned, local_dirichlet, partition_mesh, run_virtual_ranks

pytestmark = pytest.mark.gpu

EXTENT = (2.0, 0.2, 0.2)


def _set_tuning(s, **kw):
    from openifem_amd import capi
    tun = capi.Tuning()
    s.L.ifem_default_tuning(C.byref(tun))
    assert tun.inner_f32 == 1
    for k, v in kw.items():
        setattr(tun, k, v)
    for c in s.all_ctxs():
        assert s.L.ifem_set_tuning(c, C.byref(tun)) == 0


def _get(s, vec, n):
    x = np.zeros(n)
    assert s.L.ifem_vec_get(s.ctx, vec, x.ctypes.data_as(C.c_void_p)) == 0
    return x


@pytest.fixture(scope="module")
def channel16():
    """the bench's channel at 16^3 with its three attached levels, assembled once; the tests only change options and tuning"""
    from openifem_amd import capi, multigpu
    s, _, _ = multigpu.make_channel_solver(16, 0, 1, 0, None, multigrid=True)
    assert len(list(s.all_ctxs())) == 3
    s.channel_state()
    s.opts.ainv_kind = capi.AINV_MG
    s.assemble(False)
    _, n_u, n_p = s.sizes()
    g = np.arange(n_u + n_p)
    v = np.cos(0.37 * g) + 0.1 * np.sin(1.3 * g)
    defaults = {k: getattr(s.opts, k) for k in ("inner_maxit", "inner_restart", "inner_rel", "inner_rel_first", "mg_smooth_u", "mg_smooth_u_post")}
    yield s, n_u, n_p, v, defaults
    s.close()


def _reset(s, defaults):
    for k, v in defaults.items():
        setattr(s.opts, k, v)


def _precond(s, n_u, n_p, v):
    from openifem_amd import capi
    ip = capi.make_params(mu=1.0, rho=1.0, gamma=0.1, dt=1e-3)
    assert s.L.ifem_vec_set(s.ctx, capi.VEC_TMP, v.ctypes.data_as(C.c_void_p)) == 0
    rc = s.L.ifem_precond_vmult(s.ctx, C.byref(ip), C.byref(s.opts), capi.VEC_UPDATE, capi.VEC_TMP)
    assert rc == 0, s.L.ifem_last_error().decode()
    return _get(s, capi.VEC_UPDATE, n_u + n_p)


@pytest.mark.parametrize("graph_cells", [262144, 0])
@pytest.mark.parametrize("nu", [2, 1, 3])
def test_trimmed_vcycle_is_bit_identical(channel16, nu, graph_cells):
    """inner_maxit = 0: A~^-1 is exactly one V-cycle.  nu = 1: the first smoothing step (xs = x stored) is also the last pre-smoothing
    step (mode 1).  Captured as a hipGraph (the default at this size: the second and third applications are capture and replay) and eager."""
    s, n_u, n_p, v, defaults = channel16
    _reset(s, defaults)
    s.opts.inner_maxit = 0
    s.opts.mg_smooth_u = nu
    z = {}
    for knob in (0, 1):
        _set_tuning(s, inner_f32=knob, vcycle_graph_cells=graph_cells)
        z[knob] = [_precond(s, n_u, n_p, v) for _ in range(3)]
    _reset(s, defaults)
    assert np.isfinite(z[0][0]).all() and np.abs(z[0][0][:n_u]).max() > 0
    for a, b in zip(z[0], z[1]):
        d = np.abs(a - b).max()
        print(f"nu = {nu}, graph cells {graph_cells}: max abs difference of one V-cycle, inner_f32 1 against 0: {d:.3e}")
        assert d == 0.0


# Float bases against fp64 bases on this mesh (inner_f32 = 0 against 1, largest difference of the velocity part relative to its largest
# entry), measured on one MI355X in two runs of this test (the larger value of the two is kept):
#   default options      ifem_precond_vmult 5.8e-8 / 5.8e-8,  solve 3.0e-7 / 3.9e-7   (8 inner, 3 outer iterations with both)
#   GMRES(2) to 1e-6     ifem_precond_vmult 4.5e-7,           solve 8.4e-7            (17 inner, 3 outer, restart length 4 with both)
# -- the rounding of the stored columns (6e-8) through a few Gram-Schmidt sweeps, as expected.  Every bound is one decade over its own
# measured value.
F32_BASIS_MEASURED = {False: (5.8e-8, 3.9e-7), True: (4.5e-7, 8.4e-7)}  # restart -> (ifem_precond_vmult, solve)


def _fresh_channel16():
    from openifem_amd import capi, multigpu
    s, _, _ = multigpu.make_channel_solver(16, 0, 1, 0, None, multigrid=True)
    s.channel_state()
    s.opts.ainv_kind = capi.AINV_MG
    return s


@pytest.mark.parametrize("restart", [False, True])
def test_float_basis_gives_the_same_iteration_and_the_result_to_basis_rounding(restart):
    """restart: GMRES(2) to 1e-6 runs several restart cycles -- the fp64 restart residual b - A x against a float basis, and (the context's
    restart length doubles after such an application) the growth of the float bases.  A context of its own per setting: the lengthened
    restart and the back-off of the tight first solve are state of the context."""
    from openifem_amd import capi
    out = {}
    for knob in (0, 1):
        s = _fresh_channel16()
        if restart:
            s.opts.inner_restart = 2
            s.opts.inner_rel = 1e-6
            s.opts.inner_rel_first = 0.0
        _set_tuning(s, inner_f32=knob)
        s.assemble(False)
        _, n_u, n_p = s.sizes()
        g = np.arange(n_u + n_p)
        z = _precond(s, n_u, n_p, np.cos(0.37 * g) + 0.1 * np.sin(1.3 * g))[:n_u]
        grown = s.L.ifem_inner_restart_length(s.ctx)
        st = s.solve(False)
        x = _get(s, capi.VEC_UPDATE, n_u + n_p)[:n_u]
        res, bn = s.true_residual()
        assert res <= 1.05e-4 * bn
        out[knob] = (z, x, st.inner_iters, st.fgmres_iters, grown)
        s.close()
    (z0, x0, i0, f0, g0), (z1, x1, i1, f1, g1) = out[0], out[1]
    ez = np.abs(z1 - z0).max() / np.abs(z0).max()
    ex = np.abs(x1 - x0).max() / np.abs(x0).max()
    print(f"restart = {restart}: inner / outer iterations {i0, f0} (fp64 bases) {i1, f1} (float bases), restart length {g0} {g1}; "
          f"relative difference precond_vmult {ez:.3e}, solve {ex:.3e}")
    assert (i0, f0) == (i1, f1)
    if restart:
        assert g0 == g1 >= 4  # the application ran more than two restart cycles, the bases have grown
    mz, mx = F32_BASIS_MEASURED[restart]
    assert ez <= 10 * mz and ex <= 10 * mx


def test_graph_captures_per_solve_do_not_depend_on_the_basis_precision(channel16):
    """the captured cycle runs on the fixed level vectors whatever column it is applied to: two solves capture as often with float bases
    as with fp64 bases (and replay the rest)"""
    from openifem_amd import capi
    s, n_u, n_p, v, defaults = channel16
    _reset(s, defaults)
    counts = {}
    for knob in (0, 1):
        _set_tuning(s, inner_f32=knob)  # (a new tuning epoch: the graph is captured anew)
        before = capi.vcycle_graph_stats(s.L, s.ctx)
        st = [s.solve(False), s.solve(False)]
        after = capi.vcycle_graph_stats(s.L, s.ctx)
        counts[knob] = (after[0] - before[0], after[1] - before[1], sum(x.inner_iters for x in st))
    _set_tuning(s)
    print("hipGraph (captures, launches, inner iterations) of two solves, fp64 / float bases:", counts[0], counts[1])
    assert counts[1][0] == counts[0][0] >= 1
    for knob in (0, 1):  # everything but the eager first cycle of the epoch went through the graph
        assert counts[knob][1] > counts[knob][0]


def test_float_column_product_on_two_virtual_ranks_matches_the_single_context():
    """the operator product of the float solver (test aid ifem_test_uu_vmult_f32col): the ghost entries of a float column are
    exchanged as float.  Same mesh, partition and tolerance as test_gpu_mf_uniform.py::test_two_virtual_ranks_match_the_single_context"""
    from openifem_amd import capi
    m = BoxMesh((4, 2, 2), (0, 0, 0), EXTENT, kv=2)
    rng = np.random.default_rng(19)
    flag = 7
    bcs = {0: (flag, [0.3, -0.2, 0.1]), 2: (flag, [0.0] * 3), 3: (flag, [0.0] * 3), 4: (flag, [0.0] * 3), 5: (flag, [0.0] * 3)}
    dofs, vals = m.dirichlet(bcs)
    ev, pr, x = rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_dofs), rng.standard_normal(m.n_dofs)
    Pm = capi.make_params(mu=0.7, rho=1.3, gamma=0.2, dt=0.01)

    def run(nranks, variant):
        c = m.vcoords.mean(axis=1)
        cell_rank = (c[:, 0] > 1.0).astype(int) if nranks == 2 else np.zeros(m.n_cells, int)
        parts = partition_mesh(m, cell_rank, nranks)

        def work(rank, P, ctx):
            ld, lv = local_dirichlet(P, dofs, vals)
            ctx.set_constraints(0, ld, None)
            ctx.set_constraints(1, ld, lv)
            ctx.vec_set(capi.VEC_PRESENT, pr[P.ext_gdof])
            ctx.vec_set(capi.VEC_EVAL, ev[P.ext_gdof])
            ctx.assemble(Pm, False)
            if variant is not None:
                return ctx.uu_vmult(x[P.own_gdof], variant)
            ctx.vec_set(capi.VEC_TMP, x[P.own_gdof])
            rc = ctx.L.ifem_test_uu_vmult_f32col(ctx.h, capi.VEC_UPDATE, capi.VEC_TMP)
            assert rc == 0, ctx.L.ifem_last_error().decode()
            return ctx.vec_get(capi.VEC_UPDATE)

        return gather_owned(parts, run_virtual_ranks(capi, parts, work), m.n_dofs)[:3 * m.n_unodes]

    y1, y2 = run(1, None), run(2, None)
    y64 = run(1, capi.AINV_GMRES_BJACOBI_MF)
    err = np.abs(y2 - y1).max() / np.abs(y1).max()
    e64 = np.abs(y1 - y64).max() / np.abs(y64).max()
    print(f"float column product: two ranks against one context {err:.2e}; against the fp64 matrix-free operator {e64:.2e}")
    assert err <= 1e-13
    assert e64 <= 3e-5  # (the single-precision operator's own bound, test_gpu_multigrid.py) + the rounding of x to float

