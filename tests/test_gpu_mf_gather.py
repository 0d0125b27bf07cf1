"""Node gather of the matrix-free A_uu product (apply_mf.hip::k_mf_gather) with every epilogue, through the test aid
ifem_test_uu_fused_product: one product on host vectors, in the fp64 instance (double cell arithmetic, double vectors) and in the float
instance of the A_uu V-cycle (single-precision cell arithmetic, float vectors).

Reference: numpy float64 on the exported block CSR of the same (stored) assembly.  t = A_uu x; on a constrained row the kernel forms
t_r = x_r / B_rr from the inverse node block (= d_r x_r, the row of the stored matrix); the fused forms read the SINGLE-PRECISION copy of the
inverse node blocks (kernels.hpp::MfFuseT), so the reference rounds ctx.uu_block_diag(0) to float for them and not for the plain form.
  mode 0 (plain)  y = t
  mode 1          xs' = xs + x (first: xs' = x),  r' = r - t
  mode 2          mode 1, then d = a x + b B r'
  mode 3          mode 1, then d = b B r'
fp64 instance against the reference: 1e-12 of max |reference| per output vector.
Float instance against the fp64 instance of the same build, inputs representable in float: the difference is the cell kernel's
single-precision arithmetic and the float vectors, which the gather does not change.  Measured with the one-node-per-thread gather this
kernel replaced, on the shapes and forms below (largest per shape, in the order of SHAPES: 1.571e-07, 1.288e-07, 7.573e-08, 2.114e-07,
2.122e-07, 4.808e-07, 8.953e-07): at most F32_PARENT = 8.953e-07 (CylinderMesh3D, the plain form); 4 x that is allowed.  The new kernel gives
the same seven figures digit for digit: it sums a node's floats in the same order.

Shapes (chunk = 256 consecutive nodes, block b of G walks chunks b, b + G, b + 2 G, ...; a tile holds 1536 entries in the float and 768 in the
fp64 instance): 3D Q2 3x3x3 (odd cell count, node classes 1 / 2 / 4 / 8, two chunks of which the second is 87 nodes), 2D Q2 5x3 and 3D Q1
2x3x2 (one partly filled chunk), 3D Q2 12x6x6 (4225 nodes = 17 chunks: 17 blocks of one chunk by default, and with the blocks capped at 5
two blocks that pipeline 4 chunks and three that pipeline 3, the last chunk partly filled -- asserted through the launch geometry), the smallest
HangingMesh (valences 3 and 5; the hanging lines themselves are applied outside the gather, hanging.hip, so none are set), CylinderMesh(0)
(valence 5) and CylinderMesh3D(0) (valences 5 and 10; 33 chunks, the largest with 1590 entries: 5 of them take a second and one a third tile in the
fp64 instance, one a second tile in the float instance, with node lists that span two tiles; 5 chunks of the 12x6x6 box, up to 1013
entries, take a second tile in the fp64 instance)."""
import numpy as np
import pytest

from boxmesh import BoxMesh
from cylmesh import CylinderMesh, CylinderMesh3D
from hangmesh import HangingMesh

pytestmark = pytest.mark.gpu

KW = dict(mu=0.7, rho=1.3, gamma=0.2, dt=0.01)
F32_PARENT = 8.953e-07  # largest relative float-vs-fp64 difference measured with the previous gather (see the docstring)
A_CHEB, B_CHEB = 0.37, 0.81
# (mode, first); mode 0 is the plain form
FORMS = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)]


def _capi():
    from openifem_amd import capi
    return capi


def _box_bcs(dim):
    """the channel's Dirichlet set: inflow (x-) and the walls"""
    flag = 3 if dim == 2 else 7
    bcs = {0: (flag, [0.3, -0.2, 0.1][:dim]), 2: (flag, [0.0] * dim), 3: (flag, [0.0] * dim)}
    if dim == 3:
        bcs.update({4: (flag, [0.0] * dim), 5: (flag, [0.0] * dim)})
    return bcs


def _mesh(name):
    if name == "q2_3x3x3":
        return BoxMesh((3, 3, 3), (0, 0, 0), (2.0, 0.2, 0.2), kv=2), _box_bcs(3)
    if name == "q2_5x3":
        return BoxMesh((5, 3), (0, 0), (2.0, 0.2), kv=2), _box_bcs(2)
    if name == "q1_2x3x2":
        return BoxMesh((2, 3, 2), (0, 0, 0), (2.0, 0.2, 0.2), kv=1), _box_bcs(3)
    if name == "q2_12x6x6":
        return BoxMesh((12, 6, 6), (0, 0, 0), (2.0, 0.2, 0.2), kv=2), _box_bcs(3)
    if name == "hanging":
        return HangingMesh((2, 2, 2), (0, 0, 0), (1.0, 0.8, 0.6), {(0, 0, 0)}, kv=2), _box_bcs(3)
    if name == "cylinder2d":
        return CylinderMesh(0), {0: (3, [0.3, 0.0]), 2: (3, [0.0, 0.0]), 3: (3, [0.0, 0.0]), 4: (3, [0.0, 0.0])}
    if name == "cylinder3d":
        return CylinderMesh3D(0), {0: (7, [0.3, 0.0, 0.0]), 2: (7, [0.0] * 3), 3: (7, [0.0] * 3), 6: (7, [0.0] * 3)}
    raise KeyError(name)


SHAPES = ["q2_3x3x3", "q2_5x3", "q1_2x3x2", "q2_12x6x6", "hanging", "cylinder2d", "cylinder3d"]
VALENCES = {"q2_3x3x3": {1, 2, 4, 8}, "q2_5x3": {1, 2, 4}, "q1_2x3x2": {1, 2, 4, 8}, "q2_12x6x6": {1, 2, 4, 8}, "hanging": {1, 2, 3, 4, 5, 8},
            "cylinder2d": {1, 2, 4, 5}, "cylinder3d": {1, 2, 4, 5, 8, 10}}
_cache = {}


def _case(name):
    """one assembled context per shape, with its inputs and the fp64 references of every form: built once, shared, never modified"""
    if name in _cache:
        return _cache[name]
    capi = _capi()
    m, bcs = _mesh(name)
    valence = np.bincount(np.asarray(m.cell_unodes).ravel(), minlength=m.n_unodes)
    assert set(valence.tolist()) == VALENCES[name]
    rng = np.random.default_rng(len(name) + m.n_unodes)
    dofs, vals = m.dirichlet(bcs)
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    ctx.set_constraints(0, dofs, None)
    ctx.set_constraints(1, dofs, vals)
    ctx.vec_set(capi.VEC_PRESENT, rng.standard_normal(m.n_dofs))
    ctx.vec_set(capi.VEC_EVAL, rng.standard_normal(m.n_dofs))
    ctx.assemble(capi.make_params(**KW), False)
    n = m.dim * m.n_unodes
    A = ctx.export_csr(0).tocsr()[:n, :n]
    B = ctx.uu_block_diag(0)
    cons = np.zeros(n, bool)
    cons[dofs] = True
    nodes, comps = np.divmod(np.arange(n), m.dim)
    f32 = lambda v: v.astype(np.float32).astype(float)  # noqa: E731  (inputs both instances read alike)
    x, xs, r = (f32(rng.standard_normal(n)) for _ in range(3))
    r *= np.abs(A @ x).max()  # a residual of the size of the product
    ref = {}
    for mode, first in FORMS:
        Bk = B if mode == 0 else f32(B)
        t = A @ x
        t[cons] = x[cons] / Bk[nodes[cons], comps[cons], comps[cons]]
        if mode == 0:
            ref[(mode, first)] = (None, None, t)
            continue
        xs1 = x.copy() if first else xs + x
        r1 = r - t
        z = np.einsum("nij,nj->ni", Bk, r1.reshape(-1, m.dim)).ravel()
        d = None if mode == 1 else (A_CHEB * x if mode == 2 else 0.0) + B_CHEB * z
        ref[(mode, first)] = (xs1, r1, d)
    # the stored rows of the constrained dofs are their diagonal d_r = 1 / B_rr (the plain form's definition)
    assert np.abs((A @ x)[cons] - ref[(0, 0)][2][cons]).max() <= 1e-12 * np.abs(A @ x).max()
    _cache[name] = (m, ctx, x, xs, r, ref)
    return _cache[name]


def _run(ctx, prec, form, x, xs, r, block_cap=0):
    mode, first = form
    return ctx.uu_fused_product(prec, mode, x, xs, r, first=first, a=A_CHEB, b=B_CHEB, block_cap=block_cap)


def _rel(got, want):
    return max(np.abs(g - w).max() / np.abs(w).max() for g, w in zip(got, want) if w is not None)


@pytest.mark.parametrize("name", SHAPES)
def test_fp64_instance_matches_the_stored_matrix_in_every_form(name):
    m, ctx, x, xs, r, ref = _case(name)
    worst = 0.0
    for form in FORMS:
        out = _run(ctx, 0, form, x, xs, r)
        assert [o is None for o in out[:3]] == [w is None for w in ref[form]]
        e = _rel(out[:3], ref[form])
        print(f"{name} mode {form[0]} first {form[1]}: fp64 instance against the reference {e:.2e}")
        worst = max(worst, e)
    assert worst <= 1e-12


@pytest.mark.parametrize("name", SHAPES)
def test_float_instance_matches_the_fp64_instance(name):
    m, ctx, x, xs, r, ref = _case(name)
    worst = 0.0
    for form in FORMS:
        o64, o32 = _run(ctx, 0, form, x, xs, r), _run(ctx, 1, form, x, xs, r)
        e = _rel(o32[:3], o64[:3])
        print(f"{name} mode {form[0]} first {form[1]}: float instance against the fp64 instance {e:.3e}")
        worst = max(worst, e)
    print(f"{name}: largest float-vs-fp64 difference {worst:.3e}")
    assert worst <= 4 * F32_PARENT


@pytest.mark.parametrize("name", SHAPES)
def test_single_precision_cells_with_double_vectors(name):
    """the instance of a double-vector caller with ifem_tuning::mf_f32 (R = float, V = double): same bound as the float instance"""
    m, ctx, x, xs, r, ref = _case(name)
    worst = max(_rel(_run(ctx, 2, form, x, xs, r)[:3], _run(ctx, 0, form, x, xs, r)[:3]) for form in FORMS)
    print(f"{name}: single-precision cells, double vectors against the fp64 instance {worst:.3e}")
    assert worst <= 4 * F32_PARENT


@pytest.mark.parametrize("name", SHAPES)
def test_the_same_call_twice_is_bit_identical(name):
    m, ctx, x, xs, r, ref = _case(name)
    for prec in (0, 1):
        for form in FORMS:
            a, b = _run(ctx, prec, form, x, xs, r), _run(ctx, prec, form, x, xs, r)
            for u, v in zip(a[:3], b[:3]):
                assert (u is None and v is None) or np.array_equal(u, v)


def test_chunks_and_blocks_of_the_launch():
    """12 x 6 x 6 Q2: 25 * 13 * 13 = 4225 nodes = 17 chunks.  Uncapped: 17 blocks, one chunk each.  Capped at 5 blocks: blocks 0 and 1 walk 4 chunks
    through the software pipeline (0, 5, 10, 15 and 1, 6, 11, 16: the 17th has 129 nodes), blocks 2-4 walk 3; capped at 1: one block walks all 17.
    The order of a node's sum does not depend on the split: every result is bit-identical to the uncapped one."""
    m, ctx, x, xs, r, ref = _case("q2_12x6x6")
    assert m.n_unodes == 4225
    for prec in (0, 1):
        for form in FORMS:
            base = _run(ctx, prec, form, x, xs, r)
            assert base[3] == (17, 17)
            for cap, blocks in ((5, 5), (1, 1), (40, 17)):
                out = _run(ctx, prec, form, x, xs, r, block_cap=cap)
                assert out[3] == (17, blocks)
                for u, v in zip(out[:3], base[:3]):
                    assert (u is None and v is None) or np.array_equal(u, v)
    _, cyl, cx, cxs, cr, _ = _case("cylinder3d")
    assert _run(cyl, 0, (0, 0), cx, cxs, cr, block_cap=3)[3] == (33, 3)


def test_capped_blocks_on_the_cylinder_match_the_reference():
    """33 chunks on 3 blocks (11 each), 5 of them with further tiles in the fp64 instance, between chunks that have none"""
    m, ctx, x, xs, r, ref = _case("cylinder3d")
    for form in FORMS:
        out = _run(ctx, 0, form, x, xs, r, block_cap=3)
        assert _rel(out[:3], ref[form]) <= 1e-12
        assert all((u is None and v is None) or np.array_equal(u, v) for u, v in zip(out[:3], _run(ctx, 0, form, x, xs, r)[:3]))


def test_lift_of_inhomogeneous_inflow_values():
    """ifem_tuning::stored_uu = 0 with non-zero inflow values (the LIFT instantiation of the gather): right-hand side against the stored assembly's,
    on the 3 x 3 x 3 box (two chunks) -- as test_gpu_mf_uniform.py does on 3 x 2 x 2"""
    capi = _capi()
    m, bcs = _mesh("q2_3x3x3")
    rng = np.random.default_rng(41)
    dofs, vals = m.dirichlet(bcs, {0: lambda p, c: 0.3 + 0.5 * p[1] if c == 0 else 0.1 * p[1]})
    assert np.abs(vals).max() > 0
    ev, pr = 0.3 * rng.standard_normal(m.n_dofs), 0.3 * rng.standard_normal(m.n_dofs)
    rhs = []
    for stored in (1, 0):
        ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
        if not stored:
            ctx.set_tuning(stored_uu=0)
            ctx.opts.ainv_kind = capi.AINV_GMRES_BJACOBI_MF
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
