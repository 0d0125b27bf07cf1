"""Every dispatch arm of the stored-matrix product linalg.hip::spmv_uu -- ifem_tuning::spmv_pipe (0 / 1) x spmv_lanes (8 / 16 / 32 / 64), fp64 and
fp32 values, 2D and 3D, with and without the B^T x_p half, both block orders of a row (ifem_tuning::uu_row_order) -- against the product
with the exported CSR (ifem_export_csr) taken in np.longdouble, through hooks the library already has (ifem_set_tuning, ifem_uu_vmult
variants 0 and 1, ifem_system_vmult).

Meshes: 3D Q2 (4,3,3), 3D Q1 (5,4,3), 2D Q2 (5,3), 2D Q1 (4,3) on the channel extents.  No row count is a multiple of 16 (the last workgroup
of k_spmv_uu_pipe is ragged), interior Q2 rows hold more than 32 blocks (rows of several pipeline items), Q1 rows are shorter than the lane
group (idle lanes).

Row-wise bound: |err_i| <= (entries_i + 8) u (|A| |x|)_i, entries_i the stored entries of row i that take part (blocks x dim of A_uu, plus
the B^T entries of the row in the system product): no chain of additions in a row is longer than its entries plus the log2(64) = 6 steps of
the lane sum, and every product is rounded once.  The fp32-values product is compared with the same row sums of the exported values rounded
to float32 and widened: the kernel accumulates in double, only the stored values are single precision."""
import ctypes as C

import numpy as np
import pytest

from boxmesh import BoxMesh

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
EXTENT = (2.0, 0.2, 0.2)
MESHES = [(3, 2, (4, 3, 3)), (3, 1, (5, 4, 3)), (2, 2, (5, 3)), (2, 1, (4, 3))]
KW = dict(mu=0.7, rho=1.3, gamma=0.2, dt=0.01)
ARMS = [(pipe, lanes) for pipe in (0, 1) for lanes in (8, 16, 32, 64)]
STORED, STORED_F32 = 0, 1  # IFEM_AINV_GMRES_BJACOBI, _F32


def _capi():
    from openifem_amd import capi
    return capi


def _bcs(dim):
    """inflow (x-) and the walls (y-, y+, and z-, z+ in 3D)"""
    flag = 3 if dim == 2 else 7
    bcs = {0: (flag, [0.3, -0.2, 0.1][:dim]), 2: (flag, [0.0] * dim), 3: (flag, [0.0] * dim)}
    if dim == 3:
        bcs.update({4: (flag, [0.0] * dim), 5: (flag, [0.0] * dim)})
    return bcs


def _assembled(dim, kv, reps, order, seed):
    capi = _capi()
    m = BoxMesh(reps, (0,) * dim, EXTENT[:dim], kv=kv)
    rng = np.random.default_rng(seed)
    dofs, vals = m.dirichlet(_bcs(dim))
    ctx = capi.Context(dim, kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    ctx.set_tuning(uu_row_order=order)  # the blocks are ordered when the first assembly allocates the values
    ctx.set_constraints(0, dofs, None)
    ctx.set_constraints(1, dofs, vals)
    ctx.vec_set(capi.VEC_PRESENT, rng.standard_normal(m.n_dofs))
    ctx.vec_set(capi.VEC_EVAL, rng.standard_normal(m.n_dofs))
    ctx.assemble(capi.make_params(**KW), False)
    return ctx, m, rng


class _Reference:
    """row sums of the exported matrix in longdouble, computed once per context: the whole system, its A_uu block, and that block with its
    values rounded to float32"""

    def __init__(self, ctx, m, x):
        A = ctx.export_csr(0)
        self.n_u = n_u = m.dim * m.n_unodes
        rp, col, val = A.indptr.astype(np.int64), A.indices, A.data
        assert A.shape == (m.n_dofs, m.n_dofs) and np.all(np.diff(rp) > 0)
        start = rp[:-1]
        row_of = np.repeat(np.arange(len(start)), np.diff(rp))
        uu = (row_of < n_u) & (col < n_u)
        xl = x.astype(LD)[col]

        def sums(v, mask):
            t = np.where(mask, v.astype(LD) * xl, LD(0))
            return np.add.reduceat(t, start), np.add.reduceat(np.abs(t), start), np.add.reduceat(mask.astype(np.int64), start)

        self.sys = sums(val, np.ones(len(val), bool))
        self.uu = tuple(a[:n_u] for a in sums(val, uu))
        self.uu32 = tuple(a[:n_u] for a in sums(val.astype(np.float32).astype(np.float64), uu))
        self.max_blocks = int(self.uu[2].max()) // m.dim

    @staticmethod
    def ratio(got, ref):
        y, mag, entries = ref
        bound = (entries + 8) * U * mag
        err = np.abs(got.astype(LD) - y)
        assert np.all(err[bound == 0] == 0)
        return float((err[bound > 0] / bound[bound > 0]).max())


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dim,kv,reps", MESHES)
def test_every_spmv_arm_matches_the_exported_matrix(dim, kv, reps, order):
    ctx, m, rng = _assembled(dim, kv, reps, order, 17 + 2 * dim + kv)
    x = rng.standard_normal(m.n_dofs)
    ref = _Reference(ctx, m, x)
    n_u = ref.n_u
    assert m.n_unodes % 16 != 0
    assert ref.max_blocks > 32 if kv == 2 and dim == 3 else ref.max_blocks > 0
    if kv == 1:
        assert ref.max_blocks <= 27  # shorter than a group of 32 lanes: idle lanes
    worst = {}
    for pipe, lanes in ARMS:
        ctx.set_tuning(spmv_pipe=pipe, spmv_lanes=lanes)
        r = (_Reference.ratio(ctx.uu_vmult(x, STORED)[:n_u], ref.uu), _Reference.ratio(ctx.system_vmult(x), ref.sys),
             _Reference.ratio(ctx.uu_vmult(x, STORED_F32)[:n_u], ref.uu32))
        worst[(pipe, lanes)] = r
        print(f"spmv {dim}D Q{kv} {reps} uu_row_order={order} pipe={pipe} lanes={lanes}: err/bound  A_uu fp64 {r[0]:.3f}  system {r[1]:.3f}  A_uu fp32 values {r[2]:.3f}"
              f"  (longest row {ref.max_blocks} blocks)")
    ctx.close()
    bad = {k: v for k, v in worst.items() if not max(v) <= 1.0}
    assert not bad, bad


def test_invalid_lane_count_is_refused_and_the_previous_tuning_stays():
    capi = _capi()
    ctx, m, rng = _assembled(3, 2, (4, 3, 3), 1, 5)
    x = rng.standard_normal(m.n_dofs)
    ref = _Reference(ctx, m, x)
    ctx.set_tuning(spmv_pipe=0, spmv_lanes=16)
    before = ctx.uu_vmult(x, STORED)[:ref.n_u]
    t = capi.Tuning()
    ctx.L.ifem_default_tuning(C.byref(t))
    t.spmv_pipe, t.spmv_lanes = 0, 12
    assert ctx.L.ifem_set_tuning(ctx.h, C.byref(t)) == capi.E_BADPARAM
    assert b"lanes" in ctx.L.ifem_last_error()
    after = ctx.uu_vmult(x, STORED)[:ref.n_u]
    assert np.array_equal(before, after)  # the same kernel, the same bits
    assert _Reference.ratio(after, ref.uu) <= 1.0 and _Reference.ratio(ctx.system_vmult(x), ref.sys) <= 1.0
    ctx.close()
