"""A_uu by row owners (ifem_tuning::asm_rows, csrc/assemble_rows.hip) against the oracle's assembly.

On an undistorted 3D Q2 box on one rank one wavefront integrates the complete rows of up to 8 lattice nodes and stores them once: nothing
zeroes the value array and nothing adds to it.  Tolerances are the project's (test_gpu_parity._compare_assembly): matrix and right-hand side
entrywise to 1e-11 of the largest entry, M_p / diag(M_u) to 1e-12.  The edges (1.8, 0.7, 0.5) keep the axes apart; the cell counts are
the smallest at which each thing can first go wrong: (1, 2, 3) an axis with one cell and no interior vertex, owners of the last plane;
(2, 2, 2) the first vertex with 8 cells; (3, 3, 3) the first owner none of whose cells touches the boundary; (5, 4, 3) 120 owners, an
odd count, several workgroups per XCD.
"""
import numpy as np
import pytest

import orc
from boxmesh import BoxMesh

pytestmark = pytest.mark.gpu

EDGES = (1.8, 0.7, 0.5)
KW = dict(mu=0.7, rho=1.3, gamma=0.2, dt=0.01, g=(0.3, -9.8, 0.5), neumann={1: 2.5})
# full (7), single-component (1, 4) and inhomogeneous values: partly constrained node blocks occur
BCS = {0: (7, [0.3, -0.2, 0.1]), 2: (7, [0.0, 0.0, 0.0]), 3: (1, [0.05]), 4: (4, [0.02])}
MESHES = [(1, 2, 3), (2, 2, 2), (3, 3, 3), (5, 4, 3)]


def _capi():
    import openifem_amd.capi as capi
    return capi


class Case:
    """one mesh with its constraints, a context and the oracle system beside it"""

    def __init__(self, m, bcs=BCS, kw=KW, seed=2024):
        capi = _capi()
        self.m, self.kw, self.rng = m, kw, np.random.default_rng(seed)
        self.dofs, self.vals = m.dirichlet(bcs)
        self.ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
        self.ctx.set_constraints(0, self.dofs, None)
        self.ctx.set_constraints(1, self.dofs, self.vals)
        self.S = orc.System(m)
        self.S.set_constraints(0, self.dofs, None)
        self.S.set_constraints(1, self.dofs, self.vals)
        self.P, self.Po = capi.make_params(**kw), orc.make_params(**kw)

    def state(self):
        ev, pr = self.rng.standard_normal(self.m.n_dofs), self.rng.standard_normal(self.m.n_dofs)
        capi = _capi()
        self.ctx.vec_set(capi.VEC_PRESENT, pr)
        self.ctx.vec_set(capi.VEC_EVAL, ev)
        return ev, pr

    def check(self, use_nonzero, expect, label="", ev_pr=None):
        """one assembly from a fresh random state against the oracle; `expect`: the state the path must report"""
        capi = _capi()
        m = self.m
        ev, pr = ev_pr if ev_pr is not None else self.state()
        self.ctx.assemble(self.P, use_nonzero)
        assert self.ctx.asm_rows_state() == expect, label
        A, M, b = self.ctx.export_csr(0), self.ctx.export_csr(1), self.ctx.vec_get(capi.VEC_RHS)
        self.S.assemble(self.Po, use_nonzero, ev, pr)
        Ao, Mo, bo = self.S.csr("A"), self.S.csr("M"), self.S.rhs()
        dA = abs(A - Ao).max() / abs(Ao).max()
        db = np.abs(b - bo).max() / np.abs(bo).max()
        print(f"{label} cells {m.n_cells} nonzero {use_nonzero}: matrix {dA:.2e} rhs {db:.2e}")
        assert dA < 1e-11, f"{label}: matrix mismatch {dA}"
        assert db < 1e-11, f"{label}: rhs mismatch {db}"
        n_u = m.dim * m.n_unodes
        assert np.abs(M.diagonal()[:n_u] - Mo.diagonal()[:n_u]).max() / Mo.diagonal()[:n_u].max() < 1e-12, label
        assert abs(M[n_u:, n_u:] - Mo[n_u:, n_u:]).max() / abs(Mo[n_u:, n_u:]).max() < 1e-12, label
        return A, b

    def close(self):
        self.ctx.close()


def _box(reps, kv=2):
    dim = len(reps)
    return BoxMesh(reps, (0,) * dim, EDGES[:dim], kv=kv)


@pytest.mark.parametrize("reps", MESHES)
@pytest.mark.parametrize("use_nonzero", [False, True])
def test_row_owners_match_oracle(reps, use_nonzero):
    c = Case(_box(reps))
    c.check(use_nonzero, 1, "rows")
    c.close()


def test_four_assemblies_in_a_row_store_and_never_add():
    """nonzero fresh, nonzero with another evaluation point, zero, zero with another evaluation point (the cached-geometry path) on one
    context: nothing zeroes the array any more, so a kernel that adds where it must store, or leaves a block unwritten, is a mismatch"""
    c = Case(_box((3, 3, 3)))
    for use_nonzero, label in [(True, "nonzero fresh"), (True, "nonzero cached"), (False, "zero fresh"), (False, "zero cached")]:
        c.check(use_nonzero, 1, label)
    c.close()


@pytest.mark.parametrize("row_order", [0, 1])
def test_both_row_orders(row_order):
    c = Case(_box((3, 3, 3)))
    c.ctx.set_tuning(uu_row_order=row_order)
    A, _ = c.check(True, 1, f"uu_row_order {row_order}")
    assert bool(A.has_sorted_indices) == (row_order == 0), "ifem_tuning::uu_row_order did not take effect"
    c.check(False, 1, f"uu_row_order {row_order}")
    c.close()


def test_cell_launch_integrates_the_geometry_blocks_beside_the_rhs():
    c = Case(_box((3, 3, 3)))
    c.ctx.set_tuning(geo_cache=0)
    c.check(True, 1, "geo_cache 0")
    c.check(True, 1, "geo_cache 0 again")
    c.close()


def test_two_assemblies_from_one_state_are_bit_equal():
    capi = _capi()
    c = Case(_box((5, 4, 3)))
    ev_pr = c.state()
    A0, b0 = c.check(True, 1, "first", ev_pr)
    c.ctx.assemble(c.P, True)
    A1, b1 = c.ctx.export_csr(0), c.ctx.vec_get(capi.VEC_RHS)
    assert np.array_equal(A0.indices, A1.indices) and np.array_equal(A0.data, A1.data)
    assert np.array_equal(b0, b1)
    c.close()


def test_switching_the_path_on_one_context():
    c = Case(_box((3, 3, 3)))
    for rows, expect in [(1, 1), (0, 0), (1, 1)]:
        c.ctx.set_tuning(asm_rows=rows)
        c.check(True, expect, f"asm_rows {rows}")
    c.close()


def test_stored_operator_equals_the_matrix_free_one():
    c = Case(_box((3, 3, 3)))
    c.check(True, 1, "operator")
    n_u = 3 * c.m.n_unodes
    x = c.rng.standard_normal(c.m.n_dofs)
    ya, ym = c.ctx.uu_vmult(x, 0)[:n_u], c.ctx.uu_vmult(x, 3)[:n_u]
    assert np.abs(ya - ym).max() / np.abs(ya).max() < 1e-12
    c.close()


def test_imex_matrix_by_row_owners():
    """InsIMEX takes the path: no convective terms, the mass term on the scalar part, every field from the present solution"""
    capi = _capi()
    c = Case(_box((3, 3, 3)))
    pr = c.rng.standard_normal(c.m.n_dofs)
    c.ctx.vec_set(capi.VEC_PRESENT, pr)
    c.ctx.vec_set(capi.VEC_EVAL, c.rng.standard_normal(c.m.n_dofs))  # must be ignored
    c.S.imex_assemble(c.Po, True, True, pr, None)
    Ao, bo = c.S.csr("A"), c.S.rhs()
    c.ctx.imex_assemble(c.P, True, True)
    assert c.ctx.asm_rows_state() == 1
    A, b = c.ctx.export_csr(0), c.ctx.vec_get(capi.VEC_RHS)
    assert abs(A - Ao).max() / abs(Ao).max() < 1e-11
    assert np.abs(b - bo).max() / np.abs(bo).max() < 1e-11
    c.close()


def _moved_vertex():
    m = _box((3, 3, 3))
    m.vcoords = m.vcoords.copy()
    # one vertex of one cell description moved by 1e-3 of an edge: its cells are no boxes any more
    v = m.vcoords.reshape(m.n_cells, 8, 3)
    x0 = v[13, 0].copy()
    hit = np.all(np.abs(v - x0) < 1e-12, axis=2)
    v[hit] += np.array([1e-3 * EDGES[0] / 3, 0, 0])
    return m


@pytest.mark.parametrize("what", ["moved vertex", "kv=1", "2D"])
def test_refusals_keep_the_cell_kernel(what):
    if what == "moved vertex":
        c = Case(_moved_vertex())
    elif what == "kv=1":
        c = Case(_box((3, 3, 3), kv=1))
    else:
        c = Case(_box((4, 3)), bcs={0: (3, [0.3, -0.2]), 2: (3, [0.0, 0.0]), 3: (1, [0.05])}, kw=dict(KW, g=(0.3, -9.8)))
    c.check(True, -1, what)
    c.check(False, -1, what)
    c.close()


def test_scalar_operator_wanted_is_a_refusal():
    capi = _capi()
    c = Case(_box((3, 3, 3)))
    assert c.ctx.L.ifem_set_ainv_kind(c.ctx.h, capi.AINV_SCALAR_GMRES) == 0
    c.check(True, -1, "Shat")
    c.close()


def test_hanging_node_band_is_a_refusal():
    from hangmesh import HangingMesh
    capi = _capi()
    m = HangingMesh((2, 2, 2), (0, 0, 0), EDGES, {(0, 0, 0)}, kv=2)
    rng = np.random.default_rng(5)
    dofs, vals = m.dirichlet({0: (7, [0.3, -0.2, 0.1]), 2: (7, [0.0] * 3)})
    ev, pr = 0.3 * rng.standard_normal(m.n_dofs), 0.3 * rng.standard_normal(m.n_dofs)
    S = orc.System(m)
    S.set_constraints(0, dofs, None)
    S.set_constraints(1, dofs, vals)
    Ao, bo = S.assemble_affine_dense(orc.make_params(**KW), True, ev, pr, m)
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    ctx.set_constraints(0, dofs, None)
    ctx.set_constraints(1, dofs, vals)
    ctx.set_hanging_constraints(m.hang_dof, m.hang_ptr, m.hang_master, m.hang_weight)
    ctx.vec_set(capi.VEC_PRESENT, pr)
    ctx.vec_set(capi.VEC_EVAL, ev)
    ctx.assemble(capi.make_params(**KW), True)
    assert ctx.asm_rows_state() == -1
    reg = np.setdiff1d(np.arange(m.n_dofs), m.hang_dof)
    b = ctx.vec_get(capi.VEC_RHS)
    assert np.abs(b[reg] - bo[reg]).max() <= 1e-11 * np.abs(bo).max()
    x = rng.standard_normal(m.n_dofs)
    y, yo = ctx.system_vmult(x), Ao @ x
    assert np.abs(y[reg] - yo[reg]).max() <= 1e-11 * np.abs(yo).max()
    ctx.close()


def _mirror_vec(s, which):
    import ctypes as C
    capi = _capi()
    n = s.sizes()[1] + s.sizes()[2]
    v = np.zeros(n)
    assert capi.load().ifem_vec_get(s.ctx, which, v.ctypes.data_as(C.c_void_p)) == 0
    return v


def _mirror_state(s):
    import ctypes as C
    st = C.c_int32(0)
    assert _capi().load().ifem_test_asm_rows(s.ctx, 0, C.byref(st)) == 0
    return int(st.value)


def test_two_virtual_ranks_are_a_refusal():
    """a partitioned context keeps the cell kernel (ghost rows, rows summed by their owner rank only): state -1, and the assembled
    right-hand side is the single context's, which takes the row owners"""
    import ctypes as C
    import threading
    from openifem_amd import host
    capi = _capi()
    L = capi.load()
    reps, ext = (4, 2, 2), (2.0, 0.2, 0.2)
    s1 = host.InsIM(host.channel_prm(3), reps, (0, 0, 0), ext)
    s1.setup(0)
    s1.channel_state()
    s1.assemble(False)
    assert _mirror_state(s1) == 1
    t1 = s1.partition_tables()
    n_ug = t1["n_unodes_global"]
    g = np.concatenate([(t1["l2g_u"][:, None] * 3 + np.arange(3)[None, :]).ravel(), 3 * n_ug + t1["l2g_p"]])
    rhs1 = np.zeros(len(g))
    rhs1[g] = _mirror_vec(s1, capi.VEC_RHS)
    s1.close()
    w = C.c_void_p(L.ifem_local_world_create(2))
    out, errs = [None, None], []

    def work(rank):
        try:
            s = host.InsIM(host.channel_prm(3), reps, (0, 0, 0), ext)
            s.set_partition((2, 1, 1), rank, local_world=w)
            s.setup(0)
            s.channel_state()
            assert L.ifem_halo_exchange(s.ctx, capi.VEC_EVAL) == 0
            s.assemble(False)
            t = s.partition_tables()
            n_owned = 3 * t["n_unodes_owned"] + t["n_pnodes_owned"]
            rhs = np.zeros(n_owned)
            assert L.ifem_vec_get(s.ctx, capi.VEC_RHS, rhs.ctypes.data_as(C.c_void_p)) == 0
            out[rank] = (t, rhs, _mirror_state(s))
            s.close()
        except Exception:  # noqa
            import traceback
            errs.append((rank, traceback.format_exc()))

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    L.ifem_local_world_destroy(w)
    rhs = np.full(len(g), np.nan)
    for t, r, st in out:
        assert st == -1
        nuo, npo = t["n_unodes_owned"], t["n_pnodes_owned"]
        rhs[(t["l2g_u"][:nuo, None] * 3 + np.arange(3)[None, :]).ravel()] = r[:3 * nuo]
        rhs[3 * n_ug + t["l2g_p"][:npo]] = r[3 * nuo:]
    assert not np.isnan(rhs).any()
    assert np.abs(rhs - rhs1).max() / np.abs(rhs1).max() < 1e-11


def test_through_the_mirror_the_switch_changes_no_count():
    """the 16^3 channel through the host mirror with asm_rows 1, 0, 1: the same (fgmres, inner, cg_sm, cg_mp) counts three times and
    updates equal to 1e-6 of the largest entry.  One solve comes first: the first solve of a solver estimates the smoother's eigenvalues
    cold and runs its first preconditioner application tighter, whichever way the matrix was assembled"""
    import ctypes as C
    from openifem_amd import host
    capi = _capi()
    L = capi.load()
    s = host.InsIM(host.channel_prm(3), (16, 16, 16), (0, 0, 0), (2.0, 0.2, 0.2))
    s.setup(0)
    s.channel_state()
    s.assemble(False)
    s.solve(False)
    runs = []
    for rows, expect in [(1, 1), (0, 0), (1, 1)]:
        tun = capi.Tuning()
        L.ifem_default_tuning(C.byref(tun))
        tun.asm_rows = rows
        assert L.ifem_set_tuning(s.ctx, C.byref(tun)) == 0
        s.assemble(False)
        assert _mirror_state(s) == expect
        st = s.solve(False)
        runs.append(((st.fgmres_iters, st.inner_iters, st.cg_sm_iters, st.cg_mp_iters), _mirror_vec(s, capi.VEC_UPDATE)))
    s.close()
    print([r[0] for r in runs])
    assert runs[0][0] == runs[1][0] == runs[2][0]
    top = np.abs(runs[0][1]).max()
    assert np.abs(runs[1][1] - runs[0][1]).max() <= 1e-6 * top
    assert np.abs(runs[2][1] - runs[0][1]).max() <= 1e-6 * top
