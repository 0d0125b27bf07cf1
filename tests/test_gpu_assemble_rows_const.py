"""The row owners of A_uu (csrc/assemble_rows.hip) take the cell-independent terms of the element matrix from a table and contract only what
depends on the cell: the table alone, either part alone, a change of parameters on one context, owners that lack cells (absent slots of
the staged point data), and the workgroup order per XCD, all against the oracle's assembly.

Tolerances are the project's: matrix and right-hand side entrywise to 1e-11 of the largest entry (test_gpu_parity._compare_assembly),
the table to 1e-12 of the largest entry (the bound of M_p / diag(M_u): one 27-point sum per entry, nothing added from other cells).
Edges, parameters and constraints are those of test_gpu_assemble_rows.py.
"""
import numpy as np
import pytest

import orc
from boxmesh import BoxMesh

pytestmark = pytest.mark.gpu

EDGES = (1.8, 0.7, 0.5)
KW = dict(mu=0.7, rho=1.3, gamma=0.2, dt=0.01, g=(0.3, -9.8, 0.5), neumann={1: 2.5})
BCS = {0: (7, [0.3, -0.2, 0.1]), 2: (7, [0.0, 0.0, 0.0]), 3: (1, [0.05]), 4: (4, [0.02])}


def _capi():
    import openifem_amd.capi as capi
    return capi


def _box(reps):
    return BoxMesh(reps, (0, 0, 0), EDGES, kv=2)


class Case:
    """one mesh with its constraints (None: no constraint at all), a context and the oracle system beside it"""

    def __init__(self, m, bcs=BCS, seed=2025):
        capi = _capi()
        self.m, self.rng = m, np.random.default_rng(seed)
        self.ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
        self.S = orc.System(m)
        if bcs is not None:
            dofs, vals = m.dirichlet(bcs)
            for which, v in ((0, None), (1, vals)):
                self.ctx.set_constraints(which, dofs, v)
                self.S.set_constraints(which, dofs, v)

    def set_state(self, ev, pr):
        capi = _capi()
        self.ctx.vec_set(capi.VEC_PRESENT, pr)
        self.ctx.vec_set(capi.VEC_EVAL, ev)

    def random_state(self):
        return self.rng.standard_normal(self.m.n_dofs), self.rng.standard_normal(self.m.n_dofs)

    def compare(self, Ao, bo, label):
        """the context's matrix and right-hand side, which the row owners must have written, against the oracle's"""
        capi = _capi()
        assert self.ctx.asm_rows_state() == 1, label
        A, b = self.ctx.export_csr(0), self.ctx.vec_get(capi.VEC_RHS)
        dA = abs(A - Ao).max() / abs(Ao).max()
        db = np.abs(b - bo).max() / np.abs(bo).max()
        print(f"{label} cells {self.m.n_cells}: matrix {dA:.2e} rhs {db:.2e}")
        assert dA < 1e-11, f"{label}: matrix mismatch {dA}"
        assert db < 1e-11, f"{label}: rhs mismatch {db}"
        return A, b

    def check(self, kw, use_nonzero, label, ev_pr=None):
        ev, pr = ev_pr if ev_pr is not None else self.random_state()
        self.set_state(ev, pr)
        self.ctx.assemble(_capi().make_params(**kw), use_nonzero)
        self.S.assemble(orc.make_params(**kw), use_nonzero, ev, pr)
        return self.compare(self.S.csr("A"), self.S.rhs(), label)

    def check_imex(self, kw, label):
        pr = self.rng.standard_normal(self.m.n_dofs)
        self.set_state(self.rng.standard_normal(self.m.n_dofs), pr)  # the evaluation point must be ignored
        self.ctx.imex_assemble(_capi().make_params(**kw), True, True)
        self.S.imex_assemble(orc.make_params(**kw), True, True, pr, None)
        return self.compare(self.S.csr("A"), self.S.rhs(), label)

    def close(self):
        self.ctx.close()


def _single_cell_blocks(m, cell, mat):
    """[a 27][b 27][c 3][d 3] of the velocity block of `mat` for the local nodes of `cell`, and which (a, b) belong to no other cell"""
    nodes = np.asarray(m.cell_unodes).reshape(m.n_cells, 27)
    shared = np.zeros((27, 27), int)
    for other in range(m.n_cells):
        inside = np.isin(nodes[cell], nodes[other])
        shared += np.outer(inside, inside)
    dofs = (3 * nodes[cell][:, None] + np.arange(3)[None, :]).ravel()
    blocks = mat[dofs][:, dofs].toarray().reshape(27, 3, 27, 3).transpose(0, 2, 1, 3)
    return blocks, shared == 1


def test_table_equals_the_oracles_constant_element_matrix():
    """no constraints, evaluation point and present solution zero: the oracle's A_uu of a cell is the constant element matrix plus
    rho / dt M, and the IMEX matrix is the table with its mass term"""
    m = _box((1, 1, 1))  # BoxMesh takes a single cell: every block of cell 0 is its own alone
    c = Case(m, bcs=None)
    capi = _capi()
    P, Po = capi.make_params(**KW), orc.make_params(**KW)
    zero = np.zeros(m.n_dofs)
    c.S.assemble(Po, False, zero, zero)
    Ao, alone = _single_cell_blocks(m, 0, c.S.csr("A"))
    Mo, _ = _single_cell_blocks(m, 0, c.S.csr("M"))
    assert alone.all(), "a single cell shares no block"
    top = np.abs(Ao[alone]).max()
    K0 = c.ctx.rows_const(P, imex=False)
    d0 = np.abs(K0 + KW["rho"] / KW["dt"] * Mo - Ao)[alone].max() / top
    c.S.imex_assemble(Po, False, True, zero, None)
    Ai, _ = _single_cell_blocks(m, 0, c.S.csr("A"))
    K1 = c.ctx.rows_const(P, imex=True)
    d1 = np.abs(K1 - Ai)[alone].max() / np.abs(Ai[alone]).max()
    print(f"table: Newton {d0:.2e} IMEX {d1:.2e} ({int(alone.sum())} blocks)")
    assert d0 < 1e-12 and d1 < 1e-12
    # the mass term is in the IMEX table only, and only on the diagonal blocks
    off = ~np.eye(3, dtype=bool)
    assert np.array_equal(K0[:, :, off], K1[:, :, off]) and np.abs(K1 - K0)[:, :, ~off].max() > 0
    c.close()


@pytest.mark.parametrize("part", ["variable", "table"])
def test_either_part_alone(part):
    """(a) mu = gamma = 0: only the contracted terms and the mass term remain; (b) evaluation point zero: only the table and the mass term.
    A table added twice, or a mass term counted in the point data and in the table, fails one of the two"""
    c = Case(_box((3, 3, 3)))
    ev, pr = c.random_state()
    if part == "variable":
        c.check(dict(KW, mu=0.0, gamma=0.0), True, part, (ev, pr))
    else:
        c.check(KW, True, part, (np.zeros_like(ev), pr))
    c.close()


def test_parameters_change_on_one_context():
    """the table is refilled by every launch: a stale one is a mismatch"""
    c = Case(_box((3, 3, 3)))
    c.check(KW, True, "first")
    other = dict(KW, mu=3 * KW["mu"], dt=0.5 * KW["dt"], gamma=0.0)
    c.check(other, True, "other parameters")
    c.check_imex(other, "imex")
    c.check(other, True, "newton again")
    c.check(KW, False, "first parameters again")
    c.close()


@pytest.mark.parametrize("reps,use_nonzero", [((1, 2, 3), True), ((1, 2, 3), False), ((2, 1, 1), True)])
def test_owners_that_lack_cells(reps, use_nonzero):
    """(1, 2, 3): every owner lacks cells; (2, 1, 1): an owner has a single cell and most cell slots are absent"""
    c = Case(_box(reps))
    c.check(KW, use_nonzero, f"{reps}")
    c.check_imex(KW, f"{reps} imex")
    c.close()


def test_owner_ranges_per_xcd_change_no_bit():
    """(5, 4, 3): 120 owners in 30 workgroups, no multiple of 8; ifem_tuning::xcd_swizzle only renumbers workgroups (of the cell launch;
    the row owners keep the block order, profiles/r18_assemble_rows.txt): whoever integrates a cell or owns a row, the bits stay"""
    c = Case(_box((5, 4, 3)))
    ev_pr = c.random_state()
    out = []
    for sw in (1, 0):
        c.ctx.set_tuning(xcd_swizzle=sw)
        out.append(c.check(KW, True, f"xcd_swizzle {sw}", ev_pr))
    (A1, b1), (A0, b0) = out
    assert np.array_equal(A1.indptr, A0.indptr) and np.array_equal(A1.indices, A0.indices) and np.array_equal(A1.data, A0.data)
    assert np.array_equal(b1, b0)
    c.close()
