"""Adaptive refinement, host side (CPU): the numpy reference checks itself on fields with known indicators; the library's face table
against geometric neighbours; the marking rule, the level caps and the re-flagging of a refined box on hand-made criteria; the transfer
table applied in numpy; the new C ABI symbols.  Reference: FluidSolver::refine_mesh, mpi_fluid_solver.cpp:416-488."""
import os

import numpy as np
import pytest

import refine_ref as rr
from hangmesh import HangingMesh

MESHES = {
    "2d": ((3, 2), (0, 0), (1.5, 0.8), {(0, 0), (2, 1)}),
    "3d_corner": ((2, 2, 2), (0, 0, 0), (1.0, 0.8, 0.6), {(0, 0, 0)}),
    "3d_centre": ((3, 3, 3), (0, 0, 0), (1.2, 0.9, 0.6), {(1, 1, 1)}),
    "3d_all_but_centre": ((3, 3, 3), (0, 0, 0), (1.2, 0.9, 0.6),
                          {(i, j, k) for i in range(3) for j in range(3) for k in range(3)} - {(1, 1, 1)}),
    "2d_uniform": ((3, 2), (0, 0), (1.5, 0.8), set()),
    "3d_uniform": ((2, 2, 2), (0, 0, 0), (1.0, 0.8, 0.6), set()),
}


def mesh(name, kv):
    reps, p0, p1, refine = MESHES[name]
    return HangingMesh(reps, p0, p1, refine, kv=kv)


def _host():
    from openifem_amd import host
    return host


def q1_prm(dim=2):
    return _host().channel_prm(dim).replace("set Velocity degree = 2", "set Velocity degree = 1")


def host_solver(name, kv, flags=None):
    """a host-only solver (no device) on the box of MESHES[name] with its refined cells, or with the per-coarse-cell `flags`"""
    host = _host()
    reps, p0, p1, refine = MESHES[name]
    s = (host.InsIM if kv == 2 else host.SCnsIM)(host.channel_prm(len(reps)) if kv == 2 else q1_prm(len(reps)), reps, p0, p1)
    if flags is None:
        flags = np.zeros(int(np.prod(reps)), np.uint8)
        for ci in refine:
            flags[sum(c * int(np.prod(reps[:d])) for d, c in enumerate(ci))] = 1
    if np.any(flags):
        s.set_active_flags(flags, np.zeros_like(flags))
    s.setup_host_only(0)
    return s


# ---- the reference checks itself

@pytest.mark.parametrize("dim", [2, 3])
def test_reference_kink_has_its_analytic_indicator(dim):
    reps, p1 = ((4, 2), (2.0, 0.6)) if dim == 2 else ((4, 2, 2), (2.0, 0.6, 0.5))
    m = HangingMesh(reps, (0,) * dim, p1, set(), kv=1)
    x0 = 1.0  # the boundary between the second and the third cell along x
    x = rr.interpolate(m, lambda p: [abs(p[0] - x0)] + [0.0] * (dim - 1))
    eta = rr.kelly(m, x)
    lo, h = rr.boxes(m)
    touching = (np.abs(lo[:, 0] - x0) < 1e-12) | (np.abs(lo[:, 0] + h[:, 0] - x0) < 1e-12)
    area = np.prod(h[:, 1:], axis=1)
    exact = np.where(touching, np.sqrt(np.linalg.norm(h, axis=1) / 24.0 * 4.0 * area), 0.0)
    assert touching.sum() == 2 * int(np.prod(reps[1:]))
    assert np.abs(eta - exact).max() <= 1e-13 * exact.max()


@pytest.mark.parametrize("name", list(MESHES))
@pytest.mark.parametrize("kv", [1, 2])
def test_reference_polynomial_has_no_jump(name, kv):
    m = mesh(name, kv)
    fu, grad = rr.random_polynomial(m.dim, kv, np.random.default_rng(3))
    eta = rr.kelly(m, rr.interpolate(m, fu))
    assert eta.max() <= 1e-12 * max(grad(p) for p in m.unode_coords)


# ---- face table

@pytest.mark.parametrize("name", ["2d", "3d_corner", "3d_centre", "3d_all_but_centre"])
def test_face_table_matches_geometric_neighbours(name):
    host = _host()
    reps, p0, p1, _ = MESHES[name]
    m = mesh(name, 2)
    ref = rr.face_table(m)
    got = host.box_face_table(reps, p0, p1, m.vcoords)
    assert got.shape == ref.shape and np.array_equal(got, ref)
    kinds = set((ref[:, :, 0] & 0xff).ravel())
    assert {rr.FACE_BOUNDARY, rr.FACE_EQUAL, rr.FACE_COARSER, rr.FACE_FINER} <= kinds
    if name == "3d_centre":  # the fine cells see coarser neighbours on both signs of every axis
        fine = np.nonzero(rr.boxes(m)[1][:, 0] < 0.3)[0]
        assert {f for c in fine for f in range(6) if ref[c, f, 0] & 0xff == rr.FACE_COARSER} == set(range(6))
        assert {int(ref[c, f, 0]) >> 8 for c in fine for f in range(6) if ref[c, f, 0] & 0xff == rr.FACE_COARSER} == {0, 1, 2, 3}
    if name == "3d_all_but_centre":  # the coarse cell sees finer neighbours on all six faces
        coarse = int(np.argmax(rr.boxes(m)[1][:, 0]))
        assert all(ref[coarse, f, 0] == rr.FACE_FINER for f in range(6))
    # the solver's own tables (distribute_dofs_refined_box keeps the order of HangingMesh) give the same table
    s = host_solver(name, 2)
    assert np.array_equal(s.cell_tables()[3], m.vcoords)
    assert np.array_equal(s.face_table(), ref)
    s.close()


def test_face_table_of_a_uniform_solver_in_its_own_cell_order():
    # distribute_dofs_box orders the cells along a Morton curve: the table follows the solver's order, whatever it is
    s = host_solver("2d_uniform", 2)
    vc = s.cell_tables()[3]
    reps, p0, p1, _ = MESHES["2d_uniform"]
    tab = s.face_table()
    lo, hi = vc[:, 0, :], vc[:, -1, :]
    for c in range(len(vc)):
        for f in range(4):
            d, side = f // 2, f % 2
            if tab[c, f, 0] == rr.FACE_BOUNDARY:
                assert abs((hi if side else lo)[c, d] - (p1 if side else p0)[d]) < 1e-12
            else:
                k = tab[c, f, 1]
                assert tab[c, f, 0] == rr.FACE_EQUAL and abs((hi if side else lo)[c, d] - (lo if side else hi)[k, d]) < 1e-12
                assert abs(lo[c, 1 - d] - lo[k, 1 - d]) < 1e-12
    s.close()


# ---- marking

def test_marking_prefix_and_suffix_sums():
    host = _host()
    crit = np.array([5.0, 1.0, 3.0, 0.5, 0.25, 0.25])  # total 10: refine until >= 6 -> {0, 2}; coarsen until >= 4 -> {5, 4, 3, 1, 2} minus refined
    r, c = host.mark_fixed_fraction(crit)
    assert r.tolist() == [1, 0, 1, 0, 0, 0] and c.tolist() == [0, 1, 0, 1, 1, 1]
    r, c = host.mark_fixed_fraction(crit, 0.5, 0.05)  # 5 >= 5: one cell; 0.25 + 0.25 >= 0.5: two cells
    assert r.tolist() == [1, 0, 0, 0, 0, 0] and c.tolist() == [0, 0, 0, 0, 1, 1]
    rng = np.random.default_rng(11)
    for n in (1, 2, 7, 64):
        crit = rng.random(n) ** 3
        r, c = host.mark_fixed_fraction(crit)
        rr_, cr_, _ = rr.mark(crit)
        assert np.array_equal(r, rr_) and np.array_equal(c, cr_)
        assert not np.any(r & c)


def test_marking_ties_go_to_the_lower_cell_index():
    host = _host()
    crit = np.ones(10)  # refine: 6 cells reach 0.6 * 10 -> cells 0..5; coarsen: 4 cells from the end of the order -> cells 6..9
    r, c = host.mark_fixed_fraction(crit)
    assert r.tolist() == [1] * 6 + [0] * 4 and c.tolist() == [0] * 6 + [1] * 4
    crit = np.array([1.0, 2.0, 2.0, 1.0])  # order 1, 2, 0, 3: refine {1, 2} (4 >= 3.6); coarsen {3, 0, 2}: 1 + 1 < 2.4 <= 4, cell 2 is refined
    r, c = host.mark_fixed_fraction(crit)
    assert r.tolist() == [0, 1, 1, 0] and c.tolist() == [1, 0, 0, 1]
    # the criteria are compared as floats: a difference below float precision is a tie
    crit = np.array([1.0, 1.0 + 1e-12, 1.0, 1.0])
    r, _ = host.mark_fixed_fraction(crit, 0.25, 0.25)
    assert r.tolist() == [1, 0, 0, 0]


def test_marking_zero_total_flags_nothing():
    host = _host()
    r, c = host.mark_fixed_fraction(np.zeros(5))
    assert not r.any() and not c.any()
    r, c = host.mark_fixed_fraction(np.zeros(0))
    assert len(r) == 0 and len(c) == 0


def _flag_solver():
    host = _host()
    reps, p0, p1, _ = MESHES["2d"]
    return host.InsIM(host.channel_prm(2), reps, p0, p1)


def test_level_caps():
    s = _flag_solver()
    assert s.n_active_cells() == 6
    # max_grid_level: coarse cells of level 2 are not refined when max is 2, they are when it is 3
    r, c, coarse, lr = s.set_active_flags([1, 0, 0, 0, 0, 1], [0] * 6, base_level=2, min_level=2, max_level=2)
    assert not r.any() and not coarse.any() and not lr
    r, c, coarse, lr = s.set_active_flags([1, 0, 0, 0, 0, 1], [0, 1, 1, 0, 0, 0], base_level=2, min_level=2, max_level=5)
    assert r.tolist() == [1, 0, 0, 0, 0, 1] and not c.any()  # coarsen flags on cells of min_grid_level are cleared
    assert coarse.tolist() == [1, 0, 0, 0, 0, 1] and lr and s.n_active_cells() == 12
    # children: never refined again (one level), and they may coarsen because their level is base + 1 > min
    flags_r = [1] * 12
    flags_c = [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    r, c, coarse, lr = s.set_active_flags(flags_r, flags_c, base_level=2, min_level=2, max_level=5)
    assert r.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0]
    assert c.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    ref = rr.reflag([1, 0, 0, 0, 0, 1], flags_r, flags_c, 2, 2, 2, 5)
    assert np.array_equal(ref[0], r) and np.array_equal(ref[1], c) and np.array_equal(ref[2], coarse)
    # (children carrying refine AND coarsen flags: the refine flag went with the cap, the coarsen flags un-refine cell 0)
    assert coarse.tolist() == [0, 1, 1, 1, 1, 1]
    # min_grid_level = base + 1 protects the children
    r, c, coarse, lr = s.set_active_flags([0] * 21, [1] * 21, base_level=2, min_level=3, max_level=5)
    assert c.tolist() == [1] + [0] * 20 and coarse.tolist() == [0, 1, 1, 1, 1, 1]
    s.close()


def test_unrefinement_needs_all_children_and_a_box_can_return_to_uniform():
    s = _flag_solver()
    r, c, coarse, lr = s.set_active_flags([1, 0, 0, 0, 0, 1], [0] * 6)
    assert coarse.tolist() == [1, 0, 0, 0, 0, 1] and lr
    # active cells now: children of cell 0 (4), cells 1..4, children of cell 5 (4)
    co = np.zeros(12, np.uint8)
    co[[0, 1, 2]] = 1  # three of four children of cell 0
    co[8:12] = 1       # all children of cell 5
    r, c, coarse, lr = s.set_active_flags(np.zeros(12, np.uint8), co)
    assert coarse.tolist() == [1, 0, 0, 0, 0, 0] and lr
    assert np.array_equal(rr.reflag([1, 0, 0, 0, 0, 1], np.zeros(12), co, 2, 0, 0, 99)[2], coarse)
    s.setup_host_only(0)
    m = rr.mesh_from_flags(*MESHES["2d"][:3], coarse, 2)
    assert s.sizes() == (m.n_cells, m.n_u, m.n_pnodes) and len(s.hanging_lines()[0]) == len(m.hang_dof)
    # ... and back to the uniform box: no flags, no hanging lines, the lattice tables of distribute_dofs_box
    r, c, coarse, lr = s.set_active_flags(np.zeros(9, np.uint8), [1, 1, 1, 1, 0, 0, 0, 0, 0])
    assert not coarse.any() and not lr and s.n_active_cells() == 6
    s.setup_host_only(0)
    assert s.sizes()[0] == 6 and len(s.hanging_lines()[0]) == 0
    # the band refinement of the FSI drivers still works on it
    assert s.refine_band(0, 0.0, 0.5) == 2
    s.setup_host_only(0)
    assert s.sizes()[0] == 2 * 4 + 4
    s.close()


# ---- transfer table

def _poly(m, kv, seed):
    rng = np.random.default_rng(seed)
    co = rng.standard_normal((m.dim + 1, (kv + 1) ** m.dim))
    cp = rng.standard_normal(2 ** m.dim)

    def mon(p, k):
        return np.array([np.prod([p[d] ** e[d] for d in range(m.dim)]) for e in np.ndindex(*[k + 1] * m.dim)])
    return (lambda p: co[:m.dim] @ mon(p, kv)), (lambda p: cp @ mon(p, 1))


@pytest.mark.parametrize("kv", [2, 1])
def test_transfer_table_reproduces_polynomials(kv):
    host = _host()
    reps, p0, p1, _ = MESHES["2d"]
    chain = [np.zeros(6, np.uint8), np.array([1, 0, 0, 0, 0, 1], np.uint8), np.array([0, 1, 0, 0, 0, 0], np.uint8),  # refine; mixed:
             np.zeros(6, np.uint8)]                                                                                 # two coarsen, one refines; coarsen
    for k in range(len(chain) - 1):
        so, sn = host_solver("2d", kv, chain[k]), host_solver("2d", kv, chain[k + 1])
        mo, mn = rr.mesh_from_flags(reps, p0, p1, chain[k], kv), rr.mesh_from_flags(reps, p0, p1, chain[k + 1], kv)
        table = host.transfer_table(so, sn)
        if chain[k].any():  # the refined old mesh is numbered like HangingMesh; a uniform one follows the Morton curve: use its own tables
            assert np.array_equal(so.cell_tables(kv)[0], mo.cell_unodes)
        else:
            cu, cp, _, vc = so.cell_tables(kv)
            uc, pc = so.node_coords()
            mo = HangingMesh(reps, p0, p1, set(), kv=kv)
            mo.cell_unodes, mo.cell_pnodes, mo.vcoords, mo.unode_coords, mo.pnode_coords = cu, cp, vc, uc, pc
        if chain[k + 1].any():
            assert np.array_equal(sn.cell_tables(kv)[0], mn.cell_unodes)
        else:
            mn.unode_coords, mn.pnode_coords = sn.node_coords()
        fu, fp = _poly(mo, kv, 5 + k)
        xo = rr.interpolate(mo, fu, fp)
        got = rr.apply_table(mo, mn, xo, *table)
        exact = rr.interpolate(mn, fu, fp)
        assert np.abs(got - exact).max() <= 1e-13 * np.abs(exact).max()
        # and on ANY conforming field the table is the nodal transfer of the reference (lowest old cell, same point)
        xr = rr.conforming_random(mo, np.random.default_rng(9)) if chain[k].any() else np.random.default_rng(9).standard_normal(mo.n_dofs)
        assert np.abs(rr.apply_table(mo, mn, xr, *table) - rr.transfer(mo, mn, xr)).max() <= 1e-13 * np.abs(xr).max()
        so.close()
        sn.close()


# ---- C ABI

SYMBOLS = ["ifem_kelly_estimate", "ifem_transfer_solution"]
HOST_SYMBOLS = ["ifemx_face_table", "ifemx_box_face_table", "ifemx_mark_fixed_fraction", "ifemx_set_active_flags", "ifemx_transfer_table",
                "ifemx_refine_mesh"]


def test_the_new_symbols_resolve():
    import openifem_amd.capi as capi
    host = _host()
    L = host._lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ifem_hip.h")).read()
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
        assert f"int {s}(ifem_ctx *" in hdr, s
    for s in HOST_SYMBOLS:
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
    for meth in ("kelly_estimate", "transfer_solution"):
        assert hasattr(capi.Context, meth), meth
    for meth in ("refine_mesh", "face_table", "set_active_flags"):
        assert hasattr(host.FluidSolver, meth), meth
    assert capi.KC_COUNT == 18 and L.ifem_kprof_family_name(17).decode() == "refine"
    for i, s in enumerate(capi.ABI_STRUCTS):  # no struct of the interface changed
        assert L.ifem_abi_sizeof(i) == __import__("ctypes").sizeof(s)
