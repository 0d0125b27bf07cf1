"""The velocity transfers of the A_uu V-cycle from the lattice weight formula (csrc/mg_lattice.hip, ifem_tuning::mg_lattice_u) through the test
aid ifem_test_mg_lattice_transfer (path 0: the CSR kernels on the attached tables, path 1: what a cycle launches), and through ifem_solve.

Levels are box meshes (tests/boxmesh.py) attached with the tables of capi.box_prolongation.  Inputs are float32 random vectors.
Bound A, against the reference: ref = mask_out * (W (mask_in * x)) in numpy longdouble from the reference table, rounded to float32;
|y - ref| <= 2^-23 max|ref|.  Both sides are ONE float rounding of a sum of at most 125 exact products (dyadic weights times floats): the device
forms the sum in double, where it is off by at most 125 * 2^-53 sum|w x|, which moves the rounding by at most one float ulp of the entry, and an
ulp of an entry is at most 2^-23 max|ref|.
Bound B, lattice against CSR on the same pair: the same bound, 2^-23 max|y_csr|, for the same reason; the share of entries that differ at all is
printed (the two paths add the same exact products in different orders).
Every output comes back with TMG_PAD guard entries that started as NaN on the device, as did the output: an entry left out is NaN, a write past
the end is not."""
import ctypes as C
import threading

import numpy as np
import pytest

from boxmesh import BoxMesh

pytestmark = pytest.mark.gpu

LD = np.longdouble
BOUND = 2.0 ** -23
PAD = 8
EXTENT = (2.0, 0.2, 0.2)


def _capi():
    from openifem_amd import capi
    return capi


def _aid(L, h, which, path, x, n_out):
    """(y [n_out + PAD], info [4]) of ifem_test_mg_lattice_transfer on a raw context handle"""
    x = np.ascontiguousarray(x, float)
    y, info = np.zeros(n_out + PAD), np.zeros(4, np.int64)
    rc = L.ifem_test_mg_lattice_transfer(h, which, path, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p))
    assert rc == 0, L.ifem_last_error().decode()
    return y, info


class Pair:
    """two attached box levels; perm: the nodes of both renumbered at random (l2g permutations); alter: one P weight 3/8 -> 1/2 before attach"""

    def __init__(self, reps_f, reps_c, p0=None, p1=None, kv=2, perm=False, seed=1, alter=False, tuning=None, move_vertex=False):
        capi = _capi()
        dim = len(reps_f)
        p0 = (0.0,) * dim if p0 is None else p0
        p1 = EXTENT[:dim] if p1 is None else p1
        self.dim, self.kv = dim, kv
        self.mf, self.mc = BoxMesh(reps_f, p0, p1, kv=kv), BoxMesh(reps_c, p0, p1, kv=kv)
        rng = np.random.default_rng(seed)
        nf, nc = self.mf.n_unodes, self.mc.n_unodes
        # new[g]: the node id of lattice point g; l2g = its inverse
        self.new_f = rng.permutation(nf) if perm else np.arange(nf)
        self.new_c = rng.permutation(nc) if perm else np.arange(nc)
        l2g_f, l2g_c = np.argsort(self.new_f), np.argsort(self.new_c)
        vc = self.mf.vcoords
        if move_vertex:
            h = (np.array(p1) - np.array(p0)) / np.array(reps_f)
            vc = vc.copy()
            hit = np.all(np.abs(vc - (np.array(p0) + h)) < 1e-9 * h, axis=2)
            assert hit.sum() == 2 ** dim
            vc[hit] += 1e-6 * h
        self.cf = capi.Context(dim, kv, vc, self.new_f[self.mf.cell_unodes].astype(np.int32), self.mf.cell_pnodes, self.mf.cell_face_bid, nf, self.mf.n_pnodes)
        self.cc = capi.Context(dim, kv, self.mc.vcoords, self.new_c[self.mc.cell_unodes].astype(np.int32), self.mc.cell_pnodes, self.mc.cell_face_bid, nc, self.mc.n_pnodes)
        if tuning:
            self.cf.set_tuning(**tuning)
            self.cc.set_tuning(**tuning)
        Pp = capi.box_prolongation(reps_f, reps_c, 1, np.arange(self.mf.n_pnodes), np.arange(self.mc.n_pnodes)).tocsr()
        Pu = capi.box_prolongation(reps_f, reps_c, kv, l2g_f, l2g_c).tocsr()
        Pu.sort_indices()
        if alter:
            k = np.nonzero(Pu.data == 0.375)[0]
            Pu.data[k[len(k) // 2]] = 0.5  # exact in single precision: ifem_mg_attach accepts it
        inj = capi.box_injection(reps_f, reps_c, kv, l2g_c, l2g_f)
        capi.mg_attach(self.cf.L, self.cf.h, self.cc.h, Pp, Pu, inj)
        self.P = Pu
        self.R = Pu.T.tocsr()
        self.flags_f = self.flags_c = None

    def constrain(self, dofs_f, dofs_c):
        """lattice-numbered dofs (dim * lattice point + component) of the two levels, or None for a level without a constraint object"""
        dim = self.dim
        for ctx, new, dofs, n, name in ((self.cf, self.new_f, dofs_f, self.mf.n_unodes, "flags_f"), (self.cc, self.new_c, dofs_c, self.mc.n_unodes, "flags_c")):
            if dofs is None:
                continue
            dofs = np.asarray(dofs, np.int64)
            d = (dim * new[dofs // dim] + dofs % dim).astype(np.int32)
            ctx.set_constraints(0, d, None)
            f = np.zeros(n * dim, np.uint8)
            f[d] = 1
            setattr(self, name, f.reshape(n, dim))

    def close(self):
        self.cf.close()
        self.cc.close()


def _reference(W, x, f_in, f_out):
    """float32(mask_out * (W (mask_in * x))) with the sum in longdouble; x [n_cols, dim]"""
    xm = x.astype(LD)
    if f_in is not None:
        xm = np.where(f_in != 0, LD(0), xm)
    rows = np.repeat(np.arange(W.shape[0]), np.diff(W.indptr))
    ref = np.zeros((W.shape[0], x.shape[1]), LD)
    np.add.at(ref, rows, W.data.astype(LD)[:, None] * xm[W.indices])
    if f_out is not None:
        ref = np.where(f_out != 0, LD(0), ref)
    return ref.astype(np.float32).astype(np.float64)


def check(pair, tag, lattice=True, seed=3):
    """both directions by both paths: guards, Bound A for both paths, Bound B between them, and the reported state"""
    dim = pair.dim
    rng = np.random.default_rng(seed)
    nf, nc = pair.mf.n_unodes, pair.mc.n_unodes
    infos = []
    for which, W, n_in, n_out, f_in, f_out, name in ((0, pair.P, nc, nf, pair.flags_c, pair.flags_f, "P"), (1, pair.R, nf, nc, pair.flags_f, pair.flags_c, "R")):
        x = rng.standard_normal((n_in, dim)).astype(np.float32).astype(np.float64)
        y1, info = _aid(pair.cf.L, pair.cf.h, which, 1, x, n_out * dim)
        y0, _ = _aid(pair.cf.L, pair.cf.h, which, 0, x, n_out * dim)
        for y in (y0, y1):
            assert np.isnan(y[n_out * dim:]).all() and np.isfinite(y[:n_out * dim]).all(), f"{tag} {name}: guard entries or an entry left out"
        y0, y1 = y0[:n_out * dim].reshape(n_out, dim), y1[:n_out * dim].reshape(n_out, dim)
        ref = _reference(W, x, f_in, f_out)
        scale = np.abs(ref).max()
        assert scale > 0
        e1, e0, eb = np.abs(y1 - ref).max() / scale, np.abs(y0 - ref).max() / scale, np.abs(y1 - y0).max() / np.abs(y0).max()
        share = np.count_nonzero(y1 != y0) / y0.size
        print(f"{tag} {name}: path 1 against the reference {e1:.3e}, path 0 {e0:.3e}, path 1 against path 0 {eb:.3e} (bound {BOUND:.3e}); "
              f"entries that differ between the paths {share:.2e}; info {info.tolist()}")
        assert e1 <= BOUND and e0 <= BOUND, f"{tag} {name}: bound A"
        assert eb <= BOUND, f"{tag} {name}: bound B"
        if f_out is not None:
            assert not y1[f_out != 0].any()
        if lattice:
            assert info[0] == 1 and info[1] == 0 and info[2] == 0 and info[3] == 1, info
        else:
            assert info[0] == -1 and info[3] == 0, info
            assert np.array_equal(y1, y0)
        infos.append(info.copy())
    return infos


def _case(reps_f, reps_c, tag, **kw):
    pair = Pair(reps_f, reps_c, **kw)
    check(pair, tag + ", no flags")
    pair.constrain(*_channel_dofs(pair))
    check(pair, tag + ", channel flags")
    pair.close()


def _bcs(dim):
    flag = 3 if dim == 2 else 7
    bcs = {0: (flag, [0.0] * dim), 2: (flag, [0.0] * dim), 3: (flag, [0.0] * dim)}
    if dim == 3:
        bcs.update({4: (4, [0.0]), 5: (4, [0.0])})
    return bcs


def _channel_dofs(pair):
    return pair.mf.dirichlet(_bcs(pair.dim))[0], pair.mc.dirichlet(_bcs(pair.dim))[0]


# ---- shapes
SHAPES = [((4, 4, 4), (2, 2, 2)), ((4, 4, 4), (4, 2, 2)), ((4, 4, 4), (4, 4, 2)), ((2, 2, 2), (1, 1, 1)), ((6, 2, 2), (3, 1, 1))]


@pytest.mark.parametrize("reps_f,reps_c", SHAPES)
def test_box_pairs(reps_f, reps_c):
    """full and semi-coarsening (the flagship keeps x), one coarse cell per axis (the clip of the coarse cell index), an odd coarse count"""
    _case(reps_f, reps_c, f"{reps_f} -> {reps_c}")


def test_anisotropic_cells():
    _case((12, 10, 6), (6, 5, 3), "12 x 10 x 6 -> 6 x 5 x 3, h = 0.25 x 0.025 x 0.3", p0=(0.3, -0.1, 0.2), p1=(3.3, 0.15, 2.0))


@pytest.mark.parametrize("reps_f,reps_c", [((6, 4), (3, 2)), ((6, 4), (6, 2))])
def test_two_dimensions(reps_f, reps_c):
    _case(reps_f, reps_c, f"{reps_f} -> {reps_c}", p1=(2.0, 0.4))


# the restriction tile holds 4 coarse points per axis, 16 on the first kept axis and, where no axis is kept, 8 on x (mg_lattice.hip::mgl_tile):
# per axis in turn a coarse lattice of two tiles and one point, 2 coarse cells on the halved others
SEAMS = [((32, 4, 4), (16, 2, 2)),    # all halved: 33 coarse points on x, tiles of 8
         ((4, 8, 4), (2, 4, 2)),      # all halved: 9 coarse points on y, tiles of 4
         ((4, 4, 8), (2, 2, 4)),      # the same on z
         ((16, 4, 4), (16, 2, 2)),    # x kept: 33 points, tiles of 16
         ((4, 16, 4), (2, 16, 2)),    # y kept
         ((4, 4, 16), (2, 2, 16))]    # z kept


@pytest.mark.parametrize("reps_f,reps_c", SEAMS)
def test_restriction_tile_seams(reps_f, reps_c):
    _case(reps_f, reps_c, f"seams {reps_f} -> {reps_c}")


def test_random_renumbering_of_both_levels():
    _case((4, 6, 4), (4, 3, 2), "4 x 6 x 4 -> 4 x 3 x 2, both levels renumbered", perm=True, seed=5)
    _case((6, 4), (3, 2), "6 x 4 -> 3 x 2, both levels renumbered", perm=True, seed=6, p1=(2.0, 0.4))


def test_morton_ordered_mirror_chain():
    """the 16 x 8 x 8 channel through the host mirror: Morton-ordered nodes, the chain and its tables as a solve gets them.  Every pair of the
    chain takes the lattice formula with no row off it; the lattice path against the CSR path on the same pair (bound B)."""
    from openifem_amd import host
    s = host.InsIM(host.channel_prm(3), (16, 8, 8), (0, 0, 0), EXTENT)
    s.setup(0)
    s.channel_state()
    levels = [((16, 8, 8), s.ctx)] + s.mg_levels()
    assert len(levels) >= 2
    rng = np.random.default_rng(8)
    for (rf, hf), (rc, _) in zip(levels[:-1], levels[1:]):
        nf, nc = int(np.prod([2 * r + 1 for r in rf])), int(np.prod([2 * r + 1 for r in rc]))
        for which, n_in, n_out in ((0, nc, nf), (1, nf, nc)):
            x = rng.standard_normal(3 * n_in).astype(np.float32).astype(np.float64)
            y1, info = _aid(s.L, hf, which, 1, x, 3 * n_out)
            y0, _ = _aid(s.L, hf, which, 0, x, 3 * n_out)
            assert info.tolist() == [1, 0, 0, 1], (rf, rc, info)
            assert np.isnan(y1[3 * n_out:]).all() and np.isfinite(y1[:3 * n_out]).all() and np.isfinite(y0[:3 * n_out]).all()
            y0, y1 = y0[:3 * n_out], y1[:3 * n_out]
            eb = np.abs(y1 - y0).max() / np.abs(y0).max()
            print(f"mirror {rf} -> {rc} {'PR'[which]}: path 1 against path 0 {eb:.3e}; entries that differ {np.count_nonzero(y1 != y0) / y0.size:.2e}; zeros {np.count_nonzero(y0 == 0)}")
            assert eb <= BOUND
    s.close()


# ---- flags
def _interior(m, point, comp):
    nd = np.nonzero(np.all(m.unode_lattice == np.array(point), axis=1))[0]
    assert len(nd) == 1
    return np.array([m.dim * int(nd[0]) + comp])


@pytest.mark.parametrize("reps_f,reps_c", [((4, 4, 4), (4, 2, 2)), ((4, 4, 4), (2, 2, 2))])
def test_flag_patterns(reps_f, reps_c):
    pair = Pair(reps_f, reps_c)
    mf, mc = pair.mf, pair.mc
    none = np.zeros(0, np.int64)
    pair.constrain(_interior(mf, (3, 4, 5), 1), none)
    check(pair, f"{reps_f} -> {reps_c}, one interior fine dof")
    pair.constrain(none, _interior(mc, (2, 3, 1), 2))
    check(pair, f"{reps_f} -> {reps_c}, one interior coarse dof")
    face_f = 3 * mf.boundary_unodes(3) + 0  # the x component alone on the y+ face
    face_c = 3 * mc.boundary_unodes(3) + 0
    pair.constrain(face_f, face_c)
    check(pair, f"{reps_f} -> {reps_c}, one component on a face")
    pair.constrain(*_channel_dofs(pair))
    check(pair, f"{reps_f} -> {reps_c}, channel flags")
    pair.constrain(none, none)
    check(pair, f"{reps_f} -> {reps_c}, empty constraint objects")
    pair.close()


# ---- pairs that keep CSR: the state says so and path 1 is the CSR kernels bit for bit
def test_q1_velocity_keeps_csr():
    pair = Pair((4, 4, 4), (2, 2, 2), kv=1)
    pair.constrain(*_channel_dofs(pair))
    infos = check(pair, "Q1 velocity", lattice=False)
    assert all(i[1] == -1 and i[2] == -1 for i in infos)  # not eligible: never compared
    pair.close()


def test_moved_vertex_keeps_csr():
    pair = Pair((4, 4, 4), (2, 2, 2), move_vertex=True)
    assert not pair.cf.mf_uniform()[0]
    pair.constrain(*_channel_dofs(pair))
    check(pair, "one fine vertex moved by 1e-6 h", lattice=False)
    pair.close()


def test_altered_table_keeps_csr_and_the_results_are_the_tables():
    pair = Pair((4, 4, 4), (4, 2, 2), alter=True)
    pair.constrain(*_channel_dofs(pair))
    infos = check(pair, "one weight 3/8 -> 1/2", lattice=False)  # (the reference is the altered table)
    assert all(i[1] >= 1 and i[2] >= 1 for i in infos), infos  # R = P^T carries the same entry
    pair.close()


def test_hanging_node_mesh_keeps_csr():
    """a fine level with hanging-node lines above a box level; the tables are any valid ones (dyadic weights, columns in range)"""
    import scipy.sparse as sp
    from hangmesh import HangingMesh
    capi = _capi()
    mf = HangingMesh((2, 2, 2), (0, 0, 0), (1.0, 0.8, 0.6), {(0, 0, 0)}, kv=2)
    mc = BoxMesh((1, 1, 1), (0, 0, 0), (1.0, 0.8, 0.6), kv=2)
    cf = capi.Context(3, 2, mf.vcoords, mf.cell_unodes, mf.cell_pnodes, mf.cell_face_bid, mf.n_unodes, mf.n_pnodes)
    cc = capi.Context(3, 2, mc.vcoords, mc.cell_unodes, mc.cell_pnodes, mc.cell_face_bid, mc.n_unodes, mc.n_pnodes)
    cf.set_hanging_constraints(mf.hang_dof, mf.hang_ptr, mf.hang_master, mf.hang_weight)
    rng = np.random.default_rng(9)

    def table(n_rows, n_cols):
        cols = rng.integers(0, n_cols, (n_rows, 3))
        cols[:, 1] = (cols[:, 0] + 1) % n_cols
        cols[:, 2] = (cols[:, 0] + 2) % n_cols
        w = np.array([1.0, 0.75, 0.375, -0.125])[rng.integers(0, 4, (n_rows, 3))]
        return sp.csr_matrix((w.ravel(), (np.repeat(np.arange(n_rows), 3), cols.ravel())), shape=(n_rows, n_cols))

    Pu = table(mf.n_unodes, mc.n_unodes)
    capi.mg_attach(cf.L, cf.h, cc.h, table(mf.n_pnodes, mc.n_pnodes), Pu, np.zeros(mc.n_unodes, np.int32))
    for which, n_in, n_out in ((0, mc.n_unodes, mf.n_unodes), (1, mf.n_unodes, mc.n_unodes)):
        x = rng.standard_normal(3 * n_in).astype(np.float32).astype(np.float64)
        y1, info = _aid(cf.L, cf.h, which, 1, x, 3 * n_out)
        y0, _ = _aid(cf.L, cf.h, which, 0, x, 3 * n_out)
        print("hanging-node mesh:", info.tolist())
        assert info[0] == -1 and info[3] == 0
        assert np.array_equal(y1[:3 * n_out], y0[:3 * n_out]) and np.isfinite(y0[:3 * n_out]).all() and np.abs(y0[:3 * n_out]).max() > 0
    cf.close()
    cc.close()


def test_two_virtual_ranks_keep_csr():
    """the 16 x 8 x 8 mirror chain on a 2 x 1 x 1 partition, every level partitioned: each rank's pair keeps CSR"""
    from openifem_amd import capi, host
    L = capi.load()
    world, P, n = 2, (2, 1, 1), (8, 8, 8)
    s1 = host.InsIM(host.channel_prm(3), (16, 8, 8), (0, 0, 0), EXTENT)
    s1.setup(0)
    depth = s1.L.ifem_mg_depth(s1.ctx)
    s1.close()
    worlds = [C.c_void_p(L.ifem_local_world_create(world)) for _ in range(depth + 1)]
    out, errs = [None] * world, []
    n_big = 33 * 17 * 17 * 3  # the whole fine lattice: more than any rank's level holds

    def work(rank):
        try:
            s = host.InsIM(host.channel_prm(3), (16, 8, 8), (0, 0, 0), EXTENT)
            s.set_partition(P, rank, local_world=worlds[0])
            s.set_multigrid(True, 0, worlds[1:])
            s.set_mg_replica_cells(0)
            s.setup(0)
            s.channel_state()
            r = np.random.default_rng(11 + rank)
            res = []
            for which in (0, 1):
                x = r.standard_normal(n_big).astype(np.float32).astype(np.float64)
                y1, info = _aid(L, s.ctx, which, 1, x, n_big)
                y0, _ = _aid(L, s.ctx, which, 0, x, n_big)
                res.append((info.copy(), np.array_equal(y1, y0, equal_nan=True), np.count_nonzero(np.isfinite(y0) & (y0 != 0))))
            out[rank] = res
            s.close()
        except Exception:  # noqa
            import traceback
            errs.append((rank, traceback.format_exc()))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    for w in worlds:
        L.ifem_local_world_destroy(w)
    assert not errs, errs
    for res in out:
        for info, same, n_values in res:
            print("two virtual ranks:", info.tolist(), n_values)
            assert info[0] == -1 and info[1] == -1 and info[3] == 0 and same and n_values > 1000


# ---- the switch
def test_switching_off_after_a_lattice_transfer_is_the_context_that_never_had_it_on():
    reps_f, reps_c = (4, 4, 4), (4, 2, 2)
    a, b = Pair(reps_f, reps_c), Pair(reps_f, reps_c, tuning=dict(mg_lattice_u=0))
    for p in (a, b):
        p.constrain(*_channel_dofs(p))
    rng = np.random.default_rng(12)
    nf, nc = a.mf.n_unodes, a.mc.n_unodes
    for which, n_in, n_out in ((0, nc, nf), (1, nf, nc)):
        x = rng.standard_normal(3 * n_in).astype(np.float32).astype(np.float64)
        a.cf.set_tuning(mg_lattice_u=1)
        on, info = _aid(a.cf.L, a.cf.h, which, 1, x, 3 * n_out)
        assert info.tolist() == [1, 0, 0, 1]
        a.cf.set_tuning(mg_lattice_u=0)
        off, info = _aid(a.cf.L, a.cf.h, which, 1, x, 3 * n_out)
        assert info[0] == 1 and info[3] == 0  # the pair still qualifies, the switch keeps CSR
        never, info_b = _aid(b.cf.L, b.cf.h, which, 1, x, 3 * n_out)
        assert info_b[3] == 0
        assert np.array_equal(off, never, equal_nan=True)
        a.cf.set_tuning(mg_lattice_u=1)
        again, info = _aid(a.cf.L, a.cf.h, which, 1, x, 3 * n_out)
        assert info.tolist() == [1, 0, 0, 1] and np.array_equal(again, on, equal_nan=True)
    a.close()
    b.close()


def _set_tuning(s, **kw):
    from openifem_amd import capi
    tun = capi.Tuning()
    s.L.ifem_default_tuning(C.byref(tun))
    for k, v in kw.items():
        setattr(tun, k, v)
    for c in s.all_ctxs():
        assert s.L.ifem_set_tuning(c, C.byref(tun)) == 0


def test_one_linear_solve_with_the_path_on_off_on_and_the_captured_cycle():
    """16^3 mirror chain, the default solver (IFEM_AINV_MG): the same linear solve with the lattice transfers, with the CSR ones and with the
    lattice ones again.  inner_rel_first = 0 makes the solves of one context the same solve.  Iteration counts identical, updates within 1e-9 of
    the largest entry of each other.  Each setting solves twice: the cycle is captured and replayed; a flip of the switch makes the next cycle a
    new capture, never a replay of the graph of the other path."""
    from openifem_amd import capi, multigpu
    s, _, _ = multigpu.make_channel_solver(16, 0, 1, 0, None, multigrid=True)
    assert s.opts.ainv_kind == capi.AINV_MG
    s.opts.inner_rel_first = 0.0
    s.channel_state()
    s.assemble(False)
    _, n_u, n_p = s.sizes()

    def solve():
        st = s.solve(False)
        x = np.zeros(n_u + n_p)
        assert s.L.ifem_vec_get(s.ctx, capi.VEC_UPDATE, x.ctypes.data_as(C.c_void_p)) == 0
        return x, (st.fgmres_iters, st.inner_iters, st.cg_sm_iters, st.cg_mp_iters)

    runs, graphs = [], [capi.vcycle_graph_stats(s.L, s.ctx)]
    n_f = 33 ** 3
    for knob in (1, 0, 1):
        _set_tuning(s, mg_lattice_u=knob)
        first = solve()
        runs.append(solve())
        assert first[1] == runs[-1][1]
        graphs.append(capi.vcycle_graph_stats(s.L, s.ctx))
        _, info = _aid(s.L, s.ctx, 1, 1, np.ones(3 * n_f), 3 * n_f)
        assert info[0] == 1 and info[1] == 0 and info[2] == 0 and info[3] == knob, info
    scale = np.abs(runs[0][0]).max()
    d_off, d_on = np.abs(runs[1][0] - runs[0][0]).max() / scale, np.abs(runs[2][0] - runs[0][0]).max() / scale
    print(f"(fgmres, inner, cg_sm, cg_mp) iterations: {[r[1] for r in runs]}; updates against the first setting: path off {d_off:.3e}, on again "
          f"{d_on:.3e} of the largest entry; (captures, launches) of the cycle's graph: {graphs}")
    assert runs[0][1] == runs[1][1] == runs[2][1] and runs[0][1][0] > 0 and runs[0][1][1] > 0
    assert d_off <= 1e-9 and d_on <= 1e-9
    for before, after in zip(graphs[:-1], graphs[1:]):
        assert after[0] >= before[0] + 1, graphs   # every setting captured its own graph
        assert after[1] >= before[1] + 2, graphs   # and replayed it
    s.close()
