"""The kernels of csrc/mg.hip that every solve with attached levels runs through -- the CSR transfers of the two V-cycles, the entry / exit
kernels and Chebyshev updates of the cycles, the injection of the evaluation point --, each HOST LAUNCHER called once on host data through the
test aids ifem_test_mg_transfer / ifem_test_mg_vec_kernel and compared with numpy in np.longdouble on the same arrays.  The V-cycles are
preconditioners inside flexible outer solvers: a transfer that drops the tail of a long row, masks the wrong component or loses a partial sum
in its shuffle tree only costs iterations there.  Here every arm is reached on purpose:

  node transfers (mg_csr_mask + mg_csr_apply_nodes_f32: k_mg_mask<2|3>, k_mg_csr_nodes<2|3, G>), in 2D and 3D
      G     4 / 8 / 16 / 32 lanes per row, chosen by launch_csr_nodes from the mean row length (<= 6, <= 12, <= 24, above): _arm() restates the
            rule and test_the_cases_reach_every_arm_and_every_mask_pattern checks that the cases reach all four in both dimensions
      rows  empty, 1, exactly G, G + 1 (a second trip for lane 0 only) and 125 entries (several trips for every lane) in one table
      n     1, 7, 256 / G (exactly one block), 256 / G + 1 (the first row of a second block), 1001 (n G is no multiple of 256) rows
      mask  none / flag_in / flag_out / both; the per-node component patterns run over all 2^dim values; NaN in x under a fully masked column
      real  capi.box_prolongation and its transpose, Q2 and Q1, 3D 4x4x4 <- 2x2x2 and 2D 6x4 <- 3x2, flags from the lattices' boundary nodes
  scalar transfers (mg_csr_apply: k_mg_csr): the same row profiles, the real Q1 tables, and 16384 * 256 + 513 rows of one entry, which sends
      the grid-stride loop under the 16384-block cap of mgrid() into a second trip
  vector kernels (cheb_init, cheb_step, vec_recip, vec_rough, v_cvt_d2f, v_cvt_f2d, v_axpy_f32v, vc_exit, vc_exit_f32, mg_inject_nodes):
      n = 1, 255, 257, 100 003 and 4 194 304 + 513 (capped grid: a second trip of 513 entries); 1.0 planted at n - 1 and at the first index of the last trip
  node-block kernels (vc_entry, vc_entry_f32, cheb_init_block_f32: k_vc_entry<2|3, double|float>, k_cheb_init_block<2|3>) on an assembled
      3x2x2 Q2 box and a 5x3 Q2 box in 2D, with the blocks read back through ifem_uu_block_diag

Every output comes back with TMG_PAD guard entries behind it that started as NaN on the device, as did the output itself: an entry the kernel
left out is NaN, a write past the end is not.  No tolerance is tuned, each is derived from the arithmetic where it is used (u = 2^-53, the unit
roundoff of double; 2^-24 that of float)."""
import functools
import itertools

import numpy as np
import pytest

from boxmesh import BoxMesh

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
UF = 2.0 ** -24
PAD = 8
GS = (4, 8, 16, 32)
N_ROWS_BIG = 1001
N_COLS = 53
CAP = 16384                       # mg.hip::mgrid: at most this many blocks of 256 threads
N_VEC = [1, 255, 257, 100003, CAP * 256 + 513]
FLAG_SETTINGS = ("none", "in", "out", "both")


def _capi():
    from openifem_amd import capi
    return capi


def _smallest(dim):
    capi = _capi()
    m = BoxMesh([1] * dim, (0,) * dim, (1,) * dim, kv=1)
    return capi.Context(dim, 1, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)


@pytest.fixture(scope="module")
def ctxs():
    """a created context is all the transfer and vector aids need; its dim selects the node kernels: the smallest box in 2D and 3D"""
    c = {2: _smallest(2), 3: _smallest(3)}
    yield c
    for v in c.values():
        v.close()


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
def _arm(nnz, n_rows):
    """mg.hip::launch_csr_nodes: lanes per row from the mean row length"""
    mean = nnz / n_rows
    return 4 if mean <= 6 else 8 if mean <= 12 else 16 if mean <= 24 else 32


def _n_rows_of(G):
    return (1, 7, 256 // G, 256 // G + 1, N_ROWS_BIG)


def _row_lengths(G, n_rows):
    """empty, 1, G, G + 1 and -- where the mean that selects G leaves room for it -- 125 entries, the other rows filled up to a mean in the
    middle of the arm's range"""
    if n_rows == 1:
        return np.array([G + 1])
    target = {4: 3, 8: 9, 16: 18, 32: 32}[G] * n_rows
    for base in ([0, 1, G, G + 1, 125], [0, 1, G, G + 1]):
        k = n_rows - len(base)
        need = target - sum(base)
        if k < 0 or need < 0 or (k == 0 and need > 0):
            continue
        fill = [need // k + (1 if i < need % k else 0) for i in range(k)] if k else []
        fill = [max(0, f + (-1, 0, 1)[i % 3]) if i < k - k % 3 else f for i, f in enumerate(fill)]  # some variety around the same mean
        lens = np.array(base + fill)
        if _arm(lens.sum(), n_rows) == G:
            return np.random.default_rng(G * 1000 + n_rows).permutation(lens)
    raise AssertionError((G, n_rows))


@functools.lru_cache(maxsize=None)
def _synthetic(G, n_rows, dim, third=False):
    """(ptr, col, w, x [N_COLS, dim]) of one synthetic table, read-only.  Weights: products of three factors from {1, 3/4, 3/8, -1/8} (exact in
    float; third: every other weight 1/3, which is not); columns random with 0 and N_COLS - 1 present; x standard normal rounded to float; the last
    entry of every row longer than G has weight 1 and meets x = 1, so that a dropped tail moves the row by about 1"""
    rng = np.random.default_rng(7919 * G + 31 * n_rows + dim)
    lens = _row_lengths(G, n_rows)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(ptr[-1])
    col = rng.integers(0, N_COLS, nnz).astype(np.int32)
    col[0], col[-1] = 0, N_COLS - 1
    w = np.array([1.0, 0.75, 0.375, -0.125])[rng.integers(0, 4, (nnz, 3))].prod(axis=1)
    if third:
        w[::2] = 1.0 / 3.0
    x = rng.standard_normal((N_COLS, dim)).astype(np.float32).astype(np.float64)
    tails = ptr[1:][lens > G] - 1
    w[tails] = 1.0
    x[col[tails]] = 1.0
    for a in (ptr, col, w, x):
        a.setflags(write=False)
    return ptr, col, w, x


def _patterns(n, dim, seed):
    """flags [n, dim]: the component patterns of the nodes run over all 2^dim values, in a shuffled order"""
    pat = np.random.default_rng(seed).permutation(n) % (1 << dim)
    return ((pat[:, None] >> np.arange(dim)[None, :]) & 1).astype(np.uint8)


def _pattern_set(flags):
    return set((flags.astype(int) << np.arange(flags.shape[1])).sum(axis=1).tolist())


def _flags(setting, n_rows, dim):
    fi = _patterns(N_COLS, dim, 101 + dim) if setting in ("in", "both") else None
    fo = _patterns(n_rows, dim, 211 + n_rows + dim) if setting in ("out", "both") else None
    return fi, fo


def _reference(ptr, col, w, x, fi, fo):
    """ref = mask_out * (W (mask_in * x)) and mag = mask_out * (|W| (mask_in * |x|)) in longdouble, [n_rows, dim]; a masked x is SELECTED away
    (it may be NaN), not multiplied by zero"""
    n_rows, dim = len(ptr) - 1, x.shape[1]
    xm = x.astype(LD)
    if fi is not None:
        xm = np.where(fi != 0, LD(0), xm)
    rows = np.repeat(np.arange(n_rows), np.diff(ptr))
    t = w.astype(LD)[:, None] * xm[col]
    ref, mag = np.zeros((n_rows, dim), LD), np.zeros((n_rows, dim), LD)
    np.add.at(ref, rows, t)
    np.add.at(mag, rows, np.abs(t))
    if fo is not None:
        ref, mag = np.where(fo != 0, LD(0), ref), np.where(fo != 0, LD(0), mag)
    return ref, mag


def _check_nodes(ctx, tag, ptr, col, w, x, fi, fo, n_cols, w_ref=None):
    """one node transfer against its bound.  The kernel forms the exact product of two widened floats (48 bits) and adds the products in double:
    at most ceil(L / G) additions in a lane and log2 G <= 5 in the shuffle tree pass over any term, each perturbing it by (1 + d), |d| <= u;
    the sum is rounded once to float.  Hence |y - ref| <= 2^-24 |ref| + (L + 6) u mag for a row of L weights (L + 6 >= ceil(L / G) + 5 + 1)."""
    dim = ctx.dim
    n_rows = len(ptr) - 1
    got = ctx.test_mg_transfer(1, n_cols, ptr, col, w, x, fi, fo)
    assert got.shape == (n_rows * dim + PAD,)
    assert np.isnan(got[n_rows * dim:]).all(), f"{tag}: a write behind the last row"
    y = got[:n_rows * dim].reshape(n_rows, dim)
    assert not np.isnan(y).any(), f"{tag}: an entry left unwritten (or a masked NaN got through)"
    ref, mag = _reference(ptr, col, w if w_ref is None else w_ref, x, fi, fo)
    L = np.diff(ptr)[:, None]
    bound = UF * np.abs(ref) + (L + 6) * U * mag
    err = np.abs(y.astype(LD) - ref)
    ratio = float((err / np.maximum(bound, LD(np.finfo(float).tiny))).max()) if n_rows else 0.0
    print(f"{tag} dim={dim} rows={n_rows} nnz={int(ptr[-1])} arm G={_arm(int(ptr[-1]), n_rows) if n_rows else 0}: err/bound {ratio:.3f}")
    assert (err <= bound).all(), f"{tag}: err/bound {ratio}"
    if fo is not None:
        assert (y[fo != 0] == 0.0).all(), f"{tag}: a component masked by flag_out is not exactly zero"
    return y


def _with_nan(x, fi):
    """NaN in x under (some of) the fully masked columns"""
    x = x.copy()
    if fi is not None:
        full = np.nonzero(fi.all(axis=1))[0]
        assert len(full) >= 2
        x[full[::2]] = np.nan
    return x


def test_the_cases_reach_every_arm_and_every_mask_pattern():
    """the coverage the docstring claims, checked on the cases themselves (no launch)"""
    for dim in (2, 3):
        arms, pin, pout = set(), set(), set()
        for G in GS:
            for n_rows in _n_rows_of(G):
                ptr, col, _, _ = _synthetic(G, n_rows, dim)
                lens = np.diff(ptr)
                assert _arm(int(ptr[-1]), n_rows) == G
                arms.add(G)
                assert col.min() == 0 and col.max() == N_COLS - 1
                if n_rows >= 7:
                    assert {0, 1, G, G + 1} <= set(lens.tolist())
                fi, fo = _flags("both", n_rows, dim)
                pin |= _pattern_set(fi)
                pout |= _pattern_set(fo)
                assert np.isnan(_with_nan(np.zeros((N_COLS, dim)), fi)).any()
            assert 125 in np.diff(_synthetic(G, N_ROWS_BIG, dim)[0]) and 125 in np.diff(_synthetic(G, 256 // G, dim)[0])
            assert (N_ROWS_BIG * G) % 256 != 0
        assert arms == set(GS)
        assert pin == set(range(1 << dim)) and pout == set(range(1 << dim))
    n = CAP * 256 + 513
    assert (n + 255) // 256 > CAP and n > CAP * 256  # the capped grid leaves rows for a second grid-stride trip


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("dim", [2, 3])
def test_node_transfer_synthetic_tables(ctxs, dim, G):
    for n_rows in _n_rows_of(G):
        ptr, col, w, x = _synthetic(G, n_rows, dim)
        for setting in FLAG_SETTINGS:
            fi, fo = _flags(setting, n_rows, dim)
            _check_nodes(ctxs[dim], f"synthetic G={G} flags={setting}", ptr, col, w, _with_nan(x, fi), fi, fo, N_COLS)


@pytest.mark.parametrize("dim", [2, 3])
def test_node_transfer_rounds_an_inexact_weight_to_float(ctxs, dim):
    """what the kernel does with a weight single precision cannot hold (ifem_mg_attach rejects such a table; the launcher itself does not):
    it applies float(w).  Same bound, against the reference formed with np.float32(w)"""
    G = 8
    for n_rows in (256 // G + 1, N_ROWS_BIG):
        ptr, col, w, x = _synthetic(G, n_rows, dim, third=True)
        wf = w.astype(np.float32).astype(np.float64)
        assert (wf != w).sum() >= len(w) // 3
        y = _check_nodes(ctxs[dim], "w = 1/3", ptr, col, w, x, None, None, N_COLS, w_ref=wf)
        # ... and the distinction is visible at this precision: the fp64 weights give another float in some entries
        ref64, _ = _reference(ptr, col, w, x, None, None)
        assert (ref64.astype(np.float64).astype(np.float32) != y.astype(np.float32)).any()


def _boundary_flags(reps, deg, dim):
    """Dirichlet flags [n_nodes, dim] of a channel on the Q_deg lattice: every component on the y faces, the first on the inlet face, the z
    component on the z faces -- constrained dofs of both levels are dropped by the transfers"""
    N = [deg * r + 1 for r in reps]
    idx = np.stack(np.unravel_index(np.arange(int(np.prod(N))), N[::-1]), axis=-1)[:, ::-1]
    on = [(idx[:, d] == 0) | (idx[:, d] == N[d] - 1) for d in range(dim)]
    f = np.zeros((len(idx), dim), np.uint8)
    f[on[1], :] = 1
    f[idx[:, 0] == 0, 0] = 1
    if dim == 3:
        f[on[2], 2] = 1
    return f


def _box_pair(reps_f, reps_c, deg):
    capi = _capi()
    nf, nc = int(np.prod([deg * r + 1 for r in reps_f])), int(np.prod([deg * r + 1 for r in reps_c]))
    return capi._csr_pair(capi.box_prolongation(reps_f, reps_c, deg, np.arange(nf), np.arange(nc))), nf, nc


REAL = [((4, 4, 4), (2, 2, 2)), ((6, 4), (3, 2))]


@pytest.mark.parametrize("deg", [2, 1])
@pytest.mark.parametrize("reps_f,reps_c", REAL)
def test_node_transfer_real_tables(ctxs, reps_f, reps_c, deg):
    """P and R = P^T of nested box lattices with identity local-to-global maps, the constrained dofs of both levels dropped"""
    dim = len(reps_f)
    (pp, pc, pw, rp, rc, rw), nf, nc = _box_pair(reps_f, reps_c, deg)
    ff, fc = _boundary_flags(reps_f, deg, dim), _boundary_flags(reps_c, deg, dim)
    assert ff.any() and fc.any() and not ff.all() and not fc.all()
    rng = np.random.default_rng(5 + deg + dim)
    xc = rng.standard_normal((nc, dim)).astype(np.float32).astype(np.float64)
    xf = rng.standard_normal((nf, dim)).astype(np.float32).astype(np.float64)
    for fi_c, fo_f, tag in ((fc, ff, "flags"), (None, None, "no flags")):
        _check_nodes(ctxs[dim], f"P Q{deg} {tag}", pp, pc, pw, xc, fi_c, fo_f, nc)
        _check_nodes(ctxs[dim], f"R Q{deg} {tag}", rp, rc, rw, xf, fo_f, fi_c, nf)


def _check_scalar(ctx, tag, ptr, col, w, x, n_cols):
    """mg_csr_apply: one thread adds the L products of its row in order, fp64 weights.  A term passes through at most L additions and its own
    product: |y - ref| <= (L + 1) u mag (fused or not)"""
    n_rows = len(ptr) - 1
    got = ctx.test_mg_transfer(0, n_cols, ptr, col, w, x)
    assert got.shape == (n_rows + PAD,) and np.isnan(got[n_rows:]).all(), f"{tag}: a write behind the last row"
    y = got[:n_rows]
    assert not np.isnan(y).any(), f"{tag}: a row left unwritten"
    ref, mag = _reference(ptr, col, w, x[:, None], None, None)
    ref, mag = ref[:, 0], mag[:, 0]
    bound = (np.diff(ptr) + 1) * U * mag
    err = np.abs(y.astype(LD) - ref)
    ratio = float((err / np.maximum(bound, LD(np.finfo(float).tiny))).max()) if n_rows else 0.0
    print(f"{tag} rows={n_rows} nnz={int(ptr[-1])}: err/bound {ratio:.3f}")
    assert (err <= bound).all(), f"{tag}: err/bound {ratio}"


@pytest.mark.parametrize("G", GS)
def test_scalar_transfer_synthetic_tables(ctxs, G):
    """the row profiles of the node transfers (rows are serial per thread here), arbitrary double weights, 1/3 among them"""
    for n_rows in _n_rows_of(G):
        ptr, col, _, x = _synthetic(G, n_rows, 2)
        rng = np.random.default_rng(17 + G + n_rows)
        w = rng.standard_normal(len(col))
        w[::5] = 1.0 / 3.0
        xs = rng.standard_normal(N_COLS)
        lens = np.diff(ptr)
        tails = ptr[1:][lens > 1] - 1
        w[tails] = 1.0
        xs[col[tails]] = 1.0
        _check_scalar(ctxs[2], f"scalar synthetic profile {G}", ptr, col, w, xs, N_COLS)


@pytest.mark.parametrize("reps_f,reps_c", REAL)
def test_scalar_transfer_real_pressure_tables(ctxs, reps_f, reps_c):
    (pp, pc, pw, rp, rc, rw), nf, nc = _box_pair(reps_f, reps_c, 1)
    rng = np.random.default_rng(23 + len(reps_f))
    _check_scalar(ctxs[2], "P_p", pp, pc, pw, rng.standard_normal(nc), nc)
    _check_scalar(ctxs[2], "R_p", rp, rc, rw, rng.standard_normal(nf), nf)


def test_scalar_transfer_takes_a_second_grid_stride_trip(ctxs):
    """16384 * 256 + 513 rows of one entry: the grid is capped at 16384 blocks, the last 513 rows belong to the second trip"""
    n_rows, n_cols = CAP * 256 + 513, 1009
    rng = np.random.default_rng(29)
    ptr = np.arange(n_rows + 1, dtype=np.int64)
    col = rng.integers(0, n_cols, n_rows).astype(np.int32)
    col[0], col[-1] = 0, n_cols - 1
    w, x = rng.standard_normal(n_rows), rng.standard_normal(n_cols)
    w[[CAP * 256, n_rows - 1]] = 1.0
    x[col[[CAP * 256, n_rows - 1]]] = 1.0
    _check_scalar(ctxs[2], "capped grid", ptr, col, w, x, n_cols)


def test_malformed_tables_are_refused_before_any_launch(ctxs):
    capi = _capi()
    ptr, col, w, x = (a.copy() for a in _synthetic(8, 7, 2))
    bad = []
    p = ptr.copy(); p[0] = 1; bad.append((p, col))                      # does not start at 0
    p = ptr.copy(); k = int(np.argmax(np.diff(ptr) > 0)); p[k + 1] = p[k] - 1 if p[k] > 0 else -1; bad.append((p, col))  # decreasing
    c = col.copy(); c[3] = N_COLS; bad.append((ptr, c))                 # column out of range
    c = col.copy(); c[3] = -1; bad.append((ptr, c))
    for kind in (0, 1):
        xx = x[:, 0].copy() if kind == 0 else x
        for p, c in bad:
            with pytest.raises(capi.IfemError) as e:
                ctxs[2].test_mg_transfer(kind, N_COLS, p, c, w, xx)
            assert e.value.code == capi.E_BADPARAM
    with pytest.raises(capi.IfemError) as e:  # more columns than the packed entries can name: refused on the sizes alone
        L = ctxs[2].L
        one, y = np.zeros(2, np.int64), np.zeros(PAD)
        ctxs[2]._chk(L.ifem_test_mg_transfer(ctxs[2].h, 1, 1, 1 << 29, capi._ptr(one), None, None, None, None, capi._ptr(y), capi._ptr(y)))
    assert e.value.code == capi.E_BADPARAM and "29" in str(e.value)
    _check_nodes(ctxs[2], "after the refusals", ptr, col, w, x, None, None, N_COLS)  # the context is still usable


# ---- the vector kernels -------------------------------------------------------------------------------------------------------------------
def _tails(n):
    """n - 1 and the first index of the last grid-stride trip of a grid of mgrid(n) blocks of 256 threads"""
    stride = 256 * min(CAP, max(1, (n + 255) // 256))
    return sorted({n - 1, (n - 1) // stride * stride})


def _normal(seed, n, k):
    """k standard-normal vectors with 1.0 planted at the tails"""
    v = np.random.default_rng(seed).standard_normal((k, n))
    v[:, _tails(n)] = 1.0
    return v


def _out(n):
    return np.zeros(n + PAD)


def _split(tag, a, n):
    """the op's n entries; the guard behind them must still be NaN, the entries themselves must all have been written"""
    assert np.isnan(a[n:]).all(), f"{tag}: a write past the end"
    assert not np.isnan(a[:n]).any(), f"{tag}: an entry left unwritten"
    return a[:n]


def _within(tag, got, ref, bound):
    err = np.abs(got.astype(LD) - ref)
    ratio = float((err / np.maximum(bound, LD(np.finfo(float).tiny))).max()) if len(err) else 0.0
    print(f"{tag}: err/bound {ratio:.3f}")
    assert (err <= bound).all(), f"{tag}: err/bound {ratio}"


def _f32(a):
    return a.astype(np.float32)


def _same_bits(tag, got, ref, dtype):
    u = np.uint32 if dtype == np.float32 else np.uint64
    assert np.array_equal(np.ascontiguousarray(got, dtype).view(u), np.ascontiguousarray(ref, dtype).view(u)), tag


@pytest.mark.parametrize("n", N_VEC)
def test_chebyshev_updates(ctxs, n):
    """cheb_init: d = c0 dinv r, two products, 3 u |c0 dinv r| allowed.  cheb_step: x += d, r -= t, d = a d + b dinv r with the NEW r: per output
    8 u times the sum of the magnitudes of its terms (one to four roundings, fused or not); t and dinv come back unchanged"""
    capi, ctx = _capi(), ctxs[2]
    dinv, r, t, x, d = _normal(31 + n % 89, n, 5)
    c0, a, b = 0.7310585786300049, -0.6180339887498949, 1.4142135623730951
    coef = np.array([c0])
    o = _out(n)
    ctx.test_mg_vec_kernel(capi.TMG_CHEB_INIT, n, coef=coef, in0=dinv.copy(), in1=r.copy(), out0=o)
    ref = LD(c0) * dinv.astype(LD) * r.astype(LD)
    _within(f"cheb_init n={n}", _split("cheb_init", o, n), ref, 3 * U * np.abs(ref))
    xo, ro, do = (np.concatenate([v, np.zeros(PAD)]) for v in (x, r, d))
    di, ti = dinv.copy(), t.copy()
    ctx.test_mg_vec_kernel(capi.TMG_CHEB_STEP, n, coef=np.array([a, b]), in0=di, in1=ti, out0=xo, out1=ro, out2=do)
    assert np.array_equal(di, dinv) and np.array_equal(ti, t)
    xl, rl, dl, tl, vl = (v.astype(LD) for v in (x, r, d, t, dinv))
    rn = rl - tl
    _within(f"cheb_step x n={n}", _split("cheb_step x", xo, n), xl + dl, 8 * U * (np.abs(xl) + np.abs(dl)))
    _within(f"cheb_step r n={n}", _split("cheb_step r", ro, n), rn, 8 * U * (np.abs(rl) + np.abs(tl)))
    _within(f"cheb_step d n={n}", _split("cheb_step d", do, n), LD(a) * dl + LD(b) * vl * rn,
            8 * U * (np.abs(LD(a) * dl) + np.abs(LD(b) * vl * rn)))


@pytest.mark.parametrize("n", N_VEC)
def test_vec_recip_and_vec_rough(ctxs, n):
    """vec_recip: one division, within 2^-52 relative of 1 / v; +-0 map to exactly 1.  vec_rough: integer hash and exact conversions, the
    same bits as the hash restated in numpy uint64 arithmetic"""
    capi, ctx = _capi(), ctxs[2]
    v = _normal(37 + n % 89, n, 1)[0]
    zeros = [i for i in (0, 3, n // 2, n - 1) if i < n]
    v[zeros[::2]], v[zeros[1::2]] = 0.0, -0.0
    if n > 8:
        v[[5, 6]] = [1e-300, -3e200]
    o = np.concatenate([v, np.zeros(PAD)])
    ctx.test_mg_vec_kernel(capi.TMG_VEC_RECIP, n, out0=o)
    got = _split("vec_recip", o, n)
    nz = v != 0.0
    assert (got[~nz] == 1.0).all() and not np.signbit(got[~nz]).any()
    q = LD(1) / v[nz].astype(LD)
    _within(f"vec_recip n={n}", got[nz], q, 2.0 ** -52 * np.abs(q))
    for offset in (0, 7000003 * 3):
        o = _out(n)
        ctx.test_mg_vec_kernel(capi.TMG_VEC_ROUGH, n, m=offset, out0=o)
        with np.errstate(over="ignore"):
            h = (np.arange(n, dtype=np.uint64) + np.uint64(offset)) * np.uint64(0x9E3779B97F4A7C15)
            h ^= h >> np.uint64(29)
            h *= np.uint64(0xBF58476D1CE4E5B9)
            h ^= h >> np.uint64(32)
        ref = (h >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) - 0.5
        _same_bits(f"vec_rough n={n} offset={offset}", _split("vec_rough", o, n), ref, np.float64)
        assert n < 100 or (ref.min() < -0.4 and ref.max() > 0.4)


@pytest.mark.parametrize("n", N_VEC)
def test_conversions_and_the_cycle_exit(ctxs, n):
    """v_cvt_d2f, v_cvt_f2d, vc_exit, vc_exit_f32: one IEEE rounding or one float addition per entry, the same bits as numpy float32;
    normal-range values and zeros of both signs.  v_axpy_f32v: y += a x in float, one or two roundings: 2 * 2^-24 (|a x| + |y|)"""
    capi, ctx = _capi(), ctxs[2]
    x, d, y = _normal(41 + n % 89, n, 3)
    x *= np.float64(10.0) ** np.random.default_rng(n).integers(-20, 21, n)
    x[_tails(n)] = 1.0
    zeros = [i for i in (0, 2, n // 2) if i < n - 1]
    x[zeros[::2]], x[zeros[1::2]] = 0.0, -0.0
    d[zeros] = 0.0
    o = _out(n)
    ctx.test_mg_vec_kernel(capi.TMG_CVT_D2F, n, in0=x.copy(), out0=o)
    _same_bits(f"v_cvt_d2f n={n}", _split("d2f", o, n), _f32(x), np.float32)
    xf, df, yf = _f32(x), _f32(d), _f32(y)
    o = _out(n)
    ctx.test_mg_vec_kernel(capi.TMG_CVT_F2D, n, in0=xf.astype(np.float64), out0=o)
    _same_bits(f"v_cvt_f2d n={n}", _split("f2d", o, n), xf.astype(np.float64), np.float64)
    xs = _f32(x / np.maximum(1.0, np.abs(x)) * 3.0)  # of the size of d: a sum that rounds
    xs[_tails(n)] = 1.0
    for op, dt, tag in ((capi.TMG_VC_EXIT, np.float64, "vc_exit"), (capi.TMG_VC_EXIT_F32, np.float32, "vc_exit_f32")):
        o = _out(n)
        ctx.test_mg_vec_kernel(op, n, in0=xs.astype(np.float64), in1=df.astype(np.float64), out0=o)
        _same_bits(f"{tag} n={n}", _split(tag, o, n), (xs + df).astype(dt), dt)
    a = np.float32(-1.6180339887498949)
    o = np.concatenate([yf.astype(np.float64), np.zeros(PAD)])
    ctx.test_mg_vec_kernel(capi.TMG_AXPY_F32V, n, coef=np.array([float(a)]), in0=xs.astype(np.float64), out0=o)
    ax = LD(a) * xs.astype(LD)
    _within(f"v_axpy_f32v n={n}", _split("axpy", o, n), yf.astype(LD) + ax, 2 * UF * (np.abs(ax) + np.abs(yf.astype(LD))))


@pytest.mark.parametrize("n_coarse", [1, 85, 86, 33335, (CAP * 256 + 513 + 2) // 3])
@pytest.mark.parametrize("dim", [2, 3])
def test_injection_of_the_evaluation_point(ctxs, dim, n_coarse):
    """mg_inject_nodes: coarse node i takes the dim components of fine node inj[i]; -1 (another rank's node) gives exactly zero.  The kernel's
    grid-stride loop runs over n_coarse * dim entries: 255 / 258 in 3D, the capped grid at the largest size in 3D"""
    capi, ctx = _capi(), ctxs[dim]
    rng = np.random.default_rng(43 + dim + n_coarse % 89)
    m = 2 * n_coarse + 3
    inj = rng.integers(0, m, n_coarse).astype(np.int32)
    inj[rng.random(n_coarse) < 0.25] = -1
    inj[-1] = m - 1
    if n_coarse > 2:
        inj[0], inj[1] = 0, -1
    fine = rng.standard_normal((m, dim))
    o = np.zeros(n_coarse * dim + PAD)
    ctx.test_mg_vec_kernel(capi.TMG_INJECT_NODES, n_coarse, m=m, idx=inj, in0=np.ascontiguousarray(fine.reshape(-1)), out0=o)
    got = _split("inject", o, n_coarse * dim).reshape(n_coarse, dim)
    ref = np.where((inj >= 0)[:, None], fine[np.maximum(inj, 0)], 0.0)
    assert np.array_equal(got, ref)
    assert (got[inj < 0] == 0.0).all() and not np.signbit(got[inj < 0]).any()
    for bad in (-2, m):
        idx = inj.copy()
        idx[0] = bad
        with pytest.raises(capi.IfemError):
            ctx.test_mg_vec_kernel(capi.TMG_INJECT_NODES, n_coarse, m=m, idx=idx, in0=np.ascontiguousarray(fine.reshape(-1)), out0=o)


# ---- the node-block kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,reps", [(3, (3, 2, 2)), (2, (5, 3))])
def test_cycle_entry_and_block_chebyshev_start(dim, reps):
    """vc_entry / vc_entry_f32: r = float(src) bit for bit, d = c0 B r per node; cheb_init_block_f32: the same d from a float r.  B are the
    inverse node blocks of the assembled level as ifem_uu_block_diag returns them, rounded to float by the library.  The kernel forms exact
    products of widened floats, adds dim of them in double, multiplies by c0 and rounds once to float:
    |d - c0 float(B) float(r)| <= 2^-24 |ref| + 8 u |c0| (|B| |r|)"""
    capi = _capi()
    rng = np.random.default_rng(47 + dim)
    m = BoxMesh(reps, (0,) * dim, (1.0, 0.6, 0.4)[:dim], kv=2)
    m.vcoords = m.vcoords.copy()
    m.vcoords += 0.02 * rng.standard_normal(m.vcoords.shape)
    flag = 3 if dim == 2 else 7
    dofs, vals = m.dirichlet({0: (flag, [0.3, -0.2, 0.1][:dim]), 2: (flag, [0.0] * dim), 3: (1, [0.05])})
    ctx = capi.Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)
    try:
        ctx.set_constraints(0, dofs, None)
        ctx.set_constraints(1, dofs, vals)
        ctx.vec_set(capi.VEC_PRESENT, rng.standard_normal(m.n_dofs))
        ctx.vec_set(capi.VEC_EVAL, rng.standard_normal(m.n_dofs))
        ctx.assemble(capi.make_params(mu=0.7, rho=1.3, gamma=0.2, dt=0.01, g=(0.3, -9.8, 0.5)[:dim], neumann={1: 2.5}), False)
        n = dim * m.n_unodes
        B = ctx.uu_block_diag(0).reshape(m.n_unodes, dim, dim)
        Bf = _f32(B).astype(LD)
        assert np.abs(B).max() > 0 and (np.abs(B - np.transpose(B, (0, 2, 1))).max() > 0)  # full blocks: a transposed product would show
        src = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
        src[[0, n - 1]] = [0.0, 1.0]
        c0 = np.array([0.8414709848078965])
        srcf = _f32(src)

        def check(tag, d_got, r_in):
            rl = r_in.astype(LD).reshape(m.n_unodes, dim)
            ref = (LD(c0[0]) * np.einsum("nij,nj->ni", Bf, rl)).reshape(-1)
            mag = (np.abs(LD(c0[0])) * np.einsum("nij,nj->ni", np.abs(Bf), np.abs(rl))).reshape(-1)
            _within(f"{tag} dim={dim}", d_got, ref, UF * np.abs(ref) + 8 * U * mag)

        for op, x_in, tag in ((capi.TMG_VC_ENTRY, src, "vc_entry"), (capi.TMG_VC_ENTRY_F32, srcf.astype(np.float64), "vc_entry_f32")):
            r, d = _out(n), _out(n)
            ctx.test_mg_vec_kernel(op, n, coef=c0, in0=x_in.copy(), out0=r, out1=d)
            _same_bits(f"{tag} r", _split(tag + " r", r, n), srcf, np.float32)
            check(tag, _split(tag + " d", d, n), srcf)
        d = _out(n)
        ctx.test_mg_vec_kernel(capi.TMG_CHEB_INIT_BLOCK_F32, n, coef=c0, in0=srcf.astype(np.float64), out0=d)
        check("cheb_init_block_f32", _split("cheb_init_block_f32", d, n), srcf)
        with pytest.raises(capi.IfemError):  # the node-block ops take the whole level only
            ctx.test_mg_vec_kernel(capi.TMG_CHEB_INIT_BLOCK_F32, n - dim, coef=c0, in0=srcf.astype(np.float64)[:n - dim].copy(), out0=_out(n - dim))
    finally:
        ctx.close()


def test_node_block_ops_need_an_assembled_context(ctxs):
    capi = _capi()
    n = 2 * 4
    with pytest.raises(capi.IfemError) as e:
        ctxs[2].test_mg_vec_kernel(capi.TMG_VC_ENTRY, n, coef=np.ones(1), in0=np.ones(n), out0=_out(n), out1=_out(n))
    assert e.value.code == capi.E_BADPARAM


# ---- ifem_mg_attach rejects velocity weights that single precision cannot hold ----------------------------------------------------------------
def test_attach_rejects_an_inexact_velocity_weight():
    """the node transfers store pu_w / ru_w as float (mg_csr_mask): ifem_mg_attach refuses a table with a weight such as 1/3 and names the table;
    the pressure tables keep fp64 weights and may hold anything; the generator's own table attaches"""
    import scipy.sparse as sp
    capi = _capi()
    reps_f, reps_c = (4, 2), (2, 1)
    mf, mc = (BoxMesh(r, (0, 0), (1, 1), kv=2) for r in (reps_f, reps_c))
    cf, cc = (capi.Context(2, 2, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes) for m in (mf, mc))
    try:
        Pp = capi.box_prolongation(reps_f, reps_c, 1, np.arange(mf.n_pnodes), np.arange(mc.n_pnodes)).tocsr()
        Pu = capi.box_prolongation(reps_f, reps_c, 2, np.arange(mf.n_unodes), np.arange(mc.n_unodes)).tocsr()
        inj = capi.box_injection(reps_f, reps_c, 2, np.arange(mc.n_unodes), np.arange(mf.n_unodes))
        bad = Pu.copy()
        bad.data[len(bad.data) // 2] = 1.0 / 3.0
        with pytest.raises(capi.IfemError) as e:
            capi.mg_attach(cf.L, cf.h, cc.h, Pp, bad, inj)
        assert e.value.code == capi.E_BADPARAM and ("pu_w" in str(e.value) or "ru_w" in str(e.value))
        assert cf.L.ifem_mg_depth(cf.h) == 0
        Pp3 = Pp.copy()
        Pp3.data[1] = 1.0 / 3.0  # the pressure tables are unrestricted
        capi.mg_attach(cf.L, cf.h, cc.h, sp.csr_matrix(Pp3), Pu, inj)
        assert cf.L.ifem_mg_depth(cf.h) == 1
        capi.mg_attach(cf.L, cf.h, cc.h, Pp, Pu, inj)
        assert cf.L.ifem_mg_depth(cf.h) == 1
    finally:
        cf.close()
        cc.close()
