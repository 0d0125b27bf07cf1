"""numpy restatement of the pieces of FluidSolver::refine_mesh (mpi_fluid_solver.cpp:416-488) on box meshes with one level of
local refinement (tests/hangmesh.py), written from the formulas of DESIGN section 5.8 and independent of the library:

  kelly(m, x)           eta_K = sqrt(h_K / 24 * sum_F int_F sum_c [d u_c / d n]^2 ds), QGauss<dim-1>(kv + 1) on every (sub)face; face
                        neighbours are found GEOMETRICALLY from vcoords, gradients come from dense 1D Lagrange tables
  face_table(m)         those neighbours in the layout of ifem_kelly_estimate, to check the library's table against
  mark / reflag         the fixed-fraction rule on float indicators, the level caps and execute_coarsening_and_refinement
  transfer(mo, mn, x)   the nodal transfer of a block vector [u | p] from mesh mo to mesh mn
  apply_table(...)      a (cell, position) transfer table applied in numpy
"""
import itertools

import numpy as np

from hangmesh import HangingMesh

FACE_BOUNDARY, FACE_EQUAL, FACE_COARSER, FACE_FINER = range(4)


def lagrange(k, t):
    """values and derivatives at t of the k+1 Lagrange polynomials on the nodes j/k of [0, 1]"""
    xs = np.arange(k + 1) / k
    N, dN = np.ones(k + 1), np.zeros(k + 1)
    for i in range(k + 1):
        for j in range(k + 1):
            if j != i:
                N[i] *= (t - xs[j]) / (xs[i] - xs[j])
        for l in range(k + 1):
            if l == i:
                continue
            term = 1.0 / (xs[i] - xs[l])
            for j in range(k + 1):
                if j != i and j != l:
                    term *= (t - xs[j]) / (xs[i] - xs[j])
            dN[i] += term
    return N, dN


def gauss01(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def boxes(m):
    """lower corner and edges of every cell, from the vertices"""
    lo = m.vcoords[:, 0, :]
    return lo, m.vcoords[:, -1, :] - lo


def neighbours(m):
    """{(cell, face): [neighbour cells]} found geometrically: cells whose opposite face lies in the same plane and overlaps this face in
    its interior; a missing key is a boundary face.  face = 2 d + side"""
    lo, h = boxes(m)
    hi = lo + h
    tol = 1e-9 * h.min()
    out = {}
    for c in range(m.n_cells):
        for d in range(m.dim):
            for side in range(2):
                plane = hi[c, d] if side else lo[c, d]
                other = lo[:, d] if side else hi[:, d]
                cand = np.abs(other - plane) < tol
                for t in range(m.dim):
                    if t != d:
                        cand &= (np.minimum(hi[:, t], hi[c, t]) - np.maximum(lo[:, t], lo[c, t])) > tol
                cand[c] = False
                nb = np.nonzero(cand)[0]
                if len(nb):
                    out[(c, 2 * d + side)] = [int(v) for v in nb]
    return out


def _subface(m, lo, h, fine, coarse, d):
    """position of the fine cell's face within the coarse cell's face: bit t = upper half along the t-th tangential direction"""
    s, bit = 0, 0
    for t in range(m.dim):
        if t == d:
            continue
        if lo[fine, t] + 0.5 * h[fine, t] > lo[coarse, t] + 0.5 * h[coarse, t]:
            s |= 1 << bit
        bit += 1
    return s


def face_table(m):
    """int32 [n_cells, 2 dim, 1 + 2^(dim-1)] in the layout of ifem_kelly_estimate, from the geometric neighbours"""
    lo, h = boxes(m)
    ns = 2 ** (m.dim - 1)
    nbs = neighbours(m)
    tab = -np.ones((m.n_cells, 2 * m.dim, 1 + ns), np.int32)
    for c in range(m.n_cells):
        for f in range(2 * m.dim):
            nb = nbs.get((c, f))
            if nb is None:
                tab[c, f, 0] = FACE_BOUNDARY
            elif len(nb) == 1 and abs(h[nb[0], 0] - h[c, 0]) < 1e-9 * h[c, 0]:
                tab[c, f, 0], tab[c, f, 1] = FACE_EQUAL, nb[0]
            elif len(nb) == 1:
                assert h[nb[0], 0] > h[c, 0]
                tab[c, f, 0], tab[c, f, 1] = FACE_COARSER | (_subface(m, lo, h, c, nb[0], f // 2) << 8), nb[0]
            else:
                assert len(nb) == ns
                tab[c, f, 0] = FACE_FINER
                for k in nb:
                    tab[c, f, 1 + _subface(m, lo, h, k, c, f // 2)] = k
    return tab


def _normal_derivative(m, lo, h, cell, pts, d, U):
    """d u_c / d x_d of the Q_kv field with nodal values U [n_unodes, dim] in `cell` at the physical points pts [n, dim]: [n, dim]"""
    kv, dim = m.kv, m.dim
    out = np.zeros((len(pts), dim))
    loc = [tuple(reversed(t)) for t in itertools.product(*[range(kv + 1)] * dim)]  # x fastest
    for i, p in enumerate(pts):
        xi = (p - lo[cell]) / h[cell]
        tabs = [lagrange(kv, xi[e]) for e in range(dim)]
        for a, l in enumerate(loc):
            w = 1.0
            for e in range(dim):
                w *= tabs[e][1][l[e]] if e == d else tabs[e][0][l[e]]
            out[i] += w / h[cell, d] * U[m.cell_unodes[cell, a]]
    return out


def kelly(m, x):
    """eta_K [n_cells] of the velocity block of x"""
    dim, kv = m.dim, m.kv
    U = np.asarray(x, float)[:m.n_u].reshape(-1, dim)
    lo, h = boxes(m)
    hi = lo + h
    g, w = gauss01(kv + 1)
    nbs = neighbours(m)
    eta2 = np.zeros(m.n_cells)
    for (c, f), nb in nbs.items():
        d = f // 2
        tdirs = [t for t in range(dim) if t != d]
        plane = hi[c, d] if f % 2 else lo[c, d]
        for k in nb:  # the part of the face shared with k: the smaller of the two faces
            a = np.maximum(lo[c], lo[k])
            b = np.minimum(hi[c], hi[k])
            pts, wts = [], []
            for q in itertools.product(range(kv + 1), repeat=dim - 1):
                p = np.zeros(dim)
                p[d] = plane
                wt = 1.0
                for t, qi in zip(tdirs, q):
                    p[t] = a[t] + g[qi] * (b[t] - a[t])
                    wt *= w[qi] * (b[t] - a[t])
                pts.append(p)
                wts.append(wt)
            pts, wts = np.array(pts), np.array(wts)
            jump = _normal_derivative(m, lo, h, c, pts, d, U) - _normal_derivative(m, lo, h, k, pts, d, U)
            eta2[c] += wts @ (jump ** 2).sum(axis=1)
    return np.sqrt(np.linalg.norm(h, axis=1) / 24.0 * eta2)


def mark(criteria, top=0.6, bottom=0.4):
    """the marking rule on the criteria rounded to float: total = sum eta (double sums of the float values, in cell order); sort by eta
    descending, ties by ascending index; refine = shortest prefix whose sum reaches top * total, coarsen = shortest suffix whose sum
    reaches bottom * total; a cell in both is refined; total = 0 flags nothing.  Returns (refine, coarsen, sorted order)"""
    c = np.asarray(criteria, np.float32)
    n = len(c)
    refine, coarsen = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    total = 0.0
    for v in c:
        total += float(v)
    order = sorted(range(n), key=lambda i: (-float(c[i]), i))
    if not total > 0:
        return refine, coarsen, order
    s = 0.0
    for i in order:
        refine[i] = 1
        s += float(c[i])
        if s >= top * total:
            break
    s = 0.0
    for i in reversed(order):
        coarsen[i] = 1
        s += float(c[i])
        if s >= bottom * total:
            break
    coarsen[refine == 1] = 0
    return refine, coarsen, order


def reflag(coarse_flags, refine, coarsen, dim, base_level, min_level, max_level):
    """level caps (mpi_fluid_solver.cpp:433-447, plus: children are never refined) on flags per active cell, then the new per-coarse-cell
    flags: a refined cell is un-refined only if all its children carry the coarsen flag.  Returns (refine, coarsen, new coarse flags)"""
    refine, coarsen = np.array(refine, np.uint8), np.array(coarsen, np.uint8)
    new = np.zeros(len(coarse_flags), np.uint8)
    a = 0
    for c, fl in enumerate(coarse_flags):
        n = 2 ** dim if fl else 1
        level = base_level + (1 if fl else 0)
        for k in range(a, a + n):
            if level >= max_level or fl:
                refine[k] = 0
            if level == min_level:
                coarsen[k] = 0
        new[c] = (0 if coarsen[a:a + n].all() else 1) if fl else refine[a]
        a += n
    assert a == len(refine)
    return refine, coarsen, new


def mesh_from_flags(reps, p0, p1, coarse_flags, kv):
    cells = [tuple(reversed(t)) for t in itertools.product(*[range(r) for r in reps[::-1]])]  # x fastest
    return HangingMesh(reps, p0, p1, {ci for ci, fl in zip(cells, coarse_flags) if fl}, kv=kv)


def _locate(mo, lo, h, p):
    """lowest old cell whose closure holds p, and p's reference coordinates there snapped to the 1 / (2 kv) lattice every node of either mesh
    sits on (the physical coordinates carry rounding, the lattice position is exact)"""
    tol = 1e-9 * h.min()
    inside = np.all((p >= lo - tol) & (p <= lo + h + tol), axis=1)
    c = int(np.nonzero(inside)[0][0])
    return c, np.round((p - lo[c]) / h[c] * 2 * mo.kv) / (2 * mo.kv)


def _weights(k, xi):
    dim = len(xi)
    tabs = [lagrange(k, xi[e])[0] for e in range(dim)]
    loc = [tuple(reversed(t)) for t in itertools.product(*[range(k + 1)] * dim)]
    return np.array([np.prod([tabs[e][l[e]] for e in range(dim)]) for l in loc])


def transfer(mo, mn, x):
    """the finite-element function x [u | p] of mesh mo at the nodes of mesh mn"""
    dim = mo.dim
    lo, h = boxes(mo)
    x = np.asarray(x, float)
    U, P = x[:mo.n_u].reshape(-1, dim), x[mo.n_u:]
    out = np.zeros(mn.n_dofs)
    for i, p in enumerate(mn.unode_coords):
        c, xi = _locate(mo, lo, h, p)
        out[dim * i:dim * i + dim] = _weights(mo.kv, xi) @ U[mo.cell_unodes[c]]
    for i, p in enumerate(mn.pnode_coords):
        c, xi = _locate(mo, lo, h, p)
        out[mn.n_u + i] = _weights(1, xi) @ P[mo.cell_pnodes[c]]
    return out


def apply_table(mo, mn, x, u_cell, u_pos, p_cell, p_pos):
    """a transfer table (per new node: old cell, position in units of 1 / (2 deg) packed x | y << 8 | z << 16) applied in numpy"""
    dim = mo.dim
    x = np.asarray(x, float)
    U, P = x[:mo.n_u].reshape(-1, dim), x[mo.n_u:]
    out = np.zeros(mn.n_dofs)
    for i in range(mn.n_unodes):
        xi = np.array([(u_pos[i] >> (8 * e)) & 0xff for e in range(dim)]) / (2.0 * mo.kv)
        out[dim * i:dim * i + dim] = _weights(mo.kv, xi) @ U[mo.cell_unodes[u_cell[i]]]
    for i in range(mn.n_pnodes):
        xi = np.array([(p_pos[i] >> (8 * e)) & 0xff for e in range(dim)]) / 2.0
        out[mn.n_u + i] = _weights(1, xi) @ P[mo.cell_pnodes[p_cell[i]]]
    return out


def conforming_random(m, rng):
    """random values with the hanging entries interpolated from their masters (prolongation applied)"""
    x = rng.standard_normal(m.n_dofs)
    for i, d in enumerate(m.hang_dof):
        s = slice(m.hang_ptr[i], m.hang_ptr[i + 1])
        x[d] = m.hang_weight[s] @ x[m.hang_master[s]]
    return x


def interpolate(m, fu, fp=None):
    """nodal interpolant [u | p] of fu(point) -> dim values and fp(point) -> value"""
    x = np.zeros(m.n_dofs)
    x[:m.n_u] = np.array([fu(p) for p in m.unode_coords]).reshape(-1)
    if fp is not None:
        x[m.n_u:] = [fp(p) for p in m.pnode_coords]
    return x


def random_polynomial(dim, kv, rng):
    """a vector field of degree <= kv per variable (in the conforming Q_kv space of any box mesh): (f(point) -> dim values,
    g(point) -> largest |d f_c / d x_e|)"""
    exps = list(np.ndindex(*[kv + 1] * dim))
    co = rng.standard_normal((dim, len(exps)))

    def f(p):
        return co @ np.array([np.prod([p[d] ** e[d] for d in range(dim)]) for e in exps])

    def g(p):
        best = 0.0
        for k in range(dim):
            dm = np.array([e[k] * p[k] ** max(e[k] - 1, 0) * np.prod([p[d] ** e[d] for d in range(dim) if d != k]) for e in exps])
            best = max(best, np.abs(co @ dm).max())
        return best
    return f, g
