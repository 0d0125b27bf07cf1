"""Plain numpy restatement of the Spalart-Allmaras wall function at a moving FSI wall, written from the reference text:
SpalartAllmaras::update_moving_wall_distance (source/mpi_spalart_allmaras.cpp:17-127), update_boundary_condition (:130-215),
get_shear_velocity (:218-280), the effective distance of assemble (:709-719) and the shear-velocity part of FSI::find_solid_bc
(source/mpi_fsi.cpp:782-844).  Test infrastructure: the yardstick of tests/test_sa_wall_host.py and tests/test_gpu_sa_wall.py; node
points, assembly and the model's Newton loop come from tests/sa_ref.py.  It shares nothing with the HIP code.

A wall is described as the C ABI describes it (ifem_sa_wall): `vertex` [n] indices into the solid's vertex array, `normal` [n, dim], `edges`
[m, 2] POSITIONS in `vertex` (2D), shear velocities indexed by position.  The reference walks its std::map of vertex iterators, i.e. the wall
vertices in ascending solid vertex id; the loops over nodes are vectorised, the loops over edges and vertices are the reference's, in its order.
"""
import numpy as np

import sa_ref

KAPPA = 0.41
DBL_MAX = np.finfo(float).max
B, A1, A2, B1, B2, C1, C2, C3, C4 = 5.03339088, 8.14822158, -6.92870938, 7.46008761, 7.46814579, 2.54967735, 1.33016516, 3.59945911, 3.63975319


def u_plus(yp):
    """the analytical wall velocity profile of :244-250"""
    return (B + C1 * np.log((yp + A1) ** 2 + B1 ** 2) - C2 * np.log((yp + A2) ** 2 + B2 ** 2) - C3 * np.arctan2(B1, yp + A1)
            - C4 * np.arctan2(B2, yp + A2))


def get_shear_velocity(vel, init_guess, nu, dist, trace=None):
    """:218-280.  trace (a list) receives |delta| / |u_tau| of every Newton iteration: the quantity compared with 1e-2"""
    if abs(vel) < 1e-10:
        return 0.0
    if vel * dist / nu < np.sqrt(5.0):
        return vel / np.sqrt(vel * dist / nu)
    init_guess = max(init_guess, 5.0 * nu / dist)
    k3, c3 = KAPPA * KAPPA * KAPPA, 7.1 * 7.1 * 7.1
    ut = init_guess
    for _ in range(30):
        yp = ut * dist / nu
        up = u_plus(yp)
        dup = (k3 * yp * yp * yp) / (c3 + k3 * yp * yp * yp)
        ut_next = ut - (ut * up - vel) / (up + ut * dist / nu * dup)
        if trace is not None:
            trace.append(abs(ut_next - ut) / abs(ut))
        if abs(ut_next - ut) < 1e-2 * abs(ut):
            ut = ut_next
            break
        ut = ut_next
    return float(ut)


def stopping_margin(trace):
    """smallest relative distance of a traced stopping quantity from the tolerance 1e-2 (inf for an empty trace)"""
    return min((abs(t - 1e-2) / 1e-2 for t in trace), default=np.inf)


def moving_wall_distance(x, solid_vertices, vertex, edges, utau, nu):
    """:17-127 at the points x [n, dim].  Returns (d_mov, y_plus, gap): gap [n] = (second-best - best) / best over all candidate
    distances of the node (edges whose region holds the node, all vertices)."""
    x = np.asarray(x, float)
    V = np.asarray(solid_vertices, float)
    vertex = np.asarray(vertex)
    utau = np.asarray(utau, float)
    n, dim = x.shape
    min_dist = np.full(n, DBL_MAX)
    second = np.full(n, DBL_MAX)
    ut_best = np.zeros(n)

    def offer(cur, ut, mask):
        nonlocal min_dist, second, ut_best
        take = mask & (cur < min_dist)
        second = np.where(take, min_dist, np.where(mask, np.minimum(second, cur), second))
        ut_best = np.where(take, ut, ut_best)
        min_dist = np.where(take, cur, min_dist)

    if dim == 2 and edges is not None:
        for p1, p2 in np.asarray(edges).reshape(-1, 2):
            v1, v2 = V[vertex[p1]], V[vertex[p2]]
            v1_product = ((v1 - x) * (v1 - v2)).sum(axis=1)  # dot_product(v1, v0, v2)
            v2_product = ((v2 - x) * (v2 - v1)).sum(axis=1)
            inside = (v1_product > 0) & (v2_product > 0)
            measure = np.sqrt(((v2 - v1) ** 2).sum())
            ratio = v1_product / (measure * measure)
            foot = v1[None, :] + ratio[:, None] * (v2 - v1)[None, :]
            cur = np.sqrt(((x - foot) ** 2).sum(axis=1))
            offer(cur, utau[p1] + (utau[p2] - utau[p1]) * ratio, inside)
    for p in sorted(range(len(vertex)), key=lambda i: (vertex[i], i)):  # the std::map: ascending solid vertex id
        cur = np.sqrt(((x - V[vertex[p]]) ** 2).sum(axis=1))
        offer(cur, np.full(n, utau[p]), np.ones(n, bool))
    y_plus = min_dist * ut_best / nu  # compute_y_plus
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        gap = (second - min_dist) / min_dist
    return min_dist, y_plus, gap


def effective_distance(d_mov, d_fixed):
    """:711-719 with d_mov = DBL_MAX standing for an absent moving distance (value_or(fixed + 1) is never < fixed)"""
    d_mov, d_fixed = np.asarray(d_mov, float), np.asarray(d_fixed, float)
    return np.where(d_mov < d_fixed, d_mov, d_fixed)


# ---- the fluid solution at a point: Utils::GridInterpolator::point_value on the d-linear cells ----------------------------------
def _unit_coordinates(X, p):
    """Newton on the d-linear map of the cell vertices X [2^dim, dim]; None if it does not converge"""
    dim = X.shape[1]
    v = np.arange(2 ** dim)
    bits = np.stack([(v >> d) & 1 for d in range(dim)], axis=1)
    xi = np.full(dim, 0.5)
    for _ in range(30):
        w = np.where(bits == 1, xi[None, :], 1 - xi[None, :])
        N = w.prod(axis=1)
        dN = np.stack([np.where(bits[:, e] == 1, 1.0, -1.0) * np.delete(w, e, axis=1).prod(axis=1) for e in range(dim)], axis=1)
        r = N @ X - p
        J = X.T @ dN
        step = np.linalg.solve(J, r)
        xi = xi - step
        if np.abs(step).max() < 1e-14:
            return xi
    return None


def fluid_velocity_at(m, fluid, p):
    """velocity of the Q_kv field `fluid` at the point p, or None if no cell holds it (distance to the unit cell below 1e-10; the
    smallest distance, then the lowest cell index, as ifem_fsi_fluid_at_points documents)"""
    dim, kv = m.dim, m.kv
    best, best_d, best_xi = -1, np.inf, None
    X = np.asarray(m.vcoords, float)
    lo, hi = X.min(axis=1), X.max(axis=1)
    for c in np.nonzero(((p >= lo - 1e-9) & (p <= hi + 1e-9)).all(axis=1))[0]:
        xi = _unit_coordinates(X[c], p)
        if xi is None:
            continue
        dd = max(0.0, (-xi).max(), (xi - 1).max())
        if dd < best_d:
            best, best_d, best_xi = c, dd, xi
    if best < 0 or not best_d < 1e-10:
        return None
    xi = np.clip(best_xi, 0.0, 1.0)
    nodes = np.arange(kv + 1) / kv
    L = []
    for d in range(dim):
        l = np.ones(kv + 1)
        for a in range(kv + 1):
            for b in range(kv + 1):
                if b != a:
                    l[a] *= (xi[d] - nodes[b]) / (nodes[a] - nodes[b])
        L.append(l)
    a = np.arange((kv + 1) ** dim)
    w = np.ones(len(a))
    for d in range(dim):
        w = w * L[d][(a // (kv + 1) ** d) % (kv + 1)]
    U = np.asarray(fluid, float)[: dim * m.n_unodes].reshape(-1, dim)[np.asarray(m.cell_unodes)[best]]
    return w @ U


def shear_velocities(m, fluid, solid_vertices, vertex, normal, utau_prev, nu, image_distance, sample_at_image_point, traces=None):
    """mpi_fsi.cpp:782-844 for every wall vertex.  traces (a list) receives the stopping trace of every Newton solve."""
    V = np.asarray(solid_vertices, float)
    normal = np.asarray(normal, float)
    out = np.zeros(len(vertex))
    for i, v in enumerate(vertex):
        p = V[v] + image_distance * normal[i] if sample_at_image_point else V[v]
        u = fluid_velocity_at(m, fluid, p)
        if u is None:
            out[i] = 0.0  # not on this process or out of bound
            continue
        normal_velocity = (normal[i] * u).sum() * normal[i]
        tangential = np.sqrt(((u - normal_velocity) ** 2).sum())
        tr = []
        out[i] = get_shear_velocity(tangential, utau_prev[i], nu, image_distance, tr)
        if traces is not None:
            traces.append(tr)
    return out


def update_boundary_condition(m, indicator, cell_order, d_mov, y_plus, nu_present, cons, wall_function_distance, mu, rho, first_step):
    """:130-215.  cons = [(flags0, None), (flags1, values1)] over the nodes (the boundary lines, re-made by the caller); returns the two
    objects after the merge with right_object_wins and the number of lines added."""
    flags0 = np.asarray(cons[0][0]).astype(np.uint8).copy()
    flags1 = np.asarray(cons[1][0]).astype(np.uint8).copy()
    val1 = np.asarray(cons[1][1], float).copy()
    if not first_step:
        flags1, val1 = flags0.copy(), np.zeros(len(flags0))
    n = m.n_unodes
    touched = np.zeros(n, bool)
    inner = {}
    order = np.arange(m.n_cells) if cell_order is None else np.argsort(np.asarray(cell_order), kind="stable")
    cu = np.asarray(m.cell_unodes)
    for c in order:
        if indicator[c] == 1:
            for line in cu[c]:
                if touched[line]:
                    continue
                touched[line] = True
                inner[int(line)] = -nu_present[line]
            continue
        for line in cu[c]:
            d = 2.0 if d_mov[line] == DBL_MAX else d_mov[line]  # value_or(2.0)
            if d < wall_function_distance and y_plus[line] < 200.0:
                if touched[line]:
                    continue
                touched[line] = True
                inner[int(line)] = KAPPA * y_plus[line] * mu / rho - nu_present[line]
    for line, v in inner.items():
        flags0[line] = 1
        flags1[line] = 1
        val1[line] = v
    return (flags0, np.zeros(n)), (flags1, val1), len(inner)


# ---- solids of the tests ------------------------------------------------------------------------------------------------------------
def wall_of(solid, rng=None):
    """the wall description of a tests/solidmesh.py SolidMesh: its boundary vertices in an order that is NOT ascending (reversed, or shuffled by
    rng), vertex normals = mean of the adjacent boundary-face normals (mpi_fsi.cpp:795-800; 2D), edges as positions.  3D: no normals asked for
    here (zeros) and no edges."""
    ids = np.unique(solid.bfaces)
    ids = ids[::-1].copy() if rng is None else rng.permutation(ids)
    pos = {int(v): i for i, v in enumerate(ids)}
    normal = np.zeros((len(ids), solid.dim))
    edges = None
    if solid.dim == 2:
        centre = solid.vertices.mean(axis=0)
        count = np.zeros(len(ids))
        for a, b in solid.bfaces:
            t = solid.vertices[b] - solid.vertices[a]
            nrm = np.array([t[1], -t[0]]) / np.sqrt((t ** 2).sum())
            if ((solid.vertices[a] + solid.vertices[b]) / 2 - centre) @ nrm < 0:
                nrm = -nrm
            for v in (a, b):
                normal[pos[int(v)]] += nrm
                count[pos[int(v)]] += 1
        normal /= count[:, None]
        edges = np.array([[pos[int(a)], pos[int(b)]] for a, b in solid.bfaces], np.int32)
    return ids.astype(np.int32), normal, edges


def polygon_solid(n_sides, centre=(0.3713, 0.2891), radius=0.33, angle=np.sqrt(2.0), seed=5):
    """closed polygon with irregular radii around a non-lattice centre, rotated by an irrational angle, as a ring of Q1 cells between the
    polygon and a copy of it shrunk to 60 %: a SolidMesh whose OUTER boundary is the polygon (inner ring ids first, in a shuffled order, so
    that polygon order and vertex-id order differ)"""
    from solidmesh import SolidMesh
    rng = np.random.default_rng(seed + n_sides)
    th = angle + 2 * np.pi * (np.arange(n_sides) + 0.3 * rng.uniform(-0.5, 0.5, n_sides)) / n_sides
    r = radius * (1 + 0.15 * np.sin(3 * th + 0.7) + 0.05 * rng.uniform(-1, 1, n_sides))
    outer = np.asarray(centre) + np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    inner = np.asarray(centre) + 0.6 * (outer - np.asarray(centre))
    perm = rng.permutation(2 * n_sides)  # solid vertex id of (inner i) = perm[i], of (outer i) = perm[n + i]
    verts = np.zeros((2 * n_sides, 2))
    verts[perm[:n_sides]] = inner
    verts[perm[n_sides:]] = outer
    i = np.arange(n_sides)
    j = (i + 1) % n_sides
    cells = np.stack([perm[i], perm[j], perm[n_sides + i], perm[n_sides + j]], axis=1)
    s = SolidMesh(2, verts, cells)
    outer_ids = set(int(v) for v in perm[n_sides:])
    s.outer_faces = np.array([f for f in s.bfaces if int(f[0]) in outer_ids and int(f[1]) in outer_ids], np.int32)
    return s


def polygon_wall(solid, rng):
    """the wall of polygon_solid: the outer ring only"""
    full = solid.bfaces
    solid.bfaces = solid.outer_faces
    try:
        return wall_of(solid, rng)
    finally:
        solid.bfaces = full


def disc_solid(centre, radius, n=8, angle=0.3):
    """a Q1 mesh of a disc: the lattice [-1, 1]^2 under the elliptical square-to-disc map, rotated"""
    from solidmesh import lattice_solid
    c, s = np.cos(angle), np.sin(angle)

    def mapping(p):
        x, y = p[:, 0], p[:, 1]
        u, v = x * np.sqrt(1 - y * y / 2), y * np.sqrt(1 - x * x / 2)
        return np.asarray(centre) + radius * np.stack([c * u - s * v, s * u + c * v], axis=1)
    return lattice_solid((n, n), (-1, -1), (1, 1), mapping=mapping)
