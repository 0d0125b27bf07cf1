"""Plain numpy restatement of Fluid::MPI::SpalartAllmaras (reference source/mpi_spalart_allmaras.cpp): assemble (:620-862),
setup_cell_property (:409-539), run_one_step (:283-345), update_eddy_viscosity (:892-914).  Test infrastructure: the yardstick of
tests/test_sa_host.py and tests/test_gpu_sa.py, written from the reference text and sharing nothing with the HIP code -- its own
Gauss-Legendre points, Lagrange shapes, d-linear geometry and the elimination rule of distribute_local_to_global(..., true).

Conventions: a mesh is any object with dim, kv, vcoords [n_cells, 2^dim, dim], cell_unodes [n_cells, (kv+1)^dim], n_unodes,
cell_face_bid [n_cells, 2 dim] (tests/boxmesh.py, tests/cylmesh.py); local nodes and vertices are lexicographic, x fastest.
The fluid vector is [dim * n_unodes (+ pressure)] with velocity dof dim * node + c.

The ONE decision that is not the reference's text: at :757-770 the reference discards the result of std::min and returns an
uninitialised r whenever |S~| > 1e-8; here (and in csrc/sa.hip) r = min(nu0 / (S~ kappa^2 d^2), 10) there, r = 10 otherwise.
"""
import numpy as np

CV1, CV2, CV3 = 7.1, 0.7, 0.9
CB1, CB2, CT3, CT4, KAPPA = 0.1355, 0.622, 1.2, 0.5, 0.41
CW2, CW3, CN1 = 0.3, 2.0, 16.0
SIGMA = 2.0 / 3.0
CW1 = CB1 / (KAPPA * KAPPA) + (1.0 + CB2) / SIGMA
DBL_MAX = np.finfo(float).max


def _kron_all(mats):
    """tensor product with the FIRST factor fastest (x fastest)"""
    out = np.ones((1, 1))
    for m in mats:
        out = np.kron(m, out)
    return out


def tables(dim, kv):
    """phi [q, a], dphi [q, a, e] (Q_kv on equidistant nodes), dpsi [q, v, e] (Q1 geometry), w [q] at the (kv+1)^dim Gauss points"""
    n1 = kv + 1
    xq, wq = np.polynomial.legendre.leggauss(n1)
    xq, wq = (xq + 1) / 2, wq / 2
    nodes = np.arange(n1) / kv
    N = np.ones((n1, n1))
    D = np.zeros((n1, n1))
    for a in range(n1):
        for q in range(n1):
            for b in range(n1):
                if b != a:
                    N[q, a] *= (xq[q] - nodes[b]) / (nodes[a] - nodes[b])
            for c in range(n1):
                if c == a:
                    continue
                t = 1.0 / (nodes[a] - nodes[c])
                for b in range(n1):
                    if b != a and b != c:
                        t *= (xq[q] - nodes[b]) / (nodes[a] - nodes[b])
                D[q, a] += t
    L = np.stack([1 - xq, xq], axis=1)
    dL = np.stack([-np.ones(n1), np.ones(n1)], axis=1)
    phi = _kron_all([N] * dim)
    dphi = np.stack([_kron_all([D if d == e else N for d in range(dim)]) for e in range(dim)], axis=-1)
    dpsi = np.stack([_kron_all([dL if d == e else L for d in range(dim)]) for e in range(dim)], axis=-1)
    w = _kron_all([wq[:, None]] * dim)[:, 0]
    return phi, dphi, dpsi, w


def node_points(m):
    """support points of the nodes under the d-linear map of vcoords [n_unodes, dim]"""
    dim, kv = m.dim, m.kv
    n1 = kv + 1
    nu = n1 ** dim
    a = np.arange(nu)
    xi = np.stack([(a // n1 ** d) % n1 for d in range(dim)], axis=1) / kv  # [nu, dim]
    v = np.arange(2 ** dim)
    bits = np.stack([(v >> d) & 1 for d in range(dim)], axis=1)            # [nv, dim]
    wgt = np.prod(np.where(bits[None, :, :] == 1, xi[:, None, :], 1 - xi[:, None, :]), axis=2)  # [nu, nv]
    pts = np.einsum("av,cvd->cad", wgt, np.asarray(m.vcoords, float))
    out = np.zeros((m.n_unodes, dim))
    out[np.asarray(m.cell_unodes).ravel()] = pts.reshape(-1, dim)
    return out


def wall_distance(m, wall_pts):
    """setup_cell_property: d(node) = min_i |x_node - w_i|, DBL_MAX without wall points"""
    x = node_points(m)
    wall_pts = np.asarray(wall_pts, float).reshape(-1, m.dim)
    if len(wall_pts) == 0:
        return np.full(m.n_unodes, DBL_MAX)
    d = np.full(m.n_unodes, DBL_MAX)
    for w in wall_pts:
        d = np.minimum(d, np.sqrt(((w[None, :] - x) ** 2).sum(axis=1)))
    return d


def boundary_nodes(m, bid):
    """nodes on the faces with boundary id `bid` (face f = 2 d + side, deal.II order), ascending"""
    n1 = m.kv + 1
    a = np.arange(n1 ** m.dim)
    out = set()
    for c, f in zip(*np.nonzero(np.asarray(m.cell_face_bid) == bid)):
        d, side = f // 2, f % 2
        sel = ((a // n1 ** d) % n1) == (m.kv if side else 0)
        out.update(int(x) for x in np.asarray(m.cell_unodes)[c][sel])
    return np.array(sorted(out), np.int32)


def boundary_vertices(m, bids):
    """the distinct vertices of the faces whose boundary id is in `bids` [n, dim]: the wall points of setup_cell_property"""
    v = np.arange(2 ** m.dim)
    pts = []
    for bid in bids:
        for c, f in zip(*np.nonzero(np.asarray(m.cell_face_bid) == bid)):
            d, side = f // 2, f % 2
            pts.append(np.asarray(m.vcoords)[c][((v >> d) & 1) == side])
    if not pts:
        return np.zeros((0, m.dim))
    return np.unique(np.concatenate(pts).round(14), axis=0)


def cell_integrals(m, fluid, nu_eval, nu_present, wall_d, mu, rho, dt, indicator=None):
    """local matrices K [n_cells, nu, nu], right-hand sides F [n_cells, nu] of :731-842 and the branch counters"""
    dim, kv = m.dim, m.kv
    phi, dphi, dpsi, w = tables(dim, kv)
    X = np.asarray(m.vcoords, float)
    cu = np.asarray(m.cell_unodes)
    J = np.einsum("cvd,qve->cqde", X, dpsi)
    Ji = np.linalg.inv(J)
    JxW = np.abs(np.linalg.det(J)) * w[None, :]
    g = np.einsum("qae,cqek->cqak", dphi, Ji)  # physical gradients
    U = np.asarray(fluid, float)[: dim * m.n_unodes].reshape(-1, dim)[cu]  # [c, a, comp]
    u = np.einsum("qa,cak->cqk", phi, U)
    G = np.einsum("cak,cqal->cqkl", U, g)  # d u_k / d x_l
    if dim == 2:
        S = np.abs(G[..., 1, 0] - G[..., 0, 1])
    else:
        S = np.sqrt((G[..., 2, 1] - G[..., 1, 2]) ** 2 + (G[..., 0, 2] - G[..., 2, 0]) ** 2 + (G[..., 1, 0] - G[..., 0, 1]) ** 2)
    ne, n0e = np.asarray(nu_eval, float)[cu], np.asarray(nu_present, float)[cu]
    nu = np.einsum("qa,ca->cq", phi, ne)
    nu0 = np.einsum("qa,ca->cq", phi, n0e)
    gnu = np.einsum("ca,cqak->cqk", ne, g)
    ind = np.zeros(len(cu), int) if indicator is None else np.asarray(indicator).astype(int)
    lam = np.where(ind == 1, 1.0 / rho, mu / rho)[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d = np.zeros_like(nu)
        for a in range(phi.shape[1]):  # the reference's loop order (:735-738): with d = DBL_MAX partial sums may overflow, never cancel
            d = d + phi[None, :, a] * np.asarray(wall_d, float)[cu][:, a][:, None]
        chi = nu0 / lam
        ft2 = CT3 * np.exp(-CT4 * chi * chi)
        fv1 = chi ** 3 / (chi ** 3 + CV1 ** 3)
        fv2 = 1.0 - chi / (1.0 + chi * fv1)
        k2d2 = KAPPA * KAPPA * d * d
        S_bar = nu0 / k2d2 * fv2
        alt = S_bar < -CV2 * S
        S_tilde = np.where(alt, S + S * (CV2 * CV2 * S - CV3 * S_bar) / ((CV3 - 2 * CV2) * S - S_bar), S + S_bar)
        big = np.abs(S_tilde) > 1e-8
        ratio = nu0 / (S_tilde * k2d2)
        r = np.where(big, np.minimum(ratio, 10.0), 10.0)  # the stated decision
        gg = r + CW2 * (r ** 6 - r)
        fw = gg * ((1 + CW3 ** 6) / (gg ** 6 + CW3 ** 6)) ** (1.0 / 6.0)
        pos = nu0 >= 0
        P = np.where(pos, CB1 * (1 - ft2) * S_tilde, CB1 * (1 - CT3) * S)
        D = np.where(pos, (CW1 * fw - CB1 / (KAPPA * KAPPA) * ft2) / (d * d), -CW1 / (d * d))
        fn = np.where(pos, 1.0, (CN1 + chi ** 3) / (CN1 - chi ** 3))
    counters = {"nu_negative": int((~pos).sum()), "S_bar_branch": int(alt.sum()), "S_tilde_small": int((~big).sum()),
                "r_clipped": int((big & (ratio > 10.0)).sum()), "indicator": int((ind == 1).sum()) * phi.shape[0]}
    diff = (lam + fn * nu0) / SIGMA
    mass = 1.0 / dt - P + 2 * D * nu
    bvec = u - 2 * CB2 / SIGMA * gnu
    K = (np.einsum("cq,qi,qj->cij", mass * JxW, phi, phi) + np.einsum("cq,qi,cqjk,cqk->cij", JxW, phi, g, bvec)
         + np.einsum("cq,cqik,cqjk->cij", diff * JxW, g, g))
    s = ((nu - nu0) / dt + np.einsum("cqk,cqk->cq", u, gnu) - CB2 / SIGMA * np.einsum("cqk,cqk->cq", gnu, gnu) - P * nu + D * nu * nu)
    F = -(np.einsum("cq,qi->ci", s * JxW, phi) + np.einsum("cq,cqik,cqk->ci", diff * JxW, g, gnu))
    return K, F, counters


def assemble(m, fluid, nu_eval, nu_present, wall_d, mu, rho, dt, is_c=None, cval=None, indicator=None):
    """system matrix (scipy CSR [n, n]) and right-hand side with the rule of distribute_local_to_global(K, F, idx, A, b, true):
    a constrained row takes |K_ii| (the mean |diagonal| of the cell if that is zero) on its diagonal and inhomogeneity x that
    value on the right; free rows subtract K_ir c_r for the constrained columns r, which are dropped.  Returns (A, b, counters)."""
    import scipy.sparse as sp
    n = m.n_unodes
    K, F, counters = cell_integrals(m, fluid, nu_eval, nu_present, wall_d, mu, rho, dt, indicator)
    isc = np.zeros(n, bool) if is_c is None else np.asarray(is_c).astype(bool)
    cv = np.zeros(n) if cval is None else np.asarray(cval, float)
    rows, cols, vals = [], [], []
    b = np.zeros(n)
    for c, idx in enumerate(np.asarray(m.cell_unodes)):
        Ke, fe = K[c], F[c]
        avg = np.abs(np.diag(Ke)).mean()
        con = isc[idx]
        for i, gi in enumerate(idx):
            if con[i]:
                kd = abs(Ke[i, i]) if abs(Ke[i, i]) != 0 else avg
                rows.append(gi); cols.append(gi); vals.append(kd)
                b[gi] += cv[gi] * kd
                continue
            b[gi] += fe[i] - (Ke[i, con] * cv[idx[con]]).sum()
            for j, gj in enumerate(idx):
                rows.append(gi); cols.append(gj); vals.append(0.0 if con[j] else Ke[i, j])
    A = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    return A, b, counters


def eddy_viscosity(nu, mu, rho):
    """update_eddy_viscosity: mu_t = chi^3 / (chi^3 + c_v1^3) nu rho"""
    chi = np.asarray(nu, float) / (mu / rho)
    return chi ** 3 / (chi ** 3 + CV1 ** 3) * nu * rho


def run_one_step(m, fluid, nu_present, wall_d, mu, rho, dt, cons, apply_nonzero, tol, max_it, indicator=None):
    """run_one_step with a sparse LU in place of FGMRES.  cons = ((is_c0, None), (is_c1, cval1)): the zero and the nonzero object.
    Returns (new present, log [[abs, rel], ...])."""
    from scipy.sparse.linalg import spsolve
    present = np.asarray(nu_present, float).copy()
    ev = present.copy()
    cur = init = rel = 1.0
    log = []
    it = 0
    while rel > tol and cur > 1e-14:
        if it >= max_it:
            raise RuntimeError("Too many Newton iterations!")
        w = 1 if (apply_nonzero and it == 0) else 0
        isc, cv = cons[w]
        A, b, _ = assemble(m, fluid, ev, present, wall_d, mu, rho, dt, isc, cv if w == 1 else None, indicator)
        x = spsolve(A.tocsc(), b)
        if isc is not None:
            sel = np.asarray(isc).astype(bool)
            x[sel] = (np.asarray(cv, float)[sel] if w == 1 and cv is not None else 0.0)
        cur = np.linalg.norm(b)
        ev = ev + x
        if it == 0:
            init = cur
        rel = cur / init
        log.append([cur, rel])
        it += 1
    return ev, np.array(log)


# ---- inputs shared by the CPU branch-coverage test and the GPU parity test --------------------------------------------------------
PARITY_PARAMS = dict(mu=0.05, rho=1.3, dt=0.01)


def parity_mesh(name):
    from boxmesh import BoxMesh
    if name == "cyl":
        from cylmesh import CylinderMesh
        return CylinderMesh(refinements=1)
    dim, kv, reps = {"2q2": (2, 2, (5, 3)), "2q1": (2, 1, (6, 4)), "3q2": (3, 2, (3, 2, 2)), "3q1": (3, 1, (3, 3, 2))}[name]
    rng = np.random.default_rng(7 + dim + kv)
    m = BoxMesh(reps, (0,) * dim, (1.0, 0.6, 0.4)[:dim], kv=kv)
    m.vcoords = m.vcoords + 0.02 * rng.standard_normal(m.vcoords.shape)  # d-linear distorted cells, as test_assembly_matches_oracle
    return m


def parity_bids(m):
    """two boundary ids of the mesh that carry the constraints and the wall points"""
    ids = sorted(int(b) for b in np.unique(np.asarray(m.cell_face_bid)) if b >= 0)
    return ids[0], ids[2] if len(ids) > 2 else ids[-1]


def parity_inputs(name):
    """(mesh, dict of inputs) of the assembly parity test: a random fluid state with a zero-velocity patch of cells, nu~ of both
    signs with nu~_eval != nu~_present, an indicator on ~40 % of the cells, inhomogeneous constraints on two boundary ids and the
    wall points of those ids -- chosen so that every branch of :741-791 is taken somewhere (tests/test_sa_host.py asserts it)."""
    m = parity_mesh(name)
    rng = np.random.default_rng(1234 + len(name) + m.n_cells)
    dim, n = m.dim, m.n_unodes
    fluid = 0.2 * rng.standard_normal(dim * n + m.n_pnodes)  # moderate vorticity: r = nu0 / (S~ kappa^2 d^2) passes 10 near the walls
    quiet = np.unique(np.asarray(m.cell_unodes)[: max(2, m.n_cells // 4)])  # u = 0 on the first cells: S = 0 there
    fluid[:dim * n].reshape(-1, dim)[quiet] = 0.0
    present = rng.uniform(-0.1, 0.4, n)
    present[quiet[::2]] = 0.2  # chi ~ 5 where S = 0: S_bar < 0 = -c_v2 S, then S~ = 0 exactly
    present[np.asarray(m.cell_unodes)[-1]] = -0.08  # one whole cell below zero: the negative-nu~ branch at every point of it
    ev = present + 0.05 * rng.standard_normal(n)
    indicator = (rng.uniform(size=m.n_cells) < 0.53).astype(np.int32)  # ~40 % of all cells once the quiet quarter is cleared
    indicator[: max(2, m.n_cells // 4)] = 0
    b0, b1 = parity_bids(m)
    nodes = np.unique(np.concatenate([boundary_nodes(m, b0), boundary_nodes(m, b1)])).astype(np.int32)
    inhom = rng.uniform(0.05, 0.3, len(nodes))
    is_c = np.zeros(n, np.uint8)
    is_c[nodes] = 1
    cval = np.zeros(n)
    cval[nodes] = inhom
    wall = boundary_vertices(m, (b0, b1))
    return m, dict(fluid=fluid, present=present, eval=ev, indicator=indicator, nodes=nodes, inhom=inhom, is_c=is_c, cval=cval, wall=wall)


def channel_prm(n_bcs=3, ids="0, 2, 3", types="1, 0, 0", dt=0.01, end_time=0.02, tol=1e-8):
    """.prm text of the 2D channel for Fluid::MPI::SCnsIM (Q1/Q1) with a Spalart Allmaras subsection: walls y-, y+ (type 0), inflow x-
    (type 1), initial coefficient 3; no-slip walls and a uniform inflow velocity for the fluid"""
    return f"""
subsection Simulation
  set Simulation type = Fluid
  set Dimension = 2
  set Global refinements = 0, 0
  set End time = {end_time}
  set Time step size = {dt}
  set Output interval = {dt}
  set Refinement interval = 1000
  set Save interval = 1000
  set Gravity = 0.0, 0.0
end
subsection Fluid finite element system
  set Pressure degree = 1
  set Velocity degree = 1
end
subsection Fluid material properties
  set Dynamic viscosity = 0.01
  set Fluid density = 1
end
subsection Fluid solver control
  set Grad-Div stabilization = 0.1
  set Max Newton iterations = 12
  set Nonlinear system tolerance = {tol}
end
subsection Fluid Dirichlet BCs
  set Use hard-coded boundary values = 0
  set Number of Dirichlet BCs = 3
  set Dirichlet boundary id = 0, 2, 3
  set Dirichlet boundary components = 3, 3, 3
  set Dirichlet boundary values = 1, 0, 0, 0, 0, 0
end
subsection Fluid Neumann BCs
  set Number of Neumann BCs = 0
end
subsection Spalart Allmaras model
  set Number of S-A model BCs = {n_bcs}
  set S-A model boundary id = {ids}
  set S-A model boundary types = {types}
  set Initial condition coefficient = 3
  set Wall function effective distance = 0.0
  set Wall function image distance = 0.0
end
"""
