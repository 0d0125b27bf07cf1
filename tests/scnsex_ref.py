"""Plain numpy / scipy restatement of Fluid::MPI::SCnsEX (reference source/mpi_scnsex.cpp): assemble (:100-387), solve (:389-427),
run_one_step (:429-521) and run (:523-581).  Test infrastructure: the yardstick of tests/test_scnsex_host.py and
tests/test_gpu_scnsex.py, written from the reference text and sharing nothing with the HIP code: plain numpy throughout.  The volume tables (Gauss-Legendre
points, Lagrange shapes, d-linear geometry), boundary_nodes and node_points are those of tests/sa_ref.py, another numpy restatement;
the face quadrature and the elimination rule of distribute_local_to_global(..., false) are its own.

Conventions: a mesh is any object with dim, kv, vcoords [n_cells, 2^dim, dim], cell_unodes [n_cells, (kv+1)^dim], n_unodes,
cell_face_bid [n_cells, 2 dim] (tests/boxmesh.py); local nodes and vertices are lexicographic, x fastest.  Velocity and pressure
live on the SAME nodes (the class demands equal order, :12-14); the block vector is [dim * n | n] with velocity dof dim * node + c.

What is restated, not copied: the velocity matrix of :258-267 couples equal components only, so it is I_dim (x) A_v with the scalar
A_v = mu K + rho / dt M + rho M_sigma; the pressure matrix of :271-277 is A_p = (M / dt + M_sigma) / atm.  Linear systems are solved
directly (splu) where the reference runs CG + BoomerAMG to 1e-6 ||rhs||.

The ONE decision that is not the reference's text: its erase loop over the time limits (:554-566) skips the entry after an erased
one; run() removes every expired entry.
"""
import numpy as np

from sa_ref import boundary_nodes, tables

ATM = 1013250.0
CP_TO_CV = 1.4


def _gauss(n1):
    x, w = np.polynomial.legendre.leggauss(n1)
    return (x + 1) / 2, w / 2


def _lagrange(kv, x):
    """values [len(x), kv + 1] of the 1D Lagrange shapes on equidistant nodes"""
    nodes = np.arange(kv + 1) / kv
    N = np.ones((len(x), kv + 1))
    for a in range(kv + 1):
        for b in range(kv + 1):
            if b != a:
                N[:, a] *= (x - nodes[b]) / (nodes[a] - nodes[b])
    return N


def geometry(m):
    """per cell and quadrature point: JxW [c, q], physical shape gradients g [c, q, a, k]"""
    phi, dphi, dpsi, w = tables(m.dim, m.kv)
    J = np.einsum("cvd,qve->cqde", np.asarray(m.vcoords, float), dpsi)
    Ji = np.linalg.inv(J)
    JxW = np.abs(np.linalg.det(J)) * w[None, :]
    g = np.einsum("qae,cqek->cqak", dphi, Ji)
    return phi, JxW, g


def quadrature_points(m):
    """physical quadrature points [n_cells, n_q, dim] under the d-linear map (what sigma and body-force fields are evaluated at)"""
    dim, n1 = m.dim, m.kv + 1
    xq, _ = _gauss(n1)
    q = np.arange(n1 ** dim)
    xi = np.stack([xq[(q // n1 ** d) % n1] for d in range(dim)], axis=1)  # [q, dim]
    v = np.arange(2 ** dim)
    bits = np.stack([(v >> d) & 1 for d in range(dim)], axis=1)
    wgt = np.prod(np.where(bits[None, :, :] == 1, xi[:, None, :], 1 - xi[:, None, :]), axis=2)  # [q, v]
    return np.einsum("qv,cvd->cqd", wgt, np.asarray(m.vcoords, float))


def cell_matrices(m, sigma=None):
    """dense K_e, M_e, M_sigma,e [n_cells, nu, nu]; sigma [n_cells, n_q] or None (= 0, :181-187)"""
    phi, JxW, g = geometry(m)
    K = np.einsum("cq,cqik,cqjk->cij", JxW, g, g)
    M = np.einsum("cq,qi,qj->cij", JxW, phi, phi)
    sg = np.zeros_like(JxW) if sigma is None else np.asarray(sigma, float).reshape(JxW.shape)
    Ms = np.einsum("cq,qi,qj->cij", JxW * sg, phi, phi)
    return K, M, Ms


def _scatter(m, Ke):
    import scipy.sparse as sp
    cu = np.asarray(m.cell_unodes)
    nu = cu.shape[1]
    rows = np.repeat(cu, nu, axis=1).ravel()
    cols = np.tile(cu, (1, nu)).ravel()
    return sp.coo_matrix((Ke.ravel(), (rows, cols)), shape=(m.n_unodes, m.n_unodes)).tocsr()


def matrices(m, mu, rho, dt, sigma=None):
    """unconstrained A_v, A_p (scipy CSR over the nodes)"""
    K, M, Ms = cell_matrices(m, sigma)
    return _scatter(m, mu * K + rho / dt * M + rho * Ms), _scatter(m, (M / dt + Ms) / ATM)


def neumann_load(m, neumann):
    """- sum over the Neumann faces of int p_bc phi_i n [dim * n] (:312-340); neumann = {boundary id: pressure}"""
    dim, kv = m.dim, m.kv
    n1 = kv + 1
    out = np.zeros((m.n_unodes, dim))
    if not neumann:
        return out.ravel()
    xq, wq = _gauss(n1)
    X = np.asarray(m.vcoords, float)
    cu = np.asarray(m.cell_unodes)
    nq = n1 ** (dim - 1)
    v = np.arange(2 ** dim)
    bits = np.stack([(v >> d) & 1 for d in range(dim)], axis=1)
    for c, f in zip(*np.nonzero(np.asarray(m.cell_face_bid) >= 0)):
        bid = int(np.asarray(m.cell_face_bid)[c, f])
        if bid not in neumann:
            continue
        nd, side = f // 2, f % 2
        others = [d for d in range(dim) if d != nd]
        for q in range(nq):
            xi = np.zeros(dim)
            xi[nd] = float(side)
            wt, r = 1.0, q
            for d in others:
                xi[d] = xq[r % n1]
                wt *= wq[r % n1]
                r //= n1
            L = np.where(bits == 1, xi[None, :], 1 - xi[None, :])  # [v, dim]
            dpsi = np.zeros((2 ** dim, dim))
            for e in range(dim):
                t = np.where(bits[:, e] == 1, 1.0, -1.0)
                for d in range(dim):
                    if d != e:
                        t = t * L[:, d]
                dpsi[:, e] = t
            J = X[c].T @ dpsi  # d x_d / d xi_e
            # n dS = sign * det(J) J^-T e_nd d(xi_others): the outward area vector of the face
            area = (1.0 if side else -1.0) * abs(np.linalg.det(J)) * np.linalg.inv(J)[nd, :]
            N1 = [_lagrange(kv, np.array([xi[d]]))[0] for d in range(dim)]
            N = np.ones(1)
            for d in range(dim):
                N = np.kron(N1[d], N)
            out[cu[c]] -= neumann[bid] * wt * N[:, None] * area[None, :]
    return out.ravel()


def rhs_velocity(m, present, ev, rho, dt, gravity=None, body_force=None, neumann=None, geo=None, load=None):
    """:284-291 + :312-340, before any constraint: [dim * n].  geo / load: geometry(m) / neumann_load(m, neumann) computed before"""
    dim, n = m.dim, m.n_unodes
    phi, JxW, g = geo or geometry(m)
    cu = np.asarray(m.cell_unodes)
    U0 = np.asarray(present, float)[: dim * n].reshape(n, dim)[cu]
    U = np.asarray(ev, float)[: dim * n].reshape(n, dim)[cu]
    P = np.asarray(ev, float)[dim * n:][cu]
    u0 = np.einsum("qa,cak->cqk", phi, U0)
    u = np.einsum("qa,cak->cqk", phi, U)
    G = np.einsum("cak,cqal->cqkl", U, g)       # d u_k / d x_l
    gp = np.einsum("ca,cqak->cqk", P, g)
    f = rho * (u0 / dt - np.einsum("cqkl,cql->cqk", G, u)) - gp
    acc = np.zeros(dim) if gravity is None else np.asarray(gravity, float)[:dim]
    bf = 0.0 if body_force is None else np.asarray(body_force, float).reshape(u.shape)
    f = f + rho * (acc[None, None, :] + bf)
    Fe = np.einsum("cq,qi,cqk->cik", JxW, phi, f)
    out = np.zeros((n, dim))
    np.add.at(out, cu, Fe)
    return out.ravel() + (neumann_load(m, neumann) if load is None else load)


def rhs_pressure(m, present, ev, dt, geo=None):
    """:295-302: [n]"""
    dim, n = m.dim, m.n_unodes
    phi, JxW, g = geo or geometry(m)
    cu = np.asarray(m.cell_unodes)
    U = np.asarray(ev, float)[: dim * n].reshape(n, dim)[cu]
    P = np.asarray(ev, float)[dim * n:][cu]
    P0 = np.asarray(present, float)[dim * n:][cu]
    u = np.einsum("qa,cak->cqk", phi, U)
    div = np.einsum("cak,cqak->cq", U, g)
    p = np.einsum("qa,ca->cq", phi, P)
    p0 = np.einsum("qa,ca->cq", phi, P0)
    gp = np.einsum("ca,cqak->cqk", P, g)
    s = (-CP_TO_CV * (ATM + p) * div + p0 / dt - np.einsum("cqk,cqk->cq", gp, u)) / ATM
    Fe = np.einsum("cq,qi->ci", s * JxW, phi)
    out = np.zeros(n)
    np.add.at(out, cu, Fe)
    return out


class Solver:
    """One SCnsEX problem on a mesh: matrices, constraints (the non-zero set only, mpi_scnsex.h:77-80), the two solves and the
    outer loop of a time step.  is_c / cval are over the dim * n velocity dofs."""

    def __init__(self, m, mu, rho, dt, gravity=None, sigma=None, body_force=None, neumann=None):
        self.m, self.mu, self.rho, self.dt = m, mu, rho, dt
        self.gravity, self.body_force, self.neumann = gravity, body_force, dict(neumann or {})
        self.Av, self.Ap = matrices(m, mu, rho, dt, sigma)
        n = m.n_unodes
        self.is_c = np.zeros(m.dim * n, bool)
        self.cval = np.zeros(m.dim * n)
        self.present = np.zeros((m.dim + 1) * n)
        self._lu = {}
        self._geo = geometry(m)
        self._load = neumann_load(m, self.neumann)

    def set_constraints(self, dofs, vals=None):
        old = self.is_c.copy()
        self.is_c[:] = False
        self.cval[:] = 0.0
        dofs = np.asarray(dofs, np.int64)
        self.is_c[dofs] = True
        self.cval[dofs] = 0.0 if vals is None else np.asarray(vals, float)
        if (old != self.is_c).any():  # the factorisation belongs to the constrained-dof set, not to its values
            self._lu.pop("v", None)

    def velocity_operator(self):
        """block-diagonal over the components, in the interleaved dof order: P_c A_v P_c + (I - P_c) diag(A_v)"""
        import scipy.sparse as sp
        dim, n = self.m.dim, self.m.n_unodes
        blocks = []
        d = self.Av.diagonal()
        for c in range(dim):
            free = sp.diags((~self.is_c[c::dim]).astype(float))
            blocks.append(free @ self.Av @ free + sp.diags(np.where(self.is_c[c::dim], d, 0.0)))
        perm = np.arange(dim * n).reshape(n, dim).T.ravel()  # component-major position -> interleaved dof
        B = sp.block_diag(blocks).tocsr()
        Pm = sp.csr_matrix((np.ones(dim * n), (perm, np.arange(dim * n))), shape=(dim * n, dim * n))
        return (Pm @ B @ Pm.T).tocsr()

    def velocity_rhs(self, ev):
        """the explicit side with the lift: rhs_c <- P_c (rhs_c - A_v g_c); constrained rows 0"""
        dim = self.m.dim
        b = rhs_velocity(self.m, self.present, ev, self.rho, self.dt, self.gravity, self.body_force, self.neumann, self._geo,
                         self._load).reshape(-1, dim)
        g = self.cval.reshape(-1, dim)
        b = b - np.stack([self.Av @ g[:, c] for c in range(dim)], axis=1)
        b[self.is_c.reshape(-1, dim)] = 0.0
        return b.ravel()

    def pressure_rhs(self, ev):
        return rhs_pressure(self.m, self.present, ev, self.dt, self._geo)

    def _solve(self, key, make, b):
        from scipy.sparse.linalg import splu
        if key not in self._lu:
            self._lu[key] = splu(make().tocsc())
        return self._lu[key].solve(b)

    def solve_velocity(self, b):
        x = self._solve("v", self.velocity_operator, b)
        x[self.is_c] = self.cval[self.is_c]  # distribute (:424)
        return x

    def solve_pressure(self, b):
        return self._solve("p", lambda: self.Ap, b)

    def step(self, tol, max_it):
        """run_one_step (:448-503).  Returns the log [[cur, rel], ...], one line per outer iteration."""
        nv = self.m.dim * self.m.n_unodes
        ev = self.present.copy()
        last = np.zeros_like(ev)
        cur = init = rel = np.float64(1.0)
        it, log = 0, []
        while rel > tol and cur > 1e-12:
            if it >= max_it:
                raise RuntimeError("Too many iterations!")
            ev[:nv] = self.solve_velocity(self.velocity_rhs(ev))
            ev[nv:] = self.solve_pressure(self.pressure_rhs(ev))
            cur = np.float64(np.linalg.norm(ev - last))
            if it == 0:
                init = np.float64(np.linalg.norm(ev))
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = cur / init  # 0 / 0 = NaN ends the loop, as in the reference
            log.append([cur, rel])
            it += 1
            last = ev.copy()
        self.present = ev
        return np.array(log)


def make_constraints(m, bcs, fields=None, t=0.0, cache=None):
    """FluidSolver::make_constraints for Dirichlet lines: bcs = {id: (component flag, [values...])}; fields = {id: f(point, component,
    time)} replaces the values of that id.  The first line of a dof stands (ids ascending).  cache: a dict that keeps the boundary
    nodes and node points of the mesh between calls."""
    from sa_ref import node_points
    cache = {} if cache is None else cache
    pts = None
    dofs, vals, seen = [], [], set()
    for bid in sorted(bcs):
        flag, value = bcs[bid]
        comps = [c for c in range(m.dim) if flag & (1 << c)]
        if ("nodes", bid) not in cache:
            cache["nodes", bid] = boundary_nodes(m, bid)
        nodes = cache["nodes", bid]
        if fields and bid in fields and pts is None:
            if "pts" not in cache:
                cache["pts"] = node_points(m)
            pts = cache["pts"]
        for nd in nodes:
            for k, c in enumerate(comps):
                dof = m.dim * int(nd) + c
                if dof in seen:
                    continue
                seen.add(dof)
                dofs.append(dof)
                vals.append(fields[bid](pts[nd], c, t) if fields and bid in fields else value[k])
    return np.array(dofs, np.int32), np.array(vals, float)


def run(m, mu, rho, dt, end_time, bcs, fields=None, limits=None, tol=1e-6, max_it=8, gravity=None, sigma=None, body_force=None,
        neumann=None, log=None):
    """SCnsEX::run (:524-581) from a zero state.  The field time advances by dt once before set-up and again before every step while
    hard-coded fields exist; a limit below the current time removes that boundary's field (every expired entry), after which the
    constraints stay as last made.  Returns the Solver (present = the final state); log (a list) receives the outer counts."""
    S = Solver(m, mu, rho, dt, gravity, sigma, body_force, neumann)
    fields = dict(fields or {})
    limits = dict(limits or {})
    t_field = dt if fields else 0.0
    cache = {}
    S.set_constraints(*make_constraints(m, bcs, fields, t_field, cache))
    t, step = 0.0, 0
    while end_time - t > 1e-12:
        for bid in [b for b, lim in limits.items() if lim < t]:
            fields.pop(bid, None)
            del limits[bid]
        if fields:
            t_field += dt
            S.set_constraints(*make_constraints(m, bcs, fields, t_field, cache))
        step += 1
        t = step * dt
        lg = S.step(tol, max_it)
        if log is not None:
            log.append(len(lg))
    return S


# ---- the acoustic duct of tests/acoustic_duct_wave_mpi_scnsex (reference) ---------------------------------------------------------
DUCT = dict(mu=1.8e-4, rho=1.3e-3, dt=1e-7)
DUCT_BCS = {0: (1, [6.0]), 1: (1, [0.0]), 2: (2, [0.0]), 3: (2, [0.0])}
DUCT_VMAX = 5.9358  # the known answer of the restatement after 1000 steps (tests/test_scnsex_host.py)


def duct_pulse(p, component, t):
    if component == 0 and abs(p[0]) < 1e-10:
        return 6.0 * np.exp(-0.5 * ((t - 0.5e-4) / 0.15e-4) ** 2)
    return 0.0


def duct_mesh(refinements=3):
    from boxmesh import BoxMesh
    return BoxMesh((8 * 2 ** refinements, 2 * 2 ** refinements), (0, 0), (4.0, 1.0), kv=1)


def duct_run(steps, refinements=3, log=None):
    return run(duct_mesh(refinements), end_time=steps * DUCT["dt"], bcs=DUCT_BCS, fields={0: duct_pulse}, limits={0: 1.1e-4}, log=log,
               **DUCT)
