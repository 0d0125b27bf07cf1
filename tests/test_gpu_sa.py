"""Spalart-Allmaras turbulence model on the device (csrc/sa.hip, ifem_sa_*) against tests/sa_ref.py, the numpy restatement of
reference source/mpi_spalart_allmaras.cpp: wall distance, cell assembly with Dirichlet elimination, FGMRES + ILU(0) solve, the
Newton loop with the eddy viscosity, and the hand-over of that field to SCnsIM::assemble without leaving the device."""
import functools

import numpy as np
import pytest

import sa_ref
from boxmesh import BoxMesh

pytestmark = pytest.mark.gpu


def _capi():
    from openifem_amd import capi
    return capi


def _ctx(m):
    return _capi().Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)


def _sa_params(mu, rho, dt):
    return _capi().SaParams(mu, rho, dt)


# ---- 1. wall distance
def _wall_meshes(name):
    if name == "2q2":
        return BoxMesh((5, 3), (0, 0), (1.0, 0.6), kv=2)
    if name == "3q1":
        return BoxMesh((3, 3, 2), (0, 0, 0), (1.0, 0.6, 0.4), kv=1)
    from cylmesh import CylinderMesh
    return CylinderMesh(refinements=1)


@pytest.mark.parametrize("name", ["2q2", "3q1", "cyl"])
def test_wall_distance(name):
    m = _wall_meshes(name)
    wall = sa_ref.boundary_vertices(m, sa_ref.parity_bids(m))
    assert len(wall) > 4
    ctx = _ctx(m)
    far = ctx.sa_wall_distance()  # before any wall point is given
    assert (far == np.finfo(float).max).all()
    ctx.sa_set_wall_points(wall)
    d = ctx.sa_wall_distance()
    x = np.asarray(m.unode_coords, float)  # the mesh's own node coordinates: brute force, independent of sa_ref.node_points
    want = np.sqrt(((x[:, None, :] - wall[None, :, :]) ** 2).sum(axis=2)).min(axis=1)
    print(f"wall distance {name}: max rel err {np.abs(d - want).max() / want.max():.2e}")
    assert np.abs(d - want).max() <= 1e-14 * want.max()
    assert np.abs(d - sa_ref.wall_distance(m, wall)).max() <= 1e-14 * want.max()
    ctx.sa_set_wall_points(np.zeros((0, m.dim)))
    assert (ctx.sa_wall_distance() == np.finfo(float).max).all()
    ctx.sa_set_wall_points(wall)  # the node points are kept from the first call: the same distances again
    assert (ctx.sa_wall_distance() == d).all()
    ctx.close()


# ---- 2. assembly parity
@functools.lru_cache(maxsize=None)
def _parity_reference(name, use_nonzero):
    m, inp = sa_ref.parity_inputs(name)
    d = sa_ref.wall_distance(m, inp["wall"])
    A, b, _ = sa_ref.assemble(m, inp["fluid"], inp["eval"], inp["present"], d, indicator=inp["indicator"], is_c=inp["is_c"],
                              cval=inp["cval"] if use_nonzero else None, **sa_ref.PARITY_PARAMS)
    return m, inp, A, b


def _parity_context(name, use_nonzero):
    capi = _capi()
    m, inp, A, b = _parity_reference(name, use_nonzero)
    ctx = _ctx(m)
    ctx.vec_set(capi.VEC_PRESENT, inp["fluid"])
    ctx.set_indicator(inp["indicator"])
    ctx.sa_set_wall_points(inp["wall"])
    ctx.sa_set_constraints(0, inp["nodes"], None)
    ctx.sa_set_constraints(1, inp["nodes"], inp["inhom"])
    ctx.sa_vec_set(capi.SA_PRESENT, inp["present"])
    ctx.sa_vec_set(capi.SA_EVAL, inp["eval"])
    P = sa_ref.PARITY_PARAMS
    ctx.sa_assemble(_sa_params(P["mu"], P["rho"], P["dt"]), use_nonzero)
    return ctx, m, inp, A, b


@pytest.mark.parametrize("name", ["2q2", "2q1", "3q2", "3q1", "cyl"])
@pytest.mark.parametrize("use_nonzero", [False, True])
def test_assembly_parity(name, use_nonzero):
    capi = _capi()
    ctx, m, inp, A, b = _parity_context(name, use_nonzero)
    Ag = ctx.sa_export_csr()
    bg = ctx.sa_vec_get(capi.SA_RHS)
    ctx.close()
    eA = abs(Ag - A).max() / abs(A).max()
    eb = np.abs(bg - b).max() / np.abs(b).max()
    print(f"S-A assembly {name} use_nonzero={use_nonzero}: matrix {eA:.2e}, rhs {eb:.2e}")
    assert eA < 1e-11, eA
    assert eb < 1e-11, eb


def test_a_node_listed_twice_keeps_its_last_line():
    """ifem_sa_set_constraints follows ifem_set_constraints: of two lines for one node the LAST stands, whichever thread scatters it.  The
    first node of the "2q1" list is appended a second time with another value; matrix, right-hand side and the distributed update are those
    of the deduplicated constraint, and with the two entries of that node exchanged the other value stands."""
    capi = _capi()
    m, inp = sa_ref.parity_inputs("2q1")
    d = sa_ref.wall_distance(m, inp["wall"])
    P = sa_ref.PARITY_PARAMS
    first = int(inp["nodes"][0])
    nodes = np.append(inp["nodes"], first).astype(np.int32)
    vals = np.append(inp["inhom"], inp["inhom"][0] + 0.5)
    exchanged = vals.copy()
    exchanged[[0, -1]] = vals[[-1, 0]]
    ctx = _ctx(m)
    ctx.vec_set(capi.VEC_PRESENT, inp["fluid"])
    ctx.set_indicator(inp["indicator"])
    ctx.sa_set_wall_points(inp["wall"])
    ctx.sa_vec_set(capi.SA_PRESENT, inp["present"])
    ctx.sa_vec_set(capi.SA_EVAL, inp["eval"])
    for v in (vals, exchanged):
        assert v[0] != v[-1]
        cval = inp["cval"].copy()
        cval[first] = v[-1]
        A, b, _ = sa_ref.assemble(m, inp["fluid"], inp["eval"], inp["present"], d, indicator=inp["indicator"], is_c=inp["is_c"], cval=cval, **P)
        ctx.sa_set_constraints(0, nodes, None)
        ctx.sa_set_constraints(1, nodes, v)
        ctx.sa_assemble(_sa_params(P["mu"], P["rho"], P["dt"]), True)
        Ag = ctx.sa_export_csr()
        bg = ctx.sa_vec_get(capi.SA_RHS)
        ctx.sa_solve(True)
        x = ctx.sa_vec_get(capi.SA_UPDATE)
        eA = abs(Ag - A).max() / abs(A).max()
        eb = np.abs(bg - b).max() / np.abs(b).max()
        print(f"S-A duplicated line, last value {v[-1]:.4f}: matrix {eA:.2e}, rhs {eb:.2e}, update at the node {x[first]:.4f}")
        assert eA < 1e-11, eA
        assert eb < 1e-11, eb
        assert x[first] == v[-1]
        assert (x[inp["nodes"][1:]] == inp["inhom"][1:]).all()
    ctx.close()


# ---- 3. solve
@pytest.mark.parametrize("name", ["2q2", "3q1"])
@pytest.mark.parametrize("use_nonzero", [False, True])
def test_solve(name, use_nonzero):
    from scipy.sparse.linalg import spsolve
    capi = _capi()
    ctx, m, inp, A, b = _parity_context(name, use_nonzero)
    its, res = ctx.sa_solve(use_nonzero)
    x = ctx.sa_vec_get(capi.SA_UPDATE)
    ctx.close()
    lin = np.linalg.norm(A @ x - b) / np.linalg.norm(b)
    xs = spsolve(A.tocsc(), b)
    err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    print(f"S-A solve {name} use_nonzero={use_nonzero}: {its} iterations, residual {lin:.2e} of ||b||, error against LU {err:.2e}")
    assert its > 0
    assert np.linalg.norm(A @ x - b) <= 1.05e-8 * np.linalg.norm(b)
    if use_nonzero:
        assert (x[inp["nodes"]] == inp["inhom"]).all()
    else:
        assert (x[inp["nodes"]] == 0.0).all()
    assert err < 1e-6, err


def test_fluid_assembly_that_reorders_the_pattern_between_model_calls():
    """the first stored fluid assembly of a 3D Q2 context re-orders the blocks of the A_uu rows in place (ifem_tuning::uu_row_order), and the
    model's matrix lives on that pattern: values scattered before are refused by the solve, a new assembly and the ILU(0) follow the new order"""
    from scipy.sparse.linalg import spsolve
    capi = _capi()
    ctx, m, inp, A, b = _parity_context("3q2", True)
    ctx.vec_set(capi.VEC_EVAL, inp["fluid"])
    ctx.sa_solve(True)  # analyses the ILU(0) on the order of the context's creation
    ctx.scns_assemble(capi.make_scns_params(0.05, 1.3, 0.01), False)
    with pytest.raises(capi.IfemError) as e:
        ctx.sa_solve(True)
    assert e.value.code == capi.E_BADPARAM and "assemble again" in str(e.value)
    P = sa_ref.PARITY_PARAMS
    ctx.sa_assemble(_sa_params(P["mu"], P["rho"], P["dt"]), True)
    assert abs(ctx.sa_export_csr() - A).max() / abs(A).max() < 1e-11
    its, _ = ctx.sa_solve(True)
    x = ctx.sa_vec_get(capi.SA_UPDATE)
    ctx.close()
    xs = spsolve(A.tocsc(), b)
    assert its > 0 and np.linalg.norm(x - xs) / np.linalg.norm(xs) < 1e-6


# ---- 4. / 5. Newton step, eddy viscosity, and the hook fed on the device
CH = dict(mu=0.01, rho=1.0, dt=0.01, H=0.5, coef=3.0, tol=1e-8, types={0: 1, 2: 0, 3: 0})  # walls y-, y+ (type 0), inflow x- (type 1)


def _channel():
    m = BoxMesh((6, 4), (0, 0), (1.5, CH["H"]), kv=2)
    n = m.n_unodes
    y = m.unode_coords[:, 1]
    fluid = np.zeros(2 * n + m.n_pnodes)
    fluid[0:2 * n:2] = 4.0 * y * (CH["H"] - y) / CH["H"] ** 2  # parabolic profile
    is_c, cval = np.zeros(n, np.uint8), np.zeros(n)
    for bid in sorted(CH["types"]):  # make_constraints (:367-402): the first line of a node stays
        for nd in sa_ref.boundary_nodes(m, bid):
            if not is_c[nd]:
                is_c[nd] = 1
                cval[nd] = 5.0 * CH["mu"] / CH["rho"] if CH["types"][bid] == 1 else 0.0
    wall = sa_ref.boundary_vertices(m, [b for b, t in CH["types"].items() if t == 0])
    nu0 = np.full(n, CH["coef"] * CH["mu"] / CH["rho"])  # initialize_system (:561-565)
    nu0[is_c == 1] = 0.0
    return m, fluid, is_c, cval, wall, nu0


@functools.lru_cache(maxsize=None)
def _channel_reference():
    m, fluid, is_c, cval, wall, nu0 = _channel()
    d = sa_ref.wall_distance(m, wall)
    cons = ((is_c, None), (is_c, cval))
    out, nu = [], nu0
    for apply_nonzero in (True, False):
        # the residual history with a tolerance nobody reaches decides whether CH["tol"] separates two iterations cleanly
        _, full = sa_ref.run_one_step(m, fluid, nu, d, CH["mu"], CH["rho"], CH["dt"], cons, apply_nonzero, 0.0, 20)
        nu, log = sa_ref.run_one_step(m, fluid, nu, d, CH["mu"], CH["rho"], CH["dt"], cons, apply_nonzero, CH["tol"], 20)
        out.append((nu, log, full))
    return out


def _channel_run():
    """the two Newton steps on the device: (context, mesh, [(iterations, log, nu~)], mu_t as host_out of update_eddy_viscosity)"""
    capi = _capi()
    m, fluid, is_c, cval, wall, nu0 = _channel()
    nodes = np.nonzero(is_c)[0].astype(np.int32)
    ctx = _ctx(m)
    ctx.vec_set(capi.VEC_PRESENT, fluid)
    ctx.vec_set(capi.VEC_EVAL, fluid)
    ctx.sa_set_wall_points(wall)
    ctx.sa_set_constraints(0, nodes, None)
    ctx.sa_set_constraints(1, nodes, cval[nodes])
    ctx.sa_vec_set(capi.SA_PRESENT, nu0)
    P = _sa_params(CH["mu"], CH["rho"], CH["dt"])
    steps = []
    for apply_nonzero in (True, False):
        n_it, log = ctx.sa_newton_step(P, apply_nonzero, tol=CH["tol"], maxit=20)
        steps.append((n_it, log, ctx.sa_vec_get(capi.SA_PRESENT)))
    mu_t = ctx.sa_update_eddy_viscosity(P)
    return ctx, m, steps, mu_t


def test_newton_step_and_eddy_viscosity():
    ref = _channel_reference()
    ctx, m, steps, mu_t = _channel_run()
    ctx.close()
    for (nu_ref, log_ref, full), (n_it, log, nu) in zip(ref, steps):
        k = len(log_ref)
        # the tolerance separates the last two iterations of the reference by a decade on each side
        assert full[k - 1, 1] * 10 <= CH["tol"] and (k == 1 or full[k - 2, 1] >= 10 * CH["tol"]), full
        err = np.abs(nu - nu_ref).max() / np.abs(nu_ref).max()
        print(f"S-A Newton step: {n_it} iterations (reference {k}), rel residuals {log[:, 1]}, nu~ error {err:.2e}")
        assert n_it == k
        assert err < 1e-6, err
    want = sa_ref.eddy_viscosity(steps[-1][2], CH["mu"], CH["rho"])
    assert np.abs(want).max() > 0
    assert np.abs(mu_t - want).max() <= 1e-13 * np.abs(want).max()


def test_eddy_viscosity_reaches_scns_assemble_on_the_device():
    capi = _capi()
    ctx, m, steps, mu_t = _channel_run()
    P = capi.make_scns_params(CH["mu"], CH["rho"], CH["dt"])
    dofs, vals = m.dirichlet({0: (3, [1.0, 0.0]), 2: (3, [0.0, 0.0]), 3: (3, [0.0, 0.0])})

    def scns(c):
        c.set_constraints(0, dofs, None)
        c.set_constraints(1, dofs, vals)
        c.scns_assemble(P, True)
        return c.export_csr(), c.vec_get(capi.VEC_RHS)

    A1, b1 = scns(ctx)  # reads the buffer the model wrote
    ctx.close()
    fluid = _channel()[1]
    other = _ctx(m)
    other.vec_set(capi.VEC_PRESENT, fluid)
    other.vec_set(capi.VEC_EVAL, fluid)
    A0, b0 = scns(other)  # no eddy viscosity
    other.set_eddy_viscosity(mu_t)  # the host round trip the model makes unnecessary
    A2, b2 = scns(other)
    other.close()
    eA, eb = abs(A1 - A2).max() / abs(A2).max(), np.abs(b1 - b2).max() / np.abs(b2).max()
    dA = abs(A1 - A0).max() / abs(A0).max()
    print(f"SCnsIM assembly, device-fed against uploaded eddy viscosity: matrix {eA:.2e}, rhs {eb:.2e}; against none {dA:.2e}")
    assert eA <= 1e-14 and eb <= 1e-14
    assert dA > 1e-6


# ---- 6. refusals
def test_hanging_node_contexts_are_refused():
    from hangmesh import HangingMesh
    capi = _capi()
    m = HangingMesh((3, 2), (0, 0), (1.5, 0.8), {(0, 0), (2, 1)}, kv=2)
    assert len(m.hang_dof) > 0
    ctx = _ctx(m)
    ctx.set_hanging_constraints(m.hang_dof, m.hang_ptr, m.hang_master, m.hang_weight)
    P = _sa_params(0.05, 1.3, 0.01)
    calls = [lambda: ctx.sa_set_wall_points(np.zeros((1, 2))), lambda: ctx.sa_assemble(P, False), lambda: ctx.sa_solve(False),
             lambda: ctx.sa_newton_step(P, True), lambda: ctx.sa_update_eddy_viscosity(P), lambda: ctx.sa_wall_distance()]
    for call in calls:
        with pytest.raises(capi.IfemError) as e:
            call()
        assert e.value.code == capi.E_BADPARAM and "hanging nodes" in str(e.value)
    ctx.close()
    box = BoxMesh((3, 2), (0, 0), (1.5, 0.8), kv=2)
    good = _ctx(box)
    wall = sa_ref.boundary_vertices(box, (2,))
    good.sa_set_wall_points(wall)
    d = good.sa_wall_distance()
    good.close()
    assert np.abs(d - sa_ref.wall_distance(box, wall)).max() <= 1e-14


# ---- 8. host mirror
def test_host_mirror_runs_the_attached_model(tmp_path):
    """Fluid::MPI::SCnsIM + attach_turbulence_model("Spalart-Allmaras"): run() for two time steps calls the model where the reference does
    (mpi_supg_solver.cpp:456-469: model step, fluid step, ...) -- the same calls made by hand through the C ABI on a second context
    built from the mirror's own tables, constraint lines and wall points give the same nu~"""
    import glob
    import os
    from openifem_amd import host
    capi = _capi()
    dt, tol, mu, rho = 0.01, 1e-12, 0.01, 1.0
    s = host.SCnsIM(sa_ref.channel_prm(dt=dt, end_time=2 * dt, tol=tol), (6, 4), (0, 0), (1.5, 0.5))
    with pytest.raises(host.HostError, match="ExcNotImplemented"):
        s.attach_turbulence_model("k-omega")
    s.attach_turbulence_model("Spalart-Allmaras")
    s.set_output_dir(str(tmp_path), True)
    s.run()
    assert s.time()[0] == 2
    nu, eddy = s.turbulence_solution()
    node, val, wall = s.turbulence_setup()
    cu, cp, fb, vc = s.cell_tables(kv=1)
    dofs, vals = s.constraints()
    _, n_u, n_p = s.sizes()
    s.close()
    assert len(wall) == 2 * 7 and len(node) == 2 * 7 + 3 and np.abs(nu).max() > 0
    vtus = sorted(glob.glob(os.path.join(str(tmp_path), "fluid_*.vtu")))
    assert vtus and all('Name="eddy_viscosity"' in open(f).read() for f in vtus)

    ctx = capi.Context(2, 1, vc, cu, cp, fb, n_u // 2, n_p)
    ctx.set_constraints(0, dofs, None)
    ctx.set_constraints(1, dofs, vals)
    ctx.sa_set_constraints(0, node, None)
    ctx.sa_set_constraints(1, node, val)
    ctx.sa_set_wall_points(wall)
    nu0 = np.full(n_u // 2, 3.0 * mu / rho)
    nu0[node] = 0.0
    ctx.sa_vec_set(capi.SA_PRESENT, nu0)
    Ps, Pf = _sa_params(mu, rho, dt), capi.make_scns_params(mu, rho, dt)
    for apply_nonzero in (True, False):
        ctx.sa_newton_step(Ps, apply_nonzero, tol=tol, maxit=12)
        ctx.scns_newton_step(Pf, apply_nonzero, tol=tol, maxit=12)
    want = ctx.sa_vec_get(capi.SA_PRESENT)
    want_eddy = ctx.sa_update_eddy_viscosity(Ps)
    ctx.close()
    err = np.abs(nu - want).max() / np.abs(want).max()
    print(f"host mirror against the C-ABI sequence: nu~ {err:.2e}")
    assert err <= 1e-12
    assert np.abs(eddy - want_eddy).max() <= 1e-12 * np.abs(want_eddy).max()


# ---- 7. two virtual ranks
def _rank_case():
    """3D Q1 4x3x2 box: random (moderate) fluid state and positive nu~, walls z-, z+ with inhomogeneous lines, indicator on some cells"""
    m = BoxMesh((4, 3, 2), (0, 0, 0), (1.0, 0.6, 0.4), kv=1)
    rng = np.random.default_rng(2024)
    n = m.n_unodes
    fluid = 0.2 * rng.standard_normal(3 * n + m.n_pnodes)
    present = rng.uniform(0.02, 0.12, n)
    ev = present + 0.01 * rng.standard_normal(n)
    indicator = (rng.uniform(size=m.n_cells) < 0.4).astype(np.int32)
    nodes = np.unique(np.concatenate([sa_ref.boundary_nodes(m, 4), sa_ref.boundary_nodes(m, 5)])).astype(np.int32)
    inhom = rng.uniform(0.01, 0.05, len(nodes))
    wall = sa_ref.boundary_vertices(m, (4, 5))
    return m, fluid, present, ev, indicator, nodes, inhom, wall


def test_two_virtual_ranks_match_the_single_context():
    import partmesh
    from boxmesh import block_partition
    capi = _capi()
    m, fluid, present, ev, indicator, nodes, inhom, wall = _rank_case()
    P = sa_ref.PARITY_PARAMS
    Ps = _sa_params(P["mu"], P["rho"], P["dt"])

    def work(rank, part, ctx):
        ctx.vec_set(capi.VEC_PRESENT, fluid[part.ext_gdof])
        ctx.set_indicator(indicator[part.cells])
        ctx.sa_set_wall_points(wall)  # every rank passes all wall points
        loc = part.g2l_u[nodes]
        keep = loc >= 0
        ctx.sa_set_constraints(0, loc[keep].astype(np.int32), None)
        ctx.sa_set_constraints(1, loc[keep].astype(np.int32), inhom[keep])
        ctx.sa_vec_set(capi.SA_PRESENT, present[part.l2g_u])
        ctx.sa_vec_set(capi.SA_EVAL, ev[part.l2g_u])
        no = part.n_unodes_owned
        out = {"d": ctx.sa_wall_distance()}
        ctx.sa_assemble(Ps, True)
        out["A"] = ctx.sa_export_csr()
        out["b"] = ctx.sa_vec_get(capi.SA_RHS)[:no]
        out["its"], out["log"] = ctx.sa_newton_step(Ps, True, tol=1e-8, maxit=20)
        out["nu"] = ctx.sa_vec_get(capi.SA_PRESENT)
        out["eddy"] = ctx.sa_update_eddy_viscosity(Ps)
        return out

    def gather(parts, res):
        n = m.n_unodes
        A, b, nu, d = np.full((n, n), np.nan), np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
        for part, r in zip(parts, res):
            no = part.n_unodes_owned
            rows = part.l2g_u[:no]
            A[rows] = 0.0
            A[np.ix_(rows, part.l2g_u)] = r["A"].toarray()
            b[rows], nu[rows] = r["b"], r["nu"][:no]
            assert np.abs(r["d"] - sa_ref.wall_distance(m, wall)[part.l2g_u]).max() <= 1e-14  # ghosts included
            # ghost entries of nu~ and mu_t carry the owners' values after the step
            assert np.isfinite(r["nu"]).all() and np.isfinite(r["eddy"]).all()
            d[rows] = r["d"][:no]
        assert not np.isnan(A).any() and not np.isnan(b).any()
        return A, b, nu, d

    one = partmesh.partition_mesh(m, np.zeros(m.n_cells, np.int32), 1)
    A1, b1, nu1, d1 = gather(one, partmesh.run_virtual_ranks(capi, one, work, timeout=60))
    cell_rank, used = block_partition(m.reps, 2)
    assert used == 2
    two = partmesh.partition_mesh(m, cell_rank, 2)
    res = partmesh.run_virtual_ranks(capi, two, work, timeout=60)
    A2, b2, nu2, d2 = gather(two, res)
    assert len({r["its"] for r in res}) == 1, "ranks disagree on the Newton iteration count"
    for part, r in zip(two, res):  # ghosts of the result equal the owners' entries
        assert np.abs(r["nu"] - nu2[part.l2g_u]).max() == 0.0
    eA, eb, en = np.abs(A2 - A1).max() / np.abs(A1).max(), np.abs(b2 - b1).max() / np.abs(b1).max(), np.abs(nu2 - nu1).max() / np.abs(nu1).max()
    print(f"two virtual ranks against one context: wall distance {np.abs(d2 - d1).max():.2e}, matrix {eA:.2e}, rhs {eb:.2e}, nu~ after a Newton step {en:.2e}")
    assert np.abs(d2 - d1).max() <= 1e-14 * d1.max()
    assert eA <= 1e-11 and eb <= 1e-11
    assert en <= 1e-6
