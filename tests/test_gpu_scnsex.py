"""Fluid::MPI::SCnsEX on the device (csrc/scnsex.hip, ifem_scnsex_*, host.SCnsEX) against tests/scnsex_ref.py, the numpy restatement of
reference source/mpi_scnsex.cpp: the two scalar node matrices, the explicit right-hand sides with the lift of the boundary values, the
stopping rule of the CG solves, one time step, the host mirror's run, and what the solver refuses."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import scnsex_ref as R
from boxmesh import BoxMesh

pytestmark = pytest.mark.gpu

MU, RHO, DT = 1.8e-4, 1.3e-3, 3e-7  # air in cgs units, as the reference's acoustic cases; c dt / h ~ 0.05 - 0.1
GRAVITY = (3.0e2, -9.81e2, 1.5e2)
NEUMANN = {1: 40.0}                 # a pressure on the x+ boundary
NAMES = ["2q1", "2q2", "3q1", "3q2"]


def _capi():
    from openifem_amd import capi
    return capi


def _mesh(name):
    """boxes of 5x3 / 3x2x2 cells with a different edge per direction; velocity and pressure on the SAME nodes: for kv = 2 the pressure takes
    the velocity's numbering and cell_pnodes the vertex nodes of cell_unodes"""
    dim, kv = int(name[0]), int(name[2])
    m = BoxMesh((5, 3) if dim == 2 else (3, 2, 2), (0,) * dim, (1.0, 0.45) if dim == 2 else (0.9, 0.5, 0.7), kv=kv)
    n1 = kv + 1
    corner = [sum(((v >> d) & 1) * kv * n1 ** d for d in range(dim)) for v in range(2 ** dim)]
    m.cell_pnodes = np.ascontiguousarray(m.cell_unodes[:, corner])
    m.n_pnodes = m.n_unodes
    return m


def _ctx(m):
    return _capi().Context(m.dim, m.kv, m.vcoords, m.cell_unodes, m.cell_pnodes, m.cell_face_bid, m.n_unodes, m.n_pnodes)


def _params(m, dt=DT, neumann=NEUMANN, gravity=GRAVITY):
    return _capi().make_scns_params(MU, RHO, dt, g=gravity[:m.dim], neumann=neumann)


@functools.lru_cache(maxsize=None)
def _case(name):
    """mesh, inputs and the reference solver: a non-zero PML field, a body force, gravity, one Neumann boundary, inhomogeneous values on
    boundary 0 (all components) and zero normal velocity on boundary 2"""
    m = _mesh(name)
    rng = np.random.default_rng(100 + m.dim * 10 + m.kv)
    nq = (m.kv + 1) ** m.dim
    sigma = rng.uniform(0.0, 1.0e6, (m.n_cells, nq))  # of the order of 1 / dt: visible in both matrices
    bf = 50.0 * rng.standard_normal((m.n_cells, nq, m.dim))
    allc = (1 << m.dim) - 1
    bcs = {0: (allc, list(rng.uniform(1.0, 4.0, m.dim))), 2: (2, [0.0])}
    dofs, vals = R.make_constraints(m, bcs)
    vals = np.where(vals != 0.0, vals * rng.uniform(0.5, 1.5, len(vals)), 0.0)  # a different value on every node of boundary 0
    S = R.Solver(m, MU, RHO, DT, gravity=GRAVITY[:m.dim], sigma=sigma, body_force=bf, neumann=NEUMANN)
    S.set_constraints(dofs, vals)
    n = m.n_unodes
    x = np.asarray(m.unode_coords, float)
    smooth = np.zeros((m.dim + 1) * n)
    for c in range(m.dim):
        smooth[c:m.dim * n:m.dim] = 5.0 * np.sin(2.0 * x[:, c] + 0.7 * c) * np.cos(1.3 * x[:, (c + 1) % m.dim])
    smooth[m.dim * n:] = 120.0 * np.cos(2.5 * x[:, 0]) * np.sin(1.0 + 1.7 * x[:, 1])
    smooth[dofs] = vals
    return dict(m=m, sigma=sigma, bf=bf, dofs=dofs, vals=vals, S=S, smooth=smooth,
                present=np.concatenate([3.0 * rng.standard_normal(m.dim * n), 80.0 * rng.standard_normal(n)]),
                eval=np.concatenate([3.0 * rng.standard_normal(m.dim * n), 80.0 * rng.standard_normal(n)]))


def _device(name):
    k = _case(name)
    ctx = _ctx(k["m"])
    ctx.set_scns_fields(sigma_pml=k["sigma"], body_force=k["bf"])
    ctx.set_constraints(1, k["dofs"], k["vals"])
    return ctx, k


# ---- 1. matrices
@pytest.mark.parametrize("name", NAMES)
def test_matrices(name):
    ctx, k = _device(name)
    ctx.scnsex_setup(_params(k["m"]))
    Av, Ap = ctx.scnsex_export_csr(0), ctx.scnsex_export_csr(1)
    stored = ctx.uu_stored_bytes()
    ctx.close()
    S = k["S"]
    ev = abs(Av - S.Av).max() / abs(S.Av).max()
    ep = abs(Ap - S.Ap).max() / abs(S.Ap).max()
    print(f"SCnsEX matrices {name}: A_v {ev:.2e}, A_p {ep:.2e}")
    assert ev < 1e-11 and ep < 1e-11
    assert stored == 0


def test_the_matrices_follow_the_pml_field_and_the_parameters():
    """set-up is re-run when sigma or dt change"""
    ctx, k = _device("2q1")
    m = k["m"]
    ctx.scnsex_setup(_params(m))
    ctx.set_scns_fields(sigma_pml=None, body_force=k["bf"])  # a missing field is zero
    ctx.scnsex_setup(_params(m))
    Av0, Ap0 = R.matrices(m, MU, RHO, DT)
    assert abs(ctx.scnsex_export_csr(0) - Av0).max() < 1e-11 * abs(Av0).max()
    assert abs(ctx.scnsex_export_csr(1) - Ap0).max() < 1e-11 * abs(Ap0).max()
    ctx.scnsex_setup(_params(m, dt=2 * DT))
    Av1, _ = R.matrices(m, MU, RHO, 2 * DT)
    assert abs(ctx.scnsex_export_csr(0) - Av1).max() < 1e-11 * abs(Av1).max()
    ctx.close()


# ---- 2. right-hand sides
@pytest.mark.parametrize("name", NAMES)
def test_right_hand_sides(name):
    capi = _capi()
    ctx, k = _device(name)
    m, S = k["m"], k["S"]
    nv = m.dim * m.n_unodes
    ctx.vec_set(capi.VEC_PRESENT, k["present"])
    ctx.vec_set(capi.VEC_EVAL, k["eval"])
    P = _params(m)
    ctx.scnsex_assemble_rhs(P, True)
    bv = ctx.vec_get(capi.VEC_RHS)[:nv]
    ctx.scnsex_assemble_rhs(P, False)
    bp = ctx.vec_get(capi.VEC_RHS)[nv:]
    ctx.close()
    S.present = k["present"].copy()
    wv, wp = S.velocity_rhs(k["eval"]), S.pressure_rhs(k["eval"])
    ev = np.abs(bv - wv).max() / np.abs(wv).max()
    ep = np.abs(bp - wp).max() / np.abs(wp).max()
    print(f"SCnsEX right-hand sides {name}: velocity {ev:.2e}, pressure {ep:.2e}")
    assert ev < 1e-11 and ep < 1e-11
    assert (bv[k["dofs"]] == 0.0).all()
    assert (bv[np.setdiff1d(np.arange(nv), k["dofs"])] != 0.0).all()  # ... and only those


# ---- 3. stopping rule
@pytest.mark.parametrize("name", NAMES)
def test_stopping_rule(name):
    capi = _capi()
    ctx, k = _device(name)
    m, S = k["m"], k["S"]
    nv = m.dim * m.n_unodes
    ctx.vec_set(capi.VEC_PRESENT, k["present"])
    ctx.vec_set(capi.VEC_EVAL, k["eval"])
    P = _params(m)
    ctx.scnsex_assemble_rhs(P, True)
    itv, resv = ctx.scnsex_solve(True)
    ctx.scnsex_assemble_rhs(P, False)
    itp, resp = ctx.scnsex_solve(False)
    b, x = ctx.vec_get(capi.VEC_RHS), ctx.vec_get(capi.VEC_UPDATE)
    ctx.close()
    assert (x[k["dofs"]] == k["vals"]).all()  # distribute: exactly the constraint values
    x0 = x[:nv].copy()
    x0[k["dofs"]] = 0.0  # the solve left 0 there (zero start, zero right-hand side, diagonal row)
    rv = np.linalg.norm(b[:nv] - S.velocity_operator() @ x0)
    rp = np.linalg.norm(b[nv:] - S.Ap @ x[nv:])
    bnv, bnp = np.linalg.norm(b[:nv]), np.linalg.norm(b[nv:])
    print(f"SCnsEX solves {name}: velocity {itv} its, true residual {rv / bnv:.2e} (recurrence {resv / bnv:.2e}); "
          f"pressure {itp} its, {rp / bnp:.2e} ({resp / bnp:.2e})")
    assert rv <= 1e-6 * bnv * (1 + 1e-6)
    assert rp <= 1e-6 * bnp * (1 + 1e-6)


# ---- 4. one time step
@pytest.mark.parametrize("name", NAMES)
def test_one_time_step(name):
    """1e-4 of each block's largest magnitude: the device solves to a residual of 1e-6 ||rhs|| where the reference solves directly, the
    Jacobi-scaled mass-dominated matrices have condition numbers of order 10-30, and there are a few outer iterations"""
    capi = _capi()
    ctx, k = _device(name)
    m, S = k["m"], k["S"]
    nv = m.dim * m.n_unodes
    ctx.vec_set(capi.VEC_PRESENT, k["smooth"])
    st = ctx.scnsex_step(_params(m), 1e-6, 8)
    got = ctx.vec_get(capi.VEC_PRESENT)
    stored = ctx.uu_stored_bytes()
    ctx.close()
    S.present = k["smooth"].copy()
    log = S.step(1e-6, 8)
    want = S.present
    eu = np.abs(got[:nv] - want[:nv]).max() / np.abs(want[:nv]).max()
    ep = np.abs(got[nv:] - want[nv:]).max() / np.abs(want[nv:]).max()
    print(f"SCnsEX step {name}: outer {st.outer_iterations} (reference {len(log)}), CG {st.vel_iters} / {st.pre_iters}, "
          f"velocity {eu:.2e}, pressure {ep:.2e}, rel {st.rel_res:.2e} (reference {log[-1][1]:.2e})")
    assert st.outer_iterations == len(log)
    assert eu < 1e-4 and ep < 1e-4
    assert (got[k["dofs"]] == k["vals"]).all()
    assert stored == 0


def test_a_state_at_rest_takes_one_iteration_and_stays_at_rest():
    capi = _capi()
    m = _mesh("2q1")
    ctx = _ctx(m)
    dofs, vals = R.make_constraints(m, {0: (3, [0.0, 0.0]), 2: (2, [0.0])})
    ctx.set_constraints(1, dofs, vals)
    st = ctx.scnsex_step(_params(m, neumann=None, gravity=(0, 0, 0)), 1e-6, 8)
    x = ctx.vec_get(capi.VEC_PRESENT)
    ctx.close()
    assert st.outer_iterations == 1 and np.isnan(st.rel_res)
    assert (x == 0).all()


def test_too_many_iterations_is_reported():
    capi = _capi()
    ctx, k = _device("2q1")
    ctx.vec_set(capi.VEC_PRESENT, k["smooth"])
    with pytest.raises(capi.IfemError) as e:
        ctx.scnsex_step(_params(k["m"]), 1e-6, 1)
    assert e.value.code == capi.E_NEWTON_MAXIT and "Too many iterations" in str(e.value)
    ctx.close()


# ---- 7. refusals
def test_taylor_hood_contexts_are_refused():
    capi = _capi()
    m = BoxMesh((3, 2), (0, 0), (1.5, 0.8), kv=2)  # Q2 velocity, Q1 pressure
    ctx = _ctx(m)
    P = _params(m)
    for call in (lambda: ctx.scnsex_setup(P), lambda: ctx.scnsex_assemble_rhs(P, True), lambda: ctx.scnsex_solve(True),
                 lambda: ctx.scnsex_step(P), lambda: ctx.scnsex_export_csr(0)):
        with pytest.raises(capi.IfemError) as e:
            call()
        assert e.value.code == capi.E_BADPARAM and "same as pressure" in str(e.value)
    x = np.arange(ctx.n_local, dtype=float)
    ctx.vec_set(capi.VEC_PRESENT, x)  # the context is still usable
    assert (ctx.vec_get(capi.VEC_PRESENT) == x).all()
    ctx.assemble(capi.make_params(), False)
    assert ctx.rhs_norm() >= 0.0
    ctx.close()


def test_differing_node_tables_are_refused():
    capi = _capi()
    m = _mesh("2q1")
    m.cell_pnodes = np.ascontiguousarray(m.cell_pnodes[:, [1, 0, 3, 2]])  # same nodes, another local order
    ctx = _ctx(m)
    with pytest.raises(capi.IfemError) as e:
        ctx.scnsex_setup(_params(m))
    assert e.value.code == capi.E_BADPARAM and "node tables differ" in str(e.value)
    ctx.close()


def test_hanging_node_contexts_are_refused():
    from hangmesh import HangingMesh
    capi = _capi()
    m = HangingMesh((3, 2), (0, 0), (1.5, 0.8), {(0, 0), (2, 1)}, kv=1)
    assert len(m.hang_dof) > 0
    ctx = _ctx(m)
    ctx.set_hanging_constraints(m.hang_dof, m.hang_ptr, m.hang_master, m.hang_weight)
    P = _params(m)
    for call in (lambda: ctx.scnsex_setup(P), lambda: ctx.scnsex_assemble_rhs(P, False), lambda: ctx.scnsex_solve(False),
                 lambda: ctx.scnsex_step(P), lambda: ctx.scnsex_export_csr(1)):
        with pytest.raises(capi.IfemError) as e:
            call()
        assert e.value.code == capi.E_BADPARAM and "hanging nodes" in str(e.value)
    x = np.arange(ctx.n_local, dtype=float)
    ctx.vec_set(capi.VEC_EVAL, x)  # the context is still usable
    assert (ctx.vec_get(capi.VEC_EVAL) == x).all()
    ctx.close()


def test_partitioned_contexts_are_refused():
    from openifem_amd import host
    capi = _capi()
    L = capi.load()
    world = 2
    w = C.c_void_p(L.ifem_local_world_create(world))
    out, errs = [None] * world, []

    def work(rank):
        try:
            s = host.InsIM(host.channel_prm(3), (4, 2, 2), (0, 0, 0), (2.0, 0.2, 0.2))
            s.set_partition((2, 1, 1), rank, local_world=w)
            s.setup(0)
            P = capi.make_scns_params(MU, RHO, DT)
            rc = L.ifem_scnsex_setup(s.ctx, C.byref(P))
            msg = L.ifem_last_error().decode()
            rc2 = L.ifem_halo_exchange(s.ctx, capi.VEC_EVAL)  # collective: the context is still usable on both ranks
            out[rank] = (rc, msg, rc2)
            s.close()
        except Exception:  # noqa
            import traceback
            errs.append((rank, traceback.format_exc()))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    L.ifem_local_world_destroy(w)
    assert not errs, errs
    for rc, msg, rc2 in out:
        assert rc == capi.E_BADPARAM and "partitioned" in msg
        assert rc2 == 0


# ---- 5. / 6. the host mirror on the reference's acoustic duct (tests/acoustic_duct_wave_mpi_scnsex)
def _duct_prm(steps=None):
    import os
    import re
    text = open(os.path.join(os.path.dirname(__file__), "golden", "prm", "acoustic_duct_wave_mpi_scnsex.prm")).read()
    if steps is not None:
        text, n = re.subn(r"set End time\s*=\s*\S+", f"set End time = {steps * R.DUCT['dt']:.10e}", text)
        assert n == 1
    return text


def _duct_flow(prm):
    from openifem_amd import host
    flow = host.SCnsEX(prm, (8, 2), (0, 0), (4, 1))
    flow.add_hard_coded_boundary_condition(0, R.duct_pulse)
    flow.set_hard_coded_boundary_condition_time(0, 1.1e-4)
    return flow


def test_mirror_short_run(tmp_path):
    """60 steps of the duct case: the whole fields against scnsex_ref.run to 1e-4 of each block's maximum"""
    steps = 60
    path = tmp_path / "duct.prm"
    path.write_text(_duct_prm(steps))
    flow = _duct_flow(path.read_text())
    flow.set_output_dir(str(tmp_path))
    flow.run()
    assert flow.time()[0] == steps
    u, p = flow.get_current_solution()
    uc, _ = flow.node_coords()
    st = flow.last_step()
    stored = _capi().load().ifem_uu_stored_bytes(flow.ctx)
    flow.close()
    log = []
    S = R.duct_run(steps, log=log)
    m = S.m
    ij = np.rint(uc / np.array([4.0 / 64, 1.0 / 16])).astype(np.int64)
    node = ij[:, 0] + 65 * ij[:, 1]  # the mirror's (Morton) node -> the lattice node of tests/boxmesh.py
    assert np.abs(np.asarray(m.unode_coords)[node] - uc).max() < 1e-12
    wu = S.present[:2 * m.n_unodes].reshape(-1, 2)[node].ravel()
    wp = S.present[2 * m.n_unodes:][node]
    eu, ep = np.abs(u - wu).max() / np.abs(wu).max(), np.abs(p - wp).max() / np.abs(wp).max()
    print(f"SCnsEX mirror, {steps} steps: velocity {eu:.2e} of {np.abs(wu).max():.3e}, pressure {ep:.2e} of {np.abs(wp).max():.3e}; "
          f"last step outer {st.outer_iterations} (reference {log[-1]}), CG {st.vel_iters} / {st.pre_iters}")
    assert eu < 1e-4 and ep < 1e-4
    assert stored == 0


def test_mirror_refuses_taylor_hood_parameters():
    from openifem_amd import host
    prm = _duct_prm().replace("set Velocity degree = 1", "set Velocity degree = 2")
    with pytest.raises(host.HostError) as e:
        host.SCnsEX(prm, (8, 2), (0, 0), (4, 1))
    assert "Velocity degree must the same as pressure" in str(e.value)


@pytest.mark.slow
def test_reference_driver_acoustic_duct_wave_mpi_scnsex(tmp_path):
    # tests/acoustic_duct_wave_mpi_scnsex/acoustic_duct_wave_mpi_scnsex.cpp:33-64 on the host mirror with the reference's .prm: 1000
    # steps of 1e-7; vmax against the known answer of the restatement (tests/test_scnsex_host.py; the reference asserts 1e-2 of 6)
    flow = _duct_flow(_duct_prm())
    flow.set_output_dir(str(tmp_path))
    flow.run()
    v, _ = flow.get_current_solution()
    flow.close()
    print(f"SCnsEX duct, 1000 steps: vmax {v.max():.6f}")
    assert abs(v.max() - R.DUCT_VMAX) < 1e-3
