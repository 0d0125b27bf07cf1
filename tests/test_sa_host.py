"""Spalart-Allmaras model, the parts that need no GPU: the ABI of ifem_sa_params, the entry points without a device, and the
numpy yardstick tests/sa_ref.py itself -- pinned on a closed form, and its branch counters on the inputs of the GPU parity test."""
import ctypes as C

import numpy as np
import pytest

import sa_ref
from boxmesh import BoxMesh


def test_sa_params_mirror_has_the_size_the_library_was_compiled_with():
    import openifem_amd.capi as capi
    L = capi.load()
    which = capi.ABI_STRUCTS.index(capi.SaParams)
    assert which == 13
    assert L.ifem_abi_sizeof(which) == C.sizeof(capi.SaParams) == 24
    assert [f[0] for f in capi.SaParams._fields_] == ["viscosity", "rho", "dt"]
    assert (capi.SA_PRESENT, capi.SA_EVAL, capi.SA_UPDATE, capi.SA_RHS) == (0, 1, 2, 3)


def test_entry_points_fail_without_a_context():
    """a context only exists where a device does: without a device every ifem_sa_* entry point answers IFEM_E_NODEVICE (with one, a
    missing context is a bad parameter)"""
    import openifem_amd.capi as capi
    L = capi.load()
    want = capi.E_NODEVICE if L.ifem_device_count() == 0 else capi.E_BADPARAM
    p = capi.SaParams(0.05, 1.3, 0.01)
    buf = np.zeros(8)
    ptr = buf.ctypes.data_as(C.c_void_p)
    it, res = C.c_uint32(0), C.c_double(0)
    calls = {
        "ifem_sa_set_wall_points": lambda: L.ifem_sa_set_wall_points(None, 0, None),
        "ifem_sa_get_wall_distance": lambda: L.ifem_sa_get_wall_distance(None, ptr),
        "ifem_sa_set_constraints": lambda: L.ifem_sa_set_constraints(None, 0, 0, None, None),
        "ifem_sa_vec_set": lambda: L.ifem_sa_vec_set(None, capi.SA_PRESENT, ptr),
        "ifem_sa_vec_get": lambda: L.ifem_sa_vec_get(None, capi.SA_PRESENT, ptr),
        "ifem_sa_assemble": lambda: L.ifem_sa_assemble(None, C.byref(p), 0),
        "ifem_sa_solve": lambda: L.ifem_sa_solve(None, 0, C.byref(it), C.byref(res)),
        "ifem_sa_newton_step": lambda: L.ifem_sa_newton_step(None, C.byref(p), 1, 1e-6, 8, None),
        "ifem_sa_update_eddy_viscosity": lambda: L.ifem_sa_update_eddy_viscosity(None, C.byref(p), None),
        "ifem_sa_export_csr": lambda: L.ifem_sa_export_csr(None, ptr, None, None),
    }
    assert set(calls) == {s for s in capi.EXPORTS if s.startswith("ifem_sa_")}
    for name, call in calls.items():
        assert call() == want, name
        if want == capi.E_NODEVICE:
            assert "no CPU fallback" in L.ifem_last_error().decode(), name


def _lagrange_1d(kv):
    """exact mass and stiffness matrices of the Q_kv Lagrange basis on [0, 1] (polynomial integration, no quadrature)"""
    P = np.polynomial.polynomial
    nodes = np.arange(kv + 1) / kv
    basis = []
    for a in range(kv + 1):
        p = np.array([1.0])
        for b in range(kv + 1):
            if b != a:
                p = P.polymul(p, np.array([-nodes[b], 1.0]) / (nodes[a] - nodes[b]))
        basis.append(p)
    integ = lambda p: P.polyval(1.0, P.polyint(p)) - P.polyval(0.0, P.polyint(p))
    M = np.array([[integ(P.polymul(a, b)) for b in basis] for a in basis])
    K = np.array([[integ(P.polymul(P.polyder(a), P.polyder(b))) for b in basis] for a in basis])
    return M, K


def _box_mass_stiffness(m):
    """global M and K of an axis-aligned box mesh: tensor products of the 1D matrices, x fastest"""
    M1, K1 = _lagrange_1d(m.kv)
    h = (m.p1 - m.p0) / np.array(m.reps)
    Me, Ke = np.ones((1, 1)), np.zeros((1, 1))
    for d in range(m.dim):
        Ke = np.kron(K1 / h[d], Me) + np.kron(M1 * h[d], Ke)
        Me = np.kron(M1 * h[d], Me)
    n = m.n_unodes
    M, K = np.zeros((n, n)), np.zeros((n, n))
    for idx in m.cell_unodes:
        M[np.ix_(idx, idx)] += Me
        K[np.ix_(idx, idx)] += Ke
    return M, K


@pytest.mark.parametrize("dim,kv,reps", [(2, 2, (3, 2)), (3, 1, (3, 2, 2))])
def test_sa_ref_closed_form(dim, kv, reps):
    """u = 0, nu~_eval = nu~_present = c > 0, no wall points, no constraints: S = S_bar = 0 and 1 / d^2 = 0, so P = D = 0, the
    right-hand side vanishes and the matrix is M / dt + (mu / rho + c) / sigma K"""
    m = BoxMesh(reps, (0,) * dim, (1.0, 0.6, 0.4)[:dim], kv=kv)
    mu, rho, dt, c = 0.05, 1.3, 0.01, 0.2
    n = m.n_unodes
    d = sa_ref.wall_distance(m, np.zeros((0, dim)))
    assert (d == np.finfo(float).max).all()
    A, b, counters = sa_ref.assemble(m, np.zeros(dim * n), np.full(n, c), np.full(n, c), d, mu, rho, dt)
    M, K = _box_mass_stiffness(m)
    want = M / dt + (mu / rho + c) / sa_ref.SIGMA * K
    assert np.abs(A.toarray() - want).max() <= 1e-13 * np.abs(want).max()
    assert np.abs(b).max() <= 1e-13 * np.abs(want).max() * c
    assert counters["S_tilde_small"] == m.n_cells * (kv + 1) ** dim and counters["nu_negative"] == 0


@pytest.mark.parametrize("name", ["2q2", "2q1", "3q2", "3q1", "cyl"])
def test_parity_inputs_reach_every_branch(name):
    """a condition on the INPUTS of tests/test_gpu_sa.py::test_assembly_parity: each branch of :741-791 is taken at >= 1 quadrature
    point, and no coefficient is singular there (finite matrix)"""
    m, inp = sa_ref.parity_inputs(name)
    d = sa_ref.wall_distance(m, inp["wall"])
    A, b, counters = sa_ref.assemble(m, inp["fluid"], inp["eval"], inp["present"], d, indicator=inp["indicator"], is_c=inp["is_c"],
                                     cval=inp["cval"], **sa_ref.PARITY_PARAMS)
    for key in ("nu_negative", "S_bar_branch", "S_tilde_small", "r_clipped", "indicator"):
        assert counters[key] >= 1, (key, counters)
    assert np.isfinite(A.data).all() and np.isfinite(b).all()
    assert 0.2 <= inp["indicator"].mean() <= 0.6, inp["indicator"].mean()
    assert (inp["eval"] != inp["present"]).all() and (inp["inhom"] != 0).all()


# ---- host mirror: the Spalart Allmaras subsection of the .prm and the model's constraint lines (no device needed)
def test_prm_spalart_allmaras_subsection():
    import os
    from openifem_amd import host
    s = host.SCnsIM(sa_ref.channel_prm(), (6, 4), (0, 0), (1.5, 0.5))
    s.attach_turbulence_model("Spalart-Allmaras")
    s.setup_host_only(0)
    node, val, _ = s.turbulence_setup()
    uc, _ = s.node_coords()
    on = (np.abs(uc[:, 0]) < 1e-12) | (np.abs(uc[:, 1]) < 1e-12) | (np.abs(uc[:, 1] - 0.5) < 1e-12)
    assert sorted(node) == sorted(np.nonzero(on)[0]) and len(set(node)) == len(node)
    # boundary ids in ascending order, the first line of a node stays: the inflow x- (id 0, type 1) keeps its corner nodes
    want = np.where(np.abs(uc[node, 0]) < 1e-12, 5 * 0.01 / 1.0, 0.0)
    assert (val == want).all()
    # the reference's messages for inconsistent lists (parameters.cpp:338-348)
    with pytest.raises(host.HostError, match="Inconsistent boundary ids!"):
        host.SCnsIM(sa_ref.channel_prm(n_bcs=3, ids="0, 2"), (6, 4), (0, 0), (1.5, 0.5))
    with pytest.raises(host.HostError, match="Inconsistent boundary values!"):
        host.SCnsIM(sa_ref.channel_prm(n_bcs=3, types="1, 0"), (6, 4), (0, 0), (1.5, 0.5))
    with pytest.raises(host.HostError):
        host.SCnsIM(sa_ref.channel_prm(types="1, 0, 2"), (6, 4), (0, 0), (1.5, 0.5))
    # a golden .prm without the subsection: defaults, a model attaches and has no lines
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    g = host.SCnsIM(open(os.path.join(root, "tests", "golden", "prm", "fluid_body_force_mpi.prm")).read(), (8, 4), (0, 0), (8, 2))
    g.attach_turbulence_model("Spalart-Allmaras")
    g.setup_host_only(0)
    assert len(g.turbulence_setup()[0]) == 0
    with pytest.raises(host.HostError, match="ExcNotImplemented"):
        g.attach_turbulence_model("k-epsilon")
    with pytest.raises(host.HostError, match="no turbulence model attached"):
        host.SCnsIM(sa_ref.channel_prm(), (6, 4), (0, 0), (1.5, 0.5)).turbulence_setup()


def test_checkpoint_with_a_model_attached_is_refused(tmp_path):
    from openifem_amd import host
    s = host.SCnsIM(sa_ref.channel_prm(), (6, 4), (0, 0), (1.5, 0.5))
    s.attach_turbulence_model("Spalart-Allmaras")
    s.setup_host_only(0)
    with pytest.raises(host.HostError, match="not supported with a turbulence model"):
        s.save_checkpoint(str(tmp_path), 1)


def test_partitioned_solver_with_a_model_attached_is_refused():
    """the model needs the wall points of the WHOLE mesh on every rank and a partitioned mirror holds its own cells only: it refuses rather than
    compute a wall distance from a rank's share (either order of attach / set_partition)"""
    from openifem_amd import host
    for attach_first in (True, False):
        s = host.SCnsIM(sa_ref.channel_prm(), (6, 4), (0, 0), (1.5, 0.5))
        if attach_first:
            s.attach_turbulence_model("Spalart-Allmaras")
        s.set_partition((2, 1, 1), 0, local_world=None)
        if not attach_first:
            s.attach_turbulence_model("Spalart-Allmaras")
        with pytest.raises(host.HostError, match="partitioned fluid solver"):
            s.setup_host_only(0)
    # without a model the same partition sets up as before
    s = host.SCnsIM(sa_ref.channel_prm(), (6, 4), (0, 0), (1.5, 0.5))
    s.set_partition((2, 1, 1), 0, local_world=None)
    s.setup_host_only(0)
