"""The Spalart-Allmaras wall function at a moving FSI wall, the parts that need no GPU: the ABI of ifem_sa_wall and the new entry points, the
host function ifem_sa_get_shear_velocity against the numpy restatement, and the yardstick tests/sa_wall_ref.py itself on closed forms."""
import ctypes as C
import os

import numpy as np

import sa_wall_ref

MU, RHO, DIST = 0.01, 1.3, 0.02
NU = MU / RHO


def test_the_new_symbols_are_exported_declared_and_sized():
    import openifem_amd.capi as capi
    L = capi.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "ifem_hip.h")).read()
    assert len(capi.EXPORTS_SA_WALL) == 8 and not set(capi.EXPORTS_SA_WALL) & set(capi.EXPORTS)
    for s in capi.EXPORTS_SA_WALL:
        assert hasattr(L, s), s
        assert f"int {s}(" in hdr, s
    assert [f[0] for f in capi.SaWall._fields_] == ["n_vertices", "vertex", "normal", "n_edges", "edge", "image_distance", "wall_function_distance",
                                                    "sample_at_image_point"]
    assert L.ifem_abi_sizeof(capi.ABI_SA_WALL) == C.sizeof(capi.SaWall) == 64
    assert "#define IFEM_SA_NO_MOVING_WALL DBL_MAX" in hdr and capi.SA_NO_MOVING_WALL == np.finfo(float).max


def test_compute_entry_points_fail_without_a_context():
    """as the entry points of sa.hip: IFEM_E_NODEVICE where there is no device, a bad parameter for a missing context where there is one"""
    import openifem_amd.capi as capi
    L = capi.load()
    want = capi.E_NODEVICE if L.ifem_device_count() == 0 else capi.E_BADPARAM
    p = capi.SaParams(MU, RHO, 0.01)
    buf = np.zeros(8)
    ptr = buf.ctypes.data_as(C.c_void_p)
    n = C.c_int64(0)
    wall = capi.SaWall.make([0, 1], np.zeros((2, 2)), [[0, 1]], DIST, 0.1)
    calls = {
        "ifem_sa_set_moving_wall": lambda: L.ifem_sa_set_moving_wall(None, C.byref(wall)),
        "ifem_sa_set_shear_velocities": lambda: L.ifem_sa_set_shear_velocities(None, ptr),
        "ifem_sa_update_shear_velocity": lambda: L.ifem_sa_update_shear_velocity(None, C.byref(p), ptr),
        "ifem_sa_update_moving_wall_distance": lambda: L.ifem_sa_update_moving_wall_distance(None, C.byref(p), ptr, ptr),
        "ifem_sa_get_moving_wall": lambda: L.ifem_sa_get_moving_wall(None, ptr, ptr),
        "ifem_sa_update_boundary_condition": lambda: L.ifem_sa_update_boundary_condition(None, C.byref(p), 1, None, C.byref(n)),
        "ifem_sa_get_constraints": lambda: L.ifem_sa_get_constraints(None, 0, None, ptr),
    }
    assert set(calls) == set(capi.EXPORTS_SA_WALL) - {"ifem_sa_get_shear_velocity"}  # that one is a host function
    for name, call in calls.items():
        assert call() == want, name
        if want == capi.E_NODEVICE:
            assert "no CPU fallback" in L.ifem_last_error().decode(), name
    out = C.c_double(0)
    assert L.ifem_sa_get_shear_velocity(None, DIST, 1.0, 0.0, C.byref(out)) == capi.E_BADPARAM
    assert L.ifem_sa_get_shear_velocity(C.byref(p), DIST, 1.0, 0.0, None) == capi.E_BADPARAM


def _sweep():
    """(vel, init_guess): zeros and values below 1e-10, the sublayer vel d / nu < sqrt(5) (vel < 0.86 here) and the Newton branch, each from a
    cold start, from below the floor 5 nu / d, and from guesses below and above the root.
    The Newton branch is sampled where the reference's iteration is a root finder at all, y+ between 6 and 33 (vel 14 ... 165 here): its
    "derivative" kappa^3 y+^3 / (c_nu1^3 + kappa^3 y+^3) (:252-258) is not du+/dy+, so the iteration converges linearly at best.  In the numpy
    restatement it runs into its cap of 30 steps without settling for y+ below about 5.5 (residuals of order 1; from a far guess up to y+ = 5.7), and for y+ > 35 its steps fall below
    1e-2 |u_tau| while the residual is still 2e-2 ... 4e-2 of vel; in between it stops by its rule with a residual below 2e-2."""
    vels = np.concatenate([[0.0, 3e-11, -5e-11], np.geomspace(2e-10, 0.8, 9), np.geomspace(14.0, 165.0, 17)])
    return [(float(v), g) for v in vels for g in (0.0, 0.05, 1.3, 40.0)]


def test_get_shear_velocity_matches_the_numpy_restatement():
    import openifem_amd.capi as capi
    p = capi.SaParams(MU, RHO, 0.01)
    branches = {"zero": 0, "sublayer": 0, "newton": 0}
    worst, worst_root, margin = 0.0, 0.0, np.inf
    for vel, guess in _sweep():
        trace = []
        want = sa_wall_ref.get_shear_velocity(vel, guess, NU, DIST, trace)
        # the condition of the comparison: no stopping quantity within 1e-6 (relative) of the tolerance, so the iteration count cannot flip
        margin = min(margin, sa_wall_ref.stopping_margin(trace))
        assert sa_wall_ref.stopping_margin(trace) > 1e-6, (vel, guess, trace)
        got = capi.sa_get_shear_velocity(p, DIST, vel, guess)
        if abs(vel) < 1e-10:
            branches["zero"] += 1
            assert got == 0.0 and want == 0.0
            continue
        if not trace:
            branches["sublayer"] += 1
        else:
            branches["newton"] += 1
            assert len(trace) < 30, (vel, guess)  # stopped by the rule, not by the iteration cap
            root = abs(got * sa_wall_ref.u_plus(got * DIST / NU) - vel) / vel
            worst_root = max(worst_root, root)
            assert root <= 2e-2, (vel, guess, root)
        err = abs(got - want) / abs(want)
        worst = max(worst, err)
        assert err <= 1e-10, (vel, guess, got, want)
    print(f"get_shear_velocity: {branches}, worst relative difference {worst:.2e}, worst root residual {worst_root:.2e}, stopping margin {margin:.2e}")
    assert all(v > 0 for v in branches.values()), branches


def test_reference_distance_to_one_straight_edge_is_the_point_segment_distance():
    rng = np.random.default_rng(3)
    V = np.array([[0.2, 0.1], [0.9, 0.45]])
    x = rng.uniform(-0.5, 1.5, (400, 2))
    ut = np.array([0.03, 0.07])
    d, yp, _ = sa_wall_ref.moving_wall_distance(x, V, [0, 1], [[0, 1]], ut, NU)
    t = V[1] - V[0]
    s = np.clip(((x - V[0]) @ t) / (t @ t), 0.0, 1.0)
    want = np.sqrt(((x - (V[0] + s[:, None] * t)) ** 2).sum(axis=1))
    assert (s > 0).any() and (s < 1).any() and ((s > 0) & (s < 1)).any()
    assert np.abs(d - want).max() <= 1e-15 * want.max()
    assert np.abs(yp - want * (ut[0] + (ut[1] - ut[0]) * s) / NU).max() <= 1e-12 * yp.max()


def test_reference_node_beyond_a_convex_corner_takes_the_vertex():
    """the unit square's corner (1, 1): a node in the quadrant beyond it lies in no edge region, its distance is the one to the corner and its
    shear velocity the corner's; a node beside an edge takes the foot point"""
    V = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    vertex = [2, 0, 3, 1]  # not ascending
    pos = {v: i for i, v in enumerate(vertex)}
    edges = [[pos[a], pos[b]] for a, b in ((0, 1), (1, 2), (2, 3), (3, 0))]
    ut = np.array([0.01, 0.02, 0.03, 0.04])  # by position: vertex 2 has 0.01
    x = np.array([[1.3, 1.4], [1.25, 0.5]])
    d, yp, gap = sa_wall_ref.moving_wall_distance(x, V, vertex, edges, ut, NU)
    assert abs(d[0] - 0.5) <= 1e-15 and abs(yp[0] - 0.5 * 0.01 / NU) <= 1e-13 * yp[0]
    assert abs(d[1] - 0.25) <= 1e-15 and abs(yp[1] - 0.25 * (0.04 + (0.01 - 0.04) * 0.5) / NU) <= 1e-13 * yp[1]
    assert (gap > 1e-9).all()
    assert (sa_wall_ref.effective_distance([0.5, sa_wall_ref.DBL_MAX, 0.2], [0.3, 0.3, 0.3]) == [0.3, 0.3, 0.2]).all()
