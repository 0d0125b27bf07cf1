"""ifem_solver_opts::mp_solver (CPU): appended to the struct, mirrored in ctypes, 0 by default and in a zero-initialised struct."""
import ctypes as C


def test_mp_solver_is_appended_and_defaults_to_the_direct_solve():
    import openifem_amd.capi as capi
    L = capi.load()
    assert capi.SolverOpts._fields_[-1][0] == "mp_solver"  # appended: the fields before it keep their offsets
    assert L.ifem_abi_sizeof(capi.ABI_STRUCTS.index(capi.SolverOpts)) == C.sizeof(capi.SolverOpts)
    o = capi.SolverOpts()
    assert o.mp_solver == 0  # a zero-initialised struct keeps the default
    o.mp_solver = 7
    L.ifem_default_solver_opts(C.byref(o))
    assert o.mp_solver == 0
    assert "ifem_test_mp_solve" in capi.EXPORTS and hasattr(L, "ifem_test_mp_solve")
