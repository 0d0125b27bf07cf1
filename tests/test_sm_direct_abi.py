"""ifem_test_sm_solve (CPU): exported, listed, bound and declared; the direct S_m solve is a new VALUE of ifem_solver_opts::sm_mg, whose
default stays 1, and added no field to any struct of the interface."""
import ctypes as C
import os


def test_the_test_aid_is_exported_and_sm_mg_keeps_its_default():
    import openifem_amd.capi as capi
    L = capi.load()
    assert "ifem_test_sm_solve" in capi.EXPORTS and hasattr(L, "ifem_test_sm_solve")
    assert L.ifem_test_sm_solve.argtypes is not None and len(L.ifem_test_sm_solve.argtypes) == 5
    assert hasattr(capi.Context, "sm_solve")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ifem_hip_testing.h")).read()
    assert "int ifem_test_sm_solve(ifem_ctx *ctx, const ifem_solver_opts *o, const double *b, double *x, int64_t info[4]);" in hdr
    assert (capi.SM_CG, capi.SM_MG, capi.SM_DIRECT) == (0, 1, 2)
    o = capi.SolverOpts()
    L.ifem_default_solver_opts(C.byref(o))
    assert o.sm_mg == capi.SM_MG == 1


def test_the_structs_keep_their_sizes_and_last_fields():
    import openifem_amd.capi as capi
    L = capi.load()
    for i, s in enumerate(capi.ABI_STRUCTS):
        assert L.ifem_abi_sizeof(i) == C.sizeof(s)
    assert capi.Tuning._fields_[-1][0] == "uu_patch_levels" and capi.SolverOpts._fields_[-1][0] == "mp_solver"
