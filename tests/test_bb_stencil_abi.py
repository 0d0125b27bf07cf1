"""ifem_test_b_apply (CPU): exported, listed and declared; the stencil products of B and B^T added no field to any struct of the interface."""
import ctypes as C
import os

SIZES = {"MeshDesc": 64, "Partition": 200, "InsParams": 160, "SolverOpts": 152, "SolveStats": 88, "ScnsParams": 168, "Timing": 56, "Tuning": 136,
         "MgTransfer": 136, "FsiSolid": 64, "FsiStats": 32, "CommStats": 64, "KprofEntry": 32, "SaParams": 24}


def test_the_test_aid_is_exported_and_the_structs_keep_their_sizes():
    import openifem_amd.capi as capi
    L = capi.load()
    assert "ifem_test_b_apply" in capi.EXPORTS and hasattr(L, "ifem_test_b_apply")
    assert L.ifem_test_b_apply.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ifem_hip_testing.h")).read()
    assert "int ifem_test_b_apply(ifem_ctx *ctx, int which, int path, const double *x, double *y, int64_t info[4]);" in hdr
    assert {s.__name__: C.sizeof(s) for s in capi.ABI_STRUCTS} == SIZES
    for i, s in enumerate(capi.ABI_STRUCTS):
        assert L.ifem_abi_sizeof(i) == C.sizeof(s)
    assert capi.Tuning._fields_[-1][0] == "uu_patch_levels" and capi.SolverOpts._fields_[-1][0] == "mp_solver"
