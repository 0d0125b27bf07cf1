"""ifem_test_mg_transfer / ifem_test_mg_vec_kernel (CPU): exported, listed, bound with the arity of their declarations and declared in the
testing header only; the op numbers of the binding are the header's; the aids added no field to any struct of the interface."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_test_aids_are_exported_bound_and_declared():
    import openifem_amd.capi as capi
    L = capi.load()
    hdr, pub = _header("ifem_hip_testing.h"), _header("ifem_hip.h")
    for name, method in (("ifem_test_mg_transfer", "test_mg_transfer"), ("ifem_test_mg_vec_kernel", "test_mg_vec_kernel")):
        assert name in capi.EXPORTS and hasattr(L, name)
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert decl, name
        arity = len(decl.group(1).split(","))
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == arity == 11
        assert hasattr(capi.Context, method)
        assert not re.search(r"\b%s\s*\(" % name, pub)  # a test aid: not part of the drop-in surface
    assert ("int ifem_test_mg_transfer(ifem_ctx *ctx, int kind, int64_t n_rows, int64_t n_cols, const int64_t *ptr, const int32_t *col, "
            "const double *w,") in hdr
    assert ("int ifem_test_mg_vec_kernel(ifem_ctx *ctx, int op, int64_t n, int64_t m, const double *coef, const int32_t *idx, double *in0, "
            "double *in1,") in hdr


def test_the_op_numbers_of_the_binding_are_the_headers():
    import openifem_amd.capi as capi
    hdr = _header("ifem_hip_testing.h")
    ops = re.search(r"enum \{\s*(IFEM_TMG_CHEB_INIT = 0,[^}]*)\}", hdr).group(1)
    names = [s.split("=")[0].strip() for s in ops.split(",") if s.strip()]
    assert names[-1] == "IFEM_TMG_COUNT" and len(names) == 14
    for k, n in enumerate(names[:-1]):
        assert getattr(capi, n[len("IFEM_"):]) == k, n
    assert re.search(r"enum \{ IFEM_TMG_PAD = (\d+) \}", hdr).group(1) == str(capi.TMG_PAD)


def test_the_header_states_the_weight_rule_next_to_the_transfer_struct():
    pub = _header("ifem_hip.h")
    body = pub[:pub.index("} ifem_mg_transfer;")]
    assert "double(float(w)) == w" in body[body.rindex("typedef struct"):]


def test_the_structs_keep_their_sizes_and_last_fields():
    import openifem_amd.capi as capi
    L = capi.load()
    for i, s in enumerate(capi.ABI_STRUCTS):
        assert L.ifem_abi_sizeof(i) == C.sizeof(s)
    assert capi.Tuning._fields_[-1][0] == "uu_patch_levels" and capi.SolverOpts._fields_[-1][0] == "mp_solver"
    assert capi.MgTransfer._fields_[-1][0] == "inj_u" and len(capi.MgTransfer._fields_) == 17
