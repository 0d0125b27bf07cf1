"""ifem_scnsex_* (CPU): the five entry points of the explicit split solver are exported, listed, bound and declared, and added no
field to any struct of the interface."""
import ctypes as C
import os

SYMBOLS = ["ifem_scnsex_setup", "ifem_scnsex_assemble_rhs", "ifem_scnsex_solve", "ifem_scnsex_step", "ifem_scnsex_export_csr"]


def test_the_five_symbols_resolve():
    import openifem_amd.capi as capi
    L = capi.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ifem_hip.h")).read()
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
        assert f"int {s}(ifem_ctx *ctx" in hdr, s
    for meth in ("scnsex_setup", "scnsex_assemble_rhs", "scnsex_solve", "scnsex_step", "scnsex_export_csr"):
        assert hasattr(capi.Context, meth), meth


def test_the_structs_keep_their_sizes():
    import openifem_amd.capi as capi
    L = capi.load()
    for i, s in enumerate(capi.ABI_STRUCTS):
        assert L.ifem_abi_sizeof(i) == C.sizeof(s)
    assert L.ifem_abi_sizeof(capi.ABI_SCNSEX_STATS) == C.sizeof(capi.ScnsexStats) == 48
