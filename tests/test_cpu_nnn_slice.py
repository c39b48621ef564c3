"""CPU checks of the diagonal-bond slice's C ABI: pepsgpu_nnn_exchange_slice, pepsgpu_diag_dot4 and pepsgpu_diag_nnn_slice_calls are
declared in include/pepsgpu.h, exported by libpepsgpu.so and bound in peps_amd.capi (no compute call is made)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pepsgpu_nnn_exchange_slice", "pepsgpu_diag_dot4", "pepsgpu_diag_nnn_slice_calls")


def test_nnn_slice_entry_points_declared_exported_and_bound():
    from peps_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    header = open(os.path.join(ROOT, "include", "pepsgpu.h")).read()
    declared = set(re.findall(r"\b(pepsgpu_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
    # the ctypes signatures: (ctx, row1, diag_mask, val_out), (dtype, a, b, dims4, nbatch, lsum, flag, out) and (void) -> long
    bound = capi.load_library()
    assert len(bound.pepsgpu_nnn_exchange_slice.argtypes) == 4
    assert len(bound.pepsgpu_diag_dot4.argtypes) == 8
    assert len(bound.pepsgpu_diag_nnn_slice_calls.argtypes) == 0 and bound.pepsgpu_diag_nnn_slice_calls.restype is ctypes.c_long
    assert callable(getattr(capi.Context, "nnn_exchange_slice"))
    assert callable(capi.diag_dot4) and callable(capi.diag_nnn_slice_calls)
    # no slice has run in this process, and asking does not need a device
    assert capi.diag_nnn_slice_calls() == 0
