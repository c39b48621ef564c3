"""CPU checks of the device-side energy slices' C ABI: pepsgpu_nn_exchange_slice_tab and pepsgpu_onsite_slice are declared in
include/pepsgpu.h, exported by libpepsgpu.so and bound in peps_amd.capi (no compute call is made)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pepsgpu_nn_exchange_slice_tab", "pepsgpu_onsite_slice")


def test_energy_slice_entry_points_declared_exported_and_bound():
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
    # the ctypes signatures: (ctx, orientation, slice, punch_holes, table, psi_per_bond, psi, psi_ex) and
    # (ctx, orientation, slice, punch_holes, n_cand, site_table, psi, psi_cand)
    bound = capi.load_library()
    assert len(bound.pepsgpu_nn_exchange_slice_tab.argtypes) == 8
    assert len(bound.pepsgpu_onsite_slice.argtypes) == 8
    assert callable(getattr(capi.Context, "nn_exchange_slice_tab")) and callable(getattr(capi.Context, "onsite_slice"))
