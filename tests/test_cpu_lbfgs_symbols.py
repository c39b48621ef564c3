"""CPU checks of the L-BFGS entry points: every pepsgpu_lbfgs_* is declared in include/pepsgpu.h, exported by libpepsgpu.so and bound
in peps_amd.capi with the expected argument count; none of them extends the closed set of pepsgpu_opt_* names; the four shim entries
are exported by libpepshost.so (no compute call is made)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"pepsgpu_lbfgs_begin": 2, "pepsgpu_lbfgs_end": 1, "pepsgpu_lbfgs_reset": 1, "pepsgpu_lbfgs_update": 5, "pepsgpu_lbfgs_direction": 6,
       "pepsgpu_lbfgs_trial": 2, "pepsgpu_lbfgs_slope": 2, "pepsgpu_lbfgs_commit": 1, "pepsgpu_lbfgs_get_direction": 2,
       "pepsgpu_lbfgs_get_pair": 4, "pepsgpu_lbfgs_counters": 2}


def test_lbfgs_entry_points_declared_exported_and_bound():
    from peps_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    header = open(os.path.join(ROOT, "include", "pepsgpu.h")).read()
    declared = set(re.findall(r"\b(pepsgpu_[a-z0-9_]+)\s*\(", header))
    assert {n for n in declared if n.startswith("pepsgpu_lbfgs_")} == set(NEW)
    assert not any(n.startswith("pepsgpu_opt_") for n in NEW)
    lib = ctypes.CDLL(capi.LIB_PATH)
    bound = capi.load_library()
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
        assert len(getattr(bound, name).argtypes) == nargs, name
        assert callable(getattr(capi.Context, name[len("pepsgpu_"):])), name


def test_host_layer_exports_the_lbfgs_entries():
    from peps_amd import hostapi
    if not os.path.exists(hostapi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(hostapi.LIB_PATH)
    for name in ("pepshost_lbfgs_exact_sum", "pepshost_lbfgs_exact_sum_c128", "pepshost_fermion_lbfgs_exact_sum",
                 "pepshost_fermion_lbfgs_exact_sum_c128"):
        assert hasattr(lib, name), name
        assert name in hostapi.SYMBOLS, name
    assert callable(hostapi.lbfgs_optimize_exact_sum) and callable(hostapi.fermion_lbfgs_optimize_exact_sum)
    assert len(hostapi.LBFGS_FIELDS) == 14 == len(hostapi.LBFGS_DEFAULTS)
