"""CPU checks of the C ABI of spike recovery and the step selectors: the pepsgpu_guard_* entry points are declared in
include/pepsgpu.h, exported by libpepsgpu.so and bound in peps_amd.capi; the pepshost_* entries are exported by libpepshost.so and
bound in peps_amd.hostapi (no compute call is made)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (number of arguments, the capi.Context method)
NEW = {"pepsgpu_guard_base_save": (1, "opt_base_save"), "pepsgpu_guard_base_restore": (1, "opt_base_restore"),
       "pepsgpu_guard_base_clear": (1, "opt_base_clear"), "pepsgpu_guard_preview": (5, "opt_preview")}
HOST = {"pepshost_ema_track": "ema_track", "pepshost_spike_replay": "spike_replay", "pepshost_acceptance_rate_check": "acceptance_rate_check",
        "pepshost_step_select": "step_select", "pepshost_step_candidates": "step_candidates", "pepshost_validate_guards": "validate_guards",
        "pepshost_guarded_optimize_exact_sum": "guarded_optimize_exact_sum", "pepshost_guarded_vmc_optimize": "guarded_vmc_optimize"}


def test_guard_entry_points_declared_exported_and_bound():
    from peps_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    header = open(os.path.join(ROOT, "include", "pepsgpu.h")).read()
    declared = set(re.findall(r"\b(pepsgpu_[a-z0-9_]+)\s*\(", header))
    assert {n for n in declared if n.startswith("pepsgpu_guard_")} == set(NEW)
    lib = ctypes.CDLL(capi.LIB_PATH)
    bound = capi.load_library()
    for name, (nargs, method) in NEW.items():
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
        assert len(getattr(bound, name).argtypes) == nargs, name
        assert callable(getattr(capi.Context, method)), name


def test_host_layer_exports_the_guard_entries():
    from peps_amd import hostapi
    if not os.path.exists(hostapi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(hostapi.LIB_PATH)
    for name, fn in HOST.items():
        assert hasattr(lib, name), name
        assert name in hostapi.SYMBOLS, name
        assert callable(getattr(hostapi, fn)), name
    assert callable(hostapi.fermion_guarded_optimize_exact_sum)
