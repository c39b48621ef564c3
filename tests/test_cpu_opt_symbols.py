"""CPU checks of the optimizer's C ABI: every pepsgpu_opt_* entry point declared in include/pepsgpu.h is exported by libpepsgpu.so
and bound in peps_amd.capi (no compute call is made)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"pepsgpu_opt_begin": 1, "pepsgpu_opt_end": 1, "pepsgpu_opt_gradient_from_accumulators": 5, "pepsgpu_opt_set_gradient": 2,
       "pepsgpu_opt_get_gradient": 2, "pepsgpu_opt_clip": 4, "pepsgpu_opt_natural_gradient": 11, "pepsgpu_opt_step": 5,
       "pepsgpu_opt_scale_state": 2, "pepsgpu_opt_read_state": 2}


def test_opt_entry_points_declared_exported_and_bound():
    from peps_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    header = open(os.path.join(ROOT, "include", "pepsgpu.h")).read()
    declared = set(re.findall(r"\b(pepsgpu_[a-z0-9_]+)\s*\(", header))
    assert {n for n in declared if n.startswith("pepsgpu_opt_")} == set(NEW)
    lib = ctypes.CDLL(capi.LIB_PATH)
    bound = capi.load_library()
    for name, nargs in NEW.items():
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
        assert len(getattr(bound, name).argtypes) == nargs, name
        assert callable(getattr(capi.Context, name[len("pepsgpu_"):])), name


def test_host_layer_exports_the_optimizer_entries():
    from peps_amd import hostapi
    if not os.path.exists(hostapi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(hostapi.LIB_PATH)
    for name in ("pepshost_optimize_exact_sum", "pepshost_optimize_exact_sum_c128", "pepshost_lr_schedule", "pepshost_sr_step_samples",
                 "pepshost_sr_step_samples_c128"):
        assert hasattr(lib, name), name
        assert name in hostapi.SYMBOLS, name
    assert callable(hostapi.optimize_exact_sum) and callable(hostapi.lr_schedule) and callable(hostapi.sr_step_samples)
