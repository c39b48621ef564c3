"""CPU checks of the MinSR entry points: pepsgpu_minsr_direction and pepsgpu_diag_eigh are declared in include/pepsgpu.h, exported by
libpepsgpu.so and bound in peps_amd.capi; the host layer exports the MinSR step (no compute call is made)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"pepsgpu_minsr_direction": 8, "pepsgpu_diag_eigh": 7}


def test_minsr_entry_points_declared_exported_and_bound():
    from peps_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    header = open(os.path.join(ROOT, "include", "pepsgpu.h")).read()
    declared = set(re.findall(r"\b(pepsgpu_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(capi.LIB_PATH)
    bound = capi.load_library()
    for name, nargs in NEW.items():
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
        assert len(getattr(bound, name).argtypes) == nargs, name
        assert callable(getattr(capi.Context, name[len("pepsgpu_"):])), name
    # the arguments of the declarations themselves
    for name, nargs in NEW.items():
        args = re.search(r"\bint %s\s*\(([^)]*)\)\s*;" % name, header).group(1)
        assert len(args.split(",")) == nargs, (name, args)


def test_host_layer_exports_the_minsr_step():
    from peps_amd import hostapi
    if not os.path.exists(hostapi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(hostapi.LIB_PATH)
    for name in ("pepshost_minsr_step_samples", "pepshost_minsr_step_samples_c128"):
        assert hasattr(lib, name), name
        assert name in hostapi.SYMBOLS, name
    assert callable(hostapi.minsr_step_samples)
