"""CPU checks of the walker slice's C ABI: pepsgpu_walker_set_mpo_excited, pepsgpu_walker_trace_slice and
pepsgpu_diag_walker_slice_calls are declared in include/pepsgpu.h, exported by libpepsgpu.so and bound in peps_amd.capi (no compute
call is made)."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pepsgpu_walker_set_mpo_excited", "pepsgpu_walker_trace_slice", "pepsgpu_diag_walker_slice_calls")


def test_walker_slice_entry_points_declared_exported_and_bound():
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
    # the ctypes signatures: (ctx, walker, num, col, state_map, open_out), (ctx, walker, opp_level, site_map, walker_mask, out) and
    # (void) -> long
    bound = capi.load_library()
    assert len(bound.pepsgpu_walker_set_mpo_excited.argtypes) == 6
    assert len(bound.pepsgpu_walker_trace_slice.argtypes) == 6
    assert len(bound.pepsgpu_diag_walker_slice_calls.argtypes) == 0 and bound.pepsgpu_diag_walker_slice_calls.restype is ctypes.c_long
    assert callable(getattr(capi.Walker, "set_mpo_excited")) and callable(getattr(capi.Walker, "trace_slice"))
    assert callable(capi.diag_walker_slice_calls)
    # no slice has run in a fresh process, and asking does not need a device
    code = "import sys; sys.path.insert(0, sys.argv[1]); from peps_amd import capi; print(capi.diag_walker_slice_calls())"
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "0"
