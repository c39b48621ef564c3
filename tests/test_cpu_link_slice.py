"""CPU checks of the link slice's C ABI: pepsgpu_link_exchange_slice, pepsgpu_diag_link_cand and pepsgpu_diag_link_slice_calls are
declared in include/pepsgpu.h, exported by libpepsgpu.so and bound in peps_amd.capi (no compute call is made)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pepsgpu_link_exchange_slice", "pepsgpu_diag_link_cand", "pepsgpu_diag_link_slice_calls")


def test_link_slice_entry_points_declared_exported_and_bound():
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
    # the ctypes signatures: (ctx, orient, slice1, link_mask, val_out), (rows, cols, phys_dim, n, cfg, orient, row1, col1, cand_out,
    # flag_out) and (void) -> long
    bound = capi.load_library()
    assert len(bound.pepsgpu_link_exchange_slice.argtypes) == 5
    assert len(bound.pepsgpu_diag_link_cand.argtypes) == 10
    assert len(bound.pepsgpu_diag_link_slice_calls.argtypes) == 0 and bound.pepsgpu_diag_link_slice_calls.restype is ctypes.c_long
    assert callable(getattr(capi.Context, "link_exchange_slice"))
    assert callable(capi.diag_link_cand) and callable(capi.diag_link_slice_calls)
    # no slice has run in this process, and asking does not need a device
    assert capi.diag_link_slice_calls() == 0


def test_mc_energy_grad_partial_rejects_an_unknown_model():
    """ids outside xxz .. trij1j2 used to run the transverse-field Ising model silently; the refusal comes before any device work"""
    from peps_amd import hostapi, synthetic
    L, D, n = 4, 2, 2
    flat = synthetic.sitps_to_flat(synthetic.make_sitps(L, D, noise=0.5), D)
    cfgs = synthetic.make_configs(L, n, "heisenberg", seed0=13)
    old = dict(hostapi.MODEL_ID)
    hostapi.MODEL_ID["nosuch"] = 5
    try:
        with pytest.raises(ValueError):
            hostapi.mc_energy_grad_partial(flat, cfgs, np.arange(n, dtype=np.uint64), 4, "exchange", "nosuch", (), 0, 0, 1)
    finally:
        hostapi.MODEL_ID.clear()
        hostapi.MODEL_ID.update(old)
