"""CPU checks of the tensor-GEMM test entries: pepsgpu_diag_tgemm_desc, pepsgpu_diag_tgemm_route and pepsgpu_diag_tgemm_chain3
are declared in include/pepsgpu.h, exported by libpepsgpu.so and bound in peps_amd.capi; and the route table -- which kernel
tgemm_launch takes for every case of tests/test_gpu_tgemm.py -- through the route query, which touches no device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pepsgpu_diag_tgemm_desc", "pepsgpu_diag_tgemm_route", "pepsgpu_diag_tgemm_chain3")


def _lib_path():
    from peps_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return capi.LIB_PATH


def test_tgemm_entry_points_declared_exported_and_bound():
    from peps_amd import capi
    path = _lib_path()
    header = open(os.path.join(ROOT, "include", "pepsgpu.h")).read()
    declared = set(re.findall(r"\b(pepsgpu_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(path)
    for name in NEW + ("pepsgpu_diag_tgemm",):
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
    bound = capi.load_library()
    assert len(bound.pepsgpu_diag_tgemm_desc.argtypes) == 23
    assert len(bound.pepsgpu_diag_tgemm_route.argtypes) == 10
    assert len(bound.pepsgpu_diag_tgemm_chain3.argtypes) == 18
    for f in ("diag_tgemm_desc", "diag_tgemm_route", "diag_tgemm_chain3", "tgemm_desc_arrays"):
        assert callable(getattr(capi, f)), f


def _cases():
    import test_gpu_tgemm as T
    return T


@pytest.mark.parametrize("name", sorted(_cases().CASES))
def test_route_table(name):
    """The route each GPU case asserts is the route the launcher computes for it (the operands at an aligned base advanced
    by the case's element offsets)."""
    _lib_path()
    from peps_amd import capi
    T = _cases()
    types, desc, route, opts = T.CASES[name]
    desc = {k: v for k, v in desc.items() if not k.startswith("_")}
    assert capi.diag_tgemm_route(types, desc, opts.get("a_off", 0), opts.get("b_off", 0)) == tuple(route)


def test_route_rules():
    """The selection rules around the cases: a one-element offset turns a 16-byte form off, dynK and prefer_tiled leave the
    wave-per-tile kernel, upper_only leaves the skinny kernels, the fused norm is refused off the wave-per-tile kernel and with
    accumulate or batch_flag on it, a static extent 0 launches nothing, more than 65535 entries are refused."""
    _lib_path()
    from peps_amd import capi
    T = _cases()
    d = T.gemm((1, 1, 40), (1, 1, 40), (1, 1, 16), 2, a="ik", b="jk", dI2=dict(p=[40, 3]))
    q = capi.diag_tgemm_route
    assert q(capi.TG_F32, d) == (T.DIRECT, 1, 1, 0)
    assert q(capi.TG_F32, d, 1, 0) == (T.DIRECT, 0, 1, 0)
    assert q(capi.TG_F32, d, 0, 2) == (T.DIRECT, 1, 0, 0)
    assert q(capi.TG_F32, d, 4, 4) == (T.DIRECT, 1, 1, 0)
    assert q(capi.TG_F32, dict(d, acc64=1)) == (T.DIRECT, 1, 1, 1)
    assert q(capi.TG_F32, dict(d, dynK=[16, 16])) == (T.TMFMA, 0, 0, 0)
    assert q(capi.TG_F32, dict(d, prefer_tiled=1)) == (T.TMFMA, 0, 0, 0)
    assert q(capi.TG_F32, dict(d, dI2=None)) == (T.TMFMA, 0, 0, 0)      # no per-walker extent: the tiled kernel
    assert q(capi.TG_F32, dict(d, scale_out=True))[0] == T.DIRECT
    for extra in (dict(accumulate=1), dict(batch_flag=[-1, -1]), dict(prefer_tiled=1)):
        assert q(capi.TG_F32, dict(d, scale_out=True, **extra))[0] == T.REFUSED, extra
    assert q(capi.TG_F64, dict(d, scale_in=True))[0] == T.REFUSED
    assert q(capi.TG_F32, dict(d, I=(1, 1, 0)))[0] == capi.TG_ROUTE_EMPTY
    assert q(capi.TG_F32, dict(d, nbatch=65536))[0] == T.REFUSED
    sk = T.gemm((1, 1, 200), (1, 1, 32), (1, 1, 16), 1)
    assert q(capi.TG_F32_ACC64, sk)[0] == T.SK128
    assert q(capi.TG_F32_ACC64, dict(sk, upper_only=1))[0] == T.TMFMA
    assert q(capi.TG_F32_ACC64, dict(sk, J=(1, 1, 33)))[0] == T.TMFMA
    assert q(capi.TG_F64, T.gemm((1, 1, 32), (1, 1, 64), (1, 1, 16), 1))[0] == T.SK32
    assert q(capi.TG_F64, T.gemm((1, 1, 32), (1, 1, 63), (1, 1, 16), 1))[0] == T.TMFMA
    assert q(capi.TG_C128, sk)[0] == T.TMFMA
