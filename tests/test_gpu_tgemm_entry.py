"""The entry of the wave-per-tile tensor-GEMM kernels (peps_amd/csrc/tgemm.h, tg_entry_addr / tg_entry_fetch / tg_entry_arrive):
every per-entry word -- nine live extents, dynI, the selectors, batch_flag, scale_in -- is fetched as one batch of
unconditional loads, unset slots read a neutral word, and the quotients b / div are formed once per distinct divisor (not at
all when every divisor is 1).  The cases are those where such a prologue can go wrong; each runs through
pepsgpu_diag_tgemm_desc against tests/tgemm_ref.py with the checks of test_gpu_tgemm.run_case (route, every stored and every
untouched element, flop count), on integer data (bit-identical) and on float data (that file's bound).

Shapes: sub-dims of 2..5, I = 30 rows and J = 40 columns at most (two 32 x 32 tiles per entry)."""
import numpy as np
import pytest

from peps_amd import capi
from test_gpu_tgemm import DIRECT, _chain3_case, _chain3_check, gemm, run_case

pytestmark = pytest.mark.gpu

I3, J3, K3 = (2, 3, 5), (2, 4, 5), (2, 3, 4)
DIMS = dict(dI0=2, dI1=3, dI2=5, dJ0=2, dJ1=4, dJ2=5, dK0=2, dK1=3, dK2=4)
NB = 6


def _p(n, nb=NB):
    """live values of a sub-index of static size n: full, 1, between, full, and again"""
    return [n, 1, max(1, n - 1), n, max(1, n // 2), 1][:nb]


CASES = {}
# each of the nine slots the only one set
for _k, _n in DIMS.items():
    CASES["only_" + _k] = (gemm(I3, J3, K3, NB, **{_k: dict(p=_p(_n))}), {})
# all nine set (a masked I and a masked J among them); none set (dynI alone sends the launch to this kernel)
CASES["all_nine"] = (gemm(I3, J3, K3, NB, **{k: dict(p=_p(n)[::-1] if k[1] == "J" else _p(n), mask=int(k in ("dI1", "dJ0")))
                                             for k, n in DIMS.items()}), {})
CASES["none_set"] = (gemm(I3, J3, K3, NB, dynI=[30] * NB), {})
# mask 0 and 1 on I and J slots, with extents of 0 among them (mask 0: nothing stored, the sentinel stays; mask 1: zeros)
for _m in (0, 1):
    CASES["mask%d_I_J" % _m] = (gemm(I3, J3, K3, NB, dI1=dict(p=[3, 0, 2, 1, 3, 0], mask=_m), dJ2=dict(p=[5, 5, 0, 3, 1, 0], mask=_m)), {})
CASES["extent_0"] = (gemm(I3, J3, K3, NB, dI2=dict(p=[5, 0, 5, 5, 2, 5]), dJ1=dict(p=[4, 4, 0, 4, 4, 1]), dK2=dict(p=[4, 4, 4, 0, 1, 4])), {})
# stored values above the static dim (clamped) and below zero (an extent of 0)
CASES["clamped_above"] = (gemm(I3, J3, K3, NB, dI2=dict(p=[8, 5, 100, 6, 2, 7]), dJ2=dict(p=[6, 2 ** 20, 3, 9, 5, 1], mask=1),
                               dK1=dict(p=[3, 4, 1, 50, 2, 7])), {})
CASES["negative"] = (gemm(I3, J3, K3, NB, dI2=dict(p=[5, -1, 3, -(2 ** 20), 2, 5]), dJ2=dict(p=[-2, 5, 5, 3, -7, 1], mask=1),
                          dK2=dict(p=[4, 4, -1, 2, 4, 4])), {})
CASES["mul"] = (gemm(I3, J3, K3, NB, dI2=dict(p=[1, 2, 0, 3, 2, 1], mul=2), dJ1=dict(p=[1, 2, 1, 0, 2, 1], mul=3),
                     dK2=dict(p=[2, 1, 1, 2, 0, 3], mul=2)), {})
# div = 3 with six entries: 0-2 and 3-5 share their extents; two different divisors in one descriptor
CASES["div3"] = (gemm(I3, J3, K3, NB, dI2=dict(p=[5, 2], div=3), dK2=dict(p=[4, 1], div=3), dJ2=dict(p=[3, 5], div=3, mask=1)), {})
CASES["div3_div2"] = (gemm(I3, J3, K3, NB, dI2=dict(p=[5, 2], div=3), dJ2=dict(p=[5, 1, 3], div=2), dK1=dict(p=_p(3))), {})
CASES["dynI_mul"] = (gemm(I3, J3, K3, NB, dynI=[5, 2, 0, 10, 7, 3], dynI_mul=3, dJ2=dict(p=_p(5))), {})
# a selector shared by candidate pairs together with a B operand shared by pairs
_d = gemm(I3, J3, K3, NB, dI2=dict(p=_p(5)), selA=[2, 0, 1], selA_inc=1, seldivA=2, bdivB=2)
_d["selA_mul"], _d["wA"] = _d["wA"] + 4 * 3, 0
CASES["selA_seldiv2_bdivB2"] = (_d, {})
CASES["batch_flag"] = (gemm(I3, J3, K3, NB, dI2=dict(p=_p(5)), dK2=dict(p=_p(4)), batch_flag=[-1, 0, -1, 7, -1, -1]), {})
CASES["scale_in"] = (gemm(I3, J3, K3, NB, dK2=dict(p=_p(4)), scale_in=True),
                     dict(scale_in=np.array([0.5, 2.0, 4.0, 0.125, 1.0, 0.25], dtype=np.float32)))
# 320 entries: the flop counter samples every 64th entry (flop_stride 64)
CASES["nbatch_320"] = (gemm((1, 2, 5), (1, 1, 6), (1, 2, 4), 320, dI2=dict(p=[b % 6 for b in range(320)]),
                            dK2=dict(p=[1 + b % 4 for b in range(320)])), {})


@pytest.mark.parametrize("integer", [False, True], ids=["float", "int"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_case(name, integer):
    desc, opts = CASES[name]
    route = capi.diag_tgemm_route(capi.TG_F32, desc)
    assert route[0] == DIRECT, route        # every case is built for the wave-per-tile kernel
    run_case(capi.TG_F32, desc, route, integer, seed=sum(name.encode()) % 1000, **opts)


def test_entry_three_divisors_refused():
    """the kernels share at most two quotients: a third distinct divisor is an error of the launch, not a wrong result"""
    desc = gemm(I3, J3, K3, NB, dI2=dict(p=[5, 2], div=3), dJ2=dict(p=[5, 1, 3], div=2), bdivB=6)
    rng = np.random.default_rng(1)
    from test_gpu_tgemm import build
    A, B, C0 = build(capi.TG_F32, desc, rng, True)
    out = capi.diag_tgemm_desc(capi.TG_F32, desc, A, B, C0)
    assert out["status"] != 0 and "divisors" in out["error"], (out["status"], out["error"])
    assert np.array_equal(out["C"], C0)


@pytest.mark.parametrize("integer", [False, True], ids=["float", "int"])
def test_entry_chain2(integer):
    """tgemm_chain_kernel: both descriptors' words in one batch; live extents that differ between the entries, one of them 0
    (nothing stored for that entry)."""
    nb, m, l, a, p, a2, l2, u = 5, 5, 2, 4, 2, 5, 2, 3
    rng = np.random.default_rng(11)
    val = (lambda *s: rng.integers(-3, 4, size=s)) if integer else (lambda *s: rng.standard_normal(s))
    Rr, A, W = (val(nb, m, l, a).astype(np.float32), val(nb, a, p, a2).astype(np.float32), val(nb, l, p, l2, u).astype(np.float32))
    live = np.array([(5, 4, 5), (3, 2, 5), (0, 4, 4), (5, 1, 2), (1, 4, 1)])
    P, fl = capi.diag_tgemm_chain(Rr, A, W, live)
    assert np.all(fl == 0), fl
    for b in range(nb):
        ml, al, a2l = (int(x) for x in live[b])
        X = np.einsum("mla,apc->mlpc", Rr[b, :ml, :, :al].astype(np.float64), A[b, :al, :, :a2l].astype(np.float64))
        want = np.einsum("mlpc,lpqu->muqc", X, W[b].astype(np.float64))
        got = P[b, :ml, :, :, :a2l]
        if integer:
            assert np.array_equal(got, want.astype(np.float32)), b
        else:   # two chained f32 contractions, the first rounded to f32: 16 (sqrt(K1) + sqrt(K2) + 2) u |R| |A| |W|
            # elementwise, K1 = the live a, K2 = l p (the form of the chain3 bound of test_gpu_tgemm.py)
            absX = np.einsum("mla,apc->mlpc", abs(Rr[b, :ml, :, :al]).astype(np.float64), abs(A[b, :al, :, :a2l]).astype(np.float64))
            bnd = 16 * (np.sqrt(al) + np.sqrt(l * p) + 2) * 2.0 ** -24 * np.einsum("mlpc,lpqu->muqc", absX, abs(W[b]).astype(np.float64))
            assert np.all(np.abs(got - want) <= bnd), b
        # beyond the live rows and columns nothing is stored
        assert not np.any(P[b, ml:]) and not np.any(P[b, :, :, :, a2l:]), b


@pytest.mark.parametrize("integer", [False, True], ids=["float", "int"])
def test_entry_chain3(integer):
    """tgemm_chain3_kernel: the words of three descriptors in one batch; one entry with a live extent of 0 (its result is
    written as zeros in full)."""
    dims = (5, 2, 4, 2, 5, 2, 2, 4)
    x, p1, c, b1, b2, s1, s2, y = dims
    live = [(x, c, b2, y), (x - 2, c - 1, b2, 1), (0, c, b2, y), (2, 1, b2 - 3, y - 1)]
    out, out0, ref, flags, launched, _ = _chain3_case(dims, live, integer=integer, seed=5)
    assert launched == 2
    assert np.all(flags == 0)
    _chain3_check(out, ref, integer)
    assert np.all(out[2] == 0)
    for b, (vx, _, _, vy) in enumerate(live):
        assert np.all(out[b, vx:] == 0) and np.all(out[b, :, :, vy:] == 0)
