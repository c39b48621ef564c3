"""Kernel-level reference tests of the tensor GEMM (peps_amd/csrc/tgemm.h): every route of tgemm_launch and every descriptor
field the engine sets, through pepsgpu_diag_tgemm_desc, against the float64 / complex128 statement in tests/tgemm_ref.py;
and the three-stage BTen growth chain (tgemm_chain3_kernel) through pepsgpu_diag_tgemm_chain3 against einsum.

Every case names the route it is built to take and asserts it.  Operand elements no live index reaches are NaN (dead rows and
columns, the gaps between batch strides), so a dead element that leaks into a result fails the case; C starts as a finite
sentinel wherever the launch must not store (and below the diagonal of an upper_only launch), so a stray store fails it too.  Each case also runs on integer data in {-3..3}: every sum is then exact, and
the result must be bit-identical to the reference.

Floating data is held elementwise to (16 sqrt(K) u + 2 u_out) (|alpha| |op(A)| |op(B)| + |C0|)_ij, u of the accumulation type
and u_out of the output type: an f32 result of a float64 accumulation is rounded once at the store and once more where C0 is
added."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

if __name__ == "__main__":      # (the vector-ALU subprocess runs this file as a script)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from peps_amd import capi  # noqa: E402
import tgemm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53, np.complex128: 2.0 ** -53}
HIT = set()          # (route, avec, bvec, acc64) seen on the device by this process
TRIED = set()        # GPU steps started by this process (a case name, "refusals", "valu"), whatever their outcome
SENT = -12345.0      # C0 wherever the launch must not store (finite: a stored NaN cannot pass for it)
DIRECT, SK128, SK32, TMFMA, TVALU, REFUSED = (capi.TG_ROUTE_DIRECT, capi.TG_ROUTE_SKINNY_128x32, capi.TG_ROUTE_SKINNY_32x128,
                                              capi.TG_ROUTE_TILED_MFMA, capi.TG_ROUTE_TILED_VALU, capi.TG_ROUTE_REFUSED)


def _layout(first, second):
    """row-major strides over the sub-dims of `first` then `second`; returns (strides of first, of second, elements)."""
    dims = list(first) + list(second)
    st = [0] * 6
    s = 1
    for q in range(5, -1, -1):
        st[q] = s
        s *= dims[q]
    return tuple(st[:3]), tuple(st[3:]), s


def gemm(I, J, K, nbatch, a="ik", b="kj", gapA=0, gapB=0, gapC=0, **kw):
    """A descriptor of contiguous operands: A laid out [I][K] ("ik") or [K][I], B [K][J] ("kj") or [J][K], C [I][J]; the
    batch strides leave gaps of gapA / gapB / gapC elements between the entries."""
    d = dict(I=tuple(I), J=tuple(J), K=tuple(K), nbatch=nbatch)
    if a == "ik":
        d["sAi"], d["sAk"], na = _layout(I, K)
    else:
        d["sAk"], d["sAi"], na = _layout(K, I)
    if b == "kj":
        d["sBk"], d["sBj"], nbb = _layout(K, J)
    else:
        d["sBj"], d["sBk"], nbb = _layout(J, K)
    d["sCi"], d["sCj"], nc = _layout(I, J)
    d["wA"], d["wB"], d["wC"] = na + gapA, nbb + gapB, nc + gapC
    d.update(kw)
    return d


def _footprint(desc, which, b):
    """one past the largest element offset entry b can address in operand `which` over the STATIC extents (a kernel may read
    row / column 0 or a clamped k of any entry: the buffers cover all of it)."""
    g = desc.get
    bA, bB, bC = R.operand_bases(desc, b)
    span = lambda dims, st: sum((d - 1) * s for d, s in zip(dims, st))   # noqa: E731
    if which == "A":
        return bA + span(g("I"), g("sAi")) + span(g("K"), g("sAk")) + 1
    if which == "B":
        return bB + span(g("K"), g("sBk")) + span(g("J"), g("sBj")) + 1
    return bC + span(g("I"), g("sCi")) + span(g("J"), g("sCj")) + 1


def _values(rng, n, dtype, integer):
    if integer:
        v = rng.integers(-3, 4, size=n).astype(np.float64)
        if dtype == np.complex128:
            v = v + 1j * rng.integers(-3, 4, size=n)
    else:
        v = rng.standard_normal(n)
        if dtype == np.complex128:
            v = v + 1j * rng.standard_normal(n)
    return v.astype(dtype)


def build(types, desc, rng, integer, a_off=0, b_off=0, zero_entry=None, inf_entry=None):
    """Operand buffers with live data at the elements some entry reads and NaN elsewhere; C0 the sentinel where nothing is
    stored and below the diagonal of an upper_only launch (random where an accumulating launch reads it)."""
    ta, tb, tc, _ = capi.TG_TYPES[types]
    nb = desc["nbatch"]
    na = max(_footprint(desc, "A", b) for b in range(nb)) + 8     # (+8: the 16-byte loads stay inside the buffer)
    nbb = max(_footprint(desc, "B", b) for b in range(nb)) + 8
    nc = max(_footprint(desc, "C", b) for b in range(nb))
    A = np.full(a_off + na, np.nan, dtype=ta)
    B = np.full(b_off + nbb, np.nan, dtype=tb)
    for b in range(nb):
        ia, ib = R.entry_index_sets(desc, b)
        A[a_off + ia.ravel()] = _values(rng, ia.size, ta, integer)
        B[b_off + ib.ravel()] = _values(rng, ib.size, tb, integer)
    if zero_entry is not None:
        ia, _ = R.entry_index_sets(desc, zero_entry)
        A[a_off + ia.ravel()] = 0
    if inf_entry is not None:
        ia, _ = R.entry_index_sets(desc, inf_entry)
        A[a_off + ia.ravel()[0]] = np.inf
    C0 = np.full(nc, SENT, dtype=tc)
    if desc.get("accumulate"):
        r = R.tgemm_ref(desc, np.nan_to_num(A), np.nan_to_num(B), np.zeros(nc, dtype=tc), a_off, b_off)
        w = r["written"] & ~r["lower"]
        C0[w] = _values(rng, int(w.sum()), tc, integer)
    return A, B, C0


def run_case(types, desc, route, integer, seed=0, a_off=0, b_off=0, scale_in=None, zero_entry=None, inf_entry=None):
    """Launch, then check route, status, every stored and every untouched element, the flop count and the fused norm."""
    rng = np.random.default_rng(seed)
    A, B, C0 = build(types, desc, rng, integer, a_off, b_off, zero_entry, inf_entry)
    nb = desc["nbatch"]
    nl0 = np.linspace(0.5, 1.5, nb)
    out = capi.diag_tgemm_desc(types, desc, A, B, C0, a_off, b_off, scale_in=scale_in, scale_out=np.full(nb, -5.0),
                               norm_log=nl0, norm_flag=np.zeros(nb))
    assert out["status"] == 0, out["error"]
    assert out["route"] == tuple(route), (out["route"], route)
    HIT.add(out["route"])
    ta, tb, tc, tacc = capi.TG_TYPES[types]
    ref = R.tgemm_ref(desc, A, B, C0, a_off, b_off, scale_in)
    got = out["C"]
    untouched = ~ref["written"]
    assert np.array_equal(got[untouched], C0[untouched]), "stores outside the live result"
    w = ref["written"] & ~ref["lower"] & np.isfinite(ref["C"])
    acc64 = route[0] in (SK128, SK32) or (route[0] == DIRECT and route[3]) or tacc != np.float32
    u_acc = 2.0 ** -53 if acc64 else 2.0 ** -24
    u_out = U[tc]
    # (the f32 store of a float64 sum and, accumulating, the f32 addition of C0: two roundings of the output type)
    bound = (16 * np.sqrt(np.maximum(ref["K"], 1)) * u_acc + 2 * u_out) * ref["absprod"]
    if integer:
        assert np.array_equal(got[w], ref["C"][w].astype(tc)), "integer data: not bit-identical (%d of %d elements differ)" % (
            int(np.sum(got[w] != ref["C"][w].astype(tc))), int(w.sum()))
    else:
        err = np.abs(got[w] - ref["C"][w])
        bad = ~(err <= bound[w])
        assert not bad.any(), "%d of %d elements off: worst err %.3e vs bound %.3e" % (
            int(bad.sum()), int(w.sum()), float(err[bad].max()), float(bound[w][bad][np.argmax(err[bad])]))
    low = ref["lower"]
    if low.any():    # below the diagonal of an upper_only launch: untouched or correct
        same = got[low] == C0[low]
        ok = same | (np.abs(got[low] - ref["C"][low]) <= bound[low])
        assert ok.all(), "upper_only: wrong values below the diagonal"
    if nb < 256:
        assert out["flops"] == ref["flops"], (out["flops"], ref["flops"])
    if desc.get("scale_out"):
        so, nl, nf = R.fused_norm_ref(ref["norm"], nl0)
        assert np.array_equal(out["norm_flag"], nf), (out["norm_flag"], nf)
        if integer:     # the stored values are exact, so is the sum of their squares: the same float32(1 / norm)
            np.testing.assert_array_equal(out["scale_out"][nf == 0], so[nf == 0])
        else:           # the norm of the stored f32 values against that of the exact result: a rounding apart
            np.testing.assert_allclose(out["scale_out"][nf == 0], so[nf == 0], rtol=2.0 ** -21, atol=0)
        np.testing.assert_allclose(out["norm_log"], nl, rtol=0, atol=1e-6)
        assert np.all(out["scale_out"][nf == 1] == 1.0)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# The cases.  Each: name -> (types, descriptor builder, expected route, options).
def _direct(avec, bvec, acc64, nb=6):
    """wave-per-tile kernel: per-walker extents 0, 1, full and between within one launch (I static 150 = five 32-row tiles x
    two J tiles: more than four live tiles per entry), masked J, live K, a selector shared by candidate pairs (seldivA 2),
    B shared by candidate pairs (bdivB 2), alpha != 1 with accumulate.  bvec needs B contiguous along k ("jk"), avec A ("ik")
    with K % 4 == 0; a pointer offset of one element turns a vector form off (a_off / b_off)."""
    K2 = 24 if (avec or bvec) else 22
    il = [150, 0, 1, 97, 150, 33][:nb]
    jl = [40, 40, 3, 0, 17, 40][:nb]
    kl = [K2, 5, K2, 1, 9, K2][:nb]
    nslot = 3
    d = gemm((1, 1, 150), (1, 1, 40), (1, 1, K2), nb, a="ik", b="jk", gapB=4 * 9, gapC=13,
             dI2=dict(p=il), dJ2=dict(p=jl, mask=1), dK2=dict(p=kl),
             selA=[2, 0, 1], selA_inc=1, seldivA=2, bdivB=2, alpha=-0.75, accumulate=1, acc64=int(acc64))
    d["selA_mul"], d["wA"] = d["wA"] + 4 * 5, 0
    d["_nslot"] = nslot
    return d, (0 if avec else 1), (0 if bvec else 1)


CASES = {}
for _av in (True, False):
    for _bv in (True, False):
        for _a64 in (False, True):
            _d, _ao, _bo = _direct(_av, _bv, _a64)
            CASES["direct_a%d_b%d_acc%d" % (_av, _bv, _a64)] = (capi.TG_F32, _d, (DIRECT, int(_av), int(_bv), int(_a64)),
                                                               dict(a_off=_ao, b_off=_bo))

# wave-per-tile kernel, three sub-indices per group (masked middle I sub-index, dynI over the flattened I)
CASES["direct_subidx_dynI"] = (capi.TG_F32, gemm((2, 5, 7), (3, 1, 11), (2, 3, 8), 5, a="ik", b="kj", gapA=4, gapC=3,
                                                   dI1=dict(p=[5, 2, 0, 5, 3], mask=1), dJ0=dict(p=[1, 2, 3, 3, 2], div=1),
                                                   dK1=dict(p=[1, 2, 3, 3, 0]), dynI=[70, 9, 70, 33, 1], dynI_mul=1),
                               (DIRECT, 1, 0, 0), {})
# fused normalisation: entry 1 has no live row (zero norm), entry 2 is live but zero, entry 3 holds an infinity
CASES["direct_fused_norm"] = (capi.TG_F32, gemm((1, 1, 70), (1, 1, 36), (1, 1, 16), 5, dI2=dict(p=[70, 0, 40, 70, 3]),
                                                  dJ2=dict(p=[36, 36, 20, 36, 1], mask=1), scale_out=True, norm_log=True,
                                                  norm_flag=True, alpha=0.5),
                              (DIRECT, 1, 0, 0), dict(zero_entry=2, inf_entry=3))
CASES["direct_fused_norm_acc64"] = (capi.TG_F32, dict(CASES["direct_fused_norm"][1], acc64=1), (DIRECT, 1, 0, 1),
                                    dict(zero_entry=2, inf_entry=3))
# scale_in on its own
CASES["direct_scale_in"] = (capi.TG_F32, gemm((1, 1, 45), (1, 1, 33), (1, 1, 12), 4, dK2=dict(p=[12, 7, 0, 12]),
                                                scale_in=True, alpha=1.0),
                            (DIRECT, 1, 0, 0), dict(scale_in=np.array([0.5, 2.0, 3.0, 0.125], dtype=np.float32)))

# tiled 64 x 64 kernel, f32: more than TG_DYN_GRIDX I tiles with a per-walker extent, K beyond one 2048 chunk with dK and dynK,
# batch_flag, B selected through seldivB
_t = gemm((1, 1, 300), (1, 3, 30), (1, 1, 2100), 4, a="ki", b="kj", gapA=7, gapC=5, prefer_tiled=1,
          dI2=dict(p=[300, 0, 257, 65]), dJ2=dict(p=[30, 30, 1, 29]), dK2=dict(p=[2100, 2100, 2049, 3]),
          dynK=[700, 1, 700, 700], dynK_mul=3, batch_flag=[-1, -1, 0, -1])
CASES["tiled_f32"] = (capi.TG_F32, _t, (TMFMA, 0, 0, 0), {})
CASES["tiled_f32_acc64"] = (capi.TG_F32_ACC64, dict(_t, prefer_tiled=0), (TMFMA, 0, 0, 0), {})
# f32 -> f64 (Gram form, upper_only), alpha with accumulate
CASES["tiled_f32_to_f64_upper"] = (capi.TG_F32_TO_F64, gemm((1, 1, 130), (1, 1, 130), (1, 1, 40), 3, a="ki", b="kj",
                                                              upper_only=1, dI2=dict(p=[130, 70, 1], mask=1),
                                                              dJ2=dict(p=[130, 70, 1], mask=1)),
                                   (TMFMA, 0, 0, 0), {})
CASES["tiled_f64"] = (capi.TG_F64, gemm((1, 2, 40), (1, 1, 90), (1, 1, 2200), 4, a="ik", b="kj", gapA=3, gapB=9, gapC=11,
                                        dI1=dict(p=[2, 1, 0, 2]), dK2=dict(p=[2200, 2100, 1, 2049]), alpha=1.5, accumulate=1,
                                        selB=[1, 9, 0, 9, 0, 9, 2], selB_inc=2, seldivB=1, bdivA=2),
                      (TMFMA, 0, 0, 0), {})
CASES["tiled_f64"][1]["selB_mul"], CASES["tiled_f64"][1]["wB"] = CASES["tiled_f64"][1]["wB"], 0
CASES["tiled_f64_upper"] = (capi.TG_F64, gemm((1, 1, 100), (1, 1, 100), (1, 1, 30), 2, a="ki", b="kj", upper_only=1),
                            (TMFMA, 0, 0, 0), {})
CASES["tiled_c128_conj"] = (capi.TG_C128, gemm((1, 1, 70), (1, 1, 66), (1, 2, 20), 3, a="ki", b="kj", conjA=1, conjB=1,
                                               alpha=0.5, accumulate=1, dI2=dict(p=[70, 1, 64]), dK1=dict(p=[2, 1, 0])),
                            (TMFMA, 0, 0, 0), {})
CASES["tiled_c128_upper_conjA"] = (capi.TG_C128, gemm((1, 1, 90), (1, 1, 90), (1, 1, 2100), 2, a="ki", b="kj", conjA=1,
                                                      upper_only=1, dK2=dict(p=[2100, 33])),
                                   (TMFMA, 0, 0, 0), {})

# skinny float64-accumulated kernels: 128 x 32 (J <= 32) and 32 x 128 (I <= 32); K beyond one chunk with dK; dynamic rows
# beyond TG_DYN_GRIDX tiles of 128
CASES["skinny128_f32_acc64"] = (capi.TG_F32_ACC64, gemm((1, 1, 300), (1, 1, 32), (1, 1, 2100), 3, a="ik", b="kj", gapA=5,
                                                        dI2=dict(p=[300, 1, 200]), dK2=dict(p=[2100, 2048, 2049]),
                                                        dJ2=dict(p=[32, 5, 0], mask=1), alpha=-2.0, accumulate=1),
                                (SK128, 0, 0, 0), {})
CASES["skinny128_f32_to_f64"] = (capi.TG_F32_TO_F64, gemm((1, 2, 40), (1, 1, 20), (1, 1, 64), 3, a="ki", b="jk",
                                                          dynI=[80, 3, 0]), (SK128, 0, 0, 0), {})
CASES["skinny128_f64"] = (capi.TG_F64, gemm((1, 1, 129), (1, 1, 2), (1, 1, 33), 2, a="ki", b="kj"), (SK128, 0, 0, 0), {})
CASES["skinny32_f32_acc64"] = (capi.TG_F32_ACC64, gemm((1, 1, 32), (1, 1, 300), (1, 1, 2100), 3, a="ki", b="kj", gapB=3,
                                                       dJ2=dict(p=[300, 129, 1]), dK2=dict(p=[2100, 2100, 2050]),
                                                       dynK=[2100, 17, 2100]),
                               (SK32, 0, 0, 0), {})
CASES["skinny32_f32_to_f64"] = (capi.TG_F32_TO_F64, gemm((1, 1, 20), (1, 1, 200), (1, 1, 48), 2, a="ik", b="kj",
                                                         dI2=dict(p=[20, 7], mask=1), alpha=0.25, accumulate=1),
                                (SK32, 0, 0, 0), {})
CASES["skinny32_f64"] = (capi.TG_F64, gemm((1, 1, 2), (1, 1, 64), (1, 1, 2049), 2, a="ik", b="kj"), (SK32, 0, 0, 0), {})


# ---------------------------------------------------------------------------------------------------------------------------
def _run_named(name, integer):
    TRIED.add(name)
    types, desc, route, opts = CASES[name]
    desc = {k: v for k, v in desc.items() if not k.startswith("_")}
    return run_case(types, desc, route, integer, seed=zlib.crc32(name.encode()) % 1000, **opts)


@pytest.mark.parametrize("integer", [False, True], ids=["float", "int"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_tgemm_case(name, integer):
    _run_named(name, integer)


def test_tgemm_refusals():
    """scale_out with accumulate or batch_flag on the wave-per-tile kernel, and scale_out / scale_in where that kernel is not
    taken, return status 5 (and compute nothing)."""
    TRIED.add("refusals")
    base = gemm((1, 1, 40), (1, 1, 40), (1, 1, 16), 2, dI2=dict(p=[40, 3]), scale_out=True)
    rng = np.random.default_rng(3)
    for types, extra in ((capi.TG_F32, dict(accumulate=1)), (capi.TG_F32, dict(batch_flag=[-1, -1])),
                         (capi.TG_F32, dict(prefer_tiled=1)), (capi.TG_F64, {}), (capi.TG_F32_ACC64, {}),
                         (capi.TG_F32, dict(scale_out=False, scale_in=True, dynK=[16, 16]))):
        d = dict(base, **extra)
        A, B, C0 = build(types, d, rng, True)
        out = capi.diag_tgemm_desc(types, d, A, B, C0)
        assert out["status"] == 5, (extra, out["status"], out["error"])
        assert out["route"][0] == REFUSED
        assert np.array_equal(out["C"], C0)
        HIT.add(out["route"])


VALU_TYPES = {capi.TG_F32: "tiled_f32", capi.TG_F32_ACC64: "skinny128_f32_acc64", capi.TG_F32_TO_F64: "skinny32_f32_to_f64",
              capi.TG_F64: "tiled_f64", capi.TG_C128: "tiled_c128_conj"}


def _valu_main():
    """(subprocess, PEPSGPU_NO_MFMA=1) every element type on the vector-ALU tiling: the tiled cases of f32, f64 and c128,
    and the skinny cases of the two float64-accumulating f32 types (they fall back to it); and the refusal of the fused norm
    on a wave-per-tile descriptor, which has no kernel there.  Prints one JSON line of results."""
    res = {}
    for types, name in sorted(VALU_TYPES.items()):
        for integer in (False, True):
            key = "%s/%s" % (name, "int" if integer else "float")
            t, desc, _, opts = CASES[name]
            try:
                desc = {k: v for k, v in desc.items() if not k.startswith("_")}
                out = run_case(types, desc, (TVALU, 0, 0, 0), integer, seed=7, **opts)
                res[key] = ["ok", list(out["route"])]
            except AssertionError as e:
                res[key] = ["fail", str(e)[:400]]
    d, _, _ = _direct(True, False, False)
    d = {k: v for k, v in d.items() if not k.startswith("_")}
    d = dict(d, accumulate=0, scale_out=True)
    A, B, C0 = build(capi.TG_F32, d, np.random.default_rng(1), True, 0, 1)
    out = capi.diag_tgemm_desc(capi.TG_F32, d, A, B, C0, 0, 1)
    res["refuse_scale_out"] = ["ok" if out["status"] == 5 and np.array_equal(out["C"], C0) else "fail",
                               [out["status"]] + list(out["route"])]
    print(json.dumps(res))


def test_tgemm_valu_routes():
    TRIED.add("valu")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--valu"], env=dict(os.environ, PEPSGPU_NO_MFMA="1"),
                       capture_output=True, text=True, timeout=600, cwd=os.path.dirname(here))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    bad = {k: v for k, v in res.items() if v[0] != "ok"}
    assert not bad, bad
    assert len(res) == 2 * len(VALU_TYPES) + 1
    for k, v in res.items():
        if k != "refuse_scale_out":
            HIT.add(tuple(v[1]))


# ---------------------------------------------------------------------------------------------------------------------------
# tgemm_chain3_kernel: one BTen growth step with the engine's descriptors
def _chain3_ref(dims, site_t, sel, mps1, bten, mps2, live, bound=False):
    """out[b][x,s2,y] over the live extents, zeros beyond (einsum in float64).  bound: also the elementwise error bound of three
    chained f32 contractions, each rounded to f32: 16 (sqrt(K1) + sqrt(K2) + sqrt(K3) + 3) u |mps1| |bten| |site| |mps2|, with
    K1 = c, K2 = p1 b1, K3 = b2 s1 over the live bonds."""
    x, p1, c, b1, b2, s1, s2, y = dims
    nb = mps1.shape[0]
    out = np.zeros((nb, x, s2, y))
    bnd = np.zeros((nb, x, s2, y))
    for b in range(nb):
        vx, vc, vb, vy = live[b] if live is not None else (x, c, b2, y)
        m1 = mps1[b][:vx, :, :vc].astype(np.float64)
        bt = bten[b][:vc, :, :vb].astype(np.float64)
        st = site_t[sel[b]][:, :, :, :].astype(np.float64)
        m2 = mps2[b][:vb, :, :vy].astype(np.float64)
        out[b, :vx, :, :vy] = np.einsum("xpc,cab,pasd,bsy->xdy", m1, bt, st, m2, optimize=True)
        if bound:
            a = np.einsum("xpc,cab,pasd,bsy->xdy", abs(m1), abs(bt), abs(st), abs(m2), optimize=True)
            bnd[b, :vx, :, :vy] = 16 * (np.sqrt(vc) + np.sqrt(p1 * b1) + np.sqrt(vb * s1) + 3) * 2.0 ** -24 * a
    return (out, bnd) if bound else out


def _chain3_case(dims, live, perm=(0, 1, 2, 3), skip=None, offs=(0, 0, 0), seed=0, integer=False, nb=None):
    """perm: the order of the site legs (p1, b1, s1, s2) in memory (the site strides of the engine follow the site's own leg
    order).  Dead parts of every operand (beyond the live bonds) are NaN."""
    x, p1, c, b1, b2, s1, s2, y = dims
    nb = nb or len(live)
    rng = np.random.default_rng(seed)
    val = (lambda *s: rng.integers(-3, 4, size=s).astype(np.float32)) if integer else (lambda *s: rng.standard_normal(s).astype(np.float32))
    lv = live if live is not None else [(x, c, b2, y)] * nb
    mps1 = np.full((nb, x, p1, c), np.nan, np.float32)
    bten = np.full((nb, c, b1, b2), np.nan, np.float32)
    mps2 = np.full((nb, b2, s1, y), np.nan, np.float32)
    for b, (vx, vc, vb, vy) in enumerate(lv):
        mps1[b, :vx, :, :vc] = val(vx, p1, vc)
        bten[b, :vc, :, :vb] = val(vc, b1, vb)
        mps2[b, :vb, :, :vy] = val(vb, s1, vy)
    nslot = 3
    legs = (p1, b1, s1, s2)
    shape_mem = tuple(legs[q] for q in perm)
    site_t = val(nslot, *shape_mem)                                  # memory order
    inv = np.argsort(perm)
    site_logical = np.transpose(site_t, (0,) + tuple(1 + int(q) for q in inv))   # -> [slot][p1][b1][s1][s2]
    strides_mem = [int(np.prod(shape_mem[q + 1:])) for q in range(4)]
    strides = [strides_mem[int(inv[q])] for q in range(4)]
    slot = int(np.prod(legs)) + 4
    store = np.full(offs[2] + slot * nslot, np.nan, np.float32)
    for q in range(nslot):
        store[offs[2] + q * slot: offs[2] + q * slot + int(np.prod(legs))] = site_t[q].ravel()
    sel = np.array([(2 * b + 1) % nslot for b in range(nb)], np.int32)
    out0 = np.full((nb, x, s2, y), -7.0, np.float32)
    pad = lambda a, o: np.concatenate([np.full(o, np.nan, np.float32), a.ravel()])   # noqa: E731
    out, flags, launched, variant = capi.diag_tgemm_chain3(dims, strides, store, slot, sel, 1, pad(mps1, offs[0]), pad(bten, offs[1]),
                                                           mps2, out0, live=live, skip=skip, offs=offs)
    ref, bnd = _chain3_ref(dims, site_logical, sel, mps1, bten, mps2, live, bound=True)
    return out, out0, (ref, bnd), flags, launched, variant


def _chain3_check(out, refb, integer):
    ref, bnd = refb
    if integer:
        assert np.array_equal(out, ref.astype(np.float32))
    else:
        err = np.abs(out - ref)
        assert np.all(err <= bnd), "%d elements off, worst err %.3e" % (int(np.sum(~(err <= bnd))), float(np.nanmax(err)))


@pytest.mark.parametrize("integer", [False, True], ids=["float", "int"])
@pytest.mark.parametrize("dims,chunks", [((8, 2, 8, 2, 8, 2, 2, 8), 1), ((30, 4, 8, 4, 16, 2, 2, 12), 2),
                                         ((40, 4, 8, 4, 16, 2, 2, 12), 3), ((30, 2, 7, 3, 9, 3, 2, 5), 1)])
def test_chain3_chunks(dims, chunks, integer):
    """x walked in 1, 2 and 3 chunks of the 4096-float buffers (per value of x: p1 b1 b2 floats of tmp1, s1 s2 b2 of tmp2),
    live bonds that differ per entry, a selector, NaN beyond the live bonds."""
    x, p1, c, b1, b2, s1, s2, y = dims
    per = max(p1 * b1 * b2, s1 * s2 * b2)
    assert -(-x // (4096 // per)) == chunks
    live = [(x, c, b2, y), (x - 3, c - 1, b2, 1), (1, 1, 1, y), (x // 2, c, b2 - 2, y - 1)]
    out, out0, ref, flags, launched, _ = _chain3_case(dims, live, integer=integer, seed=chunks)
    assert launched == 2
    assert np.all(flags == 0)
    _chain3_check(out, ref, integer)
    # beyond the live x and y: zeros (the new BTen is written in full)
    for b, (vx, _, _, vy) in enumerate(live):
        assert np.all(out[b, vx:] == 0) and np.all(out[b, :, :, vy:] == 0)


@pytest.mark.parametrize("variant", [(1, 0, 1), (1, 0, 0), (0, 0, 1), (0, 0, 0)])
def test_chain3_alignment_variants(variant):
    """(avec1, bvec1, avec2) of the launch.  With bten_step's descriptors B1 = bten[c, b1, b2] has k stride b1 b2 > 1, so bvec1
    is never taken (the launcher's own condition; asserted here): these are the four variants the engine can reach.  avec1 is
    turned off by a one-element offset of mps1; avec2 is on when the site's b1 leg is contiguous (b1 % 4 == 0)."""
    avec1, _, avec2 = variant
    # avec2 needs the site's b1 leg at stride 1 (perm puts b1 last) with b1 % 4 == 0, p1 / s1 / s2 strides % 4 == 0 and slot % 4 == 0
    dims = (12, 2, 8, 4, 8, 2, 2, 6)
    perm = (0, 2, 3, 1) if avec2 else (0, 1, 2, 3)
    live = [(12, 8, 8, 6), (5, 3, 7, 2), (12, 8, 1, 6)]
    for integer in (False, True):
        out, _, ref, flags, launched, got = _chain3_case(dims, live, perm=perm, offs=(0 if avec1 else 1, 0, 0), integer=integer, seed=5)
        assert launched == 2 and got == variant, (got, variant)
        _chain3_check(out, ref, integer)


def test_chain3_skip_declined_and_zero_live():
    """skip entries stay untouched; shapes the launcher declines return 0 and write nothing; an entry with a live bond of 0
    (the environment of a configuration of zero amplitude: BMPSDev::live counts the non-zero states of a bond, and the
    truncation counts none for a zero matrix) gets a zero result written in full, like any entry."""
    dims = (8, 2, 8, 2, 8, 2, 2, 8)
    live = [(8, 8, 8, 8), (0, 8, 8, 8), (8, 8, 0, 8), (8, 0, 8, 8), (8, 8, 8, 0), (3, 2, 5, 4)]
    skip = np.array([0, 0, 0, 0, 0, 1], np.int32)
    out, out0, (ref, _), flags, launched, _ = _chain3_case(dims, live, skip=skip, integer=True)
    assert launched == 2
    assert np.array_equal(out[5], out0[5]), "skipped entry written"
    assert np.array_equal(out[:5], ref[:5].astype(np.float32)), "entries %s differ" % [
        b for b in range(5) if not np.array_equal(out[b], ref[b])]
    assert np.all(flags[:5] == 0), flags
    # declined by the static shapes: per value of x, p1 b1 b2 = 4 * 32 * 40 floats > 4096
    out, out0, _, flags, launched, _ = _chain3_case((4, 4, 2, 32, 40, 1, 1, 2), [(4, 2, 40, 2)] * 2)
    assert launched == 0
    assert np.array_equal(out, out0) and np.all(flags == 7)


def _zero_site_state(L, D):
    """the synthetic state with the tensor of physical state 1 at site (1, 2) set to zero: every configuration with that site
    in state 1 has amplitude exactly 0, and so has the boundary MPS of every row below it for such a walker"""
    from peps_amd import synthetic
    sitps = synthetic.make_sitps(L, D)
    sitps[1][2][1] = np.zeros_like(sitps[1][2][1])
    return sitps


def _row_traces(ctx, row):
    """amplitude of every walker through the BTens of `row` (grown from the right, f32: the three-stage chained BTen step),
    read at its first two columns"""
    from oracle.bmps import LEFT, RIGHT, HORIZONTAL
    ctx.grow_bmps_for_row(row)
    ctx.init_bten(LEFT, row)
    ctx.grow_full_bten(RIGHT, row, 2, True)
    t0 = ctx.trace(row, 0, HORIZONTAL)
    ctx.shift_bten_window(RIGHT)
    return t0, ctx.trace(row, 1, HORIZONTAL)


def test_engine_zero_amplitude_walkers_through_the_bten_chain():
    """Engine-level regression of the zero-live-bond entry of tgemm_chain3_kernel: walkers whose configuration has amplitude
    exactly 0 (their boundary MPS above row 2 is zero, so its live bonds count 0 states) share a batch with live walkers.
    The BTen growth of row 2 runs the three-stage chained step on all of them; their traces must be exactly 0 and the others
    the oracle's amplitudes.  The batch first runs with every walker live, so the memory a declined entry would leave
    behind holds environment tensors of live walkers."""
    from oracle import vmc
    from oracle.bmps import BMPSTruncateParams
    from peps_amd import synthetic
    L, D, chi, n = 6, 3, 9, 6
    sitps = _zero_site_state(L, D)
    cfgs = np.ascontiguousarray(synthetic.make_configs(L, n, "heisenberg"), dtype=np.int32)
    live = cfgs.copy()
    live[:, 1, 2] = 0
    dead = cfgs.copy()
    dead[:, 1, 2] = [1, 0, 1, 1, 0, 1]
    ctx = capi.Context(L, L, D, 2, chi, dtype=capi.F32, max_walkers=n)
    ctx.state_upload(synthetic.sitps_to_flat(sitps, D, np.float64))
    tp = BMPSTruncateParams.SVD(chi, chi, 0.0)
    for cf in (live, dead):
        ctx.set_configs(cf)
        t0, t1 = _row_traces(ctx, 2)
        # (the oracle, like the reference, refuses a boundary MPS with an exactly zero tensor: the zero amplitudes are known)
        zero = cf[:, 1, 2] == 1
        ref = np.array([0.0 if z else vmc.TPSWaveFunctionComponent(sitps, c, tp).amplitude for c, z in zip(cf, zero)])
        for t in (t0, t1):
            assert np.all(np.isfinite(t)), t
            assert np.all(t[zero] == 0), (t, zero)
            assert np.all(np.abs(t[~zero] / ref[~zero] - 1) < 1e-5), (t, ref)


def test_route_coverage():
    """Every route this build reaches was taken on the device: the direct kernel in all (avec, bvec, acc64) forms, both skinny
    forms, the tiled kernel on the matrix cores and on the vector ALUs, and the refusal.  A step this process never started
    (a run of this test alone) is run here; a step that was started and did not record its route has failed already and is
    not started again."""
    need = {(DIRECT, a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    need |= {(SK128, 0, 0, 0), (SK32, 0, 0, 0), (TMFMA, 0, 0, 0), (TVALU, 0, 0, 0)}
    if "refusals" not in TRIED:
        test_tgemm_refusals()
    if "valu" not in TRIED:
        test_tgemm_valu_routes()
    for name, (_, _, route, _) in sorted(CASES.items()):
        if tuple(route) not in HIT and name not in TRIED:
            _run_named(name, True)
    missing = need - HIT
    assert not missing, missing
    assert any(h[0] == REFUSED for h in HIT)


if __name__ == "__main__" and "--valu" in sys.argv:
    _valu_main()
