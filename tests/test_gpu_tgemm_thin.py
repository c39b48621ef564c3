"""The wave-per-tile tensor GEMM without the work its result does not need (peps_amd/csrc/tgemm.h, TG_THIN_*): columns of
M = R Tt enumerated in the memory order of Tt and its tiles stored through LDS (the m_*_new cases, three and two column tiles,
the second with columns beyond J), dead tiles and dead MFMA steps left out, the small shared B operand of Y = Tt V^T staged
in LDS.  test_every_tile_once covers no code of these items: it pins the unchanged walk of four waves over more tiles than
waves (an accumulating launch, every tile exactly once) that a tile-to-wave rotation would have touched.

None of it may change a stored bit: every case runs in two fresh child processes, one with PEPSGPU_TGEMM_THIN=0 (the kernels
without any of it) and one with the variable unset, and the results are compared byte for byte (np.array_equal on the raw
views); each is also held to the float64 statement in tests/tgemm_ref.py at the elementwise bound of
tests/test_gpu_tgemm.py, (16 sqrt(K) u + 2 u) (|alpha| |A| |B| + |C0|)_ij with u = 2^-24.

Operand elements no live index reaches are NaN, C starts as a finite sentinel (random where an accumulating launch reads it).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":      # (the child processes run this file as a script)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
from peps_amd import capi  # noqa: E402
import tgemm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = -12345.0
U32 = 2.0 ** -24
DIRECT = capi.TG_ROUTE_DIRECT
PARTIAL_K2 = [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16]


# ---------------------------------------------------------------------------------------------------------------------------
# descriptors
def desc_m(u, k2_outer):
    """M[m,(u,k2)] = sum_{(l,a)} R[m,(l,a)] Tt[l,a,k2,u] as desc_m builds it under tsw: l = 2, a = 8, m = 8, k2 = 12, six
    entries; columns enumerated (u, k2) (k2_outer = False) or (k2, u)."""
    l, a, m, k2 = 2, 8, 8, 12
    la, uk = l * a, u * k2
    live_m = [0, 1, 5, 8, 8, 5]
    live_a = [1, 4, 5, 8, 5, 8]
    live_k2 = [12, 0, 3, 8, 12, 3]
    d = dict(I=(1, 1, m), sAi=(0, 0, la), sCi=(0, 0, uk), K=(1, l, a), sAk=(0, a, 1), sBk=(0, a * uk, uk), nbatch=6,
             wA=m * la, wB=la * uk, wC=m * uk + 5, dynI=live_m, dK2=dict(p=live_a))
    if k2_outer:
        d.update(J=(1, k2, u), sBj=(0, u, 1), sCj=(0, 1, k2), dJ1=dict(p=live_k2, mask=1))
    else:
        d.update(J=(1, u, k2), sBj=(0, 1, u), sCj=(0, k2, 1), dJ2=dict(p=live_k2, mask=1))
    return d


def desc_partial(vec_a):
    """one 32 x 32 tile, K = (2, 16) with the live k2 of PARTIAL_K2, A contiguous along k2 (16-byte loads) or along i"""
    I, J, K1, K2 = 20, 24, 2, 16
    nb = len(PARTIAL_K2)
    d = dict(I=(1, 1, I), J=(1, 1, J), K=(1, K1, K2), sBk=(0, K2 * J, J), sBj=(0, 0, 1), sCi=(0, 0, J), sCj=(0, 0, 1), nbatch=nb,
             wA=I * K1 * K2, wB=K1 * K2 * J, wC=I * J, dK2=dict(p=PARTIAL_K2), alpha=0.5)
    if vec_a:
        d.update(sAi=(0, 0, K1 * K2), sAk=(0, K2, 1))
    else:
        d.update(sAi=(0, 0, 1), sAk=(0, K2 * I, I))
    return d


def desc_y(k, k2, live_k, live_k2, live_a):
    """Y[(l,a),q] = sum_{(k2,u)} Tt[l,a,k2,u] V[q,u,k2] as desc_y builds it under tsw, with the fused norm: l = 2, a = 8
    (rows beyond the live a written as zeros), u = 8, K = (k2 live, u), k rows of V (columns beyond the live k: zeros)."""
    l, a, u = 2, 8, 8
    uk = u * k2
    nb = len(live_k)
    return dict(I=(1, l, a), sAi=(0, a * uk, uk), sCi=(0, a * k, k), K=(1, k2, u), sAk=(0, u, 1), sBk=(0, 1, k2),
                J=(1, 1, k), sBj=(0, 0, uk), sCj=(0, 0, 1), nbatch=nb, wA=l * a * uk, wB=k * uk, wC=l * a * k + 3,
                dI2=dict(p=live_a, mask=1), dK1=dict(p=live_k2), dJ2=dict(p=live_k, mask=1),
                scale_in=True, scale_out=True, norm_log=True, norm_flag=True)


def desc_rot(ntj):
    """one row tile, ntj column tiles, nine entries, accumulating (a tile computed twice would be added twice)"""
    I, J, K = 20, 32 * ntj, 8
    return dict(I=(1, 1, I), J=(1, 1, J), K=(1, 1, K), sAi=(0, 0, K), sAk=(0, 0, 1), sBk=(0, 0, J), sBj=(0, 0, 1), sCi=(0, 0, J),
                sCj=(0, 0, 1), nbatch=9, wA=I * K, wB=K * J, wC=I * J + 7, dI2=dict(p=[20, 1, 20, 7, 20, 20, 13, 20, 20]),
                accumulate=1)


def kernel_cases():
    """name -> (descriptor, descriptor the operands are laid out by, seed)"""
    c = {}
    for u in (4, 8):
        c["m_u%d_old" % u] = (desc_m(u, False), desc_m(u, False), 10 + u)
        c["m_u%d_new" % u] = (desc_m(u, True), desc_m(u, False), 10 + u)      # the same operands, the other enumeration
    for v in (1, 0):
        c["partial_avec%d" % v] = (desc_partial(bool(v)),) * 2 + (20 + v,)
    for k in (8, 20):
        d = desc_y(k, 12, [0, 1, 5, k], [12, 5, 9, 1], [8, 3, 5, 8])
        c["y_k%d" % k] = (d, d, 30 + k)
    d = desc_y(32, 32, [32, 20], [32, 10], [8, 5])          # V above the LDS buffer: global loads
    c["y_above_cap"] = (d, d, 40)
    for ntj in (4, 7):
        d = desc_rot(ntj)
        c["rot_%d" % ntj] = (d, d, 50 + ntj)
    return c


def _footprint(desc, which, b):
    g = desc.get
    bA, bB, bC = R.operand_bases(desc, b)
    span = lambda dims, st: sum((d - 1) * s for d, s in zip(dims, st))   # noqa: E731
    if which == "A":
        return bA + span(g("I"), g("sAi")) + span(g("K"), g("sAk")) + 1
    if which == "B":
        return bB + span(g("K"), g("sBk")) + span(g("J"), g("sBj")) + 1
    return bC + span(g("I"), g("sCi")) + span(g("J"), g("sCj")) + 1


def operands(desc, seed):
    """A and B with live data where some entry reads and NaN elsewhere, C0 (sentinel; random where an accumulating launch
    stores), the per-entry input scales and the initial log-norms"""
    rng = np.random.default_rng(seed)
    nb = desc["nbatch"]
    na = max(_footprint(desc, "A", b) for b in range(nb)) + 8
    nbb = max(_footprint(desc, "B", b) for b in range(nb)) + 8
    nc = max(_footprint(desc, "C", b) for b in range(nb))
    A = np.full(na, np.nan, dtype=np.float32)
    B = np.full(nbb, np.nan, dtype=np.float32)
    for b in range(nb):
        ia, ib = R.entry_index_sets(desc, b)
        A[np.unique(ia)] = rng.standard_normal(np.unique(ia).size).astype(np.float32)
        B[np.unique(ib)] = rng.standard_normal(np.unique(ib).size).astype(np.float32)
    C0 = np.full(nc, SENT, dtype=np.float32)
    if desc.get("accumulate"):
        w = R.tgemm_ref(desc, np.nan_to_num(A), np.nan_to_num(B), np.zeros(nc, dtype=np.float32))["written"]
        C0[w] = rng.standard_normal(int(w.sum())).astype(np.float32)
    scale_in = np.linspace(0.5, 2.0, nb).astype(np.float32) if desc.get("scale_in") else None
    return A, B, C0, scale_in, np.linspace(0.5, 1.5, nb)


# ---------------------------------------------------------------------------------------------------------------------------
# the child: every kernel case and the engine case, results into one .npz
def engine_case():
    from peps_amd import synthetic
    L, D, chi, nw = 6, 4, 8, 64
    sitps = synthetic.make_sitps(L, D, noise=0.1)
    ctx = capi.Context(L, L, D, 2, chi, dtype=capi.F32, device=0, max_walkers=nw)
    ctx.state_upload(synthetic.sitps_to_flat(sitps, D, np.float64))
    ctx.set_configs(synthetic.make_configs(L, nw, "heisenberg"))
    ctx.profile_enable(True)
    amp = np.asarray(ctx.evaluate_amplitude(), dtype=np.float64)
    prof = ctx.profile_read()
    cats = sorted(prof)
    return dict(amp=amp, launches=np.array([prof[c]["launches"] for c in cats], dtype=np.int64),
                alg_flops=np.array([prof[c]["alg_flops"] for c in cats], dtype=np.float64), cats=np.array(cats))


def child_main(path):
    out = {}
    for name, (desc, lay, seed) in kernel_cases().items():
        A, B, C0, si, nl0 = operands(lay, seed)
        nb = desc["nbatch"]
        r = capi.diag_tgemm_desc(capi.TG_F32, desc, A, B, C0, scale_in=si, scale_out=np.full(nb, -5.0), norm_log=nl0,
                                 norm_flag=np.zeros(nb))
        out[name + "/status"] = np.array([r["status"]])
        out[name + "/route"] = np.array(r["route"])
        out[name + "/flops"] = np.array([r["flops"]], dtype=np.uint64)
        for f in ("C", "scale_out", "norm_log", "norm_flag"):
            out[name + "/" + f] = r[f]
    for k, v in engine_case().items():
        out["engine/" + k] = v
    np.savez(path, **out)


@pytest.fixture(scope="module")
def runs():
    """(switch off, switch on): the arrays of the two child processes"""
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for tag, val in (("off", "0"), ("on", None)):
            env = dict(os.environ)
            env.pop("PEPSGPU_TGEMM_THIN", None)
            if val is not None:
                env["PEPSGPU_TGEMM_THIN"] = val
            path = os.path.join(tmp, tag + ".npz")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, "child (%s) failed:\n%s\n%s" % (tag, p.stdout[-2000:], p.stderr[-4000:])
            with np.load(path) as z:
                res.append({k: z[k] for k in z.files})
    return tuple(res)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_case(runs, name, fused=False):
    """switch on and off: the same bytes; both: status, route kind, the reference, untouched elements; returns (ref, C)"""
    desc, lay, seed = kernel_cases()[name]
    A, B, C0, si, nl0 = operands(lay, seed)
    ref = R.tgemm_ref(desc, A, B, C0, 0, 0, si)
    off, on = runs
    fields = ("C", "scale_out", "norm_log", "norm_flag") if fused else ("C",)
    for f in fields:
        assert same_bytes(off[name + "/" + f], on[name + "/" + f]), "%s: %s differs between switch off and on" % (name, f)
    for r in runs:
        assert int(r[name + "/status"][0]) == 0
        assert int(r[name + "/route"][0]) == DIRECT and int(r[name + "/route"][3]) == 0, r[name + "/route"]
        assert int(r[name + "/flops"][0]) == ref["flops"]
        got = r[name + "/C"]
        assert np.array_equal(got[~ref["written"]], C0[~ref["written"]]), "%s: stores outside the live result" % name
        w = ref["written"] & np.isfinite(ref["C"])
        bound = (16 * np.sqrt(np.maximum(ref["K"], 1)) * U32 + 2 * U32) * ref["absprod"]
        err = np.abs(got[w].astype(np.float64) - ref["C"][w])
        print("%s: worst error / bound %.3f" % (name, float(np.max(err / np.maximum(bound[w], 1e-300), initial=0.0))))
        assert np.all(err <= bound[w]), "%s: %d elements off the reference" % (name, int(np.sum(err > bound[w])))
    return ref, on[name + "/C"], C0


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u", [4, 8])
def test_m_form(runs, u):
    old, new = "m_u%d_old" % u, "m_u%d_new" % u
    ref, c_old, C0 = check_case(runs, old)
    _, c_new, _ = check_case(runs, new)
    assert same_bytes(c_old, c_new), "the two column enumerations store different bytes"
    for r in runs:
        assert same_bytes(r[old + "/C"], r[new + "/C"])
    d = desc_m(u, True)
    m, uk, k2 = 8, u * 12, 12
    for b in range(d["nbatch"]):
        Cb = c_new[b * d["wC"]:b * d["wC"] + m * uk].reshape(m, u, k2)
        lm, lk = d["dynI"][b], d["dJ1"]["p"][b]
        assert np.all(Cb[:lm, :, lk:].view(np.uint32) == 0), "columns beyond the live k2 are not exact zeros"
        assert np.all(Cb[lm:] == SENT), "rows beyond the live m were stored"
        assert np.all(c_new[b * d["wC"] + m * uk:(b + 1) * d["wC"]] == SENT)


@pytest.mark.parametrize("vec_a", [1, 0])
def test_partial_rounds(runs, vec_a):
    name = "partial_avec%d" % vec_a
    check_case(runs, name)
    for r in runs:
        assert tuple(int(v) for v in r[name + "/route"]) == (DIRECT, vec_a, 0, 0)


@pytest.mark.parametrize("k", [8, 20])
def test_y_form_staged(runs, k):
    name = "y_k%d" % k
    ref, _, _ = check_case(runs, name, fused=True)
    nl0 = operands(kernel_cases()[name][1], kernel_cases()[name][2])[4]
    so, nl, nf = R.fused_norm_ref(ref["norm"], nl0)
    for r in runs:
        assert np.array_equal(r[name + "/norm_flag"], nf)
        assert int(r[name + "/norm_flag"][0]) == 1, "the entry with no live row of V must raise its flag"
        np.testing.assert_allclose(r[name + "/scale_out"][nf == 0], so[nf == 0], rtol=2.0 ** -21, atol=0)
        np.testing.assert_allclose(r[name + "/norm_log"], nl, rtol=0, atol=1e-6)


def test_y_above_lds_cap(runs):
    check_case(runs, "y_above_cap", fused=True)


@pytest.mark.parametrize("ntj", [4, 7])
def test_every_tile_once(runs, ntj):
    # accumulating launch on random C0: a tile computed twice is added twice, a tile left out keeps C0 -- both miss the reference
    ref, got, C0 = check_case(runs, "rot_%d" % ntj)
    assert ref["written"].sum() == sum(min(20, p) * 32 * ntj for p in desc_rot(ntj)["dI2"]["p"])
    assert not np.any(got[ref["written"]] == C0[ref["written"]])


def test_engine(runs):
    off, on = runs
    assert np.all(np.isfinite(on["engine/amp"])) and np.any(on["engine/amp"] != 0)
    assert same_bytes(off["engine/amp"], on["engine/amp"]), "evaluate_amplitude differs between switch off and on"
    assert np.array_equal(off["engine/cats"], on["engine/cats"])
    assert np.array_equal(off["engine/launches"], on["engine/launches"])
    assert np.array_equal(off["engine/alg_flops"], on["engine/alg_flops"])
    assert on["engine/launches"].sum() > 0


if __name__ == "__main__":
    child_main(sys.argv[1])
