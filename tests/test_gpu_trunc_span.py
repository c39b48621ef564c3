"""Span-only truncation of the low-rank sites (JrSelect::span, jacobi_rows_tiny4_kernel): where nothing is truncated only the row
space of M = R Tt leaves the site, so the kernel emits an orthonormal basis of the rows (two-pass Gram-Schmidt in the rows' own
order) instead of the singular vectors.  Kernel form through capi.diag_trunc_rows against a float64 NumPy statement of the same
rule; engine form against the float64 oracle, with the switch PEPSGPU_TRUNC_SPAN unset and 0 (child interpreters: read once).

Every bound is made from the project's own constants: eps = Eps<float>::v = 2^-24, NOISE_C = 8."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24          # Eps<float>::v (linalg.h)
NOISE_C = 8.0
JR_BR = 16                # rows of the short-row class
TOL_F32 = 1e-5            # test_gpu_parity.TOL["f32"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------
# reference and inputs
def ref_span(M):
    """float64 statement of the span path: floor (2 NOISE_C eps |M|_F)^2, rows in their own order, two passes of classical
    Gram-Schmidt against the kept rows, a row whose remainder is not above the floor is dropped."""
    M = np.asarray(M, dtype=np.float64)
    nfloor2 = 4.0 * NOISE_C ** 2 * EPS ** 2 * float(np.sum(M * M))
    Q = np.zeros((0, M.shape[1]))
    for j in range(M.shape[0]):
        r = M[j].copy()
        for _ in range(2):
            r = r - (Q @ r) @ Q
        n2 = float(r @ r)
        if n2 > nfloor2:
            Q = np.vstack([Q, r / np.sqrt(n2)])
    return Q


def graded_block(rng, mm, ln):
    """rows graded over six decades, as the rows of M = R Tt behind the pivoted factor are"""
    g = 10.0 ** (-6.0 * np.arange(mm) / max(mm - 1, 1))
    return (rng.standard_normal((mm, ln)) * g[:, None]).astype(np.float32)


def gap_block(rng, mm, ln, rank):
    """rank-deficient block made ONLY of `rank` independent rows, exact copies and power-of-two multiples of them, and zero rows (one of
    them in the middle where there is room): every operation on a dependent row is exact up to the rounding of the projections"""
    assert 0 <= rank <= min(mm, ln)
    base = rng.standard_normal((rank, ln)).astype(np.float32)
    fill = ["z" if (i % 2 == 0) else "c" for i in range(mm - rank)]
    rest = ["b"] * max(rank - 1, 0) + fill
    kinds = (["b"] if rank else []) + [rest[i] for i in rng.permutation(len(rest))]
    if fill and mm >= 3:                                  # a zero row in the middle (index 0 keeps the first independent row)
        iz, mid = kinds.index("z"), mm // 2
        kinds[iz], kinds[mid] = kinds[mid], kinds[iz]
    out = np.zeros((mm, ln), dtype=np.float32)
    seen = 0
    for j, kd in enumerate(kinds):
        if kd == "b":
            out[j] = base[seen]
            seen += 1
        elif kd == "c" and seen > 0:
            out[j] = base[rng.integers(seen)] * np.float32(2.0 ** int(rng.integers(-3, 4))) * np.float32(rng.choice([-1.0, 1.0]))
        # "z", or a copy before any base row: zero row
    return out


def check_gap_input(M, rank):
    """the generator's own promise: rank as intended and every non-zero singular value at least 100 x the floor"""
    s = np.linalg.svd(M.astype(np.float64), compute_uv=False)
    floor = 2.0 * NOISE_C * EPS * np.sqrt(float(np.sum(M.astype(np.float64) ** 2)))
    assert int(np.sum(s > 1e-12 * max(s[0], 1e-300))) == rank if rank else np.all(s == 0)
    if rank:
        assert s[rank - 1] >= 100.0 * floor, (s, floor)


def check_basis(M, V, kl, k, what):
    """orthonormality at the angle the Jacobi stops at, span residual below the floor of every dropped row, zero tail"""
    mm, ln = M.shape
    Md, Vd = M.astype(np.float64), V.astype(np.float64)
    assert 0 <= kl <= k, what
    assert np.all(V[kl:] == 0.0), what                                      # rows klive .. k-1: exact zeros
    orth = float(np.max(np.abs(Vd[:kl] @ Vd[:kl].T - np.eye(kl)))) if kl else 0.0
    res = float(np.linalg.norm(Md - (Md @ Vd[:kl].T) @ Vd[:kl]))
    b_orth = 2.0 * np.sqrt(ln) * EPS
    b_res = 2.0 * NOISE_C * EPS * np.sqrt(mm) * float(np.linalg.norm(Md))
    print("%s: orth %.3e (bound %.3e)  residual %.3e (bound %.3e)  klive %d" % (what, orth, b_orth, res, b_res, kl))
    assert orth <= b_orth, (what, orth, b_orth)
    assert res <= b_res, (what, res, b_res)


def make_batch(seed, nb, m, mm, ln):
    """walkers alternate between graded and gap inputs (one all-zero block where the batch has room); rows beyond the live count
    hold large values that no kernel may read"""
    rng = np.random.default_rng(seed)
    M = (1e3 * rng.standard_normal((nb, m, ln))).astype(np.float32)
    ranks = np.full(nb, -1)
    for b in range(nb):
        if b % 2 == 0 and not (b == 4 and nb > 4):
            M[b, :mm] = graded_block(rng, mm, ln)
        else:
            hi = min(mm - 1, ln - 2 if ln <= 8 else ln)      # rank-deficient wherever there is more than one row
            rank = 0 if b == 4 else (int(rng.integers(1, hi + 1)) if mm > 1 else 1)
            M[b, :mm] = gap_block(rng, mm, ln, rank)
            check_gap_input(M[b, :mm], rank)
            ranks[b] = rank
    return M, ranks


# ---------------------------------------------------------------------------------------------------------------------------
# kernel form
@pytest.mark.parametrize("ln", [8, 60, 64, 72, 128])
def test_span_rows_kernel(ln):
    """Both instantiations (len <= 64: four columns per lane, else eight), a partial last lane, the 64 / 65 boundary; 1 .. 16 live
    rows under a static 16 and a static 24; a single walker, a partial wave, a full block and a block plus one."""
    from peps_amd import capi
    k = JR_BR
    for mm in (1, 2, 7, 10, 16):
        for nb in (1, 5, 16, 17):
            for m in ((16, 24) if nb == 5 else (16,)):
                M, ranks = make_batch(1000 * ln + 10 * mm + nb + m, nb, m, mm, ln)
                rows = np.full(nb, mm, dtype=np.int32)
                V, kl, sw = capi.diag_trunc_rows(M, rows, k, span=True, fill=7.0)
                assert np.all((sw & 0xFF) == 0), (ln, mm, nb, sw)                  # zero sweeps: span walkers
                assert np.all((sw >> 8) == mm), (ln, mm, nb, sw)
                for b in range(nb):
                    what = "len=%d mm=%d nb=%d m=%d b=%d" % (ln, mm, nb, m, b)
                    check_basis(M[b, :mm], V[b], int(kl[b]), k, what)
                    Q = ref_span(M[b, :mm])
                    check_basis(M[b, :mm], np.vstack([Q, np.zeros((k - len(Q), ln))]), len(Q), k, what + " (reference)")
                    if ranks[b] >= 0:                                                  # gap inputs: the count is the rank, exactly
                        assert len(Q) == ranks[b], (what, len(Q), ranks[b])
                        assert int(kl[b]) == ranks[b], (what, int(kl[b]), ranks[b])
                # flag off: the sweeps and the select epilogue, reproducible as bytes
                V0, kl0, sw0 = capi.diag_trunc_rows(M, rows, k, span=False, fill=7.0)
                V1, kl1, _ = capi.diag_trunc_rows(M, rows, k, span=False, fill=7.0)
                assert V0.tobytes() == V1.tobytes() and kl0.tobytes() == kl1.tobytes()
                assert np.all((sw0 & 0xFF) >= 1) and np.all((sw0 >> 8) == mm)
                for b in range(nb):
                    if ranks[b] >= 0:
                        assert int(kl0[b]) == ranks[b]


def _orth_rows(rng, mm, ln, norms):
    q, _ = np.linalg.qr(rng.standard_normal((ln, mm)))
    return (q.T * np.asarray(norms)[:, None]).astype(np.float32)


def test_span_mixed_wave_and_fallback():
    """One batch whose first wave holds a span walker, a walker that keeps more than k directions, a walker without rows and one with
    more than 16 rows; a wave without any span walker; a wave whose walkers all fall back.  A walker that falls back reloads its
    rows and takes the sweeps and the select epilogue: as bytes what the flag-off launch gives wherever its wave holds no span
    walker, inside the two bounds and with the same live count where it shares the wave with one (other tournament size)."""
    from peps_amd import capi
    rng = np.random.default_rng(11)
    for ln in (60, 72):
        m, k, nb = 24, 6, 17
        M = (1e3 * rng.standard_normal((nb, m, ln))).astype(np.float32)
        rows = np.zeros(nb, dtype=np.int32)
        top = [1.0, 0.8, 0.6, 0.5, 0.4, 0.3]
        floor = 2.0 * NOISE_C * EPS * float(np.linalg.norm(top))
        # discarded directions just above the floor (kept by the Gram-Schmidt count, so the walker falls back) whose sum stays
        # inside the span bound: 4 x (1.3 floor)^2 < 10 floor^2
        low = top + [1.3 * floor] * 4
        for b in (0, 12, 16):
            rows[b] = 5; M[b, :5] = gap_block(rng, 5, ln, 5)           # span: 5 directions <= k
        rows[1] = 10; M[1, :10] = _orth_rows(rng, 10, ln, low)          # count 10 > k = 6, shares a wave with a span walker
        rows[2] = 0
        rows[3] = 20                                                    # the 17 .. 32-row class: not this kernel's
        rows[4:8] = (0, 20, 0, 20)                                      # a wave without span walkers
        for b in (8, 9, 10, 11):                                        # a wave whose walkers all fall back (real truncation)
            rows[b] = 10
            M[b, :10] = _orth_rows(rng, 10, ln, [1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.01, 0.01, 0.01, 0.01]) if b != 9 else _orth_rows(rng, 10, ln, low)
        rows[13:16] = (7, 0, 16)
        M[13, :7] = graded_block(rng, 7, ln)
        M[15, :16] = gap_block(rng, 16, ln, 6)
        V, kl, sw = capi.diag_trunc_rows(M, rows, k, span=True, fill=7.0)
        V0, kl0, sw0 = capi.diag_trunc_rows(M, rows, k, span=False, fill=7.0)
        for b in (2, 3, 4, 5, 6, 7, 14):                               # not taken: untouched with either flag
            assert np.all(V[b] == 7.0) and kl[b] == -1 and sw[b] == -1
            assert np.all(V0[b] == 7.0) and kl0[b] == -1 and sw0[b] == -1
        for b in (0, 12, 16):
            assert (sw[b] & 0xFF) == 0 and (sw[b] >> 8) == 5 and kl[b] == 5
            check_basis(M[b, :5], V[b], int(kl[b]), k, "mixed len=%d b=%d" % (ln, b))
        assert (sw[15] & 0xFF) == 0 and kl[15] == 6                     # 16 rows of rank 6 = k: still the span path
        check_basis(M[15, :16], V[15], 6, k, "mixed len=%d b=15" % ln)
        assert (sw[13] & 0xFF) == 0 or kl[13] == k                      # graded rows: span if the count fits, else the sweeps
        # waves without a span walker: bytes of the flag-off launch
        for b in (8, 9, 10, 11):
            assert (sw[b] & 0xFF) >= 1 and (sw[b] >> 8) == 10
            assert V[b].tobytes() == V0[b].tobytes() and kl[b] == kl0[b] and sw[b] == sw0[b], b
        # the fallback walker next to a span walker: the two bounds and the live count
        assert (sw[1] & 0xFF) >= 1 and (sw[1] >> 8) == 10
        assert kl[1] == k == kl0[1]
        check_basis(M[1, :10], V[1], int(kl[1]), k, "mixed len=%d b=1 (fell back)" % ln)
        check_basis(M[9, :10], V[9], int(kl[9]), k, "mixed len=%d b=9 (fell back)" % ln)
        # real truncation behind the fallback: orthonormal, and the residual is the discarded weight (sigma_7..10 = 0.01 each; the
        # rotation error of the kept subspace is eps sigma_1 / gap, far inside the span bound that is added)
        for b in (8, 10, 11):
            Md, Vd = M[b, :10].astype(np.float64), V[b].astype(np.float64)
            assert kl[b] == k
            assert np.max(np.abs(Vd @ Vd.T - np.eye(k))) <= 2.0 * np.sqrt(ln) * EPS
            s = np.linalg.svd(Md, compute_uv=False)
            res = np.linalg.norm(Md - (Md @ Vd.T) @ Vd)
            assert res <= np.sqrt(np.sum(s[k:] ** 2)) + 2.0 * NOISE_C * EPS * np.sqrt(10.0) * np.linalg.norm(Md)


# ---------------------------------------------------------------------------------------------------------------------------
# engine
_CHILD = r'''
import json, sys
import numpy as np
from peps_amd import capi, synthetic
out = {}
def run(tag, L, D, chi, noise, nw, trunc_err):
    sitps = synthetic.make_sitps(L, D, noise=noise)
    cfgs = synthetic.make_configs(L, nw, "heisenberg")
    ctx = capi.Context(L, L, D, 2, chi, dtype=capi.F32, max_walkers=nw)
    ctx.state_upload(synthetic.sitps_to_flat(sitps, D, np.float64))
    if trunc_err > 0:
        ctx.set_truncate_params(chi, chi, trunc_err)
    ctx.set_configs(cfgs)
    a = ctx.evaluate_amplitude()
    st = ctx.stats()
    out[tag] = {"amps": [float(x).hex() for x in a], "redone": int(st["absorptions_redone"]), "flags": int(np.sum(ctx.walker_flags() != 0))}
    ctx.close()
run("main", 4, 4, 8, 0.1, 64, 0.0)
run("terr", 4, 4, 8, 0.1, 64, 1e-6)
run("fallback", 3, 4, 3, 1.0, 8, 0.0)
print(json.dumps(out))
'''


def _amps(rec):
    return np.array([float.fromhex(x) for x in rec["amps"]])


@pytest.fixture(scope="module")
def engine_runs():
    """both settings of the switch, each in a fresh interpreter; the sweep diagnostics give the per-launch span counts"""
    runs = {}
    for name, env in (("unset", {}), ("off", {"PEPSGPU_TRUNC_SPAN": "0"})):
        e = dict(os.environ, PEPSGPU_DEBUG_SWEEPS="1", PEPSGPU_DEBUG_VERBOSE="1", **env)
        if name == "unset":
            e.pop("PEPSGPU_TRUNC_SPAN", None)
        r = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = json.loads(r.stdout.strip().splitlines()[-1])
        lines = [ln for ln in r.stderr.splitlines() if " span=" in ln]
        runs[name]["span"] = sum(int(ln.split(" span=")[1].split()[0]) for ln in lines)
        runs[name]["fell_back"] = sum(int(ln.split("span_fell_back=")[1].split()[0]) for ln in lines)
    return runs


@pytest.fixture(scope="module")
def oracle_amps():
    from oracle import vmc
    from oracle.bmps import BMPSTruncateParams
    from peps_amd import synthetic

    def f(L, D, chi, noise, nw):
        sitps = synthetic.make_sitps(L, D, noise=noise)
        cfgs = synthetic.make_configs(L, nw, "heisenberg")
        tp = BMPSTruncateParams.SVD(chi, chi, 0.0)
        return np.array([vmc.TPSWaveFunctionComponent(sitps, c, tp).amplitude for c in cfgs])
    return {"main": f(4, 4, 8, 0.1, 64), "fallback": f(3, 4, 3, 1.0, 8)}


def test_engine_amplitudes_both_settings(engine_runs, oracle_amps):
    """4 x 4, D = 4, chi = 8, the synthetic state at noise 0.1, 64 walkers, f32: inside the parity tolerance with the switch unset
    (span walkers present) and with 0 (none), and the default does not redo more absorptions."""
    for name in ("unset", "off"):
        rec = engine_runs[name]["main"]
        rel = float(np.max(np.abs(_amps(rec) / oracle_amps["main"] - 1)))
        print("switch %s: max rel err %.3e, redone %d, span walkers %d, fell back %d"
              % (name, rel, rec["redone"], engine_runs[name]["span"], engine_runs[name]["fell_back"]))
        assert rec["flags"] == 0
        assert rel < TOL_F32, (name, rel)
    assert engine_runs["unset"]["span"] > 0          # the path IS taken by default ...
    assert engine_runs["off"]["span"] == 0           # ... and not with the switch at 0
    assert engine_runs["unset"]["main"]["redone"] <= engine_runs["off"]["main"]["redone"]


def test_engine_trunc_err_does_not_take_the_path(engine_runs):
    """a truncation-error rule needs the singular values: the engine does not ask for the path, the amplitudes are byte-equal"""
    assert engine_runs["unset"]["terr"]["amps"] == engine_runs["off"]["terr"]["amps"]


def test_engine_fallback_site(engine_runs, oracle_amps):
    """3 x 3, D = 4, chi = 3 on the full-rank state (noise 1): the left part of the inner bonds has rank 4 (one open leg of
    D = 4; with chi = 4 nothing would truncate), so the bonds truncate, walkers keep more than k directions and take the sweeps;
    same tolerance against the oracle"""
    for name in ("unset", "off"):
        rec = engine_runs[name]["fallback"]
        rel = float(np.max(np.abs(_amps(rec) / oracle_amps["fallback"] - 1)))
        print("switch %s: fallback case max rel err %.3e" % (name, rel))
        assert rel < TOL_F32, (name, rel)
    assert engine_runs["unset"]["fell_back"] > 0
