"""The one-wave Gram-free factor with the rows of P placed by row parity for the dot products of a pivot step
(gram_chol_wave_split_kernel, peps_amd/csrc/linalg.h) against the kernel it stands in for (gram_chol_wave_kernel).

The placement changes which lane holds which number and nothing else, so the yardstick is byte equality: every case goes through
capi.diag_gram_chol_wave (one of the two kernels alone, then the list kernel for the walkers it hands on) with form 0 and form 1
and R_out and mlive_out are compared as raw bytes.  Form 1 alone is also held to R^T R = P^T P / max diag within the 2e-5 of
test_gram_free_lowrank_factor and to the rank window rank <= mlive <= rank + 2 (rank = min(rank of the factors, live rows, live
columns)), so that two equal wrong answers do not pass.

All inputs are products of seeded Gaussian factors rounded to f32.  Rows beyond a walker's live count and columns beyond its live
inner extent are NaN in what the kernels get: neither is ever read.

The engine case runs two fresh child processes (PEPSGPU_FACTOR_SPLIT=0 and unset): the same amplitude bytes, absorption counts,
largest live carry and launches per profile category.
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
from peps_amd import capi  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 2e-5          # of test_gram_free_lowrank_factor (f32)
MAX_PASS = 3        # the one-wave kernels take 64 + 2 * 48 = 160 rows, the list kernel 96 + 2 * 64 = 224


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def lowrank(rng, K, n, rank):
    if rank == 0:
        return np.zeros((K, n), dtype=np.float32)
    return (rng.standard_normal((K, rank)) @ rng.standard_normal((rank, n))).astype(np.float32)


def run_both(P, klive, ranks, inner=1, inner_live=None, max_pass=MAX_PASS, min_ml=None):
    """P [nb][K][n] f32 (finite everywhere), klive[b], ranks[b] of the factors; both forms, byte equality, then the loose checks
    on form 1.  Returns mlive."""
    nb, K, n = P.shape
    klive = np.asarray(klive, dtype=np.int32)
    il = None if inner_live is None else np.asarray(inner_live, dtype=np.int32)
    live = np.ones((nb, K, n), dtype=bool)
    for b in range(nb):
        live[b, klive[b]:] = False
        if il is not None:
            live[b][:, (np.arange(n) % inner) >= il[b]] = False
    Pdev = np.where(live, P, np.float32(np.nan)).astype(np.float32)
    R0, m0 = capi.diag_gram_chol_wave(Pdev, klive, inner, il, max_pass, form=0)
    R1, m1 = capi.diag_gram_chol_wave(Pdev, klive, inner, il, max_pass, form=1)
    print("mlive form 0", m0.tolist(), "form 1", m1.tolist())
    assert same_bytes(m0, m1), "mlive differs between the two forms"
    assert same_bytes(R0, R1), "R differs between the two forms: walkers %s" % sorted(set(np.argwhere(R0.view(np.uint32) != R1.view(np.uint32))[:, 0].tolist()))
    for b in range(nb):
        Pb = np.where(live[b], P[b], 0).astype(np.float64)
        ncols = int(live[b].any(axis=0).sum()) if klive[b] > 0 else 0
        rank = min(int(ranks[b]), int(klive[b]), ncols)
        assert rank <= m1[b] <= min(rank + 2, max(int(klive[b]), 0), n), (b, rank, int(m1[b]))
        if min_ml is not None:
            assert m1[b] >= min_ml, (b, int(m1[b]))
        G = Pb.T @ Pb
        sc = float(np.max(np.diag(G)))
        Rb = R1[b, :m1[b]].astype(np.float64)
        assert np.all(R1[b, m1[b]:] == 0), "rows beyond mlive were stored"
        if sc == 0.0:
            assert m1[b] == 0
            continue
        err = float(np.max(np.abs(Rb.T @ Rb * sc - G)) / sc)
        assert err < TOL, (b, rank, int(m1[b]), err)
    return m1


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 80, 96, 97, 128, 129])
def test_slot_classes(n):
    """n = live columns (inner = 1): one to four column slots and their edges; 129 is handed on by both forms"""
    rng = np.random.default_rng(1000 + n)
    nb, K = 5, 80
    P = np.stack([lowrank(rng, K, n, 10) for _ in range(nb)])
    run_both(P, [K] * nb, [10] * nb)


@pytest.mark.parametrize("K", [1, 2, 7, 63, 64, 65, 80, 112, 113, 160, 161])
def test_rows(K):
    """65: a second pass of one row; 112: exactly two passes; 113: a third; 161: more than three passes hold, declined"""
    rng = np.random.default_rng(2000 + K)
    nb, n = 5, 80
    P = np.stack([lowrank(rng, K, n, 10) for _ in range(nb)])
    run_both(P, [K] * nb, [10] * nb)


@pytest.mark.parametrize("nb", [5, 13])
def test_mixed_launch(nb):
    """different live row counts in one launch, the last block with idle waves"""
    rng = np.random.default_rng(3000 + nb)
    K, n = 161, 96
    kl = [80, 0, 113, 1, 160, 16, 64, 65, 112, 7, 161, 40, 130][:nb]
    rk = [10, 3, 12, 5, 9, 16, 4, 11, 8, 10, 6, 1, 7][:nb]
    P = np.stack([lowrank(rng, K, n, r) for r in rk])
    run_both(P, kl, rk)


@pytest.mark.parametrize("rank", [0, 1, 10, 16, 17])
def test_rank(rank):
    """17 is above the cap of the one-wave kernels: handed on, the list kernel's answer comes back (mlive >= 17)"""
    rng = np.random.default_rng(4000 + rank)
    nb, K, n = 5, 80, 96
    P = np.stack([lowrank(rng, K, n, rank) for _ in range(nb)])
    run_both(P, [K] * nb, [rank] * nb, min_ml=17 if rank == 17 else None)


def test_zero_columns_among_live_ones():
    rng = np.random.default_rng(5001)
    nb, K, n = 5, 80, 128
    P = np.stack([lowrank(rng, K, n, 10) for _ in range(nb)])
    P[:, :, [0, 5, 31, 32, 40, 64, 70, 100, 127]] = 0
    run_both(P, [K] * nb, [10] * nb)


@pytest.mark.parametrize("block", [0, 1, 2, 3])
def test_pivots_in_one_block(block):
    """The pivot rule takes the first column above the threshold: with every other column 1e-8 of the block's, all pivots lie in
    this 32-column block (the slot of the pivot takes this value at every step)."""
    rng = np.random.default_rng(5100 + block)
    nb, K, n = 5, 80, 128
    P = np.stack([lowrank(rng, K, n, 10) for _ in range(nb)]).astype(np.float64)
    scale = np.full(n, 1e-8)
    scale[32 * block:32 * block + 32] = 1.0
    run_both((P * scale).astype(np.float32), [K] * nb, [10] * nb)


def test_pivots_walk_through_the_blocks():
    """Three independent directions per 32-column block: the pivots of one factorisation go through all four slots"""
    rng = np.random.default_rng(5200)
    nb, K, n = 5, 80, 128
    P = np.zeros((nb, K, n), dtype=np.float32)
    for b in range(nb):
        for q in range(4):
            P[b][:, 32 * q:32 * q + 32] = lowrank(rng, K, 32, 3)
    run_both(P, [K] * nb, [12] * nb)


@pytest.mark.parametrize("parity", [0, 1])
def test_rows_of_one_parity_only(parity):
    rng = np.random.default_rng(5300 + parity)
    nb, K, n = 5, 80, 96
    P = np.stack([lowrank(rng, K, n, 10) for _ in range(nb)])
    P[:, (1 - parity)::2] = 0
    run_both(P, [K] * nb, [10] * nb)


def test_packed_columns():
    """columns (outer 8, inner 16) with a live inner extent per walker, as the absorption passes them: 8 .. 128 packed columns
    (one to four slots) and one to three passes in one launch"""
    rng = np.random.default_rng(6000)
    K, n, inner = 136, 128, 16
    il, kl = [], []
    for k in (16, 80, 136):
        for i in (1, 5, 8, 10, 11, 16):
            il.append(i)
            kl.append(k)
    P = np.stack([lowrank(rng, K, n, 10) for _ in il])
    run_both(P, kl, [10] * len(il), inner=inner, inner_live=il)


# ---------------------------------------------------------------------------------------------------------------------------
# the engine: two child processes
def engine_case():
    from peps_amd import synthetic
    L, D, chi, nw = 6, 8, 32, 16
    sitps = synthetic.make_sitps(L, D, noise=0.1)
    ctx = capi.Context(L, L, D, 2, chi, dtype=capi.F32, device=0, max_walkers=nw)
    ctx.state_upload(synthetic.sitps_to_flat(sitps, D, np.float64))
    ctx.set_configs(synthetic.make_configs(L, nw, "heisenberg"))
    ctx.profile_enable(True)
    amp = np.asarray(ctx.evaluate_amplitude(), dtype=np.float64)
    prof = ctx.profile_read()
    st = ctx.stats()
    cats = sorted(prof)
    return dict(amp=amp, launches=np.array([prof[c]["launches"] for c in cats], dtype=np.int64), cats=np.array(cats),
                stats=np.array([st["absorptions"], st["absorptions_redone"], st["carry_live_max"]], dtype=np.int64))


def child_main(path):
    np.savez(path, **engine_case())


@pytest.fixture(scope="module")
def runs():
    """(switch off, switch unset): the arrays of the two child processes"""
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for tag, val in (("off", "0"), ("on", None)):
            env = dict(os.environ)
            env.pop("PEPSGPU_FACTOR_SPLIT", None)
            env["PEPSGPU_DEBUG_SWEEPS"] = "1"       # (carry_live_max is collected under it only)
            if val is not None:
                env["PEPSGPU_FACTOR_SPLIT"] = val
            path = os.path.join(tmp, tag + ".npz")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, "child (%s) failed:\n%s\n%s" % (tag, p.stdout[-2000:], p.stderr[-4000:])
            with np.load(path) as z:
                res.append({k: z[k] for k in z.files})
    return tuple(res)


def test_engine(runs):
    off, on = runs
    assert np.all(np.isfinite(on["amp"])) and np.all(on["amp"] != 0)
    assert same_bytes(off["amp"], on["amp"]), "amplitudes differ between PEPSGPU_FACTOR_SPLIT=0 and unset"
    assert np.array_equal(off["stats"], on["stats"]), (off["stats"], on["stats"])
    assert on["stats"][0] > 0 and on["stats"][2] > 0
    assert np.array_equal(off["cats"], on["cats"]) and np.array_equal(off["launches"], on["launches"])
    chol = list(on["cats"]).index("cholesky")
    assert on["launches"][chol] > 0, "the factor never ran"


if __name__ == "__main__":
    child_main(sys.argv[1])
