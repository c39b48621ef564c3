"""One wave per workgroup for the one-wave Gram-free factor (peps_amd/csrc/linalg.h, launch_gram_chol_wave): the split form is
launched with one walker per 64-thread block where it ran four walkers per 256-thread block.  That changes where a wave runs and not
one floating-point operation, so the yardstick is byte equality with the launch it replaces.

Factor: capi.diag_gram_chol_wave with form 0 (gram_chol_wave_kernel, four walkers per 256-thread block -- what PEPSGPU_FACTOR_SPLIT=0
selects in the engine) against form 1 (gram_chol_wave_split_kernel, one walker per block -- the variable unset): R_out and mlive_out
as raw bytes, form 1 also against P^T P and the rank window (test_gpu_factor_split.run_both).  Walker counts 1, 3, 4, 5, 9: less
than, exactly and more than the four walkers of a 256-thread block, with and without idle waves in its last block.

Tensor GEMM: the same change was tried on the wave-per-tile kernel (one 64-thread block per tile of M = R Tt) and taken out again:
its launches got no faster (profiles/wave_slots_ab.md).  Its cases stay as a yardstick for the next attempt at
how the tiles of M are spread over waves and blocks: M-shaped products of one to nine static tiles, every case in two fresh child
processes through capi.diag_tgemm_desc, one with PEPSGPU_TGEMM_THIN=0 (the kernels without any thin item) and one with the
variable unset; C is compared byte for byte and both are held to the float64 statement of tests/tgemm_ref.py at the elementwise
bound of tests/test_gpu_tgemm.py, (16 sqrt(K) u + 2 u) (|alpha| |A| |B| + |C0|)_ij with u = 2^-24; elements outside the live
result keep the sentinel.
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
from test_gpu_factor_split import lowrank, run_both  # noqa: E402
from test_gpu_tgemm_thin import DIRECT, U32, operands, same_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

WALKERS = [1, 3, 4, 5, 9]


# ---------------------------------------------------------------------------------------------------------------------------
# the factor
def _factor_shape(name, rng, nb):
    """(P, klive, ranks, min_ml) of a shape class"""
    if name in ("cols8_rows16", "cols80_rows16"):
        n, K, rk = (8 if name == "cols8_rows16" else 80), 16, 6
    elif name == "rows80_two_passes":
        n, K, rk = 80, 80, 10
    elif name == "cols129_declined":
        n, K, rk = 129, 16, 6
    elif name == "rank17_handed_on":
        n, K, rk = 96, 80, 17
    else:
        assert name == "all_zero"
        n, K, rk = 80, 16, 0
    P = np.stack([lowrank(rng, K, n, rk) for _ in range(nb)])
    return P, [K] * nb, [rk] * nb, (17 if rk == 17 else None)


@pytest.mark.parametrize("nb", WALKERS)
@pytest.mark.parametrize("shape", ["cols8_rows16", "cols80_rows16", "rows80_two_passes", "cols129_declined", "rank17_handed_on", "all_zero"])
def test_factor_one_walker_per_block(shape, nb):
    """cols129: both launches decline every walker (-4) and fill the list, the list kernel's answer comes back; rank17: the walker
    is handed on from inside the pivot loop (mlive >= 17 is the list kernel's: the list was filled); all_zero: mlive 0, nothing
    stored"""
    rng = np.random.default_rng(7000 + 10 * nb + len(shape))
    P, kl, rk, min_ml = _factor_shape(shape, rng, nb)
    ml = run_both(P, kl, rk, min_ml=min_ml)
    if shape == "all_zero":
        assert np.all(ml == 0)


def test_factor_mixed_ranks_and_passes():
    """what leaves a slot of a 256-thread block idle: walkers of one launch with ranks 1 .. 16 and one or two passes, nine of them"""
    rng = np.random.default_rng(7900)
    K, n = 80, 80
    kl = [80, 16, 65, 1, 64, 80, 0, 40, 80]
    rk = [16, 1, 10, 5, 3, 2, 4, 12, 17]
    P = np.stack([lowrank(rng, K, n, r) for r in rk])
    run_both(P, kl, rk)


# ---------------------------------------------------------------------------------------------------------------------------
# the tensor GEMM
LIVE_K2 = [0, 1, 10, 16, 5]      # (a stored value above the static extent is clamped)


def desc_m(k2, u, nb, mask=1, live_m=None, live_k2=None, m=8, **kw):
    """M[m,(u,k2)] = sum_{(l,a)} R[m,(l,a)] Tt[l,a,k2,u] as the engine's desc_m builds it, columns enumerated (k2, u): l = 2,
    a = 8, m rows; ceil(m / 32) ceil(k2 u / 32) static tiles; mask = 1: the columns beyond the live k2 are stored as zeros, 0: not
    stored (the live tile count falls below the static one)."""
    l, a = 2, 8
    la, uk = l * a, u * k2
    d = dict(I=(1, 1, m), sAi=(0, 0, la), sCi=(0, 0, uk), K=(1, l, a), sAk=(0, a, 1), sBk=(0, a * uk, uk), nbatch=nb,
             wA=m * la, wB=la * uk, wC=m * uk + 5, dynI=(live_m or [8, 5, 8, 1, 8])[:nb], dK2=dict(p=[8, 4, 5, 8, 1][:nb]),
             J=(1, k2, u), sBj=(0, u, 1), sCj=(0, 1, k2), dJ1=dict(p=(live_k2 or LIVE_K2)[:nb], mask=mask))
    d.update(kw)
    return d


def desc_plain(ntj, nb):
    """no transposed epilogue (C unit-stride along the lanes): one row tile of 20 rows, ntj column tiles, accumulating"""
    I, J, K = 20, 32 * ntj - 3, 8
    return dict(I=(1, 1, I), J=(1, 1, J), K=(1, 1, K), sAi=(0, 0, K), sAk=(0, 0, 1), sBk=(0, 0, J), sBj=(0, 0, 1), sCi=(0, 0, J),
                sCj=(0, 0, 1), nbatch=nb, wA=I * K, wB=K * J, wC=I * J + 7, dI2=dict(p=[20, 1, 0, 7, 13][:nb]), accumulate=1)


def kernel_cases():
    """name -> (descriptor, seed)"""
    c = {}
    for tiles, (k2, u) in ((1, (16, 2)), (3, (12, 8)), (4, (16, 8))):
        for mask in (1, 0):
            c["m_%dtiles_mask%d" % (tiles, mask)] = (desc_m(k2, u, 5, mask), 100 + 10 * tiles + mask)
        c["m_%dtiles_one_entry" % tiles] = (desc_m(k2, u, 1, 1, live_m=[8], live_k2=[10]), 200 + tiles)
    c["m_dynI_0"] = (desc_m(16, 8, 5, 1, live_m=[0, 0, 0, 0, 0]), 300)                       # nothing stored
    c["m_dynI_0_one_entry"] = (desc_m(12, 8, 1, 0, live_m=[0]), 301)
    c["m_accumulate"] = (desc_m(16, 8, 5, 0, accumulate=1), 302)
    c["m_batch_flag"] = (desc_m(12, 8, 5, 1, batch_flag=[-1, 0, -1, 7, -1]), 303)             # entries 1 and 3 skipped
    # three row tiles x three column tiles, the class of the headline's bulk sites: more tiles than the four waves of a block
    c["m_9tiles"] = (desc_m(12, 8, 5, 1, live_m=[80, 5, 33, 1, 64], m=80), 310)
    c["m_9tiles_accumulate"] = (desc_m(12, 8, 5, 1, live_m=[80, 5, 33, 1, 64], m=80, accumulate=1), 311)
    c["plain_5tiles"] = (desc_plain(5, 5), 304)
    c["plain_5tiles_one_entry"] = (desc_plain(5, 1), 305)
    return c


def child_main(path):
    out = {}
    for name, (desc, seed) in kernel_cases().items():
        A, B, C0, si, _ = operands(desc, seed)
        r = capi.diag_tgemm_desc(capi.TG_F32, desc, A, B, C0, scale_in=si)
        out[name + "/status"] = np.array([r["status"]])
        out[name + "/route"] = np.array(r["route"])
        out[name + "/flops"] = np.array([r["flops"]], dtype=np.uint64)
        out[name + "/C"] = r["C"]
    np.savez(path, **out)


@pytest.fixture(scope="module")
def runs():
    """(PEPSGPU_TGEMM_THIN=0, unset): the arrays of the two child processes"""
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


@pytest.mark.parametrize("name", sorted(kernel_cases()))
def test_direct_tiles_of_m(runs, name):
    desc, seed = kernel_cases()[name]
    A, B, C0, si, _ = operands(desc, seed)
    ref = R.tgemm_ref(desc, A, B, C0, 0, 0, si)
    off, on = runs
    assert same_bytes(off[name + "/C"], on[name + "/C"]), "%s: C differs between PEPSGPU_TGEMM_THIN=0 and unset" % name
    for r in runs:
        assert int(r[name + "/status"][0]) == 0
        assert int(r[name + "/route"][0]) == DIRECT and int(r[name + "/route"][3]) == 0, r[name + "/route"]
        assert int(r[name + "/flops"][0]) == ref["flops"]
        got = r[name + "/C"]
        assert np.array_equal(got[~ref["written"]], C0[~ref["written"]]), "%s: stores outside the live result" % name
        w = ref["written"] & np.isfinite(ref["C"])
        bound = (16 * np.sqrt(np.maximum(ref["K"], 1)) * U32 + 2 * U32) * ref["absprod"]
        err = np.abs(got[w].astype(np.float64) - ref["C"][w])
        print("%s: %d stored, worst error / bound %.3f" % (name, int(w.sum()), float(np.max(err / np.maximum(bound[w], 1e-300), initial=0.0))))
        assert np.all(err <= bound[w]), "%s: %d elements off the reference" % (name, int(np.sum(err > bound[w])))
    if name.startswith("m_dynI_0"):
        assert not ref["written"].any() and np.array_equal(on[name + "/C"], C0)
    elif name == "m_batch_flag":
        wC = desc["wC"]
        for b in (1, 3):
            assert np.array_equal(on[name + "/C"][b * wC:(b + 1) * wC], C0[b * wC:(b + 1) * wC]), "a skipped entry was stored"
        assert ref["written"][:wC].any()
    else:
        assert ref["written"].any()
    if desc.get("accumulate"):     # a tile computed twice is added twice (off the reference, above), a tile left out keeps C0
        moved = ref["written"] & (ref["C"] != C0)      # (a column stored as zero adds nothing)
        assert moved.any() and not np.any(on[name + "/C"][moved] == C0[moved])


if __name__ == "__main__":
    child_main(sys.argv[1])
