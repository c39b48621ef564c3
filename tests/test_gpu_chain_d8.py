"""The leg-8 specialisation of the chained contraction pair (tgemm_chain_d8_kernel, peps_amd/csrc/tgemm_d8.h) against the generic
chained kernel it stands in for (tgemm_chain_kernel), through capi.diag_tgemm_chain_pair: the forward pair P = W (R A) and the
backward pair Tt = W (A Y) with the descriptors of the engine, the site tensor reached through a selector table.

The specialisation changes which lane, tile and wave holds an element and nothing else, so the yardstick is byte equality of the
result and of the flags between the two kernels of one launch.  So that two equal wrong answers do not pass, the leg-8 result is
also held to the float64 contraction, elementwise within
    (16 sqrt(K1) + 16 sqrt(64) + 4) u * (|W| (|A1| |B1|))_ij * |scale|,      u = 2^-24
-- the f32 bound of tests/test_gpu_tgemm.py for each of the two products, the first carried through the second.

Conventions of tests/test_gpu_tgemm.py: operand elements beyond a walker's live extents are NaN, the result starts as a finite
sentinel and must keep it wherever the pair stores nothing.

The engine case runs two fresh child processes (PEPSGPU_CHAIN_D8=0 and unset): the same amplitude bytes, and the leg-8 kernel
must have run in the second one only.
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

U32 = 2.0 ** -24
SENT = -12345.0
W_NATURAL = "natural"     # site tensor stored [l][p][l2][u]
W_PFIRST = "pfirst"       # stored [p][l2][u][l]: no leg the kernels walk along k is unit-stride


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def site_store(rng, nslots, l, p, l2, u, order):
    """(flat store, slot, strides of (l, p, l2, u), W[slot][l][p][l2][u] as float64)"""
    W = rng.standard_normal((nslots, l, p, l2, u)).astype(np.float32)
    if order == W_NATURAL:
        flat, st = W, (p * l2 * u, l2 * u, u, 1)
    else:
        flat, st = np.ascontiguousarray(W.transpose(0, 2, 3, 4, 1)), (1, l2 * u * l, u * l, l)
    return flat.ravel(), l * p * l2 * u, st, W.astype(np.float64)


def run_pair(backward, dims, lives, seed, order=W_NATURAL, nslots=2, tsw=False, scale=False, zero_fill=False, f64=False,
             expect_d8=True):
    """One launch on each kernel; byte equality, the float64 reference, the sentinel.  dims = (m, a, a2, k2, l, p, l2, u);
    lives = per walker (x, k, y): (m, a, a2) live for the forward pair, (a, a2, k2) for the backward pair."""
    rng = np.random.default_rng(seed)
    m, a, a2, k2, l, p, l2, u = dims
    nb = len(lives)
    lives = np.asarray(lives, dtype=np.int32)
    sv, slot, st, W = site_store(rng, nslots, l, p, l2, u, order)
    sel = (np.arange(nb) * 5 + 1) % nslots
    if backward:
        A1 = rng.standard_normal((nb, a, p, a2)).astype(np.float32)       # A[a, p, a2]
        B1 = rng.standard_normal((nb, l2, a2, k2)).astype(np.float32)     # Y[l2, a2, k2]
        out0 = np.full((nb, l, a, k2, u) if tsw else (nb, l, a, u, k2), SENT, dtype=np.float32)
        stat = (a, a2, k2)
    else:
        A1 = rng.standard_normal((nb, m, l, a)).astype(np.float32)        # R[m, l, a]
        B1 = rng.standard_normal((nb, a, p, a2)).astype(np.float32)       # A[a, p, a2]
        out0 = np.full((nb, m, u, l2, a2), SENT, dtype=np.float32)
        stat = (m, a, a2)
    sc = rng.uniform(0.25, 4.0, nb).astype(np.float32) if scale else None
    A1d, B1d = A1.copy(), B1.copy()
    ref = out0.astype(np.float64)
    bound = np.zeros_like(ref)
    wrote = np.zeros(ref.shape, dtype=bool)
    for b in range(nb):
        x, k, y = (int(min(v, s)) for v, s in zip(lives[b], stat))
        Wb = W[sel[b]]
        s = float(sc[b]) if scale else 1.0
        if backward:
            A1d[b, x:] = np.nan; A1d[b, :, :, k:] = np.nan
            B1d[b, :, k:] = np.nan; B1d[b, :, :, y:] = np.nan
            Al, Yl = A1[b, :x, :, :k].astype(np.float64), B1[b, :, :k, :y].astype(np.float64)
            z = np.einsum("apc,rck->aprk", Al, Yl)                         # Z1[a, p, l2, k2]
            za = np.einsum("apc,rck->aprk", np.abs(Al), np.abs(Yl))
            t = np.einsum("lpru,aprk->lauk", Wb, z) * s
            ta = np.einsum("lpru,aprk->lauk", np.abs(Wb), za) * abs(s)
            if tsw:
                t, ta = t.transpose(0, 1, 3, 2), ta.transpose(0, 1, 3, 2)
                idx = (b, slice(None), slice(0, x), slice(0, k2 if zero_fill else y), slice(None))
                if zero_fill:
                    t = np.concatenate([t, np.zeros((l, x, k2 - y, u))], axis=2)
                    ta = np.concatenate([ta, np.zeros((l, x, k2 - y, u))], axis=2)
            else:
                idx = (b, slice(None), slice(0, x), slice(None), slice(0, k2 if zero_fill else y))
                if zero_fill:
                    t = np.concatenate([t, np.zeros((l, x, u, k2 - y))], axis=3)
                    ta = np.concatenate([ta, np.zeros((l, x, u, k2 - y))], axis=3)
        else:
            A1d[b, x:] = np.nan; A1d[b, :, :, k:] = np.nan
            B1d[b, k:] = np.nan; B1d[b, :, :, y:] = np.nan
            Rl, Al = A1[b, :x, :, :k].astype(np.float64), B1[b, :k, :, :y].astype(np.float64)
            xx = np.einsum("mla,apc->mlpc", Rl, Al)                        # X[m, l, p, a2]
            xa = np.einsum("mla,apc->mlpc", np.abs(Rl), np.abs(Al))
            t = np.einsum("lpru,mlpc->murc", Wb, xx)
            ta = np.einsum("lpru,mlpc->murc", np.abs(Wb), xa)
            idx = (b, slice(0, x), slice(None), slice(None), slice(0, y))
        if x > 0 and y > 0:
            ref[idx], bound[idx], wrote[idx] = t, ta, True
    kw = dict(tsw=tsw, zero_fill=zero_fill, f64=f64, scale_in=sc)
    got, fl, launched, ran = capi.diag_tgemm_chain_pair(backward, dims, st, sv, slot, sel, A1d, B1d, lives, out0, d8=True, **kw)
    gen, flg, launched_g, ran_g = capi.diag_tgemm_chain_pair(backward, dims, st, sv, slot, sel, A1d, B1d, lives, out0, d8=False, **kw)
    assert not ran_g, "the generic request took the leg-8 kernel"
    assert ran == expect_d8, "leg-8 kernel ran: %s, expected %s" % (ran, expect_d8)
    assert launched == launched_g, (launched, launched_g)
    assert same_bytes(fl, flg), (fl.tolist(), flg.tolist())
    assert np.all(fl == 0), fl.tolist()
    diff = np.argwhere(got.view(np.uint32) != gen.view(np.uint32))
    assert diff.size == 0, "%d elements differ from the generic kernel, first %s (walkers %s)" % (
        len(diff), diff[0].tolist(), sorted(set(diff[:, 0].tolist())))
    assert np.all(got[~wrote] == np.float32(SENT)), "stored outside the live extents"
    kmax = int(max(lives[:, 1].max(), 1))
    tol = (16 * np.sqrt(kmax) + 16 * 8 + 4) * (2.0 ** -53 if f64 else U32) + (2 * U32 if f64 else 0)
    err = np.abs(got.astype(np.float64) - ref)[wrote]
    assert np.all(np.isfinite(got)), "non-finite result"
    assert np.all(err <= tol * bound[wrote] + 1e-300), "off the float64 contraction by up to %.3g of the bound" % float(
        np.max(err / np.maximum(tol * bound[wrote], 1e-300)))
    return got


D8 = (16, 16, 16, 16, 8, 8, 8, 8)      # (m, a, a2, k2, l, p, l2, u)


@pytest.mark.parametrize("backward", [False, True])
def test_stage1_tile_edges(backward):
    """8 x = 32 and 8 y = 32: one tile, the edge, one row / column past it"""
    lives = [(x, 10, y) for x in (1, 4, 5) for y in (1, 4, 5)]
    run_pair(backward, D8, lives, 100 + backward)


@pytest.mark.parametrize("backward", [False, True])
def test_stage2_tile_edges(backward):
    """x y = 32 / 33 / 64 / 65 columns in stage 2"""
    lives = [(4, 10, 8), (3, 9, 11), (8, 16, 8), (5, 12, 13), (8, 3, 4), (11, 10, 3)]
    run_pair(backward, D8, lives, 200 + backward)


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("order", [W_NATURAL, W_PFIRST])
def test_buffer_limit(backward, order):
    """x y = 96 fits the buffer, 99 and 17 x 17 are walked in chunks of x; also (20, 5) -> chunks of 19, (3, 20) -> chunks of 4"""
    dims = (20, 16, 20, 20, 8, 8, 8, 8) if not backward else (16, 20, 16, 20, 8, 8, 8, 8)
    lives = [(8, 10, 12), (9, 10, 11), (17, 12, 17), (20, 8, 5), (3, 9, 20), (12, 16, 8), (2, 5, 2)]
    run_pair(backward, dims, lives, 300 + backward, order=order)


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("kstat", [16, 17, 32])
def test_stage1_k_rounds(backward, kstat):
    """live contracted extent 1 .. 17 at static 16, 17 (no 16-byte loads: the generic kernel takes the launch) and 32"""
    dims = (12, kstat, 12, 12, 8, 8, 8, 8) if not backward else (12, 8, kstat, 12, 8, 8, 8, 8)
    lives = [(5, k, 7) for k in (1, 7, 8, 9, 16, 17)] + [(12, 0, 8), (3, kstat, 12)]
    run_pair(backward, dims, lives, 400 + 10 * kstat + backward, expect_d8=kstat % 4 == 0)


@pytest.mark.parametrize("backward", [False, True])
def test_empty_walkers(backward):
    lives = [(0, 10, 6), (6, 10, 0), (5, 10, 5), (0, 0, 0), (7, 9, 8)]
    run_pair(backward, D8, lives, 500 + backward)


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("nslots", [2, 3])
def test_selector(backward, nslots):
    """walkers of one launch on different site tensors (physical dimension 2 and 3), both storage orders"""
    lives = [(6, 10, 9), (8, 11, 8), (4, 16, 10), (9, 9, 9), (10, 10, 6), (7, 5, 13), (2, 2, 2)]
    run_pair(backward, D8, lives, 600 + 10 * nslots + backward, order=W_PFIRST, nslots=nslots)


@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("tsw", [False, True])
def test_backward_scale_and_layout(scale, tsw):
    lives = [(6, 10, 9), (8, 11, 8), (4, 16, 10), (9, 9, 11), (16, 16, 16), (1, 1, 1)]
    run_pair(True, D8, lives, 700 + 2 * scale + tsw, tsw=tsw, scale=scale)


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("leg", [4, 5, 6, 7])
def test_refused_leg_of_six(backward, leg):
    """one leg of the site tensor is 6: the launch stays on the generic kernel"""
    dims = list(D8)
    dims[leg] = 6
    lives = [(6, 10, 9), (8, 11, 8), (4, 16, 10), (9, 9, 11), (3, 7, 5)]
    run_pair(backward, tuple(dims), lives, 800 + 10 * leg + backward, expect_d8=False)


@pytest.mark.parametrize("backward", [False, True])
def test_refused_float64_form(backward):
    lives = [(6, 10, 9), (8, 11, 8), (4, 16, 10), (9, 9, 11), (3, 7, 5)]
    run_pair(backward, D8, lives, 900 + backward, f64=True, expect_d8=False)


@pytest.mark.parametrize("tsw", [False, True])
def test_refused_masked_extent(tsw):
    """the zero-filling k2 extent of the first site (Tt becomes the persistent first tensor)"""
    lives = [(6, 10, 9), (8, 11, 8), (4, 16, 10), (9, 9, 11), (3, 7, 5)]
    run_pair(True, D8, lives, 950 + tsw, tsw=tsw, zero_fill=True, expect_d8=False)


# ---------------------------------------------------------------------------------------------------------------------------
# the engine: two child processes
def engine_case():
    from peps_amd import synthetic
    L, D, chi, nw = 4, 8, 16, 16
    sitps = synthetic.make_sitps(L, D, noise=0.1)
    ctx = capi.Context(L, L, D, 2, chi, dtype=capi.F32, device=0, max_walkers=nw)
    ctx.state_upload(synthetic.sitps_to_flat(sitps, D, np.float64))
    ctx.set_configs(synthetic.make_configs(L, nw, "heisenberg"))
    amp = np.asarray(ctx.evaluate_amplitude(), dtype=np.float64)
    return dict(amp=amp, d8=np.array([capi.diag_chain_d8_launches()], dtype=np.int64))


def child_main(path):
    np.savez(path, **engine_case())


@pytest.fixture(scope="module")
def runs():
    """(switch off, switch unset): the arrays of the two child processes"""
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for tag, val in (("off", "0"), ("on", None)):
            env = dict(os.environ)
            env.pop("PEPSGPU_CHAIN_D8", None)
            if val is not None:
                env["PEPSGPU_CHAIN_D8"] = val
            path = os.path.join(tmp, tag + ".npz")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, "child (%s) failed:\n%s\n%s" % (tag, p.stdout[-2000:], p.stderr[-4000:])
            with np.load(path) as z:
                res.append({k: z[k] for k in z.files})
    return tuple(res)


def test_engine(runs):
    off, on = runs
    assert np.all(np.isfinite(on["amp"])) and np.all(on["amp"] != 0)
    assert int(off["d8"][0]) == 0, "the leg-8 kernel ran under PEPSGPU_CHAIN_D8=0"
    assert int(on["d8"][0]) > 0, "the leg-8 kernel never ran: the engine fell back to the generic kernel"
    assert same_bytes(off["amp"], on["amp"]), "amplitudes differ between PEPSGPU_CHAIN_D8=0 and unset"


if __name__ == "__main__":
    child_main(sys.argv[1])
