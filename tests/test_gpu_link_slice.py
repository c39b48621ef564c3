"""GPU tests of the device-side link slice of the triangular J1-J2 model: its candidate kernel alone against numpy,
pepsgpu_link_exchange_slice in both orientations against the per-call traces on the same context (tests/link_slice_ref.py), its error
paths, and the host-layer paths that use it (trij1j2 energy, measurement registry and gradient samples) against the hook path
(PEPSHOST_NO_DEVICE_SWEEP=1), end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import link_slice_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the project's tolerances for "slice against per-call" (tests/test_gpu_nnn_slice.py), relative to the largest reference magnitude
TOL = {"f64": 1e-12, "f32": 1e-5, "c128": 1e-12}
NW = 5
HOR, VER = ref.HOR, ref.VER


def _dtype(name):
    from peps_amd import capi
    return {"f64": capi.F64, "f32": capi.F32, "c128": capi.C128}[name]


# ---- 1. the candidate kernel alone ----
def test_link_cand_kernel_matches_numpy():
    """The five walkers of the slice test (d = 2) and five random d = 3 walkers (an exchange is not a flip) on 4 x 5: every 2 x 3 and
    every 3 x 2 window of the lattice -- the ones at each boundary among them -- both sqrt5 kinds, exact integer equality of the
    candidate table and of the flags; a window that leaves the lattice is refused."""
    from peps_amd import capi
    rows, cols = 4, 5
    tables = ((2, ref.walkers(rows, cols)), (3, np.random.default_rng(7).integers(0, 3, size=(NW, rows, cols)).astype(np.int32)))
    seen = np.zeros((2, 2, 2), dtype=bool)                       # [orient][kind][differs]
    for d, cfgs in tables:
        for orient, (dr, dc) in ((HOR, (1, 2)), (VER, (2, 1))):
            for r in range(rows - dr):
                for c in range(cols - dc):
                    cand, flag = capi.diag_link_cand(cfgs, d, orient, r, c)
                    want_cand, want_flag = ref.sqrt5_candidates(cfgs, orient, r, c)
                    assert cand.dtype == np.int32 and np.array_equal(cand, want_cand), (d, orient, r, c)
                    assert np.array_equal(flag, want_flag), (d, orient, r, c)
                    for q in (0, 1):
                        seen[orient, q, 1] |= (flag[:, q] < 0).any()
                        seen[orient, q, 0] |= (flag[:, q] > 0).any()
            for r, c in ((rows - dr, 0), (0, cols - dc), (-1, 0), (0, -1)):
                with pytest.raises(ValueError):
                    capi.diag_link_cand(cfgs, d, orient, r, c)
    assert seen.all(), seen
    with pytest.raises(ValueError):
        capi.diag_link_cand(tables[1][1], 2, HOR, 0, 0)          # a state outside [0, d)
    with pytest.raises(ValueError):
        capi.diag_link_cand(tables[0][1], 2, 2, 0, 0)            # a bad orientation


# ---- 2. / 3. the slice against the per-call traces ----
def _context(dtype, D, chi, rows, cols):
    from peps_amd import capi
    flat = ref.rect_state(rows, cols, D)
    if dtype == "c128":
        flat = flat * np.exp(2j * np.pi * np.random.default_rng(3).uniform(size=flat.shape))
    cfgs = ref.walkers(rows, cols)
    assert cfgs.shape == (NW, rows, cols)
    ctx = capi.Context(rows, cols, D, 2, chi, dtype=_dtype(dtype), max_walkers=NW)
    ctx.state_upload(flat)
    ctx.set_configs(cfgs)
    return ctx, cfgs


def _check_pair(ctx, cfgs, orient, slice1, masks, dtype, seen):
    """the slice of one row / column pair under every mask against the per-call sequence; returns the tables by mask"""
    from peps_amd import capi
    lo, hi = (capi.LEFT, capi.RIGHT) if orient == HOR else (capi.UP, capi.DOWN)
    n, rows, cols = cfgs.shape
    N = cols if orient == HOR else rows
    got, sizes = {}, {}
    for mask in masks:
        got[mask] = ctx.link_exchange_slice(orient, slice1, mask)
        sizes[mask] = (ctx.bten2_stack_size(lo), ctx.bten2_stack_size(hi))
    want, want_sizes = ref.per_call_reference(ctx, cfgs, orient, slice1)
    differ, exists = ref.differ_table(cfgs, orient, slice1), ref.exists_table(cfgs, orient, slice1)
    for kind in range(4):
        seen[kind, 1] |= differ[..., kind].any()
        seen[kind, 0] |= (~differ[..., kind] & exists[None, :, kind]).any()
    scale = np.max(np.abs(want))
    for mask in masks:
        val = got[mask]
        assert val.shape == (n, N - 1, 4) and val.dtype == want.dtype
        assert sizes[mask] == want_sizes, (orient, slice1, mask, sizes[mask], want_sizes)
        for kind in range(4):
            v, w, df = val[..., kind], want[..., kind], differ[..., kind]
            if not (mask >> kind) & 1:
                assert np.all(v == 0.0), (orient, slice1, mask, kind)     # masked off: exactly zero
                continue
            assert np.all(v[~df] == 0.0), (orient, slice1, mask, kind)    # identity moves and positions without the link: exactly zero
            err = np.max(np.abs(v - w)[df]) / scale if df.any() else 0.0
            print("link slice", dtype, "orient", orient, "pair", slice1, "mask", mask, "kind", kind, "rel err", err)
            assert err < TOL[dtype], (orient, slice1, mask, kind, err)
    return got


GRID = [("f64", 3, 7, 4), ("f32", 3, 7, 4), ("c128", 3, 7, 4), ("f64", 6, 36, 4), ("f64", 6, 36, 6)]


@pytest.mark.parametrize("dtype,D,chi,rows", GRID)
def test_horizontal_link_slice_matches_the_per_call_traces(dtype, D, chi, rows):
    """Every row pair of a full row pass on rows x 5, masks 15, 12, 3, 8 and 4, against ReplaceNNNSiteTrace / ReplaceSqrt5DistTwoSiteTrace
    per link.  The shapes are those of tests/test_gpu_nnn_slice.py for its reason: at D = 6, chi = 36 the closure operands cross the
    32-wide tile of trace_dot4_kernel in one index at a time on 4 x 5 (outer row pairs) and in both at once on 6 x 5 (middle pair).
    Under mask 3 the two diagonal kinds are also those of nnn_exchange_slice(row, 3)."""
    from peps_amd import capi
    cols = 5
    ctx, cfgs = _context(dtype, D, chi, rows, cols)
    seen = np.zeros((4, 2), dtype=bool)                          # [kind][differs]
    ctx.generate_bmps_approach(capi.UP)
    for row in range(rows - 1):
        got = _check_pair(ctx, cfgs, HOR, row, (15, 12, 3, 8, 4), dtype, seen)
        nnn = ctx.nnn_exchange_slice(row, 3)
        scale = np.max(np.abs(nnn))
        assert scale > 0 and np.max(np.abs(got[3][..., :2] - nnn)) < TOL[dtype] * scale, row
        assert np.array_equal(got[3][..., :2] == 0.0, nnn == 0.0)
        if row + 2 < rows:
            ctx.shift_bmps_window(capi.DOWN)
    assert seen.all(), seen                                      # both "differs" and "equal" occurred for every kind
    ctx.close()


@pytest.mark.parametrize("dtype,D,chi,cols", GRID)
def test_vertical_link_slice_matches_the_per_call_traces(dtype, D, chi, cols):
    """Every column pair of a full column pass on 5 x cols (the transposed shapes; five rows: two ShiftBTen2Window(DOWN) per pair),
    masks 12, 8 and 4, against ReplaceSqrt5DistTwoSiteTrace(VERTICAL) per steep link."""
    from peps_amd import capi
    rows = 5
    ctx, cfgs = _context(dtype, D, chi, rows, cols)
    seen = np.zeros((4, 2), dtype=bool)
    ctx.generate_bmps_approach(capi.LEFT)
    for col in range(cols - 1):
        _check_pair(ctx, cfgs, VER, col, (12, 8, 4), dtype, seen)
        if col + 2 < cols:
            ctx.shift_bmps_window(capi.RIGHT)
    assert seen[2:].all() and not seen[:2].any(), seen           # the steep kinds both ways; a column pair has no diagonal kinds
    ctx.close()


@pytest.mark.parametrize("cols", [2, 3])
def test_link_and_diagonal_slices_on_the_smallest_lattices(cols):
    """3 x 2 and 3 x 3, f64, D = 3, chi = 7: the lattices at which the loop bounds of the walk bite.  Two columns: a row pair is one
    plaquette without a sqrt5 window (mask 12 is all zeros); three columns: exactly one sqrt5 window beside two plaquettes; three rows:
    a column pair is one window and no ShiftBTen2Window.  Every row pair under masks 15, 12 and 3 (mask 3 also against
    nnn_exchange_slice) and every column pair under masks 12, 8 and 4, against the per-call traces, BTen2 stack sizes included.  Every
    kind the lattice has occurs with differing and with equal end states."""
    from peps_amd import capi
    rows, dtype = 3, "f64"
    ctx, cfgs = _context(dtype, 3, 7, rows, cols)
    seen = {HOR: np.zeros((4, 2), dtype=bool), VER: np.zeros((4, 2), dtype=bool)}
    ctx.generate_bmps_approach(capi.UP)
    for row in range(rows - 1):
        got = _check_pair(ctx, cfgs, HOR, row, (15, 12, 3), dtype, seen[HOR])
        if cols == 2:
            assert np.all(got[12] == 0.0), row
        nnn = ctx.nnn_exchange_slice(row, 3)
        scale = np.max(np.abs(nnn))
        assert scale > 0 and np.max(np.abs(got[3][..., :2] - nnn)) < TOL[dtype] * scale, row
        assert np.array_equal(got[3][..., :2] == 0.0, nnn == 0.0)
        if row + 2 < rows:
            ctx.shift_bmps_window(capi.DOWN)
    ctx.generate_bmps_approach(capi.LEFT)
    for col in range(cols - 1):
        _check_pair(ctx, cfgs, VER, col, (12, 8, 4), dtype, seen[VER])
        if col + 2 < cols:
            ctx.shift_bmps_window(capi.RIGHT)
    for orient, n in ((HOR, rows), (VER, cols)):
        exists = np.any([ref.exists_table(cfgs, orient, s) for s in range(n - 1)], axis=(0, 1))
        assert list(exists) == ([True, True, cols > 2, cols > 2] if orient == HOR else [False, False, True, True])
        assert seen[orient][exists].all() and not seen[orient][~exists].any(), (orient, seen[orient])
    ctx.close()


# ---- 4. error paths ----
def test_link_slice_error_paths():
    from peps_amd import capi
    rows, cols = 4, 5
    ctx, cfgs = _context("f64", 3, 7, rows, cols)
    lib, h = ctx._l, ctx._h
    val = np.zeros((NW, cols - 1, 4))
    call = lambda orient, s, mask, buf=val: lib.pepsgpu_link_exchange_slice(h, orient, s, mask, capi._dp(buf) if buf is not None else None)
    # before any boundary MPS exists for the pair: status 3
    assert call(HOR, 0, 15) == 3
    assert call(VER, 0, 12) == 3
    ctx.generate_bmps_approach(capi.UP)
    bad = ((HOR, -1, 15), (HOR, rows - 1, 15), (VER, -1, 12), (VER, cols - 1, 12),      # a slice outside the lattice
           (HOR, 0, 0), (HOR, 0, 16), (VER, 0, 0), (VER, 0, 16),                         # mask 0 or 16
           (VER, 0, 13), (VER, 0, 14), (VER, 0, 1),                                      # a vertical call with bit 0 or 1
           (2, 0, 12), (-1, 0, 12))                                                      # a bad orientation
    for orient, s, mask in bad:
        assert call(orient, s, mask) == 1, (orient, s, mask)
        with pytest.raises(ValueError):
            ctx.link_exchange_slice(orient, s, mask)
    assert call(HOR, 0, 15, None) == 1                               # null buffer
    # a configuration override is active: refused (the slice reads the walkers' own table), usable again once it is cleared
    ctx.cfg_override_slice(capi.HORIZONTAL, 1, 1 - cfgs[:, 1, :])
    assert call(HOR, 0, 15) == 3
    ctx.cfg_override_slice(capi.HORIZONTAL, 1)
    # the context computes a correct slice afterwards
    got = ctx.link_exchange_slice(HOR, 0, 15)
    want, _ = ref.per_call_reference(ctx, cfgs, HOR, 0)
    differ = ref.differ_table(cfgs, HOR, 0)
    assert differ.any() and np.max(np.abs(got - want)[differ]) < 1e-12 * np.max(np.abs(want))
    assert np.all(got[~differ] == 0.0)
    ctx.close()
    # a column pair needs three rows
    ctx2 = capi.Context(2, 4, 3, 2, 7, dtype=capi.F64, max_walkers=NW)
    ctx2.state_upload(ref.rect_state(2, 4, 3))
    ctx2.set_configs(ref.walkers(2, 4))
    ctx2.generate_bmps_approach(capi.LEFT)
    val2 = np.zeros((NW, 1, 4))
    assert ctx2._l.pepsgpu_link_exchange_slice(ctx2._h, VER, 0, 12, capi._dp(val2)) == 1
    ctx2.close()


# ---- 5. the host layer, end to end ----
_E2E = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from peps_amd import capi, hostapi, synthetic

def cx(a):
    a = np.asarray(a)
    return [[float(x.real), float(x.imag)] for x in a.ravel()] if np.iscomplexobj(a) else [float(x) for x in a.ravel()]

L, D, chi, n = 6, 4, 12, 12
J2 = (0.4,)
flat = synthetic.sitps_to_flat(synthetic.make_sitps(L, D, noise=0.5), D)
cflat = flat * np.exp(2j * np.pi * np.random.default_rng(3).uniform(size=flat.shape))
cfgs = synthetic.make_configs(L, n, "heisenberg", seed0=13)
seeds = np.arange(n, dtype=np.uint64) + 90
out, calls = {}, 0          # calls: trij1j2 energy / measurement passes made
for name, dt in (("f64", 1), ("f32", 0)):
    o = {}
    for holes in (True, False):
        _, en, _, psi = hostapi.energy_and_holes(flat, cfgs, chi, "trij1j2", J2, holes, dt)
        calls += 1
        key = "trij1j2" + ("_holes" if holes else "")
        o[key + "_energy"], o[key + "_psi"] = cx(en), cx(psi)
    obs, _ = hostapi.measure(flat, cfgs, chi, "trij1j2", J2, dtype=dt)
    calls += 1
    for k in ("energy", "bond_energy_h", "bond_energy_v", "bond_energy_ur", "SmSp_row", "SpSm_row"):
        o["trij1j2_measure_" + k] = cx(obs[k])
    out[name] = o
packed, _, _ = hostapi.mc_energy_grad_partial(flat, cfgs, seeds, chi, "exchange", "trij1j2", J2, 1, 2, 1)
calls += 2                  # one energy pass per sample
out["f64"]["trij1j2_exchange_packed"] = cx(packed)
links, nnn = capi.diag_link_slice_calls(), capi.diag_nnn_slice_calls()      # after the last trij1j2 pass of the real element types
packed, _, _ = hostapi.mc_energy_grad_partial(flat, cfgs, seeds, chi, "exchange", "triangle", (), 1, 2, 1)
out["f64"]["triangle_exchange_packed"] = cx(packed)
out["triangle_link_calls"] = capi.diag_link_slice_calls() - links       # (the triangular model has its diagonal slice, no link slice)
_, en, _, psi = hostapi.energy_and_holes_complex(cflat, cfgs, chi, "trij1j2", J2, False)
calls += 1
out["c128"] = {"trij1j2_energy": cx(en), "trij1j2_psi": cx(psi)}
out["passes"] = calls
out["link_calls"] = capi.diag_link_slice_calls()
out["nnn_calls"] = nnn
print(json.dumps(out))
"""


def test_host_layer_link_slices_match_the_hook_path():
    """End to end on 6 x 6, D = 4, chi = 12, 12 walkers, in child processes with and without PEPSHOST_NO_DEVICE_SWEEP=1: trij1j2
    energy_and_holes (with and without holes, f64 and f32), its measure registry, energy_and_holes_complex, and mc_energy_grad_partial
    with the exchange updater for trij1j2 and triangle (holes on the device) -- the device slices against the per-bond hooks.  The
    process-wide counter proves which path ran: 0 under the hooks, (Ly - 1) + (Lx - 1) link slices per trij1j2 pass on the device, and
    no diagonal slice (pepsgpu_nnn_exchange_slice) in the trij1j2 passes.  The f64 energies are also the oracle's, at the tolerance of
    tests/test_gpu_host.py."""
    from peps_amd import synthetic
    from oracle import vmc
    from oracle.bmps import BMPSTruncateParams
    L, D, chi, n = 6, 4, 12, 12
    res = {}
    for name, env in (("device", {}), ("hook", {"PEPSHOST_NO_DEVICE_SWEEP": "1"})):
        r = subprocess.run([sys.executable, "-c", _E2E, ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stderr[-2000:]
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print("link slice calls: device", res["device"]["link_calls"], "hook", res["hook"]["link_calls"], "passes", res["device"]["passes"])
    assert res["hook"]["link_calls"] == 0 and res["hook"]["nnn_calls"] == 0
    assert res["device"]["link_calls"] == res["device"]["passes"] * ((L - 1) + (L - 1))
    assert res["device"]["nnn_calls"] == 0                         # counted after the last trij1j2 pass of the real element types
    assert res["device"]["triangle_link_calls"] == 0
    for dt in ("f64", "f32", "c128"):
        tol = TOL[dt]
        assert set(res["hook"][dt]) == set(res["device"][dt])
        for key in res["hook"][dt]:
            a, b = np.array(res["device"][dt][key]), np.array(res["hook"][dt][key])
            if a.ndim == 2:
                a, b = a[:, 0] + 1j * a[:, 1], b[:, 0] + 1j * b[:, 1]
            assert a.shape == b.shape and a.size > 0, (dt, key)
            scale = max(np.max(np.abs(b)), 1e-300)
            if key.endswith("packed"):
                print(dt, key, np.max(np.abs(a - b)) / np.sum(np.abs(b)))
                assert np.max(np.abs(a - b)) < tol * np.sum(np.abs(b)), (dt, key)
            else:
                print(dt, key, np.max(np.abs(a - b)) / scale)
                assert np.max(np.abs(a - b)) < tol * scale, (dt, key, np.max(np.abs(a - b)) / scale)
    # the oracle on every walker (tolerance of tests/test_gpu_host.py for float64)
    s = synthetic.make_sitps(L, D, noise=0.5)
    cfgs = synthetic.make_configs(L, n, "heisenberg", seed0=13)
    model = vmc.SpinOneHalfTriJ1J2HeisenbergSqrPEPS(0.4)
    tp = BMPSTruncateParams.SVD(chi, chi, 0.0)
    for w in range(n):
        e, _, _ = model.CalEnergyAndHoles(s, vmc.TPSWaveFunctionComponent(s, cfgs[w], tp), False)
        for key in ("trij1j2_energy", "trij1j2_holes_energy"):
            got = res["device"]["f64"][key][w]
            print("oracle", key, w, abs(got - e))
            assert abs(got - e) < 1e-9 * max(1.0, abs(e)) * 10, (key, w, got, e)

