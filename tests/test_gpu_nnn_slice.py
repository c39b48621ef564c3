"""GPU tests of the device-side diagonal-bond slice: trace_dot4_kernel alone against numpy, pepsgpu_nnn_exchange_slice against the
per-plaquette calls on the same context (tests/nnn_slice_ref.py), its error paths, and the host-layer paths that use it (J1-J2 and
triangular Heisenberg energy, gradient samples and the measurement registry) against the hook path (PEPSHOST_NO_DEVICE_SWEEP=1),
end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nnn_slice_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the project's tolerances for "slice against per-bond calls" (tests/test_gpu_energy_slices.py), relative to the largest reference magnitude
TOL = {"f64": 1e-12, "f32": 1e-5, "c128": 1e-12}
ROWS, COLS, NW = 4, 5, 5


def _dtype(name):
    from peps_amd import capi
    return {"f64": capi.F64, "f32": capi.F32, "c128": capi.C128}[name]


# ---- 1. the kernel alone ----
@pytest.mark.parametrize("dims", [(7, 3, 3, 7), (36, 6, 6, 36), (1, 3, 3, 5), (33, 1, 2, 65), (32, 8, 8, 32)])
@pytest.mark.parametrize("dtype", ["f32", "f64", "c128"])
def test_dot4_kernel_matches_einsum(dims, dtype):
    """res = sum a[i][j][k][l] b[l][k][j][i] exp(lsum) for 5 entries, one flagged.  Bound: any two summation orders of N exactly
    representable products differ by at most 2 N u sum |a b| (u = 2^-53; float32 products are exact in float64, float64 and complex
    products add their own rounding, far inside the margin); the factor 2 on top is margin: |err| <= 4 N 2^-53 sum |a b| exp(lsum)."""
    from peps_amd import capi
    I, J, K, L = dims
    nb, N = 5, I * J * K * L
    rng = np.random.default_rng(1000 * I + L)
    np_t = {"f32": np.float32, "f64": np.float64, "c128": np.complex128}[dtype]

    def draw(shape):
        x = rng.normal(size=shape)
        if dtype == "c128":
            x = x + 1j * rng.normal(size=shape)
        return x.astype(np_t)
    a, b = draw((nb, I, J, K, L)), draw((nb, L, K, J, I))
    lsum = rng.uniform(-3.0, 3.0, size=nb)
    flag = np.full(nb, -1, dtype=np.int32)
    flag[2] = 1
    got = capi.diag_dot4(a, b, lsum, flag)
    wide = np.complex128 if dtype == "c128" else np.float64
    a64, b64 = a.astype(wide), b.astype(wide)
    want = np.array([np.einsum("ijkl,lkji", a64[e], b64[e]) for e in range(nb)]) * np.exp(lsum)
    mag = np.array([np.einsum("ijkl,lkji", np.abs(a64[e]), np.abs(b64[e])) for e in range(nb)]) * np.exp(lsum)
    bound = 4.0 * N * 2.0 ** -53 * mag
    err = np.abs(got - want)
    print("dot4", dims, dtype, "err / bound =", (err / bound)[flag < 0])
    assert got.dtype == wide
    assert got[2] == 0.0                                          # the flagged entry: exactly zero
    live = flag < 0
    assert np.all(np.abs(want[live]) > 0) and np.all(err[live] <= bound[live]), (err, bound)
    # without flags every entry is computed
    got_all = capi.diag_dot4(a, b, lsum)
    assert np.all(np.abs(got_all - want) <= bound) and np.array_equal(got_all[live], got[live])


# ---- 2. the slice against the per-plaquette calls ----
def _context(dtype, D, chi, rows=ROWS):
    from peps_amd import capi
    flat = ref.rect_state(rows, COLS, D)
    if dtype == "c128":
        flat = flat * np.exp(2j * np.pi * np.random.default_rng(3).uniform(size=flat.shape))
    cfgs = ref.walkers(rows, COLS)
    assert cfgs.shape == (NW, rows, COLS)
    ctx = capi.Context(rows, COLS, D, 2, chi, dtype=_dtype(dtype), max_walkers=NW)
    ctx.state_upload(flat)
    ctx.set_configs(cfgs)
    return ctx, cfgs


def _differ(cfgs, row):
    """[n][cols - 1][2]: the two ends of the diagonal differ"""
    return np.stack([np.stack([np.not_equal(*ref.diagonal_ends(cfgs, row, col, kind)) for kind in (0, 1)], axis=-1)
                     for col in range(COLS - 1)], axis=1)


@pytest.mark.parametrize("dtype,D,chi,rows", [("f64", 3, 7, ROWS), ("f32", 3, 7, ROWS), ("c128", 3, 7, ROWS), ("f64", 6, 36, ROWS),
                                              ("f64", 6, 36, 6)])
def test_nnn_slice_matches_the_per_plaquette_calls(dtype, D, chi, rows):
    """Every row pair of a full row pass, masks 3, 1 and 2, against the per-plaquette calls.  D = 6, chi = 36 on the 4 x 5 lattice: the
    boundary bonds of 36 sit at the outer row pairs only (closure operands 1 x 6 x 6 x 36 and 36 x 6 x 6 x 1, the middle pair has 6 x 6 x 6
    x 6), so the kernel's tiles cross 32 in one index at a time; on 6 x 5 the middle row pair has 36 on both sides (36 x 6 x 6 x 36: both
    indices cross the tile at once, inside the slice)."""
    from peps_amd import capi
    ctx, cfgs = _context(dtype, D, chi, rows)
    tol = TOL[dtype]
    seen = np.zeros((2, 2), dtype=bool)                          # [kind][differs]
    ctx.generate_bmps_approach(capi.UP)
    for row in range(rows - 1):
        got, sizes = {}, {}
        for mask in (3, 1, 2):
            got[mask] = ctx.nnn_exchange_slice(row, mask)
            sizes[mask] = (ctx.bten2_stack_size(capi.LEFT), ctx.bten2_stack_size(capi.RIGHT))
        want, want_sizes = ref.per_plaquette_reference(ctx, cfgs, row)
        differ = _differ(cfgs, row)
        for kind in (0, 1):
            seen[kind, 1] |= differ[..., kind].any()
            seen[kind, 0] |= (~differ[..., kind]).any()
        scale = np.max(np.abs(want))
        for mask in (3, 1, 2):
            val = got[mask]
            assert val.shape == (NW, COLS - 1, 2) and val.dtype == want.dtype
            assert sizes[mask] == want_sizes, (row, mask, sizes[mask], want_sizes)
            for kind in (0, 1):
                v, w, df = val[..., kind], want[..., kind], differ[..., kind]
                if not (mask >> kind) & 1:
                    assert np.all(v == 0.0), (row, mask, kind)    # masked off: exactly zero
                    continue
                assert np.all(v[~df] == 0.0), (row, mask, kind)   # identity moves: exactly zero
                err = np.max(np.abs(v - w)[df]) / scale if df.any() else 0.0
                print("nnn slice", dtype, D, "row", row, "mask", mask, "kind", kind, "rel err", err)
                assert err < tol, (row, mask, kind, err)
        if row + 2 < rows:
            ctx.shift_bmps_window(capi.DOWN)
    assert seen.all(), seen                                      # both "differs" and "equal" occurred for each diagonal kind
    ctx.close()


# ---- 3. error paths ----
def test_nnn_slice_error_paths():
    from peps_amd import capi
    ctx, cfgs = _context("f64", 3, 7)
    lib, h = ctx._l, ctx._h
    val = np.zeros((NW, COLS - 1, 2))
    # before any boundary MPS exists for the row pair: status 3 (the DOWN stack holds its vacuum only)
    assert lib.pepsgpu_nnn_exchange_slice(h, 0, 3, capi._dp(val)) == 3
    ctx.generate_bmps_approach(capi.UP)
    for row, mask in ((-1, 3), (ROWS - 1, 3), (0, 0), (0, 4)):
        assert lib.pepsgpu_nnn_exchange_slice(h, row, mask, capi._dp(val)) == 1, (row, mask)
        with pytest.raises(ValueError):
            ctx.nnn_exchange_slice(row, mask)
    assert lib.pepsgpu_nnn_exchange_slice(h, 0, 3, None) == 1      # null buffer
    # a configuration override is active: refused (the slice reads the walkers' own table), usable again once it is cleared
    ctx.cfg_override_slice(capi.HORIZONTAL, 1, 1 - cfgs[:, 1, :])
    assert lib.pepsgpu_nnn_exchange_slice(h, 0, 3, capi._dp(val)) == 3
    ctx.cfg_override_slice(capi.HORIZONTAL, 1)
    # the context computes a correct slice afterwards
    got = ctx.nnn_exchange_slice(0, 3)
    want, _ = ref.per_plaquette_reference(ctx, cfgs, 0)
    differ = _differ(cfgs, 0)
    assert differ.any() and np.max(np.abs(got - want)[differ]) < 1e-12 * np.max(np.abs(want))
    assert np.all(got[~differ] == 0.0)
    ctx.close()


# ---- 4. the host layer, end to end ----
_E2E = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from peps_amd import capi, hostapi, synthetic

def cx(a):
    a = np.asarray(a)
    return [[float(x.real), float(x.imag)] for x in a.ravel()] if np.iscomplexobj(a) else [float(x) for x in a.ravel()]

L, D, chi, n = 6, 4, 12, 12
J1J2 = (1.0, 1.0, 0.5, 0.4, 0.0)
flat = synthetic.sitps_to_flat(synthetic.make_sitps(L, D, noise=0.5), D)
cflat = flat * np.exp(2j * np.pi * np.random.default_rng(3).uniform(size=flat.shape))
cfgs = synthetic.make_configs(L, n, "heisenberg", seed0=13)
seeds = np.arange(n, dtype=np.uint64) + 90
out, calls = {}, 0          # calls: energy / measurement passes made
for name, dt in (("f64", 1), ("f32", 0)):
    o = {}
    for model, prm in (("j1j2", J1J2), ("triangle", ())):
        for holes in (True, False):
            _, en, _, psi = hostapi.energy_and_holes(flat, cfgs, chi, model, prm, holes, dt)
            calls += 1
            key = model + ("_holes" if holes else "")
            o[key + "_energy"], o[key + "_psi"] = cx(en), cx(psi)
        obs, _ = hostapi.measure(flat, cfgs, chi, model, prm, dtype=dt)
        calls += 1
        for k in ("energy", "bond_energy_h", "bond_energy_v", "bond_energy_dr", "bond_energy_ur", "SmSp_row", "SpSm_row"):
            if k in obs:
                o[model + "_measure_" + k] = cx(obs[k])
    out[name] = o
packed, _, _ = hostapi.mc_energy_grad_partial(flat, cfgs, seeds, chi, "tnn3", "j1j2", J1J2, 1, 2, 1)
calls += 2                  # one energy pass per sample
out["f64"]["j1j2_tnn3_packed"] = cx(packed)
_, en, _, psi = hostapi.energy_and_holes_complex(cflat, cfgs, chi, "j1j2", J1J2, False)
calls += 1
out["c128"] = {"j1j2_energy": cx(en), "j1j2_psi": cx(psi)}
out["passes"] = calls
out["slice_calls"] = capi.diag_nnn_slice_calls()
print(json.dumps(out))
"""


def test_host_layer_nnn_slices_match_the_hook_path():
    """End to end on 6 x 6, D = 4, chi = 12, 12 walkers, in child processes with and without PEPSHOST_NO_DEVICE_SWEEP=1:
    energy_and_holes for j1j2 and triangle (with and without holes, f64 and f32), their measure registries, mc_energy_grad_partial with
    the three-site updater on j1j2, and energy_and_holes_complex for j1j2 -- the device slices against the per-bond hooks.  The process-wide
    slice counter proves which path ran: 0 under the hooks, exactly (Ly - 1) per energy or measurement pass on the device.  The f64
    J1-J2 energies are also the oracle's, at the tolerance of tests/test_gpu_host.py::test_j1j2_energy_fixed_configs_and_exact_sum."""
    from peps_amd import synthetic
    from oracle import vmc
    from oracle.bmps import BMPSTruncateParams
    L, D, chi, n = 6, 4, 12, 12
    res = {}
    for name, env in (("device", {}), ("hook", {"PEPSHOST_NO_DEVICE_SWEEP": "1"})):
        r = subprocess.run([sys.executable, "-c", _E2E, ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stderr[-2000:]
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print("slice calls: device", res["device"]["slice_calls"], "hook", res["hook"]["slice_calls"], "passes", res["device"]["passes"])
    assert res["hook"]["slice_calls"] == 0
    assert res["device"]["slice_calls"] == (L - 1) * res["device"]["passes"]
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
    for key in ("j1j2_measure_bond_energy_dr", "j1j2_measure_bond_energy_ur", "j1j2_measure_SmSp_row", "j1j2_measure_SpSm_row",
                "triangle_measure_bond_energy_ur", "triangle_measure_SmSp_row"):
        assert key in res["device"]["f64"], key
    assert "triangle_measure_bond_energy_dr" not in res["device"]["f64"]   # the triangular model reports its one diagonal only
    # the oracle on every walker (tolerance of test_j1j2_energy_fixed_configs_and_exact_sum for float64)
    s = synthetic.make_sitps(L, D, noise=0.5)
    cfgs = synthetic.make_configs(L, n, "heisenberg", seed0=13)
    model = vmc.SquareSpinOneHalfJ1J2XXZModelOBC(1.0, 1.0, 0.5, 0.4, 0.0)
    tp = BMPSTruncateParams.SVD(chi, chi, 0.0)
    for w in range(n):
        e, _, _ = model.CalEnergyAndHoles(s, vmc.TPSWaveFunctionComponent(s, cfgs[w], tp), False)
        for key in ("j1j2_energy", "j1j2_holes_energy"):
            got = res["device"]["f64"][key][w]
            print("oracle", key, w, abs(got - e))
            assert abs(got - e) < 1e-9 * max(1.0, abs(e)) * 10, (key, w, got, e)
