"""GPU tests of the device-side energy slices: pepsgpu_onsite_slice (one-site moves, TFIM) and pepsgpu_nn_exchange_slice_tab
(exchange moves of every element type, pair table, psi per bond), each against the per-site / per-bond calls on the same context,
and the host-layer paths that use them against the hook path (PEPSHOST_NO_DEVICE_SWEEP=1), end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from peps_amd import synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, D, CHI, NW = 6, 4, 12, 8
TOL = {"f64": 1e-12, "f32": 1e-5, "c128": 1e-12}


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _state(dtype):
    from peps_amd import capi
    flat = synthetic.sitps_to_flat(synthetic.make_sitps(L, D, noise=0.5), D)
    if dtype == "c128":
        flat = flat * np.exp(2j * np.pi * np.random.default_rng(3).uniform(size=flat.shape))
    cfgs = synthetic.make_configs(L, NW, "heisenberg", seed0=13)
    ctx = capi.Context(L, L, D, 2, CHI, dtype={"f64": capi.F64, "f32": capi.F32, "c128": capi.C128}[dtype], max_walkers=NW)
    ctx.state_upload(flat)
    ctx.set_configs(cfgs)
    return ctx, cfgs


def _passes():
    """(orientation, BMPS approach, window shift, BTen low / high side) of the row pass and of the column pass"""
    from peps_amd import capi
    return ((capi.HORIZONTAL, capi.UP, capi.DOWN, capi.LEFT, capi.RIGHT), (capi.VERTICAL, capi.LEFT, capi.RIGHT, capi.UP, capi.DOWN))


def _site(orient, s, j):
    from peps_amd import capi
    return (s, j) if orient == capi.HORIZONTAL else (j, s)


def _onsite_reference(ctx, orient, lo, hi, s, table, holes):
    """the per-site sequence: InitBTen, GrowFullBTen(.., 1), Trace, per site (PunchHole and) ReplaceOneSiteTrace + ShiftBTenWindow"""
    ctx.init_bten(lo, s)
    ctx.grow_full_bten(hi, s, 1, True)
    psi = ctx.trace(*_site(orient, s, 0), orient)
    cfg = ctx.get_configs()
    vals = []
    for j in range(L):
        r, c = _site(orient, s, j)
        if holes:
            ctx.punch_hole_store(r, c, orient)
        vals.append(ctx.replace_one_trace(r, c, orient, table[cfg[:, r, c]]))
        if j + 1 < L:
            ctx.shift_bten_window(hi)
    return psi, np.stack(vals, axis=1)


def _exchange_reference(ctx, orient, lo, hi, s, cand_of_bond, per_bond, remain=2):
    """the per-bond sequence: InitBTen, GrowFullBTen(.., remain), Trace, per bond (Trace and) ReplaceNNSiteTrace + ShiftBTenWindow"""
    ctx.init_bten(lo, s)
    ctx.grow_full_bten(hi, s, remain, True)
    psi0 = ctx.trace(*_site(orient, s, 0), orient)
    psis, exs = [], []
    for j in range(L - 1):
        r, c = _site(orient, s, j)
        if per_bond:
            psis.append(ctx.trace(r, c, orient))
        exs.append(ctx.replace_nn_trace(r, c, orient, cand_of_bond(j))[:, 0])
        if remain == 1 or j + 2 < L:
            ctx.shift_bten_window(hi)
    return psi0, (np.stack(psis, axis=1) if per_bond else None), np.stack(exs, axis=1)


@pytest.mark.parametrize("dtype", ["f64", "f32", "c128"])
def test_onsite_slice_matches_the_per_site_calls(dtype):
    ctx, _ = _state(dtype)
    tol = TOL[dtype]
    tables = (np.array([[1], [0]], dtype=np.int32), np.array([[1, 0], [0, 1]], dtype=np.int32))     # the TFIM flip; flip + keep
    for orient, approach, step, lo, hi in _passes():
        ctx.generate_bmps_approach(approach)
        for s in range(L):
            for table in tables:
                psi, cand = ctx.onsite_slice(orient, s, table)
                assert cand.shape == (NW, L, table.shape[1])
                psi_r, cand_r = _onsite_reference(ctx, orient, lo, hi, s, table, False)
                assert _rel(psi, psi_r) < tol and _rel(cand, cand_r) < tol, (orient, s, _rel(psi, psi_r), _rel(cand, cand_r))
            if s + 1 < L:
                ctx.shift_bmps_window(step)
    ctx.close()


def test_onsite_slice_stores_the_holes_of_the_per_site_calls():
    """punch_holes: the holes the slice leaves in HBM are those pepsgpu_punch_hole (out == NULL) stores site by site -- read back
    through the gradient accumulators of two contexts"""
    from peps_amd import capi
    flip = np.array([[1], [0]], dtype=np.int32)
    rng = np.random.default_rng(5)
    psi_w, e_w = rng.uniform(0.5, 1.5, NW), rng.normal(size=NW)
    grads = []
    for use_slice in (True, False):
        ctx, _ = _state("f64")
        ctx.generate_bmps_approach(capi.UP)
        for row in range(L):
            if use_slice:
                ctx.onsite_slice(capi.HORIZONTAL, row, flip, punch_holes=True)
            else:
                _onsite_reference(ctx, capi.HORIZONTAL, capi.LEFT, capi.RIGHT, row, flip, True)
            if row + 1 < L:
                ctx.shift_bmps_window(capi.DOWN)
        ctx.grad_reset()
        ctx.grad_accumulate(psi_w, e_w)
        grads.append(ctx.grad_read())
        ctx.close()
    for a, b in zip(grads[0], grads[1]):
        assert np.max(np.abs(b)) > 0 and _rel(a, b) < 1e-12


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_exchange_slice_tab_without_table_is_the_real_exchange_slice(dtype):
    """a NULL table and psi_per_bond = 0 on a real context: bit for bit pepsgpu_nn_exchange_slice (with and without holes)"""
    ctx, _ = _state(dtype)
    for orient, approach, step, lo, hi in _passes():
        ctx.generate_bmps_approach(approach)
        for s in range(L):
            for holes in (False, True):
                a = ctx.nn_exchange_slice(orient, s, holes)
                b = ctx.nn_exchange_slice_tab(orient, s, holes)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (orient, s, holes)
            if s + 1 < L:
                ctx.shift_bmps_window(step)
    ctx.close()


def test_exchange_slice_tab_on_a_complex_context():
    from peps_amd import capi
    ctx, cfgs = _state("c128")
    with pytest.raises(ValueError):                       # the real-only entry point keeps its contract
        ctx.nn_exchange_slice(capi.HORIZONTAL, 0)
    for orient, approach, step, lo, hi in _passes():
        ctx.generate_bmps_approach(approach)
        for s in range(L):
            for holes in (False, True):
                psi, ex = ctx.nn_exchange_slice_tab(orient, s, holes)
                remain = 1 if holes else 2

                def cand(j):
                    (r1, c1), (r2, c2) = _site(orient, s, j), _site(orient, s, j + 1)
                    return np.stack([cfgs[:, r2, c2], cfgs[:, r1, c1]], axis=-1)[:, None, :]
                psi_r, _, ex_r = _exchange_reference(ctx, orient, lo, hi, s, cand, False, remain)
                assert psi.dtype == np.complex128 and _rel(psi, psi_r) < 1e-12
                differ = np.stack([cfgs[:, _site(orient, s, j)[0], _site(orient, s, j)[1]]
                                   != cfgs[:, _site(orient, s, j + 1)[0], _site(orient, s, j + 1)[1]] for j in range(L - 1)], axis=1)
                assert differ.any() and (~differ).any()
                assert np.max(np.abs(ex - ex_r)[differ]) < 1e-12 * np.max(np.abs(ex_r))
                # an identical exchange is skipped: psi of the slice
                assert np.array_equal(ex[~differ], np.broadcast_to(psi[:, None], ex.shape)[~differ])
            if s + 1 < L:
                ctx.shift_bmps_window(step)
    ctx.close()


def _fermion_exchange_table(st, order):
    """TPSWaveFunctionComponent::ExchangeTable of the host layer: the exchange of two sites adjacent in the mode order over pairs
    of extended states (state + d * variant)"""
    from peps_amd import fermion
    d = st.d
    dp = fermion.NVAR * d
    n = lambda a: int(st.nf[a]) % 2
    tab = np.zeros((dp * dp, 2), dtype=np.int32)
    for e1 in range(dp):
        for e2 in range(dp):
            a1, v1, a2, v2 = e1 % d, e1 // d, e2 % d, e2 // d
            c1, c2 = e1, e2
            row_ok = order == fermion.ROW and v1 < 2 and v2 < 2
            col_ok = order == fermion.COL and v1 >= 2 and v2 >= 2
            if row_ok or col_ok:
                a, b = a2, a1
                before = ((v1 & 1) ^ n(a1)) if row_ok else (v1 & 1)
                if row_ok:
                    c1, c2 = a + d * (before ^ n(a)), b + d * (before ^ n(a) ^ n(b))
                else:
                    c1, c2 = a + d * (2 + before), b + d * (2 + (before ^ n(a)))
            tab[e1 * dp + e2] = (c1, c2)
    return tab


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_exchange_slice_tab_fermionic_table_and_psi_per_bond(dtype):
    """the fermionic exchange as a table with psi per bond on fermion.random_even_state, against Trace + ReplaceNNSiteTrace per bond
    with the candidates built independently (extended states of the exchanged configuration)"""
    from peps_amd import capi, fermion
    st = fermion.random_even_state(L, L, 3, seed=11)
    fc = np.stack([np.random.default_rng(100 + k).permutation(np.r_[np.zeros(18, dtype=int), np.ones(18, dtype=int)]).reshape(L, L)
                   for k in range(NW)])
    ctx = capi.Context(L, L, st.D, fermion.NVAR * st.d, CHI, dtype=capi.F64 if dtype == "f64" else capi.F32, max_walkers=NW)
    ctx.state_upload(st.extended_flat())
    tol = TOL[dtype]
    for (orient, approach, step, lo, hi), order in zip(_passes(), (fermion.ROW, fermion.COL)):
        ctx.set_configs(st.ext_config(fc, order))
        tab = _fermion_exchange_table(st, order)
        ctx.generate_bmps_approach(approach)
        for s in range(L):
            psi, ex = ctx.nn_exchange_slice_tab(orient, s, False, tab, psi_per_bond=True)
            assert psi.shape == (NW, L - 1)

            def cand(j):
                (r1, c1), (r2, c2) = _site(orient, s, j), _site(orient, s, j + 1)
                new = fc.copy()
                new[:, r1, c1], new[:, r2, c2] = fc[:, r2, c2], fc[:, r1, c1]
                ne = st.ext_config(new, order)
                return np.stack([ne[:, r1, c1], ne[:, r2, c2]], axis=-1)[:, None, :]
            _, psi_r, ex_r = _exchange_reference(ctx, orient, lo, hi, s, cand, True)
            assert _rel(psi, psi_r) < tol, (orient, s, _rel(psi, psi_r))
            differ = np.stack([fc[:, _site(orient, s, j)[0], _site(orient, s, j)[1]]
                               != fc[:, _site(orient, s, j + 1)[0], _site(orient, s, j + 1)[1]] for j in range(L - 1)], axis=1)
            assert differ.any()
            assert np.max(np.abs(ex - ex_r)[differ]) < tol * np.max(np.abs(ex_r)), (orient, s)
            assert np.array_equal(ex[~differ], psi[~differ])          # identity moves: psi of the bond
            if s + 1 < L:
                ctx.shift_bmps_window(step)
    ctx.close()


def test_energy_slice_error_paths():
    from peps_amd import capi
    ctx, _ = _state("f64")
    ctx.generate_bmps_approach(capi.UP)
    with pytest.raises(IndexError):                       # table entry outside [0, d): code 4
        ctx.onsite_slice(capi.HORIZONTAL, 0, np.array([[2], [0]], dtype=np.int32))
    bad = np.zeros((4, 2), dtype=np.int32)
    bad[3] = (0, 5)
    with pytest.raises(IndexError):
        ctx.nn_exchange_slice_tab(capi.HORIZONTAL, 0, False, bad)
    with pytest.raises(ValueError):                       # slice outside the lattice
        ctx.onsite_slice(capi.HORIZONTAL, L, np.array([[1], [0]], dtype=np.int32))
    with pytest.raises(ValueError):
        ctx.nn_exchange_slice_tab(capi.VERTICAL, -1)
    tab = np.array([1, 0], dtype=np.int32)
    psi, val = np.zeros(NW), np.zeros(NW * L)
    lib, h = ctx._l, ctx._h
    assert lib.pepsgpu_onsite_slice(h, capi.HORIZONTAL, 0, 0, 0, capi._ip(tab), capi._dp(psi), capi._dp(val)) == 1       # n_cand < 1
    assert lib.pepsgpu_onsite_slice(h, 2, 0, 0, 1, capi._ip(tab), capi._dp(psi), capi._dp(val)) == 1                     # orientation
    assert lib.pepsgpu_onsite_slice(h, capi.HORIZONTAL, 0, 0, 1, None, capi._dp(psi), capi._dp(val)) == 1                # null table
    assert lib.pepsgpu_nn_exchange_slice_tab(h, capi.HORIZONTAL, 0, 0, None, 0, capi._dp(psi), None) == 1                 # null buffer
    # the context still works after the refused calls
    p, _ = ctx.onsite_slice(capi.HORIZONTAL, 0, np.array([[1], [0]], dtype=np.int32))
    assert np.all(np.isfinite(p)) and np.max(np.abs(p)) > 0
    ctx.close()


_E2E = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from peps_amd import hostapi, synthetic, fermion

def cx(a):
    a = np.asarray(a)
    return [[float(x.real), float(x.imag)] for x in a.ravel()] if np.iscomplexobj(a) else [float(x) for x in a.ravel()]

L, D, chi, n = 6, 4, 12, 12
flat = synthetic.sitps_to_flat(synthetic.make_sitps(L, D, noise=0.5), D)
cflat = flat * np.exp(2j * np.pi * np.random.default_rng(3).uniform(size=flat.shape))
cfgs = synthetic.make_configs(L, n, "heisenberg", seed0=13)
seeds = np.arange(n, dtype=np.uint64) + 90
st = fermion.random_even_state(L, L, 3, seed=11)
fc = np.stack([np.random.default_rng(100 + k).permutation(np.r_[np.zeros(18, dtype=int), np.ones(18, dtype=int)]).reshape(L, L)
               for k in range(n)])
# a t-J state (0 up, 1 down: odd; 2 empty): the occupied component of the spinless generator twice, differently weighted
tj = fermion.random_even_state(L, L, 3, seed=12)
rng = np.random.default_rng(4)
tj = fermion.FermionState([[[t[0], t[0] * rng.uniform(0.5, 1.5, size=t[0].shape), t[1]] for t in row] for row in tj.tensors], tj.par, [1, 1, 0])
tc = np.stack([np.random.default_rng(200 + k).permutation(np.r_[np.zeros(12, dtype=int), np.ones(12, dtype=int), 2 * np.ones(12, dtype=int)]).reshape(L, L)
               for k in range(n)])
out = {}
for name, dt in (("f64", 1), ("f32", 0)):
    o = {}
    _, en, _, psi = hostapi.energy_and_holes(flat, cfgs, chi, "tfim", (0.7,), False, dt)
    o["tfim_energy"], o["tfim_psi"] = cx(en), cx(psi)
    packed, _, _ = hostapi.mc_energy_grad_partial(flat, cfgs, seeds, chi, "exchange", "tfim", (0.7,), 1, 2, dt)
    o["tfim_packed"] = cx(packed)
    obs, _ = hostapi.measure(flat, cfgs, chi, "tfim", (0.7,), dtype=dt)
    o["tfim_sigma_x"], o["tfim_measure_energy"] = cx(obs["sigma_x"]), cx(obs["energy"])
    _, en, psi = hostapi.fermion_energy(st, fc, chi, 1.0, 0.7, dt, "spinless")
    o["spinless_energy"], o["spinless_psi"] = cx(en), cx(psi)
    _, en, psi = hostapi.fermion_energy(tj, tc, chi, 1.0, 0.2, dt, "tj", 0.4, 0.1)
    o["tj_energy"], o["tj_psi"] = cx(en), cx(psi)
    out[name] = o
o = {}
for model, prm in (("xxz", (1.0, 0.8, 0.1)), ("tfim", (0.7,))):
    _, en, _, psi = hostapi.energy_and_holes_complex(cflat, cfgs, chi, model, prm, False)
    o[model + "_energy"], o[model + "_psi"] = cx(en), cx(psi)
out["c128"] = o
print(json.dumps(out))
"""


def test_host_layer_energy_slices_match_the_hook_path():
    """End to end, in child processes with and without PEPSHOST_NO_DEVICE_SWEEP=1: TFIM energy_and_holes and mc_energy_grad_partial
    (holes on the device), the TFIM measure registry (sigma_x, energy), energy_and_holes_complex for xxz and tfim, fermion_energy for
    spinless and t-J -- the device slices against the per-site / per-bond hooks"""
    res = {}
    for name, env in (("device", {}), ("hook", {"PEPSHOST_NO_DEVICE_SWEEP": "1"})):
        r = subprocess.run([sys.executable, "-c", _E2E, ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stderr[-2000:]
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    for dt in ("f64", "f32", "c128"):
        tol = TOL[dt]
        for key in res["hook"][dt]:
            a, b = np.array(res["device"][dt][key]), np.array(res["hook"][dt][key])
            if a.ndim == 2:
                a, b = a[:, 0] + 1j * a[:, 1], b[:, 0] + 1j * b[:, 1]
            assert a.shape == b.shape and a.size > 0, (dt, key)
            scale = max(np.max(np.abs(b)), 1e-300)
            if key.endswith("packed"):
                assert np.max(np.abs(a - b)) < tol * np.sum(np.abs(b)), (dt, key)
            else:
                assert np.max(np.abs(a - b)) < tol * scale, (dt, key, np.max(np.abs(a - b)) / scale)
