"""GPU tests of the device-side fermionic diagonal-hop slice and of the t-t'-J model built on it: nnn_hop_cand_kernel alone against numpy,
pepsgpu_nnn_hop_slice_fermion against the per-plaquette calls on the same context, its refusals, the t-J model end to end (slice, hook and
fresh paths of the host layer, f32 against f64, the restated reference hook on the oracle), an exact-summation anchor against a dense
Jordan-Wigner Hamiltonian, and the Python slice path of the spinless model."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tj_nnn_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the project's tolerances for "slice against per-bond calls" (tests/test_gpu_nnn_slice.py:20), relative to the largest reference magnitude
TOL = {"f64": 1e-12, "f32": 1e-5, "c128": 1e-12}
SHAPES = [((4, 4), 4, 16), ((3, 5), 3, 9)]                        # the shapes of the twisted-environment test (tests/test_gpu_fermion.py)
NW = 6


def _dtype(name):
    from peps_amd import capi
    return {"f64": capi.F64, "f32": capi.F32, "c128": capi.C128}[name]


def _state(kind, rows, cols, D, cplx=False):
    from peps_amd import fermion
    st = ref.tj_state(rows, cols, D) if kind == "tj" else fermion.random_even_state(rows, cols, D, seed=31)
    if cplx:      # a phase per element keeps the parity structure
        rng = np.random.default_rng(3)
        st = fermion.FermionState([[[a * np.exp(2j * np.pi * rng.uniform(size=a.shape)) for a in site] for site in row]
                                   for row in st.tensors], st.par, st.nf)
    return st


def _configs(st, n, seed=17):
    """random physical configurations with an even fermion number (the states are parity even)"""
    rng = np.random.default_rng(seed)
    cfgs = rng.integers(0, st.d, size=(n, st.rows, st.cols))
    empty, full = int(np.nonzero(st.nf == 0)[0][0]), int(np.nonzero(st.nf == 1)[0][0])
    for c in cfgs:
        if st.nf[c].sum() % 2 == 1:
            c[0, 0] = empty if st.nf[c[0, 0]] else full
    return cfgs


def _ctx(st, chi, dtype, n):
    from peps_amd import capi
    ctx = capi.Context(st.rows, st.cols, st.D, 4 * st.d, chi, dtype=_dtype(dtype), max_walkers=n)
    ctx.state_upload(st.extended_flat(st.D))
    return ctx


def _hopped(cfg, a, b):
    new = cfg.copy()
    new[..., a[0], a[1]], new[..., b[0], b[1]] = cfg[..., b[0], b[1]], cfg[..., a[0], a[1]]
    return new


def _plaquette(x, row, col):
    return np.stack([x[:, row, col], x[:, row + 1, col], x[:, row + 1, col + 1], x[:, row, col + 1]], axis=-1)


def _expected_candidates(st, cfgs, row, col):
    """numpy statement of nnn_hop_cand_kernel: (cand [n][2][4], sign [n][2], allowed [n][2]) of the plaquette (row, col)"""
    from peps_amd import fermion
    n, rows, cols = cfgs.shape
    occ = (st.nf[cfgs] % 2).reshape(n, -1)
    cand, sign, allowed = [], [], []
    for a, b in (((row, col), (row + 1, col + 1)), ((row + 1, col), (row, col + 1))):
        ia, ib = sorted((a[0] * cols + a[1], b[0] * cols + b[1]))
        ok = occ[:, a[0] * cols + a[1]] != occ[:, b[0] * cols + b[1]]
        cand.append(_plaquette(st.ext_config(_hopped(cfgs, a, b), fermion.ROW), row, col))
        sign.append(np.where(ok, 1 - 2 * (occ[:, ia + 1:ib].sum(axis=1) % 2), 0))
        allowed.append(ok)
    return np.stack(cand, axis=1), np.stack(sign, axis=1), np.stack(allowed, axis=1)


# ---- (a) the candidate kernel alone ----
@pytest.mark.parametrize("kind,nf", [("spinless", [1, 0]), ("tj", [1, 1, 0])])
@pytest.mark.parametrize("shape", [(3, 4), (4, 3)])
def test_hop_candidate_kernel_matches_numpy(shape, kind, nf):
    """Integer-exact over every plaquette: the hopped extended states are FermionState.ext_config of the hopped configuration, the sign is
    the row-major Jordan-Wigner string, the flag is -1 exactly where the occupation differs at the two ends.  64 random configurations
    plus rows that are all empty and all occupied."""
    from peps_amd import capi, fermion
    rows, cols = shape
    st = _state(kind, rows, cols, 2)
    assert st.nf.tolist() == nf
    rng = np.random.default_rng(5)
    cfgs = rng.integers(0, st.d, size=(66, rows, cols))
    cfgs[64, 0, :], cfgs[64, rows - 1, :] = st.d - 1, 0            # an all-empty and an all-occupied row
    cfgs[65, 1, :], cfgs[65, 0, :] = st.d - 1, 0
    ext = st.ext_config(cfgs, fermion.ROW)
    n_allowed = 0
    for row in range(rows - 1):
        for col in range(cols - 1):
            cand, sign, flag = capi.diag_fermion_hop_cand(ext, nf, row, col)
            w_cand, w_sign, w_ok = _expected_candidates(st, cfgs, row, col)
            assert np.array_equal(flag, np.where(w_ok, -1, 1)), (row, col)
            assert np.array_equal(sign, w_sign), (row, col)
            assert np.array_equal(cand[w_ok], w_cand[w_ok]), (row, col)
            n_allowed += int(w_ok.sum())
    assert n_allowed > 100
    with pytest.raises(ValueError):
        capi.diag_fermion_hop_cand(ext, nf, rows - 1, 0)


# ---- (b) the slice against the per-plaquette calls ----
def _per_plaquette_reference(ctx, st, cfgs, row):
    """the row-pair body of peps_amd.fermion.nnn_hop_energy_local, returning the raw numbers: psi [n][cols - 1] and jw psi'
    [n][cols - 1][2] (0 where the hop is forbidden; both 0 at a plaquette where no walker has an allowed hop)"""
    from peps_amd import capi, fermion
    n, rows, cols = cfgs.shape
    d = st.d
    ext = st.ext_config(cfgs, fermion.ROW)
    flip = np.where(ext // d == 0, ext + d, ext - d).astype(np.int32)
    psi = np.zeros((n, cols - 1), dtype=ctx._ot)
    val = np.zeros((n, cols - 1, 2), dtype=ctx._ot)
    try:
        ctx.bten2_select_set(0)
        ctx.grow_full_bten2(capi.RIGHT, row, 2, True)
        ctx.init_bten2(capi.LEFT, row)
        ctx.bten2_select_set(1)
        ctx.cfg_override_slice(capi.HORIZONTAL, row, flip[:, row, :])
        ctx.grow_full_bten2(capi.RIGHT, row, 2, True)
        ctx.cfg_override_slice(capi.HORIZONTAL, row + 1, flip[:, row + 1, :])
        ctx.init_bten2(capi.LEFT, row)
        for col in range(cols - 1):
            cand, sign, ok = _expected_candidates(st, cfgs, row, col)
            if ok.any():
                psi[:, col] = ctx.replace_plaquette_trace(row, col, _plaquette(ext, row, col)[:, None, :], 0, 0)[:, 0]
                val[:, col, :] = np.where(ok, sign * ctx.replace_plaquette_trace(row, col, cand, 1, 1), 0.0)
            if col < cols - 2:
                ctx.grow_bten2_step(capi.LEFT, row)
                ctx.bten2_select_set(0)
                ctx.cfg_override_slice(capi.HORIZONTAL, row + 1, None)
                ctx.grow_bten2_step(capi.LEFT, row)
                ctx.bten2_select_set(1)
                ctx.cfg_override_slice(capi.HORIZONTAL, row + 1, flip[:, row + 1, :])
    finally:
        ctx.cfg_override_slice(capi.HORIZONTAL, 0, None)
        ctx.bten2_select_set(0)
    return psi, val


@pytest.mark.parametrize("dtype", ["f64", "f32", "c128"])
@pytest.mark.parametrize("kind", ["spinless", "tj"])
@pytest.mark.parametrize("shape,D,chi", SHAPES)
def test_hop_slice_matches_the_per_plaquette_calls(shape, D, chi, kind, dtype):
    """Every row pair of a row pass, diag_mask 3, 1 and 2: psi and jw psi' of the slice against the per-plaquette calls on the same
    context; masked-off and forbidden entries are exactly zero; the context is left as it was found (set 0, no override: the plain
    plaquette trace still gives psi, Trace is unchanged)."""
    from peps_amd import capi, fermion
    rows, cols = shape
    st = _state(kind, rows, cols, D, dtype == "c128")
    cfgs = _configs(st, NW)
    ctx = _ctx(st, chi, dtype, NW)
    ctx.set_configs(st.ext_config(cfgs, fermion.ROW))
    ctx.generate_bmps_approach(capi.UP)
    tol, nonzero = TOL[dtype], 0
    for row in range(rows - 1):
        ctx.init_bten(capi.LEFT, row)
        ctx.grow_full_bten(capi.RIGHT, row, 1, True)
        trace0 = ctx.trace(row, 0, capi.HORIZONTAL)
        w_psi, w_val = _per_plaquette_reference(ctx, st, cfgs, row)
        scale = max(np.max(np.abs(w_val)), np.max(np.abs(w_psi)))
        assert scale > 0
        for mask in (3, 1, 2):
            psi, val = ctx.nnn_hop_slice_fermion(row, st.nf % 2, mask)
            assert psi.shape == w_psi.shape and val.shape == w_val.shape and val.dtype == w_val.dtype
            for k in (0, 1):
                if not (mask >> k) & 1:
                    assert np.all(val[..., k] == 0.0), (row, mask, k)
                    continue
                assert np.all(val[..., k][w_val[..., k] == 0.0] == 0.0), (row, mask, k)       # forbidden hops: exactly zero
                err = np.max(np.abs(val[..., k] - w_val[..., k])) / scale
                print("hop slice", shape, kind, dtype, "row", row, "mask", mask, "kind", k, "rel err", err)
                assert err < tol, (row, mask, k, err)
            # psi where the plaquette has an allowed hop on a requested diagonal, 0 elsewhere
            live = np.zeros(cols - 1, dtype=bool)
            for k in (0, 1):
                if (mask >> k) & 1:
                    live |= (w_val[..., k] != 0.0).any(axis=0)
            assert np.all(psi[:, ~live] == 0.0)
            err = np.max(np.abs(psi[:, live] - w_psi[:, live])) / scale if live.any() else 0.0
            print("hop slice", shape, kind, dtype, "row", row, "mask", mask, "psi rel err", err)
            assert err < tol, (row, mask, err)
            if mask == 3:
                nonzero += int(np.count_nonzero(val))
            # the state is restored: set 0 and the walkers' own table answer the plain calls
            if live.any():
                col = int(np.nonzero(live)[0][-1])
                again = ctx.replace_plaquette_trace(row, col, None, 0, 0)
                assert np.max(np.abs(again - w_psi[:, col])) / scale < tol, (row, mask)
            assert np.max(np.abs(ctx.trace(row, 0, capi.HORIZONTAL) - trace0)) <= tol * np.max(np.abs(trace0))
        if row + 2 < rows:
            ctx.shift_bmps_window(capi.DOWN)
    assert nonzero > 10, nonzero
    assert np.all(ctx.walker_flags() == 0)
    ctx.close()


# ---- (c) refusals ----
def test_hop_slice_refusals_leave_the_context_usable():
    from peps_amd import capi, fermion
    (rows, cols), D, chi = SHAPES[1]
    st = _state("tj", rows, cols, D)
    cfgs = _configs(st, NW)
    ctx = _ctx(st, chi, "f64", NW)
    ext = st.ext_config(cfgs, fermion.ROW)
    ctx.set_configs(ext)
    lib, h = ctx._l, ctx._h
    occ = np.ascontiguousarray(st.nf % 2, dtype=np.int32)
    psi, val = np.zeros((NW, cols - 1)), np.zeros((NW, cols - 1, 2))

    def call(row=0, d=st.d, o=occ, mask=3, p=psi, v=val):
        return lib.pepsgpu_nnn_hop_slice_fermion(h, row, d, None if o is None else capi._ip(o), mask, None if p is None else capi._dp(p),
                                                 None if v is None else capi._dp(v))

    def valid():
        got_psi, got_val = ctx.nnn_hop_slice_fermion(0, occ, 3)
        assert np.max(np.abs(got_val - want[1])) < 1e-12 * scale and np.max(np.abs(got_psi - want[0])) < 1e-12 * scale

    # a boundary MPS of the row pair is missing (the DOWN stack holds its vacuum only): PEPSGPU_ESTATE
    assert call() == 3
    ctx.generate_bmps_approach(capi.UP)
    want = _per_plaquette_reference(ctx, st, cfgs, 0)
    scale = np.max(np.abs(want[1]))
    assert np.count_nonzero(want[1]) > 10
    valid()
    refusals = [("row -1", dict(row=-1), 1), ("row rows - 1", dict(row=rows - 1), 1), ("mask 0", dict(mask=0), 1), ("mask 4", dict(mask=4), 1),
                ("null occ", dict(o=None), 1), ("null psi", dict(p=None), 1), ("null val", dict(v=None), 1),
                ("4 d != phys_dim", dict(d=st.d - 1), 1), ("4 d != phys_dim", dict(d=st.d + 1, o=np.r_[occ, 0].astype(np.int32)), 1),
                ("occ entry 2", dict(o=np.array([1, 2, 0], dtype=np.int32)), 1), ("occ entry -1", dict(o=np.array([1, -1, 0], dtype=np.int32)), 1)]
    for name, kw, status in refusals:
        assert call(**kw) == status, name
        valid()
    with pytest.raises(ValueError):
        ctx.nnn_hop_slice_fermion(0, occ, 0)
    # an override that is active on entry: PEPSGPU_ESTATE; usable once it is cleared
    ctx.cfg_override_slice(capi.HORIZONTAL, 1, ext[:, 1, :])
    assert call() == 3
    ctx.cfg_override_slice(capi.HORIZONTAL, 1)
    valid()
    # a column-major table (variants 2 / 3) in the row pair: PEPSGPU_ESTATE
    ctx.set_configs(st.ext_config(cfgs, fermion.COL))
    ctx.generate_bmps_approach(capi.UP)
    assert call() == 3
    with pytest.raises(RuntimeError):
        ctx.nnn_hop_slice_fermion(0, occ, 3)
    ctx.set_configs(ext)
    ctx.generate_bmps_approach(capi.UP)
    valid()
    assert np.all(ctx.walker_flags() == 0)
    ctx.close()


# ---- (d) the t-J model end to end ----
_E2E = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from peps_amd import capi, hostapi
import tj_nnn_ref as ref
import test_gpu_tj_nnn as t

out = {}
for (rows, cols), D, chi in t.SHAPES:
    st = ref.tj_state(rows, cols, D)
    cfgs = t._configs(st, t.NW)
    for name, dt in (("f64", 1), ("f32", 0)):
        before = capi.diag_nnn_hop_slice_calls()
        _, en, _ = hostapi.fermion_energy(st, cfgs, chi, 1.0, 0.1, dt, "tj", 0.4, 0.3, 0.7)
        _, en0, _ = hostapi.fermion_energy(st, cfgs, chi, 1.0, 0.1, dt, "tj", 0.4, 0.3, 0.0)
        out["%dx%d_%s" % (rows, cols, name)] = {"energy": [float(x) for x in en], "energy_t2_0": [float(x) for x in en0],
                                                "calls": capi.diag_nnn_hop_slice_calls() - before}
print(json.dumps(out))
"""


def test_tj_t2_energy_slice_hook_fresh_f32_and_oracle():
    """E_loc of SquaretJVModel(1, 0.7, 0.4, 0.1, 0.3) through the host layer in child processes: the device slice (default), the
    per-plaquette hook path (PEPSHOST_NO_DEVICE_SWEEP=1) and fresh amplitudes (PEPSHOST_NNN_FRESH=1) agree to 1e-9 max(1, |E|) in f64;
    f32 is within 2e-5 of f64; f64 equals the restated reference hook on the oracle's amplitudes to 1e-8 max(1, |E|); the slice counter
    grows by rows - 1 per energy call on the slice path only."""
    from oracle.bmps import BMPSTruncateParams
    res = {}
    for name, env in (("slice", {}), ("hook", {"PEPSHOST_NO_DEVICE_SWEEP": "1"}), ("fresh", {"PEPSHOST_NNN_FRESH": "1"})):
        r = subprocess.run([sys.executable, "-c", _E2E, ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    for (rows, cols), D, chi in SHAPES:
        key = "%dx%d_" % (rows, cols)
        e64 = np.array(res["slice"][key + "f64"]["energy"])
        e0 = np.array(res["slice"][key + "f64"]["energy_t2_0"])
        assert np.max(np.abs(e64 - e0)) > 1e-3                      # t2 matters on these walkers
        for path in ("hook", "fresh"):
            other = np.array(res[path][key + "f64"]["energy"])
            err = np.max(np.abs(e64 - other) / np.maximum(1.0, np.abs(other)))
            print("t-t'-J", (rows, cols), "slice against", path, "f64:", err)
            assert err < 1e-9, (path, err)
        for path in ("slice", "hook", "fresh"):
            e32 = np.array(res[path][key + "f32"]["energy"])
            err = np.max(np.abs(e32 - e64) / np.maximum(1.0, np.abs(e64)))
            print("t-t'-J", (rows, cols), path, "f32 against f64:", err)
            assert err < 2e-5, (path, err)
            for dt in ("f64", "f32"):                               # one t2 != 0 energy call per entry (the t2 = 0 call runs no diagonal pass)
                assert res[path][key + dt]["calls"] == (rows - 1 if path == "slice" else 0), (path, dt, res[path][key + dt]["calls"])
        st = ref.tj_state(rows, cols, D)
        fs = ref.oracle_view(st)
        cfgs = _configs(st, NW)
        tp = BMPSTruncateParams.SVD(chi, chi, 0.0)
        for w, cfg in enumerate(cfgs):
            want, count = ref.tj_local_energy(fs, cfg, tp, 1.0, 0.7, 0.4, 0.1, 0.3)
            print("t-t'-J oracle", (rows, cols), w, "allowed diagonals", count, abs(e64[w] - want))
            assert abs(e64[w] - want) < 1e-8 * max(1.0, abs(want)), (w, e64[w], want)


# ---- (e) the independent anchor on the device ----
def test_tj_t2_exact_sum_on_the_device_equals_the_dense_hamiltonian():
    """All 729 configurations of the 2 x 3 t-J state as one batch, f64, chi = 64 (exact): the |psi|^2-weighted mean of the device's
    E_loc at t2 = 0.7 is the Rayleigh quotient of the dense Jordan-Wigner t-t'-J Hamiltonian to 1e-9 relative (the f64 amplitude tolerance)."""
    from peps_amd import capi, fermion
    rows, cols = 2, 3
    st = ref.tj_state(rows, cols, 2)
    cfgs = ref.all_tj_configs(rows, cols)
    cfgs = cfgs[np.sum(cfgs != ref.EMPTY, axis=(1, 2)) % 2 == 0]    # the parity-even configurations: the others have amplitude zero
    assert len(cfgs) == 365
    ctx = _ctx(st, 64, "f64", len(cfgs))
    before = capi.diag_nnn_hop_slice_calls()
    bonds = {}
    e, psis = fermion.tj_energy(ctx, st, cfgs, 1.0, 0.4, 0.1, 0.3, 0.7, bonds)
    assert capi.diag_nnn_hop_slice_calls() == before + rows - 1
    assert np.count_nonzero(bonds["dr"]) + np.count_nonzero(bonds["ur"]) >= 600
    psi = fermion.evaluate_amplitude(ctx, st, cfgs)
    full = np.zeros(3 ** (rows * cols))
    full[cfgs.reshape(len(cfgs), -1) @ (3 ** np.arange(rows * cols - 1, -1, -1))] = psi
    quot = ref.rayleigh(ref.dense_ttj_hamiltonian(rows, cols, 1.0, 0.7, 0.4, 0.1, 0.3), full)
    w = np.abs(psi) ** 2
    mean = np.sum(w * e) / np.sum(w)
    print("t-t'-J 2x3 on the device: E = %.12f, dense H %.12f, rel diff %.2e" % (mean, quot, abs(mean - quot) / abs(quot)))
    assert abs(mean - quot) < 1e-9 * abs(quot)
    assert np.all(ctx.walker_flags() == 0)
    ctx.close()


# ---- (f) the spinless model ----
@pytest.mark.parametrize("dtype", ["f64", "f32", "c128"])
@pytest.mark.parametrize("shape,D,chi", SHAPES)
def test_spinless_slice_path_equals_the_local_path_per_bond(shape, D, chi, dtype):
    from peps_amd import fermion
    rows, cols = shape
    st = _state("spinless", rows, cols, D, dtype == "c128")
    cfgs = _configs(st, NW)
    ctx = _ctx(st, chi, dtype, NW)
    b_slice, b_local = {}, {}
    e_slice, _ = fermion.spinless_fermion_energy(ctx, st, cfgs, 1.0, 0.5, 0.7, b_slice, nnn="slice")
    e_local, _ = fermion.spinless_fermion_energy(ctx, st, cfgs, 1.0, 0.5, 0.7, b_local, nnn="local")
    assert np.count_nonzero(b_local["dr"]) + np.count_nonzero(b_local["ur"]) > 10
    for key in ("dr", "ur"):
        err = np.max(np.abs(b_slice[key] - b_local[key])) / np.max(np.abs(b_local[key]))
        print("spinless", shape, dtype, key, err)
        assert err < TOL[dtype], (key, err)
    assert np.all(ctx.walker_flags() == 0)
    ctx.close()
