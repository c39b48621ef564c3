"""GPU tests of the Hubbard model: the U(1) x U(1) sector updater (MCUpdateSquareNNHubbardU1U1OBC, square_hubbard_u1u1_updater.h:90-158;
pepsgpu_sweep_slice_sector) and SquareHubbardModel (square_hubbard_model.h:76-263; pepsgpu_nn_hop_slice_fermion).

Shapes 3 x 4 and 4 x 3, D = 3, chi = 9, 8 walkers: slices of length >= 3 (the window shifts), non-square (a row / column mix-up shows),
edge legs of dimension 1.  The first two configurations are laid out by hand so that sectors of size 4, 2 and 1 and every hop class
(one electron, three electrons, up-down, down-up, doublon next to an empty site) occur on a horizontal and on a vertical bond.
The device slices against the per-bond hook path (PEPSHOST_NO_DEVICE_SWEEP=1) run in two child processes, once for the module.
The convention itself is pinned on the CPU (tests/test_cpu_hubbard.py); the restatements are in tests/hubbard_ref.py."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hubbard_ref as ref  # noqa: E402
from oracle.bmps import BMPSTruncateParams  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"f64": 1e-12, "f32": 1e-5, "c128": 1e-12}            # TOL of tests/test_gpu_tnn3.py
E_TOL = {"f64": 1e-9, "f32": 5e-5}                           # test_gpu_fermion.py::test_cpp_host_layer_fermion_energy: tol * 10 * max(1, |E|)
T, U, MU = 1.0, 3.0, 0.4
D, CHI, NW = 3, 9, 8
SHAPES = [(3, 4), (4, 3)]
HAND_3x4 = np.array([[[1, 2, 0, 3], [2, 1, 1, 3], [0, 3, 3, 1]],
                     [[0, 3, 2, 1], [3, 0, 1, 2], [1, 1, 0, 0]]])


def configs(shape, n=NW, seed=11):
    """n parity-even configurations; the first two by hand (3 x 4 as above, 4 x 3 their transposes)"""
    rows, cols = shape
    rng = np.random.default_rng(seed + rows)
    out = rng.integers(0, 4, size=(n, rows, cols))
    hand = HAND_3x4 if shape == (3, 4) else HAND_3x4.transpose(0, 2, 1)
    if hand.shape[1:] == (rows, cols):
        out[:2] = hand
    odd = ~ref.is_even(out)
    out[odd, -1, -1] = np.array([1, 0, 3, 2])[out[odd, -1, -1]]          # flip the parity of the last site
    return out.astype(np.int32)


def bond_classes(cfgs):
    """{orientation: (set of sector sizes, set of hop classes)} over all bonds of the configurations"""
    def cls(a, b):
        if {a, b} == {0, 3}:
            return "doublon-empty"
        if (a, b) == (1, 2):
            return "up-down"
        if (a, b) == (2, 1):
            return "down-up"
        if 3 in (a, b) and a != b:
            return "one electron"
        if 0 in (a, b) and a != b:
            return "three electrons"
        return None
    out = {"h": (set(), set()), "v": (set(), set())}
    for c in cfgs:
        for s1, s2 in ref.nn_bonds(*c.shape):
            key = "h" if s1[0] == s2[0] else "v"
            out[key][0].add(len(ref.sector(int(c[s1]), int(c[s2]))))
            out[key][1].add(cls(int(c[s1]), int(c[s2])))
    return out


def _ctx(state, dtype, n, chi=CHI):
    from peps_amd import capi
    ctx = capi.Context(state.rows, state.cols, state.D, 4 * state.d, chi, dtype=dtype, max_walkers=n)
    ctx.state_upload(state.extended_flat(state.D))
    return ctx


def _dtype(name):
    from peps_amd import capi
    return {"f64": capi.F64, "f32": capi.F32, "c128": capi.C128}[name]


def _state(shape, name="f64"):
    return ref.hubbard_state(shape[0], shape[1], D, phase_seed=7 if name == "c128" else None)


@pytest.mark.parametrize("shape", SHAPES)
def test_preconditions_of_the_shapes(shape):
    """sector sizes {1, 2, 4} and all five hop classes on a horizontal and on a vertical bond of the first two configurations; every
    configuration parity even; no walker with |psi| < 1e-6 x median"""
    from peps_amd import fermion
    cfgs = configs(shape)
    assert np.all(ref.is_even(cfgs))
    got = bond_classes(cfgs[:2])
    for key in ("h", "v"):
        assert got[key][0] == {1, 2, 4}, (key, got[key][0])
        assert got[key][1] >= {"one electron", "three electrons", "up-down", "down-up", "doublon-empty"}, (key, got[key][1])
    st = _state(shape)
    assert all(st.tensors[r][c][0].shape[k] == 1 for r in range(st.rows) for c in range(st.cols)
               for k, edge in enumerate((c == 0, r == st.rows - 1, c == st.cols - 1, r == 0)) if edge)
    ctx = _ctx(st, _dtype("f64"), NW)
    amp = np.abs(fermion.evaluate_amplitude(ctx, st, cfgs))
    ctx.close()
    assert np.all(amp > 1e-6 * np.median(amp)), amp


# ---- the candidate kernel ----
@pytest.mark.parametrize("shape", SHAPES)
def test_sector_candidate_kernel_equals_the_numpy_rule(shape):
    """pepsgpu_diag_sector_cand on every bond, both mode orders: slot k < m holds the extended states of the pair with candidate k in
    place (FermionState.ext_config of the changed configuration), slot k >= m the walker's own; meta = (m, init).  Exact.  The bosonic
    mode returns the table's states."""
    from peps_amd import capi, fermion
    st = _state(shape)
    cfgs = configs(shape)
    rows, cols = shape
    tab = fermion.hubbard_sector_table()
    for s1, s2 in ref.nn_bonds(rows, cols):
        hor = s1[0] == s2[0]
        order, orient = (fermion.ROW, capi.HORIZONTAL) if hor else (fermion.COL, capi.VERTICAL)
        ext = st.ext_config(cfgs, order)
        cand, meta = capi.diag_sector_cand(ext, tab, orient, s1[0] * cols + s1[1], s2[0] * cols + s2[1], nf=fermion.HUBBARD_NF)
        bos, bmeta = capi.diag_sector_cand(cfgs, tab, orient, s1[0] * cols + s1[1], s2[0] * cols + s2[1])
        for w, c in enumerate(cfgs):
            valid = ref.sector(int(c[s1]), int(c[s2]))
            assert tuple(meta[w]) == (len(valid), valid.index((int(c[s1]), int(c[s2])))) == tuple(bmeta[w])
            for k in range(4):
                new = c.copy()
                if k < len(valid):
                    new[s1], new[s2] = valid[k]
                ne = st.ext_config(new, order)
                assert tuple(cand[w, k]) == (int(ne[s1]), int(ne[s2])), (s1, s2, w, k)
                assert tuple(bos[w, k]) == (int(new[s1]), int(new[s2])), (s1, s2, w, k)


# ---- the device slices against the hook path, in child processes ----
_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from peps_amd import hostapi
import hubbard_ref as ref
import test_gpu_hubbard as tg

def cx(a):
    a = np.asarray(a)
    return [[float(x.real), float(x.imag)] for x in a.ravel()] if np.iscomplexobj(a) else [float(x) for x in a.ravel()]

out = {}
seeds = np.arange(tg.NW, dtype=np.uint64) + 83
prm = (tg.T, tg.U, tg.MU)
for shape in tg.SHAPES:
    tag = "%dx%d" % shape
    cfgs = tg.configs(shape)
    for name, dt in (("f64", 1), ("f32", 0), ("c128", 1)):
        st = tg._state(shape, name)
        c, a, r = hostapi.fermion_mc_sweeps(st, cfgs, seeds, tg.CHI, 2, dt, updater="hubbard_u1u1")
        out["sweep_%s_%s" % (name, tag)] = {"cfg": c.tolist(), "amp": cx(a), "rate": cx(r), "start": cfgs.tolist()}
    st = tg._state(shape)
    for name, dt in (("f64", 1), ("f32", 0)):
        amps, en, psi = hostapi.fermion_energy(st, cfgs, tg.CHI, tg.T, dtype=dt, model="hubbard", U=tg.U, mu=tg.MU)
        out["energy_%s_%s" % (name, tag)] = {"amp": cx(amps), "energy": cx(en), "psi": cx(psi)}
    obs, (pm, pe) = hostapi.fermion_observables(st, cfgs, tg.CHI, "hubbard", prm)
    out["obs_" + tag] = {k: cx(v) for k, v in obs.items()}
    stats, _, en, cf, rates = hostapi.fermion_measure(st, cfgs, seeds, tg.CHI, 1, 2, 1, "hubbard", prm, updater="hubbard_u1u1")
    out["measure_" + tag] = {"stats": {k: [cx(v[0]), cx(v[1])] for k, v in stats.items()}, "energy": cx(en), "cfg": cf.tolist(), "rate": cx(rates)}
# the 3 x 3 chain of the oracle test
st = ref.hubbard_state(3, 3, tg.D)
c3 = tg.configs((3, 3), 4)
c, a, r = hostapi.fermion_mc_sweeps(st, c3, seeds[:4], tg.CHI, 2, 1, updater="hubbard_u1u1")
out["chain_3x3"] = {"cfg": c.tolist(), "amp": cx(a), "rate": cx(r), "start": c3.tolist()}
from peps_amd import capi
out["calls"] = {"sector": capi.diag_sector_slice_calls(), "hop": capi.diag_hop_slice_calls()}
print(json.dumps(out))
"""


def _as_array(v):
    a = np.asarray(v)
    return a[..., 0] + 1j * a[..., 1] if a.ndim == 2 else a


@pytest.fixture(scope="module")
def both_paths():
    res = {}
    for name, env in (("device", {}), ("hook", {"PEPSHOST_NO_DEVICE_SWEEP": "1"})):
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    return res


def test_the_two_children_took_the_two_paths(both_paths):
    assert both_paths["device"]["calls"]["sector"] > 0 and both_paths["device"]["calls"]["hop"] > 0
    assert both_paths["hook"]["calls"] == {"sector": 0, "hop": 0}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", ["f64", "f32", "c128"])
def test_sector_slice_sweep_equals_the_hook_path(both_paths, name, shape):
    """two sweeps: identical configurations and accept rates, amplitudes within 1e-12 (f64, complex) / 1e-5 (f32); some walker moved;
    N_up and N_down of every walker conserved"""
    key = "sweep_%s_%dx%d" % ((name,) + shape)
    dev, hook = both_paths["device"][key], both_paths["hook"][key]
    assert dev["cfg"] == hook["cfg"], key
    assert np.array_equal(np.array(dev["rate"]), np.array(hook["rate"])), key
    a, b = _as_array(dev["amp"]), _as_array(hook["amp"])
    rel = np.max(np.abs(a - b)) / np.max(np.abs(b))
    print(key, "max |amp_device - amp_hook| / max |amp| = %.2e" % rel, "rates", dev["rate"])
    assert rel < TOL[name], (key, rel)
    assert dev["cfg"] != dev["start"], "no walker moved: %s" % key
    assert max(dev["rate"]) > 0
    c, s = np.array(dev["cfg"]), np.array(dev["start"])
    assert np.array_equal(ref.N_UP[c].sum(axis=(1, 2)), ref.N_UP[s].sum(axis=(1, 2)))
    assert np.array_equal(ref.N_DN[c].sum(axis=(1, 2)), ref.N_DN[s].sum(axis=(1, 2)))


def test_f64_chain_equals_the_updater_restated_on_the_oracle(both_paths):
    """3 x 3, 4 walkers, 2 sweeps on the same std::mt19937 streams: the configurations and the accept counts are those of
    hubbard_ref.MCUpdateSquareNNHubbardU1U1OBC on the oracle's contractor"""
    dev = both_paths["device"]["chain_3x3"]
    st = ref.hubbard_state(3, 3, D)
    fs = ref.oracle_view(st)
    tp = BMPSTruncateParams.SVD(CHI, CHI, 0.0)
    start = np.array(dev["start"])
    moved = 0
    for w in range(4):
        cfg = start[w].astype(np.int64).copy()
        upd = ref.MCUpdateSquareNNHubbardU1U1OBC(seed=83 + w)
        amp, count = fs.amplitude(cfg, tp), 0
        for _ in range(2):
            a1, a2, amp = upd.sweep(fs, cfg, amp, tp)
            count += a1 + a2
        assert np.array_equal(cfg, np.array(dev["cfg"][w])), w
        assert int(round(dev["rate"][w] * 12 * 2)) == count and abs(dev["rate"][w] * 24 - count) < 1e-9, (w, dev["rate"][w], count)
        moved += int(np.any(cfg != start[w]))
    assert moved > 0


# ---- the sector slice on a bosonic context against pepsgpu_sweep_slice_fullspace ----
def test_sector_slice_with_a_full_table_equals_the_fullspace_slice():
    """d = 2 bosonic context, a table that lists all four states for every pair: the same configurations and accept counts as
    pepsgpu_sweep_slice_fullspace on the same words, amplitudes within 1e-12 (f64), two words per bond"""
    from peps_amd import capi, synthetic
    rows, cols = 3, 4
    flat = np.ascontiguousarray(synthetic.sitps_to_flat(synthetic.make_sitps(4, D, noise=0.5), D)[:rows, :cols])
    cfgs = np.random.default_rng(4).integers(0, 2, size=(NW, rows, cols)).astype(np.int32)
    tab = np.array([[4, a * 2 + b, 0, 0, 0, 1, 1, 0, 1, 1] for a in range(2) for b in range(2)], dtype=np.int32)
    words = np.random.default_rng(5).integers(0, 2 ** 32, size=(rows + cols, NW, 2 * 3), dtype=np.uint64).astype(np.uint32)
    res = []
    for kind in ("sector", "fullspace"):
        ctx = capi.Context(rows, cols, D, 2, CHI, dtype=capi.F64, max_walkers=NW)
        ctx.state_upload(flat)
        ctx.set_configs(cfgs)
        amp = ctx.evaluate_amplitude()
        acc_total, k = np.zeros(NW, dtype=np.int64), 0
        for orient, approach, step, S, N in ((capi.HORIZONTAL, capi.UP, capi.DOWN, rows, cols), (capi.VERTICAL, capi.LEFT, capi.RIGHT, cols, rows)):
            ctx.generate_bmps_approach(approach)
            for s in range(S):
                wd = words[k][:, :2 * (N - 1)]
                k += 1
                if kind == "sector":
                    amp, cons, acc, _ = ctx.sweep_slice_sector(orient, s, tab, wd, amp)
                    assert np.all(cons == 2 * (N - 1))
                else:
                    amp, acc, _ = ctx.sweep_slice_fullspace(orient, s, 2, wd, amp)
                acc_total += acc
                if s + 1 < S:
                    ctx.shift_bmps_window(step)
        res.append((ctx.get_configs().copy(), acc_total, amp))
        ctx.close()
    assert np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1], res[1][1]) and res[0][1].sum() > 0
    assert np.max(np.abs(res[0][2] - res[1][2])) < 1e-12 * np.max(np.abs(res[1][2]))
    assert not np.array_equal(res[0][0], cfgs)


# ---- the hop slice ----
def _passes():
    from peps_amd import capi, fermion
    return ((capi.HORIZONTAL, fermion.ROW, capi.UP, capi.DOWN), (capi.VERTICAL, fermion.COL, capi.LEFT, capi.RIGHT))


@pytest.mark.parametrize("name", ["f64", "f32", "c128"])
def test_hop_slice_without_holes_returns_the_bytes_of_the_pair_slice(name):
    from peps_amd import capi, fermion
    shape = (3, 4)
    st, cfgs = _state(shape, name), configs(shape)
    table, _ = fermion.hubbard_hop_table()
    ctx = _ctx(st, _dtype(name), NW)
    before = capi.diag_hop_slice_calls(), capi.diag_pair_slice_calls()
    slices = 0
    for orient, order, approach, step in _passes():
        ctx.set_configs(st.ext_config(cfgs, order))
        ctx.generate_bmps_approach(approach)
        S = shape[0] if orient == capi.HORIZONTAL else shape[1]
        for s in range(S):
            psi_p, _, pair = ctx.nn_pair_slice_fermion(orient, s, fermion.HUBBARD_NF, table, None)
            psi_h, hop = ctx.nn_hop_slice_fermion(orient, s, fermion.HUBBARD_NF, table)
            assert psi_p.tobytes() == psi_h.tobytes() and pair.tobytes() == hop.tobytes(), (name, orient, s)
            assert np.count_nonzero(hop) > 0 and np.all(psi_h != 0)
            slices += 1
            if s + 1 < S:
                ctx.shift_bmps_window(step)
    ctx.close()
    assert capi.diag_hop_slice_calls() - before[0] == slices and capi.diag_pair_slice_calls() - before[1] == slices


@pytest.mark.parametrize("name", ["f64", "f32", "c128"])
def test_hop_slice_with_holes_equals_the_per_site_and_per_bond_calls(name):
    """punch_holes = 1 on every row: psi and the hops equal Trace + ReplaceNNSiteTrace per bond on a second context that walks the row
    pass call by call (GrowFullBTen(.., 1), PunchHole per site, ShiftBTenWindow after every bond); the holes stored in HBM equal that
    context's per-site pepsgpu_punch_hole -- compared through the gradient accumulators that read them (real element types) and, for
    every element type, through the hole of the row's last site, which the environments the slice leaves still serve; TOL"""
    from peps_amd import capi, fermion
    shape = (3, 4)
    rows, cols = shape
    st, cfgs = _state(shape, name), configs(shape)
    table, _ = fermion.hubbard_hop_table()
    ctx, ctx2 = _ctx(st, _dtype(name), NW), _ctx(st, _dtype(name), NW)
    ext = st.ext_config(cfgs, fermion.ROW)
    for c in (ctx, ctx2):
        c.set_configs(ext)
        c.generate_bmps_approach(capi.UP)
    tol = TOL[name]
    for row in range(rows):
        psi, hop = ctx.nn_hop_slice_fermion(capi.HORIZONTAL, row, fermion.HUBBARD_NF, table, punch_holes=True)
        if row == 0:
            psi_w = np.real(psi[:, 0])                   # the amplitude of the decorated network the holes belong to
        # the per-site / per-bond path of the row pass on the second context
        ctx2.init_bten(capi.LEFT, row)
        ctx2.grow_full_bten(capi.RIGHT, row, 1, True)
        holes2 = []
        for col in range(cols):
            ctx2.punch_hole_store(row, col, capi.HORIZONTAL)
            holes2.append(ctx2.punch_hole(row, col, capi.HORIZONTAL))
            if col + 1 < cols:
                a, b = cfgs[:, row, col], cfgs[:, row, col + 1]
                pc = table[a * 4 + b]
                has = pc[:, :, 0] >= 0
                cands, signs = [], []
                for k in range(2):
                    new = cfgs.copy()
                    new[:, row, col], new[:, row, col + 1] = np.where(has[:, k], pc[:, k, 0], a), np.where(has[:, k], pc[:, k, 1], b)
                    ne = st.ext_config(new, fermion.ROW)
                    cands.append(np.stack([ne[:, row, col], ne[:, row, col + 1]], axis=-1))
                    signs.append(st.sigma(new) / st.sigma(cfgs))
                psi2 = ctx2.trace(row, col, capi.HORIZONTAL)
                res = ctx2.replace_nn_trace(row, col, capi.HORIZONTAL, np.stack(cands, axis=1))
                assert np.max(np.abs(psi[:, col] - psi2)) < tol * np.max(np.abs(psi2)), (row, col)
                for k in range(2):
                    want = np.where(has[:, k], signs[k] * res[:, k], 0.0)
                    assert np.max(np.abs(hop[:, col, k] - want)) <= tol * np.max(np.abs(psi2)) * max(1.0, float(np.max(np.abs(want / psi2)))), (row, col, k)
                    assert np.all(hop[~has[:, k], col, k] == 0)
                ctx2.shift_bten_window(capi.RIGHT)
        h1 = ctx.punch_hole(row, cols - 1, capi.HORIZONTAL)
        assert np.max(np.abs(h1 - holes2[-1])) < tol * np.max(np.abs(holes2[-1])), row
        if row + 1 < rows:
            ctx.shift_bmps_window(capi.DOWN)
            ctx2.shift_bmps_window(capi.DOWN)
    if name != "c128":
        e_w = np.linspace(-1.0, 2.0, NW)
        grads = []
        for c in (ctx, ctx2):
            c.grad_reset()
            c.grad_accumulate(psi_w, e_w)
            grads.append(c.grad_read())
        for g1, g2 in zip(*grads):
            assert np.max(np.abs(g2)) > 0 and np.max(np.abs(g1 - g2)) < tol * np.max(np.abs(g2))
    ctx.close()
    ctx2.close()


# ---- SquareHubbardModel through the host layer ----
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", ["f64", "f32"])
def test_hubbard_local_energy_slice_path_hook_path_and_oracle(both_paths, name, shape):
    """E_loc of SquareHubbardModel along the slice path, along the hook path and from hubbard_ref.cal_energy on the oracle's contractor at
    chi = 9; the Python driver (fermion.hubbard_energy, slice and calls) gives the same numbers"""
    from peps_amd import fermion
    key = "energy_%s_%dx%d" % ((name,) + shape)
    dev, hook = np.array(both_paths["device"][key]["energy"]), np.array(both_paths["hook"][key]["energy"])
    st, cfgs = _state(shape), configs(shape)
    fs = ref.oracle_view(st)
    tp = BMPSTruncateParams.SVD(CHI, CHI, 0.0)
    want = np.array([np.real(ref.cal_energy(fs, c, tp, T, U, MU)[0]) for c in cfgs])
    tol = E_TOL[name] * 10 * np.maximum(1.0, np.abs(want))
    print(key, "max |E_slice - E_oracle| = %.2e, |E_hook - E_oracle| = %.2e, |E_slice - E_hook| = %.2e; max |E| = %.3g"
          % (np.max(np.abs(dev - want)), np.max(np.abs(hook - want)), np.max(np.abs(dev - hook)), np.max(np.abs(want))))
    assert np.all(np.abs(dev - want) < tol) and np.all(np.abs(hook - want) < tol) and np.all(np.abs(dev - hook) < tol)
    amp = np.array(both_paths["device"][key]["amp"])
    ref_amp = np.array([fs.amplitude(c, tp) for c in cfgs])
    assert np.max(np.abs(amp / ref_amp - 1)) < E_TOL[name]
    ctx = _ctx(st, _dtype(name), NW)
    for hop in ("slice", "calls"):
        e, _ = fermion.hubbard_energy(ctx, st, cfgs, T, U, MU, hop=hop)
        assert np.all(np.abs(e - want) < tol), hop
    e, _ = fermion.hubbard_energy(ctx, st, cfgs, T, U, MU, punch_holes=True)
    assert np.all(np.abs(e - want) < tol)
    ctx.close()


def _even_2x2():
    cfgs = ref.all_configs(2, 2)
    return cfgs[ref.is_even(cfgs)].astype(np.int32)


def _dense_quotient(state):
    """the Rayleigh quotient of the dense Hubbard H over the oracle's amplitudes of all configurations of a 2 x 2 state (exact chi)"""
    fs = ref.oracle_view(state)
    tp = BMPSTruncateParams.SVD(16, 16, 0.0)
    cfgs = ref.all_configs(2, 2)
    even = ref.is_even(cfgs)
    psi = np.zeros(len(cfgs))
    for k in np.nonzero(even)[0]:
        psi[k] = fs.amplitude(cfgs[k], tp)
    return float(np.real(ref.rayleigh(_dense_quotient.H, psi)))


_dense_quotient.H = ref.dense_hubbard_hamiltonian(2, 2, T, U, MU)


def test_exact_sum_energy_equals_the_dense_rayleigh_quotient():
    """2 x 2, D = 2, exact chi: the exact-sum energy through the host layer over the 128 even configurations == <psi|H|psi> / <psi|psi> of
    the dense Jordan-Wigner H to 1e-10"""
    from peps_amd import hostapi
    st = ref.hubbard_state(2, 2, 2)
    cfgs = _even_2x2()
    assert len(cfgs) == 128
    e, _ = hostapi.fermion_exact_sum(st, cfgs, 16, T, batch=64, dtype=1, model="hubbard", U=U, mu=MU)
    want = _dense_quotient(st)
    print("exact sum: E = %.15g, dense quotient = %.15g, difference %.2e" % (e, want, abs(e - want)))
    assert abs(e - want) < 1e-10


def test_gradient_of_one_sgd_step_equals_finite_differences_of_the_dense_quotient():
    """One plain-SGD step of fermion_optimize_exact_sum(model="hubbard") on 2 x 2 in f64: g = (theta_0 - theta_1) / lr is
    <E_loc O> - E <O> = dE/dtheta / 2 for a real state.  dE/dtheta by central differences (h = 1e-5) of the dense quotient over oracle
    amplitudes: differencing error ~ h^2 ~ 1e-10, rounding ~ 1e-11, tolerance 1e-6 max |g|.  Parity-forbidden entries exactly zero."""
    from peps_amd import fermion, hostapi
    st = ref.hubbard_state(2, 2, 2)
    cfgs = _even_2x2()
    lr = 0.5
    energies, stored = hostapi.fermion_optimize_exact_sum(st, cfgs, 16, "hubbard", (T, U, MU), "sgd", lr, (0.0, 0.0, 0.0), 1, dtype=1, batch=64)
    assert abs(energies[0] - _dense_quotient(st)) < 1e-10
    theta0 = np.zeros_like(stored)
    allowed = np.zeros(stored.shape, dtype=bool)
    for r in range(2):
        for c in range(2):
            pl, pd, pr, pu = st.par[r][c]
            tot = pl[:, None, None, None] + pd[None, :, None, None] + pr[None, None, :, None] + pu[None, None, None, :]
            for s in range(4):
                a = st.tensors[r][c][s]
                sl = (r, c, s) + tuple(slice(0, k) for k in a.shape)
                theta0[sl] = a
                allowed[sl] = (tot + ref.NF[s]) % 2 == 0
    g = (theta0 - stored) / lr
    assert np.all(g[~allowed] == 0.0) and np.all(stored[~allowed] == 0.0)
    gmax = float(np.max(np.abs(g)))
    assert gmax > 1e-3
    rng = np.random.default_rng(6)
    h, worst, checked = 1e-5, 0.0, 0
    for r in range(2):
        for c in range(2):
            for s in rng.permutation(4)[:2]:
                nzs = np.argwhere(allowed[r, c, s])
                ix = tuple(nzs[rng.integers(len(nzs))])
                vals = []
                for sgn in (+1, -1):
                    tens = [[[t.copy() for t in site] for site in row] for row in st.tensors]
                    tens[r][c][s][ix] += sgn * h
                    vals.append(_dense_quotient(fermion.FermionState(tens, st.par, list(ref.NF))))
                fd = (vals[0] - vals[1]) / (2 * h)
                worst = max(worst, abs(2 * g[(r, c, s) + ix] - fd) / 2)
                checked += 1
    print("gradient: max |g| = %.3e, max |g - dE/dtheta / 2| = %.3e over %d entries" % (gmax, worst, checked))
    assert checked == 8
    assert worst < 1e-6 * gmax


@pytest.mark.parametrize("shape", SHAPES)
def test_observables_equal_the_oracle_restatement(both_paths, shape):
    """charge, spin_z, double_occupancy exactly; energy and the per-bond energies against hubbard_ref.cal_energy (f64 tolerance of the
    energy test); slice path == hook path within the same tolerance; the Python registry (fermion.hubbard_observables) agrees"""
    from peps_amd import fermion
    tag = "obs_%dx%d" % shape
    dev, hook = both_paths["device"][tag], both_paths["hook"][tag]
    st, cfgs = _state(shape), configs(shape)
    n = len(cfgs)
    assert set(dev) == {"energy", "charge", "spin_z", "double_occupancy", "bond_energy_h", "bond_energy_v"} == set(hook)
    assert np.array_equal(np.array(dev["charge"]).reshape(n, -1), (ref.N_UP[cfgs] + ref.N_DN[cfgs]).reshape(n, -1))
    assert np.array_equal(np.array(dev["spin_z"]).reshape(n, -1), (0.5 * (ref.N_UP[cfgs] - ref.N_DN[cfgs])).reshape(n, -1))
    assert np.array_equal(np.array(dev["double_occupancy"]).reshape(n, -1), (cfgs == 0).astype(float).reshape(n, -1))
    fs = ref.oracle_view(st)
    tp = BMPSTruncateParams.SVD(CHI, CHI, 0.0)
    ctx = _ctx(st, _dtype("f64"), NW)
    py, _ = fermion.hubbard_observables(ctx, st, cfgs, T, U, MU)
    ctx.close()
    for w, c in enumerate(cfgs):
        bonds = {}
        e, _ = ref.cal_energy(fs, c, tp, T, U, MU, bonds)
        tol = E_TOL["f64"] * 10 * max(1.0, abs(e), float(np.max(np.abs(bonds["h"]))), float(np.max(np.abs(bonds["v"]))))
        for key, want in (("energy", np.array([e])), ("bond_energy_h", bonds["h"].ravel()), ("bond_energy_v", bonds["v"].ravel())):
            for got in (np.array(dev[key]).reshape(n, -1)[w], np.array(hook[key]).reshape(n, -1)[w], py[key][w]):
                assert np.max(np.abs(got - np.real(want))) < tol, (key, w)
    assert np.count_nonzero(np.array(dev["bond_energy_h"])) > 0 and np.count_nonzero(np.array(dev["bond_energy_v"])) > 0


@pytest.mark.parametrize("shape", SHAPES)
def test_measurer_with_the_sector_updater_runs_identical_chains_on_both_paths(both_paths, shape):
    """fermion_measure(updater="hubbard_u1u1"), 1 warm-up sweep and 2 samples on the same streams: the final configurations and the
    accept rates of the two paths are identical, and so are the statistics of every observable that is a function of the
    configuration (charge, spin_z, double_occupancy)"""
    tag = "measure_%dx%d" % shape
    dev, hook = both_paths["device"][tag], both_paths["hook"][tag]
    assert dev["cfg"] == hook["cfg"] and dev["rate"] == hook["rate"]
    assert dev["cfg"] != configs(shape).tolist()
    assert set(dev["stats"]) == {"energy", "charge", "spin_z", "double_occupancy", "bond_energy_h", "bond_energy_v"} == set(hook["stats"])
    for key in ("charge", "spin_z", "double_occupancy"):
        assert dev["stats"][key] == hook["stats"][key], key
    assert np.max(np.abs(np.array(dev["stats"]["energy"][1]))) > 0                # the walkers sample different energies


@pytest.mark.parametrize("shape", SHAPES)
def test_measurer_statistics_are_identical_on_both_paths(both_paths, shape):
    """The same runs: every mean, every standard error and every energy sample of the slice path equals the hook path's, bit for bit.
    (A slice scales its mantissas by exp(log-scale) in the kernel, a per-bond call by default with std::exp on the host, and the two
    exponentials may differ in the last bit: with the host form the mean of bond_energy_h[3] on 3 x 4 came out 5.6e-17 off.  The hooks of
    the Hubbard model and updater therefore ask for the kernel's form, pepsgpu_trace_scaling.)"""
    tag = "measure_%dx%d" % shape
    dev, hook = both_paths["device"][tag], both_paths["hook"][tag]
    worst = {key: max(float(np.max(np.abs(np.array(dev["stats"][key][k]) - np.array(hook["stats"][key][k])))) for k in range(2))
             for key in dev["stats"]}
    print(tag, "max |slice - hook| per key:", worst, "energy samples:", float(np.max(np.abs(np.array(dev["energy"]) - np.array(hook["energy"])))))
    assert dev["stats"] == hook["stats"]
    assert dev["energy"] == hook["energy"]


@pytest.mark.parametrize("name", ["f64", "f32", "c128"])
def test_per_bond_calls_with_device_scaling_return_the_bits_of_the_slice(name):
    """pepsgpu_trace_scaling(1): Trace + ReplaceNNSiteTrace per bond return psi and the hops of pepsgpu_nn_hop_slice_fermion byte for byte,
    rows and columns of 3 x 4; switched off again the calls return the host-scaled numbers, equal within 4 eps"""
    from peps_amd import capi, fermion
    shape = (3, 4)
    st, cfgs = _state(shape, name), configs(shape)
    table, _ = fermion.hubbard_hop_table()
    ctx, ctx2 = _ctx(st, _dtype(name), NW), _ctx(st, _dtype(name), NW)
    differing = 0
    for orient, order, approach, step in _passes():
        ext = st.ext_config(cfgs, order)
        for c in (ctx, ctx2):
            c.set_configs(ext)
            c.generate_bmps_approach(approach)
        S = shape[0] if orient == capi.HORIZONTAL else shape[1]
        lo, hi = (capi.LEFT, capi.RIGHT) if orient == capi.HORIZONTAL else (capi.UP, capi.DOWN)
        for s in range(S):
            psi, hop = ctx.nn_hop_slice_fermion(orient, s, fermion.HUBBARD_NF, table)
            ctx2.trace_scaling(True)
            psi2, _, hop2 = fermion._pair_slice_by_calls(ctx2, st, cfgs, orient, order, lo, hi, s, table)
            ctx2.trace_scaling(False)
            psi3, _, hop3 = fermion._pair_slice_by_calls(ctx2, st, cfgs, orient, order, lo, hi, s, table)
            assert psi.tobytes() == psi2.tobytes() and hop.tobytes() == hop2.tobytes(), (name, orient, s)
            assert np.max(np.abs(psi3 - psi)) <= 4 * 2.220446049250313e-16 * np.max(np.abs(psi))
            assert np.max(np.abs(hop3 - hop)) <= 4 * 2.220446049250313e-16 * np.max(np.abs(hop))
            differing += int(np.sum(psi3 != psi) + np.sum(hop3 != hop))
            if s + 1 < S:
                ctx.shift_bmps_window(step)
                ctx2.shift_bmps_window(step)
    print(name, "entries whose host-scaled value differs from the kernel-scaled one:", differing)
    ctx.close()
    ctx2.close()


# ---- the contract of the two C calls ----
def test_refusals_leave_the_configuration_untouched_and_the_context_usable():
    from peps_amd import capi, fermion
    shape = (3, 4)
    rows, cols = shape
    st, cfgs = _state(shape), configs(shape)
    ctx = _ctx(st, _dtype("f64"), NW)
    ext = st.ext_config(cfgs, fermion.ROW)
    ctx.set_configs(ext)
    amp0 = ctx.evaluate_amplitude()
    ctx.set_configs(ext)                                                           # (a fresh Init: the boundary MPS stacks are empty again)
    lib, h = ctx._l, ctx._h
    tab, (htab, _) = fermion.hubbard_sector_table(), fermion.hubbard_hop_table()
    occ = np.array(fermion.HUBBARD_NF, dtype=np.int32)
    words = (np.arange(NW * 2 * (cols - 1), dtype=np.uint64) * 2654435761 % 2 ** 32).astype(np.uint32).reshape(NW, -1)
    wp = words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    a, ci, ai = amp0.copy(), np.zeros(NW, dtype=np.int32), np.zeros(NW, dtype=np.int32)
    si = np.zeros((NW, cols), dtype=np.int32)

    def sector(orient=capi.HORIZONTAL, slice_=0, d=4, occ_=occ, maxc=4, table=tab, nwords=words.shape[1], wptr=wp, amp=a):
        return lib.pepsgpu_sweep_slice_sector(h, orient, slice_, d, None if occ_ is None else capi._ip(occ_), maxc,
                                              None if table is None else capi._ip(table), nwords, wptr,
                                              None if amp is None else capi._dp(amp), capi._ip(ci), capi._ip(ai), capi._ip(si))

    EINVAL, ESTATE, ERANGE = 1, 3, 4
    # no boundary MPS yet
    assert sector() == ESTATE
    ctx.generate_bmps_approach(capi.UP)
    assert sector(orient=2) == EINVAL and sector(slice_=rows) == EINVAL and sector(slice_=-1) == EINVAL
    assert sector(table=None) == EINVAL and sector(amp=None) == EINVAL and sector(wptr=None) == EINVAL
    assert sector(nwords=2 * (cols - 1) - 1) == EINVAL
    assert sector(maxc=0) == EINVAL and sector(maxc=17) == EINVAL
    assert sector(d=3) == EINVAL and sector(occ_=None) == EINVAL                 # 4 d != 16; a bosonic table on a 16-state context
    bad = tab.copy(); bad[5, 0] = 5                                                # m > max_cand
    assert sector(table=bad) == EINVAL
    bad = tab.copy(); bad[6, 1] = 3                                                # the initial slot is not the pair itself
    assert sector(table=bad) == EINVAL
    bad = tab.copy(); bad[6, 2] = -1                                               # a -1 in a used slot
    assert sector(table=bad) == EINVAL
    bad = tab.copy(); bad[15, 4:6] = (3, 3)                                        # a state in an unused slot
    assert sector(table=bad) == EINVAL
    bad = tab.copy(); bad[6, 2:4] = (1, 3)                                         # (up, down) -> (up, empty): changes the parity of the pair
    assert sector(table=bad) == EINVAL
    bad = tab.copy(); bad[6, 2] = 4                                                # a state outside [0, d)
    assert sector(table=bad) == ERANGE
    bad_occ = occ.copy(); bad_occ[1] = 2
    assert sector(occ_=bad_occ) == EINVAL
    # states of the other mode order in the slice
    assert np.array_equal(ctx.get_configs(), ext)
    ctx.set_configs(st.ext_config(cfgs, fermion.COL))
    ctx.generate_bmps_approach(capi.UP)
    assert sector() == ESTATE
    assert np.array_equal(ctx.get_configs(), st.ext_config(cfgs, fermion.COL))
    # the hop slice: its own refusals
    psi, hop = np.zeros((NW, cols - 1)), np.zeros((NW, cols - 1, 2))

    def hops(orient=capi.HORIZONTAL, slice_=0, d=4, occ_=occ, table=htab, out=hop):
        return lib.pepsgpu_nn_hop_slice_fermion(h, orient, slice_, 1, d, None if occ_ is None else capi._ip(occ_),
                                                None if table is None else capi._ip(table), capi._dp(psi), None if out is None else capi._dp(out))
    assert hops() == ESTATE                                                        # column-major states in a row slice
    ctx.set_configs(ext)
    assert hops() == ESTATE                                                        # no boundary MPS
    ctx.generate_bmps_approach(capi.UP)
    assert hops(orient=3) == EINVAL and hops(slice_=rows) == EINVAL and hops(d=2) == EINVAL
    assert hops(occ_=None) == EINVAL and hops(table=None) == EINVAL and hops(out=None) == EINVAL
    badh = htab.copy(); badh[6, 0] = (1, 3)                                        # changes the parity of the pair
    assert hops(table=badh) == EINVAL
    badh = htab.copy(); badh[6, 0, 0] = -1                                         # a candidate with only one -1
    assert hops(table=badh) == EINVAL
    # an active override
    ctx.cfg_override_slice(capi.HORIZONTAL, 0, ext[:, 0, :])
    assert sector() == ESTATE and hops() == ESTATE
    ctx.cfg_override_slice(capi.HORIZONTAL, 0, None)
    assert np.array_equal(ctx.get_configs(), ext)
    # the next valid calls succeed
    assert hops() == 0 and np.all(psi != 0)
    amp, cons, acc, states = ctx.sweep_slice_sector(capi.HORIZONTAL, 0, tab, words, amp0, nf=fermion.HUBBARD_NF)
    m = np.array([[len(ref.sector(int(x), int(y))) for x, y in zip(row[:-1], row[1:])] for row in cfgs[:, 0, :]])
    assert np.all(cons % 2 == 0) and np.all(cons <= 2 * (cols - 1)) and np.all(np.abs(amp) > 0)
    assert np.all(cons[acc == 0] == 2 * np.sum(m[acc == 0] > 1, axis=1))          # a walker that never moved drew on its m > 1 bonds only
    assert np.array_equal(states % 4, ctx.get_configs()[:, 0, :] % 4)
    ctx.close()
