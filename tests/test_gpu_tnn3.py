"""GPU tests of the three-site exchange updater (MCUpdateSquareTNN3SiteExchange, square_3site_updater.h:28-158): the device-side slice
(pepsgpu_sweep_slice_tnn3) against the per-triple hook path (PEPSHOST_NO_DEVICE_SWEEP=1) in child processes -- bosonic f64 / f32 /
complex, a non-square lattice, a d = 3 state (six permutations per triple) and the reference's 6x6 t-J state in f64 / f32 --, the
carried f32 amplitude against a fresh evaluation, and the C call's own contract (reset, no draw for equal triples, status codes).
The f64 chain, the energy-gradient loop and MCPEPSMeasurer are checked against the reference's updater restated on the oracle
(tests/tnn3_ref.py)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from peps_amd import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tnn3_ref  # noqa: E402
from oracle import vmc  # noqa: E402
from oracle.bmps import BMPSTruncateParams  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"f64": 1e-12, "f32": 1e-5, "c128": 1e-12}

_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from peps_amd import hostapi, synthetic, fermion
from oracle import vmc
from oracle.bmps import BMPSTruncateParams

def cx(a):
    a = np.asarray(a)
    return [[float(x.real), float(x.imag)] for x in a.ravel()] if np.iscomplexobj(a) else [float(x) for x in a.ravel()]

def shuffled(base, n, seed):
    return np.stack([np.random.default_rng(seed + k).permutation(base.ravel()).reshape(base.shape) for k in range(n)]).astype(np.int32)

n, chi, sweeps = 8, 12, 2
seeds = np.arange(n, dtype=np.uint64) + 31
out = {}
L, D = 6, 4
sitps = synthetic.make_sitps(L, D, noise=0.5)
flat = synthetic.sitps_to_flat(sitps, D)
cfgs = synthetic.make_configs(L, n, "heisenberg", seed0=5)
for name, dt in (("b64", 1), ("b32", 0)):
    c, a, r = hostapi.mc_sweeps(flat, cfgs, seeds, chi, "tnn3", sweeps, dt)
    out[name] = {"cfg": c.tolist(), "amp": cx(a), "rate": cx(r), "start": cfgs.tolist()}
    if dt == 0:      # the carried f32 amplitude against the oracle's EvaluateAmplitude of the final configuration
        tp = BMPSTruncateParams.SVD(chi, chi, 0.0)
        ref = np.array([vmc.TPSWaveFunctionComponent(sitps, cc, tp).amplitude for cc in c])
        out[name]["fresh"] = cx(ref)
cflat = flat * np.exp(2j * np.pi * np.random.default_rng(3).uniform(size=flat.shape))
c, a, r = hostapi.mc_sweeps_complex(cflat, cfgs, seeds, chi, "tnn3", sweeps)
out["c128"] = {"cfg": c.tolist(), "amp": cx(a), "rate": cx(r), "start": cfgs.tolist()}
# a non-square 5 x 4 lattice cut from the 6 x 6 state (open bonds of the cut edge: their first index)
f54 = np.ascontiguousarray(flat[:5, :4])
c54 = shuffled(np.r_[np.zeros(10, dtype=int), np.ones(10, dtype=int)].reshape(5, 4), n, 50)
c, a, r = hostapi.mc_sweeps(f54, c54, seeds, chi, "tnn3", sweeps, 1)
out["b64_5x4"] = {"cfg": c.tolist(), "amp": cx(a), "rate": cx(r), "start": c54.tolist()}
# d = 3: triples of three different states (six permutations)
f3 = synthetic.sitps_to_flat(synthetic.make_sitps(4, 3, d=3, noise=0.5), 3)
c3 = shuffled(np.r_[np.zeros(5, dtype=int), np.ones(5, dtype=int), 2 * np.ones(6, dtype=int)].reshape(4, 4), n, 70)
c, a, r = hostapi.mc_sweeps(f3, c3, seeds, 9, "tnn3", sweeps, 1)
out["b64_d3"] = {"cfg": c.tolist(), "amp": cx(a), "rate": cx(r), "start": c3.tolist()}
# the reference's 6x6 t-J state (0 up, 1 down, 2 hole), walkers from count-preserving shuffles of its configuration0; chi = 48
# (at chi = 16 the truncation alone puts the column-pass amplitude 3e-3 from a fresh row-major evaluation, in f64 as in f32)
d = os.path.join(sys.argv[1], "tests", "golden", "ref_fixtures", "tps_tJ_6x6Hole2_J0.3_D8_fU1")
st = fermion.FermionState.load(d)
c0 = np.loadtxt(os.path.join(d, "configuration0"), dtype=int).reshape(6, 6)
ct = shuffled(c0, 4, 90)
for name, dt in (("tj64", 1), ("tj32", 0)):
    c, a, r = hostapi.fermion_mc_sweeps(st, ct, seeds[:4], 48, 1, dt, updater="tnn3")
    out[name] = {"cfg": c.tolist(), "amp": cx(a), "rate": cx(r), "start": ct.tolist()}
    if dt == 0:      # ... against the float64 evaluation of the final configuration, signs included
        amps, _, _ = hostapi.fermion_energy(st, c, 48, 1.0, 0.0, 1, "tj", 0.3, 0.0)
        out[name]["fresh"] = cx(amps)
print(json.dumps(out))
"""


def _as_array(v):
    a = np.asarray(v)
    return a[..., 0] + 1j * a[..., 1] if a.ndim == 2 else a


@pytest.fixture(scope="module")
def both_paths():
    res = {}
    for name, env in (("device", {}), ("hook", {"PEPSHOST_NO_DEVICE_SWEEP": "1"})):
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    return res


@pytest.mark.parametrize("case", ["b64", "b32", "c128", "b64_5x4", "b64_d3", "tj64", "tj32"])
def test_device_slice_equals_hook_path(both_paths, case):
    """identical configurations and accept rates, amplitudes within 1e-12 (f64, complex) / 1e-5 (f32); the chains moved"""
    dev, hook = both_paths["device"][case], both_paths["hook"][case]
    assert dev["cfg"] == hook["cfg"], case
    assert np.array_equal(np.array(dev["rate"]), np.array(hook["rate"])), case
    a, b = _as_array(dev["amp"]), _as_array(hook["amp"])
    tol = TOL["f32" if case.endswith("32") else "f64"]
    assert np.max(np.abs(a - b)) < tol * np.max(np.abs(b)), (case, np.max(np.abs(a - b)) / np.max(np.abs(b)))
    assert dev["cfg"] != dev["start"], "no walker moved: %s" % case
    assert max(dev["rate"]) > 0


@pytest.mark.parametrize("case", ["b64", "b32", "c128", "b64_5x4", "b64_d3", "tj64", "tj32"])
def test_moves_conserve_the_state_counts(both_paths, case):
    """a permutation of three states conserves Sz and the particle numbers of every walker"""
    dev = both_paths["device"][case]
    for c, s in zip(dev["cfg"], dev["start"]):
        assert sorted(np.ravel(c).tolist()) == sorted(np.ravel(s).tolist())


@pytest.mark.parametrize("case", ["b32", "tj32"])
def test_f32_carried_amplitude_equals_fresh_evaluation(both_paths, case):
    dev = both_paths["device"][case]
    a, ref = _as_array(dev["amp"]), _as_array(dev["fresh"])
    assert np.all(np.sign(a) == np.sign(ref)), case
    assert np.max(np.abs(a / ref - 1)) < 1e-4, (case, np.max(np.abs(a / ref - 1)))


def _ctx(rows, cols, cfgs, dtype=None):
    from peps_amd import capi
    D, chi = 3, 9
    flat = synthetic.sitps_to_flat(synthetic.make_sitps(max(rows, cols), D, noise=0.5), D)[:rows, :cols]
    ctx = capi.Context(rows, cols, D, 2, chi, dtype=capi.F64 if dtype is None else dtype, max_walkers=len(cfgs))
    ctx.state_upload(np.ascontiguousarray(flat))
    ctx.set_configs(np.asarray(cfgs, dtype=np.int32))
    return ctx


def test_c_call_contract():
    from peps_amd import capi
    L, n = 4, 3
    cfgs = np.zeros((n, L, L), dtype=np.int32)
    cfgs[1, 2] = 1                          # walker 1: row 2 all "1"; row 0 stays all "0" for every walker
    cfgs[2, :, 1] = 1
    ctx = _ctx(L, L, cfgs)
    words = np.arange(n * 2 * (L - 2), dtype=np.uint32).reshape(n, -1) * 2654435761
    # a row of equal states: no trace, no draw, no move; the amplitude is the trace of the first window
    ctx.generate_bmps_approach(capi.UP)
    amp, cons, acc, st = ctx.sweep_slice_tnn3(capi.HORIZONTAL, 0, words)
    ctx.init_bten(capi.LEFT, 0)
    ctx.grow_full_bten(capi.RIGHT, 0, 3, True)
    ref = ctx.replace_tnn_trace(0, 0, capi.HORIZONTAL)
    assert np.array_equal(cons[:2], [0, 0]) and np.array_equal(acc[:2], [0, 0])
    assert np.array_equal(st[:2], np.zeros((2, L), dtype=np.int32))
    # walker 2 has "0 1 0 0": its first triple draws; its second draws unless the first move made it "0 0 0"
    assert cons[2] == (2 if acc[2] == 1 and st[2, 1] == st[2, 2] == st[2, 3] else 4), (cons[2], acc[2], st[2])
    assert np.max(np.abs(amp[:2] - ref[:2])) < 1e-12 * np.max(np.abs(ref[:2]))
    assert np.all(np.abs(amp) > 0)
    before = ctx.get_configs().copy()
    lib, h = ctx._l, ctx._h
    a, ci, ai, si = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros((n, L), dtype=np.int32)
    wp = words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    args = lambda: (capi._dp(a), capi._ip(ci), capi._ip(ai), capi._ip(si))
    assert lib.pepsgpu_sweep_slice_tnn3(h, capi.HORIZONTAL, 1, None, 2 * (L - 2) - 1, wp, *args()) == 1   # too few words
    assert lib.pepsgpu_sweep_slice_tnn3(h, 2, 1, None, words.shape[1], wp, *args()) == 1                  # orientation
    assert lib.pepsgpu_sweep_slice_tnn3(h, capi.VERTICAL, L, None, words.shape[1], wp, *args()) == 1      # slice
    bad = np.ascontiguousarray(np.tile(np.r_[3, 0, np.zeros(18, dtype=int)], (8, 1)), dtype=np.int32)
    bad[5, 4] = 2                                                                                        # state outside [0, 2)
    assert lib.pepsgpu_sweep_slice_tnn3(h, capi.HORIZONTAL, 1, capi._ip(bad), words.shape[1], wp, *args()) == 4
    assert np.array_equal(ctx.get_configs(), before)
    ctx.close()
    # fewer than three rows: refused
    c2 = np.zeros((1, 2, 5), dtype=np.int32)
    c2[0, 0, 1] = 1
    ctx = _ctx(2, 5, c2)
    ctx.generate_bmps_approach(capi.UP)
    w2 = np.zeros((1, 6), dtype=np.uint32)
    with pytest.raises(ValueError):
        ctx.sweep_slice_tnn3(capi.HORIZONTAL, 0, w2)
    assert np.array_equal(ctx.get_configs(), c2)
    ctx.close()


# ---- against the reference's updater restated on the oracle (tests/tnn3_ref.py) ----
F64 = 1


def _rect_state(rows, cols, D, d=2, seed_noise=0.5):
    """a rows x cols open state cut from a square synthetic one (the cut edges keep the first index of their bond: dimension 1), as
    oracle tensors and as the upload layout"""
    L = max(rows, cols)
    sq = synthetic.make_sitps(L, D, d=d, noise=seed_noise)
    s = [[[t[:, :1, :, :] if r == rows - 1 else t for t in sq[r][c]] for c in range(cols)] for r in range(rows)]
    s = [[[t[:, :, :1, :] if c == cols - 1 else t for t in s[r][c]] for c in range(cols)] for r in range(rows)]
    flat = np.zeros((rows, cols, d, D, D, D, D))
    for r in range(rows):
        for c in range(cols):
            for k in range(d):
                t = s[r][c][k]
                flat[r, c, k, :t.shape[0], :t.shape[1], :t.shape[2], :t.shape[3]] = t
    return s, flat


def _count_configs(rows, cols, counts, n, seed):
    base = np.concatenate([np.full(k, v) for v, k in enumerate(counts)])
    assert base.size == rows * cols
    return np.stack([np.random.default_rng(seed + k).permutation(base).reshape(rows, cols) for k in range(n)]).astype(np.int32)


def _oracle_chain(s, cfg, chi, seed, n_sweeps):
    comp = vmc.TPSWaveFunctionComponent(s, cfg, BMPSTruncateParams.SVD(chi, chi, 0.0))
    upd = tnn3_ref.MCUpdateSquareTNN3SiteExchange(seed=seed)
    rates = [upd(s, comp)[0] for _ in range(n_sweeps)]
    return comp, upd, rates


@pytest.mark.parametrize("rows,cols,d,counts", [(4, 4, 2, (8, 8)), (5, 4, 2, (10, 10)), (4, 4, 3, (5, 5, 6))])
def test_f64_chain_equals_reference_restatement(rows, cols, d, counts):
    """same std::mt19937 streams, two sweeps, f64 device slices: the configurations are the restated reference's, the amplitudes
    agree within 1e-8 and the accept rates within 1e-12 (4x4, a non-square 5x4, and d = 3 with six permutations per triple)"""
    from peps_amd import hostapi
    D, chi, n = 3, 9, 4
    s, flat = _rect_state(rows, cols, D, d)
    cfgs = _count_configs(rows, cols, counts, n, 300 + rows * 10 + d)
    seeds = np.arange(n, dtype=np.uint64) + 61
    out_cfg, amps, rates = hostapi.mc_sweeps(flat, cfgs, seeds, chi, "tnn3", 2, F64)
    moved = 0
    for w in range(n):
        comp, _, r = _oracle_chain(s, cfgs[w], chi, int(seeds[w]), 2)
        assert np.array_equal(comp.config, out_cfg[w]), w
        assert abs(amps[w] / comp.amplitude - 1) < 1e-8, (w, amps[w], comp.amplitude)
        assert abs(rates[w] - np.mean(r)) < 1e-12, (w, rates[w], r)
        moved += int(np.any(comp.config != cfgs[w]))
    assert moved > 0


def test_energy_grad_loop_runs_the_reference_chain():
    """pepshost_mc_energy_grad_partial with updater 2: after the warm-up and sample sweeps the walkers stand where the restated
    reference's chains stand, with the same accept rate over the samples"""
    from peps_amd import hostapi
    L, D, chi, n = 4, 3, 9, 4
    s, flat = _rect_state(L, L, D)
    cfgs = synthetic.make_configs(L, n, "heisenberg", seed0=17)
    seeds = np.arange(n, dtype=np.uint64) + 71
    params = (1.0, 1.0, 0.5, 0.4, 0.0)
    _, out_cfg, acc = hostapi.mc_energy_grad_partial(flat, cfgs, seeds, chi, "tnn3", "j1j2", params, 1, 2, F64)
    for w in range(n):
        comp, _, r = _oracle_chain(s, cfgs[w], chi, int(seeds[w]), 3)
        assert np.array_equal(comp.config, out_cfg[w]), w
        assert abs(acc[w] - np.mean(r[1:])) < 1e-12, (w, acc[w], r)


def test_mc_measurer_tnn3_identical_chain_statistics():
    """MCPEPSMeasurer with the three-site updater on the J1-J2 model: warm-up + samples on the same std::mt19937 streams as the
    restated reference's chains (f64); per-walker sample means, and mean / standard error across the walkers, agree"""
    from peps_amd import hostapi
    from oracle import statistics
    L, D, chi = 4, 3, 9
    s, flat = _rect_state(L, L, D)
    cfgs = synthetic.make_configs(L, 4, "heisenberg")
    seeds = np.array([21, 22, 23, 24], dtype=np.uint64)
    warm, nsamp, between = 2, 3, 2
    params = (1.0, 1.0, 0.5, 0.4, 0.0)
    model = vmc.SquareSpinOneHalfJ1J2XXZModelOBC(*params)
    means = []
    for w in range(len(cfgs)):
        comp, upd, _ = _oracle_chain(s, cfgs[w], chi, int(seeds[w]), warm)
        acc = {}
        for _ in range(nsamp):
            for _ in range(between):
                upd(s, comp)
            obs = vmc.SquareNNNModelMeasurementSolver(model).EvaluateObservables(s, comp)
            for k, v in obs.items():
                acc[k] = acc.get(k, 0.0) + np.asarray(v, dtype=np.float64)
        means.append({k: v / nsamp for k, v in acc.items()})
    run_cfgs = cfgs.copy()
    got, _ = hostapi.measure(flat, run_cfgs, chi, "j1j2", params, seeds=seeds, updater="tnn3", warmup_sweeps=warm, n_samples=nsamp,
                             sweeps_between_samples=between, dtype=F64)
    assert set(got) == set(means[0])
    for key in means[0]:
        stack = np.stack([m[key] for m in means])
        mean, err = statistics.gather_statistic_list_of_data(stack)
        assert np.max(np.abs(got[key][0] - mean)) < 1e-8 * max(1.0, np.max(np.abs(mean))), key
        assert np.max(np.abs(got[key][1] - err)) < 1e-8 * max(1.0, np.max(np.abs(err))), key
