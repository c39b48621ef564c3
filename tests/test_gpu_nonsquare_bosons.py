"""GPU tests of the bosonic models of the host layer on NON-SQUARE lattices: energy_and_holes (holes on the host and no holes), measure
and -- for the J1-J2 model -- mc_energy_grad_partial (holes resident on the device) of xxz, j1j2, triangle, tfim on 2 x 3, 3 x 2 and
3 x 4 and of trij1j2 on 3 x 4 and 4 x 3 (its steep and flat links need three rows and three columns), D = 2, chi = 8, 4 walkers,
float64 and float32.

Every other bosonic host-layer test builds its state with synthetic.make_sitps(L, ...), which is square: rows and columns (lx and
ly) swapped somewhere in the traversal of the solvers would pass all of them.  The states here are rows x cols with boundary legs of
dimension 1, packed by hand to the upload layout.  The configurations are random Sz-balanced shuffles (iid bits for the TFIM), not the
checkerboard: on the checkerboard the two spins of every diagonal are equal and no diagonal exchange term runs.

(a) the device slices against the per-bond hook path (PEPSHOST_NO_DEVICE_SWEEP=1), two child processes started once for the module,
    to the TOL of tests/test_gpu_energy_slices.py;
(b) float64 against the NumPy oracle (oracle/vmc.py: CalEnergyAndHoles and the measurement solvers), energies, holes, psi lists and
    registries, to the 1e-9 of tests/test_gpu_host.py::test_xxz_energy_and_holes_fixed_configs.  At chi = 8 these lattices contract
    without truncation."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import vmc
from oracle.bmps import BMPSTruncateParams

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, CHI, NW = 2, 8, 4
TOL = {"f64": 1e-12, "f32": 1e-5}                 # TOL of tests/test_gpu_energy_slices.py
ORACLE_TOL = 1e-9                                 # tests/test_gpu_host.py::test_xxz_energy_and_holes_fixed_configs
SMALL = [(2, 3), (3, 2), (3, 4)]
MODELS = {"xxz": ((1.0, 0.8, 0.1), SMALL), "j1j2": ((1.0, 0.8, 0.5, 0.4, 0.1), SMALL), "triangle": ((), SMALL),
          "tfim": ((0.7,), SMALL), "trij1j2": ((0.3,), [(3, 4), (4, 3)])}
CASES = [(m, s) for m, (_, shapes) in MODELS.items() for s in shapes]
GRAD_MODEL = "j1j2"                               # mc_energy_grad_partial: NN slices with resident holes + the NNN slice


def make_state(rows, cols):
    """[row][col][s] -> (L, D, R, U) tensors, boundary legs of dimension 1: a positive product plus noise (amplitudes of one sign: no walker sits
    on a node)"""
    rng = np.random.default_rng(100 * rows + cols)
    sitps = []
    for r in range(rows):
        row = []
        for c in range(cols):
            shp = (1 if c == 0 else D, 1 if r == rows - 1 else D, 1 if c == cols - 1 else D, 1 if r == 0 else D)
            row.append([np.einsum("i,j,k,l->ijkl", *[rng.uniform(0.5, 1.5, size=k) for k in shp]) + 0.25 * rng.standard_normal(shp)
                        for _ in range(2)])
        sitps.append(row)
    return sitps


def to_flat(sitps):
    """the upload layout [row][col][s][L][D][R][U], zero padded to D^4 per component"""
    rows, cols = len(sitps), len(sitps[0])
    flat = np.zeros((rows, cols, 2, D, D, D, D))
    for r in range(rows):
        for c in range(cols):
            for s in range(2):
                t = sitps[r][c][s]
                flat[r, c, s, :t.shape[0], :t.shape[1], :t.shape[2], :t.shape[3]] = t
    return flat


def make_configs(model, rows, cols):
    rng = np.random.default_rng(7 + 10 * rows + cols)
    if model == "tfim":
        return rng.integers(0, 2, size=(NW, rows, cols)).astype(np.int32)
    base = np.array([0, 1] * (rows * cols // 2), dtype=np.int32)
    return np.stack([rng.permutation(base).reshape(rows, cols) for _ in range(NW)])


_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from peps_amd import capi, hostapi
import test_gpu_nonsquare_bosons as tb

out = {}
for model, shape in tb.CASES:
    prm = tb.MODELS[model][0]
    flat, cfgs = tb.to_flat(tb.make_state(*shape)), tb.make_configs(model, *shape)
    for name, dt in (("f64", 1), ("f32", 0)):
        o = {}
        amps, en, holes, psi = hostapi.energy_and_holes(flat, cfgs, tb.CHI, model, prm, True, dt)
        o["amps"], o["energy"], o["holes"], o["psi"] = amps.tolist(), en.tolist(), holes.ravel().tolist(), psi.tolist()
        _, en, _, psi = hostapi.energy_and_holes(flat, cfgs, tb.CHI, model, prm, False, dt)
        o["energy_noholes"], o["psi_noholes"] = en.tolist(), psi.tolist()
        obs, (pm, pe) = hostapi.measure(flat, cfgs, tb.CHI, model, prm, dtype=dt)
        o["obs"] = {k: v.tolist() for k, v in obs.items()}
        o["psi_mean"], o["psi_rel_err"] = pm.tolist(), pe.tolist()
        if model == tb.GRAD_MODEL:
            seeds = np.arange(tb.NW, dtype=np.uint64) + 90
            packed, cf, acc = hostapi.mc_energy_grad_partial(flat, cfgs, seeds, tb.CHI, "exchange", model, prm, 1, 2, dt)
            o["packed"], o["mc_cfg"], o["mc_acc"] = packed.tolist(), cf.tolist(), acc.tolist()
        out["%s_%dx%d_%s" % (model, shape[0], shape[1], name)] = o
out["calls"] = {"nnn": capi.diag_nnn_slice_calls(), "link": capi.diag_link_slice_calls()}
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def both_paths():
    res = {}
    for name, env in (("device", {}), ("hook", {"PEPSHOST_NO_DEVICE_SWEEP": "1"})):
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    return res


@functools.lru_cache(maxsize=None)
def oracle(model, shape):
    """per walker: (amplitude, energy, holes [row][col], psi list, registry, psi summary) of the NumPy oracle"""
    prm = MODELS[model][0]
    sitps, cfgs = make_state(*shape), make_configs(model, *shape)
    tp = BMPSTruncateParams.SVD(CHI, CHI, 0.0)
    om = {"xxz": vmc.SquareSpinOneHalfXXZModelOBC, "j1j2": vmc.SquareSpinOneHalfJ1J2XXZModelOBC, "triangle": vmc.SpinOneHalfTriHeisenbergSqrPEPS,
          "trij1j2": vmc.SpinOneHalfTriJ1J2HeisenbergSqrPEPS, "tfim": vmc.TransverseFieldIsingSquareOBC}[model]
    out = []
    for c in cfgs:
        comp = vmc.TPSWaveFunctionComponent(sitps, c, tp)
        e, holes, psis = om(*prm).CalEnergyAndHoles(sitps, comp, True)
        ms = om(*prm) if model in ("trij1j2", "tfim") else vmc.SquareNNNModelMeasurementSolver(om(*prm))
        obs = ms.EvaluateObservables(sitps, vmc.TPSWaveFunctionComponent(sitps, c, tp))
        if model == "triangle":
            obs.pop("bond_energy_dr")             # (the model's registry keeps the interacting diagonal only)
        out.append((comp.amplitude, e, holes, psis, obs, ms.last_psi_summary))
    return out


def test_the_two_children_took_the_two_paths(both_paths):
    assert both_paths["device"]["calls"]["nnn"] > 0 and both_paths["device"]["calls"]["link"] > 0
    assert both_paths["hook"]["calls"] == {"nnn": 0, "link": 0}


def test_the_configurations_run_the_diagonal_terms():
    """some walker has unequal spins on a diagonal of each kind, and on a flat and a steep link of the triangular J1-J2 model"""
    for model, shape in CASES:
        if model == "tfim":
            continue
        c = make_configs(model, *shape)
        assert np.all(c.sum(axis=(1, 2)) == shape[0] * shape[1] // 2)
        assert np.any(c[:, :-1, :-1] != c[:, 1:, 1:]) and np.any(c[:, 1:, :-1] != c[:, :-1, 1:]), (model, shape)
        if model == "trij1j2":
            assert np.any(c[:, 1:, :-2] != c[:, :-1, 2:]) and np.any(c[:, 2:, :-1] != c[:, :-2, 1:]), shape


def _flatten(o, prefix=""):
    for k, v in o.items():
        if isinstance(v, dict):
            yield from _flatten(v, prefix + k + ".")
        else:
            yield prefix + k, np.asarray(v, dtype=np.float64)


@pytest.mark.parametrize("name", ["f64", "f32"])
@pytest.mark.parametrize("model,shape", CASES)
def test_device_slices_equal_the_hook_path(both_paths, model, shape, name):
    key = "%s_%dx%d_%s" % (model, shape[0], shape[1], name)
    dev, hook = dict(_flatten(both_paths["device"][key])), dict(_flatten(both_paths["hook"][key]))
    assert set(dev) == set(hook)
    assert ("packed" in hook) == (model == GRAD_MODEL)
    for k, b in hook.items():
        a = dev[k]
        assert a.shape == b.shape and a.size > 0, (key, k)
        if k in ("mc_cfg", "mc_acc"):             # the same chain
            assert np.array_equal(a, b), (key, k)
            continue
        if k == "psi_rel_err":                    # (a difference of nearly equal amplitudes over their mean: absolute)
            assert np.max(np.abs(a - b)) < TOL[name], (key, k)
            continue
        diff = float(np.max(np.abs(a - b)))
        scale = float(np.sum(np.abs(b))) if k == "packed" else max(float(np.max(np.abs(b))), 1e-300)
        print(key, k, "max |device - hook| / scale = %.2e" % (diff / scale))
        assert diff < TOL[name] * scale, (key, k, diff / scale)


@pytest.mark.parametrize("path", ["device", "hook"])
@pytest.mark.parametrize("model,shape", CASES)
def test_f64_energy_holes_and_registry_equal_the_oracle(both_paths, model, shape, path):
    rows, cols = shape
    got = both_paths[path]["%s_%dx%d_f64" % (model, rows, cols)]
    tol = ORACLE_TOL
    holes = np.asarray(got["holes"]).reshape(NW, rows, cols, D, D, D, D)
    psi, psi_nh = np.asarray(got["psi"]), np.asarray(got["psi_noholes"])
    nz = 0
    for w, (a, e, h, ps, obs, (pm, prel)) in enumerate(oracle(model, shape)):
        assert abs(got["amps"][w] / a - 1) < tol
        for en in (got["energy"][w], got["energy_noholes"][w]):
            assert abs(en - e) < tol * max(1.0, abs(e)) * 10, (w, en, e)
        for r in range(rows):
            for c in range(cols):
                hr = h[r][c]
                hd = holes[w, r, c][:hr.shape[0], :hr.shape[1], :hr.shape[2], :hr.shape[3]]
                assert np.max(np.abs(hd - hr)) < tol * 10 * np.max(np.abs(hr)), (w, r, c)
        for p in (psi, psi_nh):                   # psi along every row (TFIM: rows only) and column
            assert p.shape[0] == len(ps) == (rows if model == "tfim" else rows + cols)
            assert np.max(np.abs(p[:, w] / np.array(ps) - 1)) < tol * 10
        assert set(got["obs"]) == set(obs)
        for key, want in obs.items():
            want = np.asarray(want, dtype=np.float64)
            have = np.asarray(got["obs"][key][w])
            assert have.shape == want.shape, key
            assert np.max(np.abs(have - want)) < tol * 10 * max(1.0, np.max(np.abs(want))), (key, w)
        assert abs(got["psi_mean"][w] / pm - 1) < tol * 10
        assert abs(got["psi_rel_err"][w] - prel) < tol * 10
        if model != "tfim":
            nz += np.count_nonzero(obs["SpSm_row"]) + np.count_nonzero(obs["SmSp_row"])
    assert model == "tfim" or nz > 0              # the off-diagonal channel of the middle row is exercised
