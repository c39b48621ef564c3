"""The pair slice of the fermionic measurement solvers (pepsgpu_nn_pair_slice_fermion) against the per-bond hook path
(PEPSHOST_NO_DEVICE_SWEEP=1) of the C++ host layer on one GPU: hostapi.fermion_observables samples/s at the C5-like shape (8x8, D = 6,
chi = 24) of a t-J-like state (the occupied component of the spinless generator twice, differently weighted), SquaretJVModel(1, 0, 0.4,
0.1, 0.3), 256 walkers, f32 and f64.

The two paths run as alternating child processes (slice, hook, slice, hook, ...), each under its own time limit; the first failure ends
the run.  Per path: every value, the median and (max - min) / median; `resolved` says whether every slice child is above every hook
child.  Both are paths of THIS build: the parent commit has no fermionic measurement to compare with.

    python scripts/bench_pair_slice.py [--reps 3] [--calls 2] [--walkers 256] [--out profiles/pair_slice_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, D, CHI = 8, 6, 24
CASES = ("f32", "f64")
PRM = (1.0, 0.4, 0.1, 0.3, 0.0)


def child(root, dtype, n, calls):
    sys.path.insert(0, root)
    import numpy as np
    from peps_amd import capi, fermion, hostapi
    dt = 0 if dtype == "f32" else 1
    st = fermion.random_even_state(L, L, D, seed=12)
    rng = np.random.default_rng(4)
    st = fermion.FermionState([[[t[0], t[0] * rng.uniform(0.5, 1.5, size=t[0].shape), t[1]] for t in row] for row in st.tensors], st.par,
                              [1, 1, 0])
    pool = np.r_[np.zeros(22, dtype=int), np.ones(22, dtype=int), 2 * np.ones(20, dtype=int)]
    cfgs = np.stack([np.random.default_rng(100 + k).permutation(pool).reshape(L, L) for k in range(n)])
    obs, _ = hostapi.fermion_observables(st, cfgs, CHI, "tj", PRM, dtype=dt)          # warm-up: context, kernels
    t0 = time.time()
    for _ in range(calls):
        obs, _ = hostapi.fermion_observables(st, cfgs, CHI, "tj", PRM, dtype=dt)
    return {"samples_per_s": n * calls / (time.time() - t0), "e_mean": float(np.mean(obs["energy"])),
            "sc_abs_mean": float(np.mean(np.abs(obs["SC_bond_singlet_h"]))), "pair_slice_calls": capi.diag_pair_slice_calls()}


def run_child(dtype, n, calls, hook, timeout):
    env = dict(os.environ)
    env.pop("PEPSHOST_NO_DEVICE_SWEEP", None)
    if hook:
        env["PEPSHOST_NO_DEVICE_SWEEP"] = "1"
    cmd = ["timeout", "-k", "10", str(int(timeout)), sys.executable, os.path.abspath(__file__), "--child", ROOT, dtype, str(n), "--calls",
           str(calls)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:                               # a fault, an abort or the time limit: nothing more is started
        raise SystemExit("child %s %s failed (%d): %s" % (dtype, "hook" if hook else "slice", r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def summary(figs, key):
    v = sorted(f[key] for f in figs)
    return {"median": round(v[len(v) // 2], 1), "spread": round((v[-1] - v[0]) / v[len(v) // 2], 3), "all": [round(f[key], 1) for f in figs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--walkers", type=int, default=256)
    ap.add_argument("--cases", default="", help="comma list of f32 / f64 (default: both)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_slice_bench.json"))
    ap.add_argument("--child", nargs=3, metavar=("ROOT", "DTYPE", "WALKERS"))
    ap.add_argument("--timeout", type=float, default=300.0)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child[0], a.child[1], int(a.child[2]), a.calls)))
        return
    cases = tuple(a.cases.split(",")) if a.cases else CASES
    res = {"metric": "samples/s of fermion_observables (C++ host layer, SquaretJVModel registry with SC_bond_singlet_h / _v): device pair "
                     "slice vs per-bond hook path of the same build",
           "shape": {"L": L, "D": D, "chi": CHI, "walkers": a.walkers}, "reps": a.reps, "calls": a.calls}
    for dtype in cases:
        figs = {"slice": [], "hook": []}
        for _ in range(a.reps):
            for path in ("slice", "hook"):
                figs[path].append(run_child(dtype, a.walkers, a.calls, path == "hook", a.timeout))
        assert all(f["pair_slice_calls"] == 0 for f in figs["hook"]) and all(f["pair_slice_calls"] > 0 for f in figs["slice"])
        entry = {path: summary(figs[path], "samples_per_s") for path in figs}
        entry["resolved"] = min(entry["slice"]["all"]) > max(entry["hook"]["all"])
        entry["speedup_of_medians"] = round(entry["slice"]["median"] / entry["hook"]["median"], 2)
        entry["e_mean_slice_minus_hook"] = figs["slice"][0]["e_mean"] - figs["hook"][0]["e_mean"]
        entry["sc_abs_mean_slice_minus_hook"] = figs["slice"][0]["sc_abs_mean"] - figs["hook"][0]["sc_abs_mean"]
        res["tj_%s" % dtype] = entry
        print("tj %s: %s" % (dtype, json.dumps(entry)), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
