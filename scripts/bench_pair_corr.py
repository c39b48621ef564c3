"""The singlet-pair correlation SC_singlet_pair_corr of the t-J measurement solver (SingletPairCorrelationMixin: per reference bond
pepsgpu_walker_set_mpo_excited_pair + one pepsgpu_walker_pair_trace_slice per walker and target row) against its per-call hook path
(PEPSHOST_NO_DEVICE_SWEEP=1, which also turns every other device slice of the measurement off) on one GPU: hostapi.fermion_observables
samples/s at 8x8, D = 4, chi = 16 of a t-J-like state (the occupied component of the spinless generator twice, differently weighted),
SquaretJVModel(1, 0, 0.4, 0.1, 0.3), f32 and f64, with the correlation off, with ONE selected reference bond and with ALL reference
bonds.  The configurations hold 20 holes of 64 sites, so that (empty, empty) reference bonds occur.

The two paths run as alternating child processes (slice, hook, slice, hook, ...), each under its own time limit; the first failure ends
the run.  Per path and leg: every value, the median and (max - min) / median; cost_s_per_sample = 1 / on - 1 / off is the correlation's
own cost.  Both are paths of THIS build -- the correlation is a capability the parent commit does not have, the hook path is the only
baseline there is -- and no ratio is fixed in advance.

    python scripts/bench_pair_corr.py [--reps 3] [--calls 1] [--walkers 64] [--out profiles/pair_corr_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, D, CHI = 8, 4, 16
CASES = ("f32", "f64")
PRM = (1.0, 0.4, 0.1, 0.3, 0.0)
ONE_BOND = ((3, 3),)
LEGS = (("off", None), ("one", ONE_BOND), ("all", ()))


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
    out = {}
    for leg, bonds in LEGS:
        kw = {} if bonds is None else {"sc_pair_corr": True, "ref_bonds": bonds}
        run = lambda: hostapi.fermion_observables(st, cfgs, CHI, "tj", PRM, dtype=dt, **kw)
        obs, _ = run()                                  # warm-up: context, kernels
        assert ("SC_singlet_pair_corr" in obs) == (bonds is not None)
        t0 = time.time()
        for _ in range(calls):
            obs, _ = run()
        out[leg + "_samples_per_s"] = n * calls / (time.time() - t0)
        if bonds is not None:
            v = obs["SC_singlet_pair_corr"]
            out[leg + "_values"] = int(v.shape[1])
            out[leg + "_nonzero"] = int(np.count_nonzero(v))
            out[leg + "_abs_sum"] = float(np.sum(np.abs(v)))
    out["pair_trace_slice_calls"] = capi.diag_walker_pair_slice_calls()
    return out


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
    f = json.loads(r.stdout.strip().splitlines()[-1])
    for leg in ("one", "all"):
        f[leg + "_cost_s_per_sample"] = 1.0 / f[leg + "_samples_per_s"] - 1.0 / f["off_samples_per_s"]
    return f


def summary(figs, key, digits):
    v = sorted(f[key] for f in figs)
    return {"median": round(v[len(v) // 2], digits), "spread": round((v[-1] - v[0]) / abs(v[len(v) // 2]), 3),
            "all": [round(f[key], digits) for f in figs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--cases", default="", help="comma list of f32 / f64 (default: both)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_corr_bench.json"))
    ap.add_argument("--child", nargs=3, metavar=("ROOT", "DTYPE", "WALKERS"))
    ap.add_argument("--timeout", type=float, default=300.0)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child[0], a.child[1], int(a.child[2]), a.calls)))
        return
    cases = tuple(a.cases.split(",")) if a.cases else CASES
    res = {"metric": "samples/s of fermion_observables (C++ host layer, SquaretJVModel registry) with SC_singlet_pair_corr off, with one "
                     "selected reference bond and with all reference bonds; cost_s_per_sample = 1 / on - 1 / off; slice = "
                     "pepsgpu_walker_set_mpo_excited_pair + pepsgpu_walker_pair_trace_slice, hook = PEPSHOST_NO_DEVICE_SWEEP=1 (every "
                     "device slice off) of the same build",
           "shape": {"L": L, "D": D, "chi": CHI, "walkers": a.walkers, "one_bond": list(ONE_BOND[0])}, "reps": a.reps, "calls": a.calls}
    for dtype in cases:
        figs = {"slice": [], "hook": []}
        for _ in range(a.reps):
            for path in ("slice", "hook"):
                figs[path].append(run_child(dtype, a.walkers, a.calls, path == "hook", a.timeout))
        assert all(f["pair_trace_slice_calls"] == 0 for f in figs["hook"]) and all(f["pair_trace_slice_calls"] > 0 for f in figs["slice"])
        entry = {}
        for key, digits in (("off_samples_per_s", 2), ("one_samples_per_s", 2), ("all_samples_per_s", 2), ("one_cost_s_per_sample", 6),
                            ("all_cost_s_per_sample", 6)):
            entry[key] = {path: summary(figs[path], key, digits) for path in figs}
        for leg in ("one", "all"):
            entry[leg + "_values"] = figs["slice"][0][leg + "_values"]
            entry[leg + "_nonzero"] = figs["slice"][0][leg + "_nonzero"]
            entry[leg + "_abs_sum_slice_minus_hook"] = figs["slice"][0][leg + "_abs_sum"] - figs["hook"][0][leg + "_abs_sum"]
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
