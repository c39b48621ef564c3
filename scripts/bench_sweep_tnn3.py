"""Sweeps/s of the three-site exchange updater (MCUpdateSquareTNN3SiteExchange) on one GPU, device-side slices
(pepsgpu_sweep_slice_tnn3) against the per-triple hook path (PEPSHOST_NO_DEVICE_SWEEP=1) at equal walker counts:
  C3      10x10 J1-J2 shape, D = 6, chi = 24 (f32, f64)
  tJ      8x8 t-J-like fZ2-graded state (up, down, hole), D = 6, chi = 24 (f64)
and, for scale, the nearest-neighbour exchange updater on C3 (device slices only, "nn_exchange").
The two paths run as alternating child processes (device, hook, device, hook, ...); the figure of a path is the median over its
children (statistics.median), reported with the spread (max / min - 1) of those children.  Prints one JSON line.

    python scripts/bench_sweep_tnn3.py [--walkers 128] [--reps 5] [--sweeps 1] [--out profiles/sweep_tnn3_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (("C3", "f32", "tnn3"), ("C3", "f64", "tnn3"), ("tJ", "f64", "tnn3"), ("C3", "f32", "exchange"))


def child(workload, dtype, updater, n, sweeps):
    sys.path.insert(0, ROOT)
    import numpy as np
    from peps_amd import fermion, hostapi, synthetic
    dt = 0 if dtype == "f32" else 1
    seeds = np.arange(n, dtype=np.uint64) + 7
    if workload == "tJ":
        L = 8
        base = fermion.random_even_state(L, L, 6, seed=12)
        rng = np.random.default_rng(4)
        st = fermion.FermionState([[[t[0], t[0] * rng.uniform(0.5, 1.5, size=t[0].shape), t[1]] for t in row] for row in base.tensors],
                                  base.par, [1, 1, 0])
        cfgs = np.stack([np.random.default_rng(200 + k).permutation(np.r_[np.zeros(28, dtype=int), np.ones(28, dtype=int),
                                                                          2 * np.ones(8, dtype=int)]).reshape(L, L) for k in range(n)])
        run = lambda c: hostapi.fermion_mc_sweeps(st, c, seeds, 24, sweeps, dt, updater=updater)[0]
    else:
        L = 10
        flat = synthetic.sitps_to_flat(synthetic.make_sitps(L, 6), 6)
        cfgs = synthetic.make_configs(L, n, "heisenberg")
        run = lambda c: hostapi.mc_sweeps(flat, c, seeds, 24, updater, sweeps, dt)[0]
    cfgs = run(cfgs)                                    # warm-up: context, kernels
    t0 = time.time()
    run(cfgs)
    return n * sweeps / (time.time() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_tnn3_bench.json"))
    ap.add_argument("--child", nargs=3, metavar=("WORKLOAD", "DTYPE", "UPDATER"))
    ap.add_argument("--timeout", type=float, default=600.0)
    a = ap.parse_args()
    if a.child:
        print(json.dumps({"sweeps_per_s": child(a.child[0], a.child[1], a.child[2], a.walkers, a.sweeps)}))
        return
    res = {"metric": "walker sweeps/s, device slice vs hook path", "walkers": a.walkers, "reps": a.reps, "sweeps": a.sweeps}
    for workload, dtype, updater in CASES:
        paths = ("device", "hook") if updater == "tnn3" else ("device",)
        figs = {p: [] for p in paths}
        for _ in range(a.reps):
            for path in paths:
                env = dict(os.environ)
                env.pop("PEPSHOST_NO_DEVICE_SWEEP", None)
                if path == "hook":
                    env["PEPSHOST_NO_DEVICE_SWEEP"] = "1"
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", workload, dtype, updater, "--walkers", str(a.walkers),
                                    "--sweeps", str(a.sweeps)], env=env, capture_output=True, text=True, timeout=a.timeout)
                if r.returncode != 0:
                    raise SystemExit("child %s %s %s %s failed (%d): %s" % (workload, dtype, updater, path, r.returncode, r.stderr[-2000:]))
                figs[path].append(json.loads(r.stdout.strip().splitlines()[-1])["sweeps_per_s"])
        med = {p: statistics.median(v) for p, v in figs.items()}
        key = "%s_%s%s" % (workload, dtype, "" if updater == "tnn3" else "_nn_exchange")
        res[key] = {p: round(med[p], 2) for p in paths}
        res[key].update({p + "_all": [round(x, 2) for x in figs[p]] for p in paths})
        res[key].update({p + "_spread": round(max(figs[p]) / min(figs[p]) - 1, 3) for p in paths})
        if "hook" in med:
            res[key]["speedup"] = round(med["device"] / med["hook"], 2)
        print(key, res[key], file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
