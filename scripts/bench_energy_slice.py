"""E_loc samples/s of the energy pass on one GPU, device-side energy slices (pepsgpu_onsite_slice / pepsgpu_nn_exchange_slice_tab)
against the per-site / per-bond hook path (PEPSHOST_NO_DEVICE_SWEEP=1) at equal walker counts, for three workloads:
  C2    8x8 transverse-field Ising, D = 4, chi = 16 (f32, f64)
  cxxz  8x8 XXZ on a complex state, D = 4, chi = 16 (complex float64)
  C5    8x8 spinless t-V, fZ2-graded, D = 6, chi = 24 (f32, f64)
The two paths run as alternating child processes (device, hook, device, hook, ...); the figure of a path is the median over its
children.  Prints one JSON line.

    python scripts/bench_energy_slice.py [--walkers 256] [--reps 3] [--calls 2] [--out profiles/energy_slice_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (("C2", "f32"), ("C2", "f64"), ("cxxz", "c128"), ("C5", "f32"), ("C5", "f64"))


def child(workload, dtype, n, calls):
    sys.path.insert(0, ROOT)
    import numpy as np
    from peps_amd import fermion, hostapi, synthetic
    dt = 0 if dtype == "f32" else 1
    L = 8
    if workload == "C5":
        st = fermion.random_even_state(L, L, 6, seed=11)
        rng = np.random.default_rng(1)
        cfgs = np.stack([rng.permutation(np.r_[np.zeros(32, dtype=int), np.ones(32, dtype=int)]).reshape(L, L) for _ in range(n)])
        run = lambda: hostapi.fermion_energy(st, cfgs, 24, 1.0, 1.0, dt, "spinless")
    else:
        flat = synthetic.sitps_to_flat(synthetic.make_sitps(L, 4), 4)
        if workload == "C2":
            cfgs = synthetic.make_configs(L, n, "tfim")
            run = lambda: hostapi.energy_and_holes(flat, cfgs, 16, "tfim", (3.0,), False, dt)
        else:
            cflat = flat * np.exp(2j * np.pi * np.random.default_rng(3).uniform(size=flat.shape))
            cfgs = synthetic.make_configs(L, n, "heisenberg")
            run = lambda: hostapi.energy_and_holes_complex(cflat, cfgs, 16, "xxz", (1.0, 1.0, 0.0), False)
    run()                                               # warm-up: context, kernels
    t0 = time.time()
    for _ in range(calls):
        run()
    return n * calls / (time.time() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "energy_slice_bench.json"))
    ap.add_argument("--child", nargs=2, metavar=("WORKLOAD", "DTYPE"))
    ap.add_argument("--timeout", type=float, default=600.0)
    a = ap.parse_args()
    if a.child:
        print(json.dumps({"samples_per_s": child(a.child[0], a.child[1], a.walkers, a.calls)}))
        return
    res = {"metric": "E_loc samples/s (energy pass, no holes), device slice vs hook path", "walkers": a.walkers, "reps": a.reps,
           "calls": a.calls}
    for workload, dtype in CASES:
        figs = {"device": [], "hook": []}
        for _ in range(a.reps):
            for path in ("device", "hook"):
                env = dict(os.environ)
                env.pop("PEPSHOST_NO_DEVICE_SWEEP", None)
                if path == "hook":
                    env["PEPSHOST_NO_DEVICE_SWEEP"] = "1"
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", workload, dtype, "--walkers", str(a.walkers),
                                    "--calls", str(a.calls)], env=env, capture_output=True, text=True, timeout=a.timeout)
                if r.returncode != 0:
                    raise SystemExit("child %s %s %s failed (%d): %s" % (workload, dtype, path, r.returncode, r.stderr[-2000:]))
                figs[path].append(json.loads(r.stdout.strip().splitlines()[-1])["samples_per_s"])
        dev, hook = sorted(figs["device"])[len(figs["device"]) // 2], sorted(figs["hook"])[len(figs["hook"]) // 2]
        res["%s_%s" % (workload, dtype)] = {"device": round(dev, 1), "hook": round(hook, 1), "speedup": round(dev / hook, 2),
                                             "device_all": [round(x, 1) for x in figs["device"]],
                                             "hook_all": [round(x, 1) for x in figs["hook"]]}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
