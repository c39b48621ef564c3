"""Sweeps/s of the Hubbard U(1) x U(1) sector updater (MCUpdateSquareNNHubbardU1U1OBC) on one GPU, device-side slices
(pepsgpu_sweep_slice_sector) against the per-bond hook path (PEPSHOST_NO_DEVICE_SWEEP=1) at equal walker counts:
  hubbard  8x8 fZ2-graded Hubbard state (up-down, up, down, empty), D = 6, chi = 24 (f32, f64), quarter of the sites each state
and, for scale, the nearest-neighbour exchange updater on the same state (device slices only, "nn_exchange").
The two paths run as alternating child processes (device, hook, device, hook, ...); the figure of a path is the median over its
children (statistics.median), reported with the spread (max / min - 1) of those children.  --parent-root names a checkout of the
parent commit with its libraries built: ONE child of that build runs the exchange updater (the sector updater does not exist there), so
that the file shows the two builds agree on the workload they share.  Prints one JSON line; no gate.

    python scripts/bench_sector_sweep.py [--walkers 128] [--reps 5] [--sweeps 1] [--parent-root DIR] [--out profiles/sector_sweep_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (("f32", "hubbard_u1u1"), ("f64", "hubbard_u1u1"), ("f64", "exchange"))


def child(root, dtype, updater, n, sweeps):
    sys.path.insert(0, root)
    import numpy as np
    from peps_amd import fermion, hostapi
    dt = 0 if dtype == "f32" else 1
    seeds = np.arange(n, dtype=np.uint64) + 7
    L = 8
    a, b = fermion.random_even_state(L, L, 6, seed=12), fermion.random_even_state(L, L, 6, seed=29)
    st = fermion.FermionState([[[ta[1], ta[0], tb[0], tb[1]] for ta, tb in zip(ra, rb)] for ra, rb in zip(a.tensors, b.tensors)],
                              a.par, [0, 1, 1, 0])
    cfgs = np.stack([np.random.default_rng(200 + k).permutation(np.repeat(np.arange(4), L * L // 4)).reshape(L, L) for k in range(n)])
    run = lambda c: hostapi.fermion_mc_sweeps(st, c, seeds, 24, sweeps, dt, updater=updater)[0]
    cfgs = run(cfgs)                                    # warm-up: context, kernels
    t0 = time.time()
    run(cfgs)
    return n * sweeps / (time.time() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sector_sweep_bench.json"))
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--child", nargs=3, metavar=("ROOT", "DTYPE", "UPDATER"))
    ap.add_argument("--timeout", type=float, default=600.0)
    a = ap.parse_args()
    if a.child:
        print(json.dumps({"sweeps_per_s": child(a.child[0], a.child[1], a.child[2], a.walkers, a.sweeps)}))
        return

    def run_child(root, dtype, updater, path):
        env = dict(os.environ)
        env.pop("PEPSHOST_NO_DEVICE_SWEEP", None)
        if path == "hook":
            env["PEPSHOST_NO_DEVICE_SWEEP"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, dtype, updater, "--walkers", str(a.walkers),
                            "--sweeps", str(a.sweeps)], env=env, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            raise SystemExit("child %s %s %s failed (%d): %s" % (dtype, updater, path, r.returncode, r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])["sweeps_per_s"]

    res = {"metric": "walker sweeps/s, device slice vs hook path", "walkers": a.walkers, "reps": a.reps, "sweeps": a.sweeps}
    for dtype, updater in CASES:
        paths = ("device", "hook") if updater == "hubbard_u1u1" else ("device",)
        figs = {p: [] for p in paths}
        for _ in range(a.reps):
            for path in paths:
                figs[path].append(run_child(ROOT, dtype, updater, path))
        med = {p: statistics.median(v) for p, v in figs.items()}
        key = "hubbard_%s%s" % (dtype, "" if updater == "hubbard_u1u1" else "_nn_exchange")
        res[key] = {p: round(med[p], 2) for p in paths}
        res[key].update({p + "_all": [round(x, 2) for x in figs[p]] for p in paths})
        res[key].update({p + "_spread": round(max(figs[p]) / min(figs[p]) - 1, 3) for p in paths})
        if "hook" in med:
            res[key]["speedup"] = round(med["device"] / med["hook"], 2)
        print(key, res[key], file=sys.stderr, flush=True)
    if a.parent_root:
        res["hubbard_f64_nn_exchange_parent_build"] = round(run_child(os.path.abspath(a.parent_root), "f64", "exchange", "device"), 2)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
