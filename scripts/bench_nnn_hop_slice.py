"""The fermionic diagonal-hop slice (pepsgpu_nnn_hop_slice_fermion) against the per-plaquette path (PEPSHOST_NO_DEVICE_SWEEP=1) of the
C++ host layer on one GPU: E_loc samples/s at the C5 shape (8x8, D = 6, chi = 24), 256 walkers, t2 = 0.7.

Cases:
  spinless  the synthetic spinless state (peps_amd.fermion.random_even_state), SquareSpinlessFermion(1, 0.7, 0.5)
  tj        a t-J-like state (the occupied component twice, differently weighted), SquaretJVModel(1, 0.7, 0.4, 0.1, 0.3)
each in f32 and f64.  The two paths run as alternating child processes (slice, hook, slice, hook, ...), each under its own time limit;
the first failure ends the run.  Per path: every value, the median and (max - min) / median; `resolved` says whether every slice child
is above every hook child.  The switch is process-wide: a hook child also runs the nearest-neighbour bonds through their hooks, so
the t2 = 0 figure of every child (same switch) is kept beside it; the diagonal pass alone costs 1 / rate(t2) - 1 / rate(0) per sample.

--parent-root DIR: a checkout of the parent commit with its libraries built; its default path (the per-plaquette calls) is run once per
spinless case.  The t-J case has no parent figure: the parent refuses t2 != 0 there.

    python scripts/bench_nnn_hop_slice.py [--reps 3] [--calls 2] [--walkers 256] [--parent-root DIR] [--out profiles/nnn_hop_slice_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, D, CHI = 8, 6, 24
CASES = (("spinless", "f32"), ("spinless", "f64"), ("tj", "f32"), ("tj", "f64"))


def child(root, model, dtype, n, calls):
    sys.path.insert(0, root)
    import numpy as np
    from peps_amd import capi, fermion, hostapi
    dt = 0 if dtype == "f32" else 1
    st = fermion.random_even_state(L, L, D, seed=12)
    rng = np.random.default_rng(4)
    if model == "tj":
        st = fermion.FermionState([[[t[0], t[0] * rng.uniform(0.5, 1.5, size=t[0].shape), t[1]] for t in row] for row in st.tensors],
                                  st.par, [1, 1, 0])
        pool = np.r_[np.zeros(22, dtype=int), np.ones(22, dtype=int), 2 * np.ones(20, dtype=int)]
        energy = lambda t2: hostapi.fermion_energy(st, cfgs, CHI, 1.0, 0.1, dt, "tj", 0.4, 0.3, t2)
    else:
        pool = np.r_[np.zeros(32, dtype=int), np.ones(32, dtype=int)]
        energy = lambda t2: hostapi.fermion_energy(st, cfgs, CHI, 1.0, 0.5, dt, "spinless", t2=t2)
    cfgs = np.stack([np.random.default_rng(100 + k).permutation(pool).reshape(L, L) for k in range(n)])
    out = {}
    for key, t2 in (("t2_0", 0.0), ("t2", 0.7)):
        _, en, _ = energy(t2)                           # warm-up: context, kernels
        t0 = time.time()
        for _ in range(calls):
            _, en, _ = energy(t2)
        out[key + "_samples_per_s"] = n * calls / (time.time() - t0)
        out[key + "_e_mean"] = float(np.mean(en))
    out["hop_slice_calls"] = capi.diag_nnn_hop_slice_calls() if hasattr(capi, "diag_nnn_hop_slice_calls") else 0
    return out


def run_child(root, model, dtype, n, calls, hook, timeout):
    env = dict(os.environ)
    env.pop("PEPSHOST_NO_DEVICE_SWEEP", None)
    env.pop("PEPSHOST_NNN_FRESH", None)
    if hook:
        env["PEPSHOST_NO_DEVICE_SWEEP"] = "1"
    cmd = ["timeout", "-k", "10", str(int(timeout)), sys.executable, os.path.abspath(__file__), "--child", root, model, dtype, str(n),
           "--calls", str(calls)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:                               # a fault, an abort or the time limit: nothing more is started
        raise SystemExit("child %s %s %s failed (%d): %s" % (model, dtype, "hook" if hook else "slice", r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def summary(figs, key):
    v = sorted(f[key] for f in figs)
    return {"median": round(v[len(v) // 2], 1), "spread": round((v[-1] - v[0]) / v[len(v) // 2], 3), "all": [round(f[key], 1) for f in figs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--walkers", type=int, default=256)
    ap.add_argument("--cases", default="", help="comma list of model:dtype (default: all)")
    ap.add_argument("--parent-root", default="", help="checkout of the parent commit with built libraries (spinless cases, one child each)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nnn_hop_slice_bench.json"))
    ap.add_argument("--child", nargs=4, metavar=("ROOT", "MODEL", "DTYPE", "WALKERS"))
    ap.add_argument("--timeout", type=float, default=300.0)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child[0], a.child[1], a.child[2], int(a.child[3]), a.calls)))
        return
    cases = tuple(tuple(c.split(":")) for c in a.cases.split(",")) if a.cases else CASES
    res = {"metric": "E_loc samples/s of fermion_energy (C++ host layer, no holes) at t2 = 0.7: device hop slice vs per-plaquette path",
           "shape": {"L": L, "D": D, "chi": CHI, "walkers": a.walkers}, "reps": a.reps, "calls": a.calls, "not_run": []}
    for model, dtype in cases:
        figs = {"slice": [], "hook": []}
        for _ in range(a.reps):
            for path in ("slice", "hook"):
                figs[path].append(run_child(ROOT, model, dtype, a.walkers, a.calls, path == "hook", a.timeout))
        assert all(f["hop_slice_calls"] == 0 for f in figs["hook"]) and all(f["hop_slice_calls"] > 0 for f in figs["slice"])
        entry = {path: {"t2": summary(figs[path], "t2_samples_per_s"), "t2_0": summary(figs[path], "t2_0_samples_per_s")} for path in figs}
        entry["resolved"] = min(entry["slice"]["t2"]["all"]) > max(entry["hook"]["t2"]["all"])
        entry["speedup_of_medians"] = round(entry["slice"]["t2"]["median"] / entry["hook"]["t2"]["median"], 2)
        entry["e_mean_slice_minus_hook"] = figs["slice"][0]["t2_e_mean"] - figs["hook"][0]["t2_e_mean"]
        if model == "spinless" and a.parent_root:
            p = run_child(os.path.abspath(a.parent_root), model, dtype, a.walkers, a.calls, False, a.timeout)
            entry["parent_default_path"] = {"t2": round(p["t2_samples_per_s"], 1), "t2_0": round(p["t2_0_samples_per_s"], 1)}
        elif model == "spinless":
            res["not_run"].append("parent build, %s %s" % (model, dtype))
        res["%s_%s" % (model, dtype)] = entry
        print("%s %s: %s" % (model, dtype, json.dumps(entry)), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
