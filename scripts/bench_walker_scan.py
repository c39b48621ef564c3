"""The structure-factor pass of the measurement (MeasureStructureFactor: pepsgpu_walker_set_mpo_excited + pepsgpu_walker_trace_slice,
one call per source site and target row) against its per-call body (PEPSHOST_NO_DEVICE_SWEEP=1: one trace and one growth step per
column, which also turns every other device slice of the measurement off) and against a build of the parent commit, on one GPU at
equal walker counts.

Throughput cases (host.measure samples/s of the XXZ model with the structure factor on, params[7] = 1, and off):
  8x8, D = 4, chi = 16 (f32, f64; 256 walkers)        10x10, D = 6, chi = 24 (f32; 256 walkers)
The pass's own cost per sample is the difference 1 / on - 1 / off.  The paths run as alternating child processes (device, hook,
device, hook, ...); the figure of a path is the median over its children, every value and the spread (max - min over the median) are
kept.  --parent-root DIR (a built checkout of the parent commit) adds one child of that build per case: the figure that counts is
the device path against it.  `device_above_all` says whether EVERY device child lies above EVERY hook and parent child; no ratio is
fixed in advance.

    python scripts/bench_walker_scan.py [--reps 3] [--calls 1] [--cases 8:4:16:f32:256,...] [--parent-root DIR]
                                        [--out profiles/walker_scan_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((8, 4, 16, "f32", 256), (8, 4, 16, "f64", 256), (10, 6, 24, "f32", 256))
XXZ = (1.0, 1.0, 0.0)


def child(root, L, D, chi, dtype, n, calls):
    sys.path.insert(0, root)
    from peps_amd import capi, hostapi, synthetic
    dt = 0 if dtype == "f32" else 1
    flat = synthetic.sitps_to_flat(synthetic.make_sitps(L, D), D)
    cfgs = synthetic.make_configs(L, n, "heisenberg")
    out = {}
    for name, params in (("off", XXZ), ("on", XXZ + (0.0, 0.0, 0.0, 0.0, 1.0))):
        run = lambda: hostapi.measure(flat, cfgs, chi, "xxz", params, dtype=dt)
        obs, _ = run()                                  # warm-up: context, kernels
        assert ("SpSm_cross" in obs) == (name == "on")
        t0 = time.time()
        for _ in range(calls):
            run()
        out[name + "_samples_per_s"] = n * calls / (time.time() - t0)
    counter = getattr(capi, "diag_walker_slice_calls", None)      # (the parent build has no walker slice)
    out["walker_slice_calls"] = counter() if counter else -1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--cases", default="", help="comma list of L:D:chi:dtype:walkers (default: all)")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit: one child of it per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walker_scan_bench.json"))
    ap.add_argument("--child", nargs=6, metavar=("ROOT", "L", "D", "CHI", "DTYPE", "WALKERS"))
    ap.add_argument("--timeout", type=float, default=900.0)
    a = ap.parse_args()
    if a.child:
        c = a.child
        print(json.dumps(child(c[0], int(c[1]), int(c[2]), int(c[3]), c[4], int(c[5]), a.calls)))
        return
    cases = CASES
    if a.cases:
        cases = tuple((int(L), int(D), int(chi), d, int(n)) for L, D, chi, d, n in (c.split(":") for c in a.cases.split(",")))
    res = {"metric": "host.measure samples/s (XXZ) with the structure factor on and off; pass_s_per_sample = 1 / on - 1 / off; "
                     "device = walker slices, hook = PEPSHOST_NO_DEVICE_SWEEP=1 (every device slice off), parent_build = the parent commit",
           "reps": a.reps, "calls": a.calls}

    def run_child(root, case, hook):
        env = dict(os.environ)
        env.pop("PEPSHOST_NO_DEVICE_SWEEP", None)
        if hook:
            env["PEPSHOST_NO_DEVICE_SWEEP"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root] + [str(x) for x in case] + ["--calls", str(a.calls)],
                           env=env, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            raise SystemExit("child %s (%s, hook=%s) failed (%d): %s" % (case, root, hook, r.returncode, r.stderr[-2000:]))
        f = json.loads(r.stdout.strip().splitlines()[-1])
        f["pass_s_per_sample"] = 1.0 / f["on_samples_per_s"] - 1.0 / f["off_samples_per_s"]
        return f

    for case in cases:
        figs = {"device": [], "hook": []}
        for _ in range(a.reps):
            for path in ("device", "hook"):
                figs[path].append(run_child(ROOT, case, path == "hook"))
        assert all(f["walker_slice_calls"] == 0 for f in figs["hook"]) and all(f["walker_slice_calls"] > 0 for f in figs["device"])
        parent = run_child(os.path.abspath(a.parent_root), case, False) if a.parent_root else None
        entry = {}
        for leg, digits in (("on_samples_per_s", 2), ("off_samples_per_s", 2), ("pass_s_per_sample", 6)):
            med, spread, every = {}, {}, {}
            for path in ("device", "hook"):
                v = sorted(f[leg] for f in figs[path])
                med[path], spread[path] = v[len(v) // 2], (v[-1] - v[0]) / v[len(v) // 2]
                every[path] = [round(f[leg], digits) for f in figs[path]]
            entry[leg] = {"device": round(med["device"], digits), "hook": round(med["hook"], digits),
                          "device_spread": round(spread["device"], 3), "hook_spread": round(spread["hook"], 3),
                          "device_all": every["device"], "hook_all": every["hook"]}
            if parent:
                entry[leg]["parent_build"] = round(parent[leg], digits)
            if leg == "on_samples_per_s":
                others = every["hook"] + ([entry[leg]["parent_build"]] if parent else [])
                entry[leg]["device_above_all"] = min(every["device"]) > max(others)
        res["%dx%d_D%d_chi%d_%s_%d" % (case[0], case[0], case[1], case[2], case[3], case[4])] = entry
        print("%s: %s" % (case, json.dumps(entry)), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
