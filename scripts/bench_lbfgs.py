#!/usr/bin/env python
"""Cost of the L-BFGS calls at the C4 shape (12x12, D = 8, d = 2, float32 context, history 10 full), and of one trial point of a
line search two ways:

  device  pepsgpu_lbfgs_trial (theta = theta_base + alpha d, device state = T(theta), one pass) + pepsgpu_lbfgs_slope (<g, d>)
  host    theta_base + alpha d in NumPy + pepsgpu_state_upload, then pepsgpu_opt_get_gradient + the dot in NumPy: the state upload and
          the gradient read-back a line search on the caller's side pays per trial

Neither variant includes the evaluation of the trial state (the same work in both).  The device children also time
pepsgpu_lbfgs_update (a pushed pair: fused difference pass + its two Gram rows) and pepsgpu_lbfgs_direction (dots with the 20 history
vectors, recursion on the host, combination, base copies).  Each variant runs in child processes of its own, the two alternating
(device, host, device, ...); a child warms up, then times `--reps` repetitions with a host clock around calls that end in a device
synchronise.  Reported: medians over all repetitions of all children, the spread and every single value.  No gate: a measurement only.

    python scripts/bench_lbfgs.py [--children 3] [--reps 20] [--out profiles/lbfgs_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS = COLS = 12
D, DP, CHI = 8, 2, 8
HISTORY = 10
ALPHA = 0.37


def child(mode, reps, warmup):
    import numpy as np
    from peps_amd import capi
    rng = np.random.default_rng(0)
    shape = (ROWS, COLS, DP, D, D, D, D)
    mask = np.zeros(shape)
    for r in range(ROWS):
        for c in range(COLS):
            mask[r, c, :, :(1 if c == 0 else D), :(1 if r == ROWS - 1 else D), :(1 if c == COLS - 1 else D), :(1 if r == 0 else D)] = 1.0
    h = (0.5 + rng.random(shape)) * mask                    # a diagonal quadratic: g = h (theta - t)
    t = rng.standard_normal(shape) * mask
    ctx = capi.Context(ROWS, COLS, D, DP, CHI, dtype=capi.F32, max_walkers=1)
    ctx.state_upload(rng.standard_normal(shape) * mask)
    ctx.opt_begin()
    times = {}

    def timed(name, k, fn):
        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        if k >= warmup:
            times.setdefault(name, []).append(t1 - t0)
        return out

    if mode == "device":
        ctx.lbfgs_begin(HISTORY)
        for k in range(warmup + max(reps, HISTORY + 1)):
            ctx.opt_set_gradient(h * (ctx.opt_read_state() - t))
            timed("update", k if k > HISTORY else -1, lambda: ctx.lbfgs_update())           # timed once the ring is full
            timed("direction", k if k > HISTORY else -1, lambda: ctx.lbfgs_direction())
            timed("trial_and_slope", k, lambda: (ctx.lbfgs_trial(ALPHA), ctx.lbfgs_slope()))
            ctx.lbfgs_commit()
        assert ctx.lbfgs_counters()["history"] == HISTORY
    else:
        theta_base = ctx.opt_read_state()
        d = -(h * (theta_base - t))
        ctx.opt_set_gradient(-d)
        for k in range(warmup + reps):
            def trial():
                ctx.state_upload(theta_base + ALPHA * d)
                g = ctx.opt_get_gradient()
                return float(np.sum(g * d))
            timed("trial_and_slope", k, trial)
    ctx.close()
    print("BENCH_LBFGS " + json.dumps({"mode": mode, "seconds": times}))


def summary(v):
    import numpy as np
    a = np.sort(np.asarray(v))
    return {"median_ms": 1e3 * float(np.median(a)), "min_ms": 1e3 * float(a[0]), "max_ms": 1e3 * float(a[-1]),
            "q25_ms": 1e3 * float(np.percentile(a, 25)), "q75_ms": 1e3 * float(np.percentile(a, 75)), "n": int(a.size),
            "all_ms": [1e3 * float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("device", "host"))
    ap.add_argument("--children", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbfgs_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.warmup)
    got = {"device": {}, "host": {}}
    per_child = {"device": [], "host": []}
    for k in range(a.children):
        for mode in ("device", "host"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:          # a child that failed ends the measurement: nothing more is started on the device
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit("child %s #%d failed with status %d" % (mode, k, r.returncode))
            line = [x for x in r.stdout.splitlines() if x.startswith("BENCH_LBFGS ")][-1]
            sec = json.loads(line[len("BENCH_LBFGS "):])["seconds"]
            for name, v in sec.items():
                got[mode].setdefault(name, []).extend(v)
            per_child[mode].append(summary(sec["trial_and_slope"])["median_ms"])
    out = {"metric": "L-BFGS at the C4 shape: history update, direction, and one trial point of a line search device-resident vs host round trip",
           "shape": {"rows": ROWS, "cols": COLS, "D": D, "phys_dim": DP, "dtype": "f32", "padded_elements": ROWS * COLS * DP * D ** 4,
                     "history_size": HISTORY},
           "protocol": {"children_per_variant": a.children, "reps_per_child": a.reps, "warmup_per_child": a.warmup, "order": "device, host alternating",
                        "clock": "time.perf_counter around calls that end in a stream synchronise",
                        "excluded": "the evaluation of the trial state (identical in both variants)"},
           "device": {name: summary(v) for name, v in got["device"].items()}, "host": {name: summary(v) for name, v in got["host"].items()},
           "device_children_trial_median_ms": per_child["device"], "host_children_trial_median_ms": per_child["host"]}
    out["host_over_device_trial_median"] = out["host"]["trial_and_slope"]["median_ms"] / out["device"]["trial_and_slope"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
    for mode in ("device", "host"):
        for name, s in out[mode].items():
            print("%s %s: median %.3f ms [%.3f, %.3f] n = %d" % (mode, name, s["median_ms"], s["min_ms"], s["max_ms"], s["n"]))
    print("children trial medians: device %s host %s" % (per_child["device"], per_child["host"]))


if __name__ == "__main__":
    main()
