#!/usr/bin/env python
"""Tail of one optimisation iteration at the C4 shape (12x12, D = 8, d = 2, float32 context), two ways:

  device  pepsgpu_opt_gradient_from_accumulators + pepsgpu_opt_step(Adam): gradient, moments and master parameters stay in HBM
  host    pepsgpu_grad_read + the same Adam update in NumPy on the padded arrays + pepsgpu_state_upload

Each variant runs in child processes of its own, the two alternating (device, host, device, ...); a child warms up, then times
`--reps` repetitions with a host clock around calls that end in a device synchronise.  Reported: the median over all repetitions
of all children of a variant, the spread (min, max, quartiles) and every single value.  No gate: a measurement only.

    python scripts/bench_opt_step.py [--children 3] [--reps 20] [--out profiles/opt_step_bench.json]

--case fermion: the same protocol for a fermionic state at the C5 shape (8x8, D = 6, d = 2: 8 decorated components per site), float32
and float64 contexts, written to profiles/opt_step_fermion_bench.json:

  device  pepsgpu_opt_gradient_from_accumulators (finish, fold and projection in one kernel) + pepsgpu_opt_step(Adam)
  host    pepsgpu_grad_read + NumPy finish + fermion.fold_gradient + NumPy Adam on the stored components + extended_flat +
          pepsgpu_state_upload -- the round trip a fermionic run makes without the decoration-aware optimizer
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
ADAM = (0.9, 0.999, 1e-8, 0.0)
LR = 0.02


def child(mode, reps, warmup):
    import numpy as np
    from peps_amd import capi
    rng = np.random.default_rng(0)
    shape = (ROWS, COLS, DP, D, D, D, D)
    mask = np.zeros(shape)
    for r in range(ROWS):
        for c in range(COLS):
            mask[r, c, :, :(1 if c == 0 else D), :(1 if r == ROWS - 1 else D), :(1 if c == COLS - 1 else D), :(1 if r == 0 else D)] = 1.0
    theta = rng.standard_normal(shape) * mask
    ctx = capi.Context(ROWS, COLS, D, DP, CHI, dtype=capi.F32, max_walkers=1)
    ctx.state_upload(theta)
    ctx.grad_reset()                       # the accumulators are resident (zeros: the kernels and copies move the same bytes)
    e_sum, w_sum = -3.0, 2.0
    times = []
    if mode == "device":
        ctx.opt_begin()
        for k in range(warmup + reps):
            ctx.sync()
            t0 = time.perf_counter()
            ctx.opt_gradient_from_accumulators(e_sum, w_sum)
            ctx.opt_step(2, LR, ADAM)      # ends in a stream synchronise
            t1 = time.perf_counter()
            if k >= warmup:
                times.append(t1 - t0)
    else:
        m1, m2, t = np.zeros(shape), np.zeros(shape), 0
        for k in range(warmup + reps):
            ctx.sync()
            t0 = time.perf_counter()
            so, seo = ctx.grad_read()
            e = e_sum / w_sum
            g = (seo - e * so) / w_sum
            t += 1
            m1 = ADAM[0] * m1 + (1 - ADAM[0]) * g
            m2 = ADAM[1] * m2 + (1 - ADAM[1]) * g * g
            den = 1.0 / (np.sqrt(m2 / (1 - ADAM[1] ** t)) + ADAM[2])
            theta = theta - LR * den * (m1 / (1 - ADAM[0] ** t))
            ctx.state_upload(theta)        # ends in a stream synchronise
            t1 = time.perf_counter()
            if k >= warmup:
                times.append(t1 - t0)
    ctx.close()
    print("BENCH_OPT_STEP " + json.dumps({"mode": mode, "seconds": times}))


F_ROWS = F_COLS = 8
F_D, F_CHI = 6, 24


def child_fermion(mode, reps, warmup, dtype):
    import numpy as np
    from peps_amd import capi, fermion
    st = fermion.random_even_state(F_ROWS, F_COLS, F_D, seed=0)
    ctx = capi.Context(F_ROWS, F_COLS, F_D, 4 * st.d, F_CHI, dtype=capi.F32 if dtype == "f32" else capi.F64, max_walkers=1)
    ctx.state_upload(st.extended_flat())
    ctx.grad_reset()
    e_sum, w_sum = -3.0, 2.0
    times = []
    if mode == "device":
        ctx.fermion_decoration_set(st)
        ctx.opt_begin()
        for k in range(warmup + reps):
            ctx.sync()
            t0 = time.perf_counter()
            ctx.opt_gradient_from_accumulators(e_sum, w_sum)
            ctx.opt_step(2, LR, ADAM)
            t1 = time.perf_counter()
            if k >= warmup:
                times.append(t1 - t0)
    else:
        theta = np.zeros((F_ROWS, F_COLS, st.d) + (F_D,) * 4)
        for r in range(F_ROWS):
            for c in range(F_COLS):
                for q in range(st.d):
                    a = st.tensors[r][c][q]
                    theta[(r, c, q) + tuple(slice(0, n) for n in a.shape)] = a
        m1, m2, t = np.zeros(theta.shape), np.zeros(theta.shape), 0
        for k in range(warmup + reps):
            ctx.sync()
            t0 = time.perf_counter()
            so, seo = ctx.grad_read()
            e = e_sum / w_sum
            g = fermion.fold_gradient(st, (seo - e * so) / w_sum)
            t += 1
            m1 = ADAM[0] * m1 + (1 - ADAM[0]) * g
            m2 = ADAM[1] * m2 + (1 - ADAM[1]) * g * g
            den = 1.0 / (np.sqrt(m2 / (1 - ADAM[1] ** t)) + ADAM[2])
            theta = theta - LR * den * (m1 / (1 - ADAM[0] ** t))
            st = fermion.FermionState.from_stored(st, theta)
            ctx.state_upload(st.extended_flat())
            t1 = time.perf_counter()
            if k >= warmup:
                times.append(t1 - t0)
    ctx.close()
    print("BENCH_OPT_STEP " + json.dumps({"mode": mode, "dtype": dtype, "seconds": times}))


def run_children(a, extra):
    got = {"device": [], "host": []}
    per_child = {"device": [], "host": []}
    for k in range(a.children):
        for mode in ("device", "host"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--reps", str(a.reps), "--warmup", str(a.warmup)] + extra,
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:          # a child that failed ends the measurement: nothing more is started on the device
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit("child %s #%d failed with status %d" % (mode, k, r.returncode))
            line = [x for x in r.stdout.splitlines() if x.startswith("BENCH_OPT_STEP ")][-1]
            sec = json.loads(line[len("BENCH_OPT_STEP "):])["seconds"]
            got[mode] += sec
            per_child[mode].append(sec)
    return got, per_child


def main_fermion(a):
    out = {"metric": "one optimisation iteration's tail for a fermionic state at the C5 shape: finish + fold + Adam step, device-resident vs host round trip",
           "shape": {"rows": F_ROWS, "cols": F_COLS, "D": F_D, "d": 2, "phys_dim": 8, "padded_elements": F_ROWS * F_COLS * 8 * F_D ** 4},
           "protocol": {"children_per_variant": a.children, "reps_per_child": a.reps, "warmup_per_child": a.warmup, "order": "device, host alternating",
                        "clock": "time.perf_counter around calls that end in a stream synchronise", "accumulators": "zeros"}}
    for dtype in ("f32", "f64"):
        got, per_child = run_children(a, ["--case", "fermion", "--dtype", dtype])
        out[dtype] = {"device": summary(got["device"]), "host": summary(got["host"]),
                      "device_children_median_ms": [summary(x)["median_ms"] for x in per_child["device"]],
                      "host_children_median_ms": [summary(x)["median_ms"] for x in per_child["host"]]}
        out[dtype]["host_over_device_median"] = out[dtype]["host"]["median_ms"] / out[dtype]["device"]["median_ms"]
        print("%s: device median %.3f ms [%.3f, %.3f], host median %.3f ms [%.3f, %.3f]" % (
            dtype, out[dtype]["device"]["median_ms"], out[dtype]["device"]["min_ms"], out[dtype]["device"]["max_ms"],
            out[dtype]["host"]["median_ms"], out[dtype]["host"]["min_ms"], out[dtype]["host"]["max_ms"]))
    path = a.out or os.path.join(ROOT, "profiles", "opt_step_fermion_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f)
        f.write("\n")


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
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", choices=("boson", "fermion"), default="boson")
    ap.add_argument("--dtype", choices=("f32", "f64"), default="f32")
    a = ap.parse_args()
    if a.child:
        return child_fermion(a.child, a.reps, a.warmup, a.dtype) if a.case == "fermion" else child(a.child, a.reps, a.warmup)
    if a.case == "fermion":
        return main_fermion(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "opt_step_bench.json")
    got, per_child = run_children(a, [])
    elems = ROWS * COLS * DP * D ** 4
    out = {"metric": "one optimisation iteration's tail at the C4 shape: finish + Adam step, device-resident vs host round trip",
           "shape": {"rows": ROWS, "cols": COLS, "D": D, "phys_dim": DP, "dtype": "f32", "padded_elements": elems},
           "protocol": {"children_per_variant": a.children, "reps_per_child": a.reps, "warmup_per_child": a.warmup, "order": "device, host alternating",
                        "clock": "time.perf_counter around calls that end in a stream synchronise", "accumulators": "zeros"},
           "device": summary(got["device"]), "host": summary(got["host"]),
           "device_children_median_ms": [summary(x)["median_ms"] for x in per_child["device"]],
           "host_children_median_ms": [summary(x)["median_ms"] for x in per_child["host"]]}
    out["host_over_device_median"] = out["host"]["median_ms"] / out["device"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("device", "host")}))
    print("device median %.3f ms [%.3f, %.3f], host median %.3f ms [%.3f, %.3f]" % (
        out["device"]["median_ms"], out["device"]["min_ms"], out["device"]["max_ms"], out["host"]["median_ms"], out["host"]["min_ms"],
        out["host"]["max_ms"]))


if __name__ == "__main__":
    main()
