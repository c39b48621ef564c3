"""The diagonal-bond energy slice (pepsgpu_nnn_exchange_slice) against the per-plaquette hook path (PEPSHOST_NO_DEVICE_SWEEP=1) on one
GPU at equal walker counts, and its closing kernel against the accumulating-GEMM loop it replaces.

Throughput cases (E_loc samples/s of the energy pass without holes, and of the measurement pass):
  j1j2  10x10 J1-J2 XXZ, D = 6, chi = 24 (f32, f64; 256 and 2048 walkers)
  cj1j2 8x8 J1-J2 XXZ on a complex state, D = 4, chi = 16 (complex float64; 256 walkers)
  tri   10x10 triangular Heisenberg, D = 6, chi = 24 (f32; 256 and 2048 walkers)
The two paths run as alternating child processes (device, hook, device, hook, ...); the figure of a path is the median over its
children, every value and the spread (max - min over the median) are kept.

Closure (--closure, needs rocprofv3 on the PATH): for the shapes 24 x 6 x 6 x 24 and 32 x 8 x 8 x 32 of a 6 x 6 lattice's middle
row pair, us per launch of trace_dot4_kernel (one entry per walker x diagonal) and of the finish_dot4 loop of one
pepsgpu_replace_nnn_trace call (D accumulating tensor-GEMM launches per diagonal), each from ONE `rocprofv3 --kernel-trace --stats`
run of a child process (no counters in that run), the kernel's achieved GB/s (2 n sizeof(T) bytes per entry over its time) and the
kernel launches per plaquette of both paths, counted in the traces.

    python scripts/bench_nnn_slice.py [--reps 3] [--calls 2] [--cases j1j2:f32:256,...] [--closure] [--out profiles/nnn_slice_bench.json]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (("j1j2", "f32", 256), ("j1j2", "f32", 2048), ("j1j2", "f64", 256), ("j1j2", "f64", 2048), ("cj1j2", "c128", 256),
         ("tri", "f32", 256), ("tri", "f32", 2048))
J1J2 = (1.0, 1.0, 0.5, 0.5, 0.0)
CLOSURE_SHAPES = ((6, 24), (8, 32))                     # (D, chi): the closure's operands are chi x D x D x chi
CLOSURE_WALKERS = 256


def child(workload, dtype, n, calls):
    sys.path.insert(0, ROOT)
    import numpy as np
    from peps_amd import capi, hostapi, synthetic
    dt = 0 if dtype == "f32" else 1
    L, D, chi = (8, 4, 16) if workload == "cj1j2" else (10, 6, 24)
    flat = synthetic.sitps_to_flat(synthetic.make_sitps(L, D), D)
    cfgs = synthetic.make_configs(L, n, "heisenberg")
    model, prm = ("triangle", ()) if workload == "tri" else ("j1j2", J1J2)
    if workload == "cj1j2":
        flat = flat * np.exp(2j * np.pi * np.random.default_rng(3).uniform(size=flat.shape))
        energy = lambda: hostapi.energy_and_holes_complex(flat, cfgs, chi, model, prm, False)
        measure = lambda: hostapi.measure(flat, cfgs, chi, model, prm)
    else:
        energy = lambda: hostapi.energy_and_holes(flat, cfgs, chi, model, prm, False, dt)
        measure = lambda: hostapi.measure(flat, cfgs, chi, model, prm, dtype=dt)
    out = {}
    for name, run in (("energy", energy), ("measure", measure)):
        run()                                           # warm-up: context, kernels
        t0 = time.time()
        for _ in range(calls):
            run()
        out[name + "_samples_per_s"] = n * calls / (time.time() - t0)
    out["nnn_slice_calls"] = capi.diag_nnn_slice_calls()
    return out


def closure_child(kind, D, chi, dtype):
    """the program one rocprofv3 run traces: `dot4` = trace_dot4_kernel alone on operands of the shape; `loop` = the per-plaquette
    calls of the middle row pair of a 6 x 6 lattice (their finish_dot4 loops are read out of the trace); `slice` = the slice of it"""
    sys.path.insert(0, ROOT)
    import numpy as np
    from peps_amd import capi, synthetic
    np_t = {"f32": np.float32, "f64": np.float64}[dtype]
    n = CLOSURE_WALKERS
    if kind == "dot4":
        rng = np.random.default_rng(0)
        a = rng.normal(size=(2 * n, chi, D, D, chi)).astype(np_t)
        b = rng.normal(size=(2 * n, chi, D, D, chi)).astype(np_t)
        for _ in range(5):
            capi.diag_dot4(a, b, np.zeros(2 * n))
        return
    L, row = 6, 2
    flat = synthetic.sitps_to_flat(synthetic.make_sitps(L, D), D)
    cfgs = np.repeat(np.arange(L)[None, :, None] % 2, L, axis=2)          # row stripes: the ends of every diagonal differ
    cfgs = np.repeat(cfgs, n, axis=0).astype(np.int32)
    ctx = capi.Context(L, L, D, 2, chi, dtype=capi.F32 if dtype == "f32" else capi.F64, max_walkers=n)
    ctx.state_upload(flat)
    ctx.set_configs(cfgs)
    ctx.generate_bmps_approach(capi.UP)
    for _ in range(row):
        ctx.shift_bmps_window(capi.DOWN)
    for _ in range(2):                                                      # (the first pass warms up)
        if kind == "slice":
            ctx.nnn_exchange_slice(row, 3)
            continue
        ctx.init_bten2(capi.LEFT, row)
        ctx.grow_full_bten2(capi.RIGHT, row, 2, True)
        for col in range(L - 1):
            for d in (capi.LEFTUP_TO_RIGHTDOWN, capi.LEFTDOWN_TO_RIGHTUP):
                ends = ((row, col), (row + 1, col + 1)) if d == capi.LEFTUP_TO_RIGHTDOWN else ((row + 1, col), (row, col + 1))
                cand = np.stack([cfgs[:, ends[1][0], ends[1][1]], cfgs[:, ends[0][0], ends[0][1]]], axis=-1)[:, None, :]
                ctx.replace_nnn_trace(row, col, d, capi.HORIZONTAL, cand)
            ctx.shift_bten2_window(capi.RIGHT, row)
    ctx.close()


def _trace(kind, D, chi, dtype, timeout):
    """one rocprofv3 --kernel-trace --stats run of closure_child; returns the kernel dispatches [(name, ns)] in start order"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "kt", "--", sys.executable,
               os.path.abspath(__file__), "--closure-child", kind, str(D), str(chi), dtype]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            raise SystemExit("rocprofv3 run %s failed (%d): %s" % (kind, r.returncode, (r.stderr or r.stdout)[-2000:]))
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise SystemExit("rocprofv3 wrote no kernel trace for %s" % kind)
        rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    return [(x["Kernel_Name"], int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) for x in rows]


def closure(timeout):
    out = {}
    for D, chi in CLOSURE_SHAPES:
        for dtype in ("f32", "f64"):
            size = 4 if dtype == "f32" else 8
            elems = chi * D * D * chi
            dot = [ns for name, ns in _trace("dot4", D, chi, dtype, timeout) if "trace_dot4_kernel" in name][1:]     # (drop the first launch)
            # the per-plaquette calls: every pepsgpu_replace_nnn_trace ends  ... add_logs_kernel, D accumulating GEMM launches; the second
            # pass, the interior plaquettes (columns 1 .. 3: both operands chi x D x D x chi)
            loop_tr = _trace("loop", D, chi, dtype, timeout)
            marks = [i for i, (name, _) in enumerate(loop_tr) if "add_logs_kernel" in name]
            calls = marks[-10:]                                               # second pass: the last 2 (L - 1) calls of the child
            if len(calls) != 10 or not all("tgemm" in name for i in calls for name, _ in loop_tr[i + 1:i + 1 + D]):
                raise SystemExit("closure: the trace of the per-plaquette calls does not end in 10 x (add_logs_kernel, %d tensor GEMMs)" % D)
            loops = [sum(ns for _, ns in loop_tr[i + 1:i + 1 + D]) for i in calls]
            interior = [loops[2 * col + k] for col in (1, 2, 3) for k in (0, 1)]
            slice_tr = _trace("slice", D, chi, dtype, timeout)
            sd = [i for i, (name, _) in enumerate(slice_tr) if "trace_dot4_kernel" in name]
            if len(sd) < 5:
                raise SystemExit("closure: the trace of the slice holds fewer than 5 trace_dot4_kernel launches")
            sd = sd[-5:]                                                      # second pass: one closure per plaquette
            # the launches of one interior plaquette, window shift included: from one closure to the next (slice), over the two calls
            # of a plaquette (hook)
            count = lambda tr: {"kernels": len(tr), "tensor_gemms": sum("tgemm" in name for name, _ in tr)}
            launches = {"slice": count(slice_tr[sd[1]:sd[2]]), "hook": count(loop_tr[calls[2]:calls[4]])}
            dot_us = sorted(dot)[len(dot) // 2] / 1e3
            loop_us = sorted(interior)[len(interior) // 2] / 1e3
            # (the slice closes BOTH diagonals of a plaquette with one launch of 2 x walkers entries; the hook path runs one loop of
            # walkers entries per diagonal)
            out["%dx%dx%dx%d_%s" % (chi, D, D, chi, dtype)] = {
                "walkers": CLOSURE_WALKERS,
                "dot4_us_per_launch_2_diagonals": round(dot_us, 2), "dot4_all_us": [round(x / 1e3, 2) for x in dot],
                "finish_dot4_loop_us_per_diagonal": round(loop_us, 2), "finish_dot4_loop_us_2_diagonals": round(2 * loop_us, 2),
                "finish_dot4_loop_all_us": [round(x / 1e3, 2) for x in interior],
                "dot4_GBps": round(2.0 * elems * size * 2 * CLOSURE_WALKERS / (dot_us * 1e-6) / 1e9, 1),
                "launches_per_plaquette": launches}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--cases", default="", help="comma list of workload:dtype:walkers (default: all)")
    ap.add_argument("--closure", action="store_true", help="also time the closure kernel against the finish_dot4 loop (rocprofv3)")
    ap.add_argument("--no-throughput", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nnn_slice_bench.json"))
    ap.add_argument("--child", nargs=3, metavar=("WORKLOAD", "DTYPE", "WALKERS"))
    ap.add_argument("--closure-child", nargs=4, metavar=("KIND", "D", "CHI", "DTYPE"))
    ap.add_argument("--timeout", type=float, default=900.0)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child[0], a.child[1], int(a.child[2]), a.calls)))
        return
    if a.closure_child:
        closure_child(a.closure_child[0], int(a.closure_child[1]), int(a.closure_child[2]), a.closure_child[3])
        return
    cases = CASES
    if a.cases:
        cases = tuple((w, d, int(n)) for w, d, n in (c.split(":") for c in a.cases.split(",")))
    res = {"metric": "E_loc samples/s of the energy pass (no holes) and of the measurement pass, device slices vs hook path",
           "reps": a.reps, "calls": a.calls}
    for workload, dtype, n in ([] if a.no_throughput else cases):
        figs = {"device": [], "hook": []}
        for _ in range(a.reps):
            for path in ("device", "hook"):
                env = dict(os.environ)
                env.pop("PEPSHOST_NO_DEVICE_SWEEP", None)
                if path == "hook":
                    env["PEPSHOST_NO_DEVICE_SWEEP"] = "1"
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", workload, dtype, str(n), "--calls", str(a.calls)],
                                   env=env, capture_output=True, text=True, timeout=a.timeout)
                if r.returncode != 0:
                    raise SystemExit("child %s %s %d %s failed (%d): %s" % (workload, dtype, n, path, r.returncode, r.stderr[-2000:]))
                figs[path].append(json.loads(r.stdout.strip().splitlines()[-1]))
        assert all(f["nnn_slice_calls"] == 0 for f in figs["hook"]) and all(f["nnn_slice_calls"] > 0 for f in figs["device"])
        entry = {}
        for leg in ("energy", "measure"):
            med, spread, every = {}, {}, {}
            for path in ("device", "hook"):
                v = sorted(f[leg + "_samples_per_s"] for f in figs[path])
                med[path], spread[path] = v[len(v) // 2], (v[-1] - v[0]) / v[len(v) // 2]
                every[path] = [round(f[leg + "_samples_per_s"], 1) for f in figs[path]]
            entry[leg] = {"device": round(med["device"], 1), "hook": round(med["hook"], 1), "speedup": round(med["device"] / med["hook"], 2),
                          "device_spread": round(spread["device"], 3), "hook_spread": round(spread["hook"], 3),
                          "device_all": every["device"], "hook_all": every["hook"]}
        res["%s_%s_%d" % (workload, dtype, n)] = entry
        print("%s %s %d: %s" % (workload, dtype, n, json.dumps(entry)), file=sys.stderr, flush=True)
    if a.closure:
        res["closure"] = closure(a.timeout)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
