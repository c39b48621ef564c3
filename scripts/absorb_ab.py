#!/usr/bin/env python3
"""A/B of two builds of libpepsgpu.so on the row absorption: bit identity of the results and identity of the launch pattern.

    python scripts/absorb_ab.py --ref PATH/TO/OTHER/libpepsgpu.so [--out profiles/absorb_split_ab.json] [--only SUBSTR]

For every case one fresh subprocess per library (PEPSGPU_LIB selects it) evaluates the amplitudes, contracts column 0 and
traces it, and reads stats() and the event profile.  Between the two libraries the script asserts
  - the amplitude arrays (row route and column trace) are equal as raw bytes,
  - stats(): absorptions, absorptions_redone, jacobi_launches, carry_live_max are equal,
  - launches and alg_flops are equal in every profile category.
Cases: the smallest at which each stage of the absorption still runs (see CASES).  The first failure ends the run.

    python scripts/absorb_ab.py --worker CASE_NAME --states DIR      (internal: one case on the library of PEPSGPU_LIB)
    python scripts/absorb_ab.py --prep --states DIR                  (internal: the input states; also for a profiler run of a worker)
    python scripts/absorb_ab.py --trace-list KERNEL_TRACE.csv        ordered (kernel, grid, block, LDS bytes) of a rocprofv3 --kernel-trace
                                                                     run of a worker, one per line: diff the lists of the two builds
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32, F64, C128 = 0, 1, 3
ENV_8x8_F32 = ["PEPSGPU_PIVOT_CHOL=0", "PEPSGPU_ROWS_QR=0", "PEPSGPU_NO_MIDROUTE=1", "PEPSGPU_NO_RANK_ADAPT=1", "PEPSGPU_PRECISE=0",
               "PEPSGPU_PRECISE=2", "PEPSGPU_ACC64=15", "PEPSGPU_FORCE_ROWS_CAP=16", "PEPSGPU_FORCE_SKIP_FALLBACK=1"]


def _cases():
    """name -> (state, L, D, chi, dtype, walkers, env)"""
    c = {}
    # the 4x4 D = 8 reference state with chi = 8: edge sites, the general kernels, the fused factor
    for dt, tag in ((F32, "f32"), (F64, "f64"), (C128, "c128")):
        c["real4x4_chi8_" + tag] = ("real4", 4, 8, 8, dt, 4, {})
    # the 8x8 tiling, D = 8, chi = 32, 4 walkers: two-level pivoted mid route, rows_qr, f64 pivot route, mgemm_dense, triangular carry
    for dt, tag in ((F32, "f32"), (F64, "f64")):
        c["real8x8_" + tag] = ("real8", 8, 8, 32, dt, 4, {})
    for kv in ENV_8x8_F32:
        k, v = kv.split("=")
        c["real8x8_f32_" + kv] = ("real8", 8, 8, 32, F32, 4, {k: v})
    c["real8x8_f64_PEPSGPU_F64_PIVOT=0"] = ("real8", 8, 8, 32, F64, 4, {"PEPSGPU_F64_PIVOT": "0"})
    # complex: random phases on the 8x8 tiling
    c["real8x8_c128"] = ("real8ph", 8, 8, 32, C128, 4, {})
    c["real8x8_c128_PEPSGPU_F64_PIVOT=0"] = ("real8ph", 8, 8, 32, C128, 4, {"PEPSGPU_F64_PIVOT": "0"})
    # the low-rank synthetic state: hints, skipped fallbacks, the fused norm
    c["lowrank8x8_f32_nw64"] = ("low8", 8, 8, 32, F32, 64, {})
    # full rank with D chi > 256 (static shapes beyond 256 columns)
    c["fullrank8x8_D8_chi36_f32"] = ("full8", 8, 8, 36, F32, 3, {})
    return c


CASES = _cases()


def _configs(state, L, n):
    from peps_amd import synthetic
    if state.startswith("real"):
        return synthetic.make_configs_near_neel(L, n, seed0=211)
    return synthetic.make_configs(L, n, "heisenberg", seed0=5)


def prep(states_dir):
    """The input states, made once (by the library of PEPSGPU_LIB) so that both builds read the same bytes."""
    from peps_amd import capi, hostapi, synthetic
    fixture = os.path.join(ROOT, "tests", "golden", "ref_fixtures", synthetic.REAL_FIXTURE)
    f4 = hostapi.load_sitps(fixture, 8)
    for name, L in (("real4", 4), ("real8", 8)):
        flat = synthetic.tile_flat_state(f4, L)
        ctx = capi.Context(L, L, 8, 2, 32, dtype=capi.F64, max_walkers=1)     # psi(checkerboard) = O(1)
        ctx.state_upload(flat)
        ctx.set_configs(synthetic.checkerboard(L)[None])
        psi = float(ctx.evaluate_amplitude()[0])
        ctx.close()
        flat = flat * abs(psi) ** (-1.0 / (L * L))
        np.save(os.path.join(states_dir, name + ".npy"), flat)
        if L == 8:
            np.save(os.path.join(states_dir, "real8ph.npy"), flat * np.exp(2j * np.pi * np.random.default_rng(5).uniform(size=flat.shape)))
    np.save(os.path.join(states_dir, "low8.npy"), synthetic.sitps_to_flat(synthetic.make_sitps(8, 8, noise=0.1), 8, np.float64))
    np.save(os.path.join(states_dir, "full8.npy"), synthetic.sitps_to_flat(synthetic.make_sitps(8, 8, noise=1.0), 8, np.float64))


def worker(name, states_dir):
    from peps_amd import capi
    state, L, D, chi, dt, n, _ = CASES[name]
    flat = np.load(os.path.join(states_dir, state + ".npy"))
    cfgs = _configs(state, L, n)
    ctx = capi.Context(L, L, D, 2, chi, dtype=dt, max_walkers=n)
    ctx.state_upload(flat)
    ctx.set_configs(cfgs)
    ctx.profile_enable(True)
    amp = ctx.evaluate_amplitude()
    ctx.grow_bmps_for_col(0)
    ctx.init_bten(capi.UP, 0)
    ctx.grow_full_bten(capi.DOWN, 0, 2, True)
    col = ctx.trace(0, 0, capi.VERTICAL)
    st = ctx.stats()
    prof = ctx.profile_read()
    flags = ctx.walker_flags()
    ctx.close()
    print("RESULT " + json.dumps({
        "lib": capi.LIB_PATH, "amp_bytes": np.ascontiguousarray(amp).tobytes().hex(), "col_bytes": np.ascontiguousarray(col).tobytes().hex(),
        "amp0": [float(np.real(amp[0])), float(np.imag(amp[0]))], "flags": int(np.count_nonzero(flags)),
        "stats": {k: st[k] for k in ("absorptions", "absorptions_redone", "jacobi_launches", "carry_live_max")},
        "profile": {k: {"launches": v["launches"], "alg_flops": v["alg_flops"]} for k, v in prof.items()}}))


def trace_list(path):
    import csv
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        print("%s grid=(%s,%s,%s) block=(%s,%s,%s) lds=%s" % (
            r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["Workgroup_Size_Y"],
            r["Workgroup_Size_Z"], r["LDS_Block_Size"]))


def _run(args, env, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT, **env), timeout=timeout)
    if r.returncode != 0:
        raise SystemExit("absorb_ab: %s failed (exit %d):\n%s\n%s" % (args, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", help="the other build of libpepsgpu.so")
    ap.add_argument("--lib", default=os.path.join(ROOT, "peps_amd", "lib", "libpepsgpu.so"), help="this tree's build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "absorb_split_ab.json"))
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per subprocess")
    ap.add_argument("--worker")
    ap.add_argument("--prep", action="store_true")
    ap.add_argument("--states")
    ap.add_argument("--trace-list")
    a = ap.parse_args()
    if a.trace_list:
        return trace_list(a.trace_list)
    if a.prep:
        return prep(a.states)
    if a.worker:
        return worker(a.worker, a.states)
    if not a.ref:
        ap.error("--ref is required")
    libs = {"ref": os.path.abspath(a.ref), "tree": os.path.abspath(a.lib)}
    report = {"libs": {k: os.path.relpath(v, ROOT) for k, v in libs.items()}, "cases": {}, "all_equal": False}
    with tempfile.TemporaryDirectory() as states:
        _run(["--prep", "--states", states], {"PEPSGPU_LIB": libs["tree"]}, a.timeout)
        for name, case in CASES.items():
            if a.only not in name:
                continue
            res = {}
            for which, lib in libs.items():
                out = _run(["--worker", name, "--states", states], dict(case[6], PEPSGPU_LIB=lib), a.timeout)
                res[which] = json.loads([l for l in out.split("\n") if l.startswith("RESULT ")][0][7:])
                assert res[which]["lib"] == lib, res[which]["lib"]
            r, t = res["ref"], res["tree"]
            checks = {"amplitude_bytes_equal": r["amp_bytes"] == t["amp_bytes"], "column_trace_bytes_equal": r["col_bytes"] == t["col_bytes"],
                      "stats_equal": r["stats"] == t["stats"], "profile_launches_and_alg_flops_equal": r["profile"] == t["profile"]}
            report["cases"][name] = {"checks": checks, "amp0": t["amp0"], "walkers_flagged": t["flags"], "stats": t["stats"],
                                     "launches": {k: v["launches"] for k, v in t["profile"].items()}}
            print("%-44s %s  %s" % (name, "EQUAL " if all(checks.values()) else "DIFFER", json.dumps(t["stats"])), flush=True)
            if not all(checks.values()):
                report["cases"][name]["ref"] = {"stats": r["stats"], "profile": r["profile"], "amp0": r["amp0"]}
                report["cases"][name]["tree_profile"] = t["profile"]
                json.dump(report, open(a.out, "w"), indent=1)
                raise SystemExit("absorb_ab: case %s differs: %s" % (name, json.dumps(checks)))
    report["all_equal"] = True
    json.dump(report, open(a.out, "w"), indent=1)
    print("absorb_ab: %d cases, all equal -> %s" % (len(report["cases"]), a.out))


if __name__ == "__main__":
    main()
