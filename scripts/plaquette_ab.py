#!/usr/bin/env python3
"""A/B of two builds of libpepsgpu.so on the two-row (BTen2) traces and the row-pair / column-pair slices: bit identity of every result and
identity of the launch pattern.

    python scripts/plaquette_ab.py --ref PATH/TO/OTHER/libpepsgpu.so [--ref-name TEXT] [--out profiles/plaquette_closure_ab.json] [--only SUBSTR]

For every case one fresh subprocess per library (PEPSGPU_LIB selects it) runs the calls of the case on input states made once and read
by both.  Between the two libraries the script asserts
  - every output array is equal as raw bytes,
  - the bten2_stack_size values (all four positions) after each call are equal,
  - launches and alg_flops are equal in every event-profile category.
Cases, 4 walkers each, f32 / f64 / c128 (see _cases): nnn_exchange_slice and nnn_hop_slice_fermion over every row pair with masks 3, 1
and 2 (the hop slice followed by the plain plaquette trace and Trace: the restored state), replace_nnn_trace (both orientations, both
diagonals, ncand 0 and 2), replace_sqrt5_trace (both orientations), replace_plaquette_trace between sets (0, 0) and (1, 1) under a slice
override, link_exchange_slice on the 4 x 5 state of the diagonal slice, HORIZONTAL over every row pair with masks 15, 12, 3, 8 and 4, then
VERTICAL over every column pair with masks 12, 8 and 4.  The hop lattices are 3 x 4 and 4 x 3 with the (D, chi)
tests/test_gpu_tj_nnn.py uses for three and for four rows.
The first failure ends the run.  A "speed" entry already in the output file is kept.

    python scripts/plaquette_ab.py --worker CASE_NAME --states DIR      (internal: one case on the library of PEPSGPU_LIB)
    python scripts/plaquette_ab.py --prep --states DIR                  (internal: the input states; also for a profiler run of a worker)
A case that differs: diff the ordered kernel lists of one worker under the two builds (scripts/absorb_ab.py --trace-list).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

NW = 4
DTYPES = ("f32", "f64", "c128")
HOP_SHAPES = {"3x4": (3, 4, 3, 9), "4x3": (4, 3, 4, 16)}          # rows, cols, D, chi


def _cases():
    """name -> (family, state file stem, parameters)"""
    c = {}
    for dt in DTYPES:
        c["nnn_slice_4x5_" + dt] = ("slice", "rect", dt)
        c["link_slice_4x5_" + dt] = ("link", "rect", dt)
        for kind in ("spinless", "tj"):
            for shape in HOP_SHAPES:
                c["hop_slice_%s_%s_%s" % (kind, shape, dt)] = ("hop", "%s_%s" % (kind, shape), dt)
        c["nnn_sqrt5_traces_" + dt] = ("traces", "square", dt)
        c["plaquette_sets_" + dt] = ("sets", "square", dt)
    return c


CASES = _cases()


def _phases(x, seed=3):
    return x * np.exp(2j * np.pi * np.random.default_rng(seed).uniform(size=x.shape))


def prep(d):
    """The input states and configurations, made once so that both builds read the same bytes ("_c": with a phase per element)."""
    import nnn_slice_ref
    import tj_nnn_ref
    from peps_amd import fermion, synthetic
    rect = nnn_slice_ref.rect_state(4, 5, 3)
    np.save(os.path.join(d, "rect.npy"), rect)
    np.save(os.path.join(d, "rect_c.npy"), _phases(rect))
    np.save(os.path.join(d, "rect_cfg.npy"), nnn_slice_ref.walkers(4, 5)[1:1 + NW])
    sq = synthetic.sitps_to_flat(synthetic.make_sitps(5, 3), 3, np.float64)
    np.save(os.path.join(d, "square.npy"), sq)
    np.save(os.path.join(d, "square_c.npy"), _phases(sq))
    np.save(os.path.join(d, "square_cfg.npy"), synthetic.make_configs(5, NW, "heisenberg"))
    for kind in ("spinless", "tj"):
        for shape, (rows, cols, D, _) in HOP_SHAPES.items():
            st = tj_nnn_ref.tj_state(rows, cols, D) if kind == "tj" else fermion.random_even_state(rows, cols, D, seed=31)
            rng = np.random.default_rng(17)
            cfgs = rng.integers(0, st.d, size=(NW, rows, cols))
            empty, full = int(np.nonzero(st.nf == 0)[0][0]), int(np.nonzero(st.nf == 1)[0][0])
            for cf in cfgs:                                       # an even fermion number: the states are parity even
                if st.nf[cf].sum() % 2 == 1:
                    cf[0, 0] = empty if st.nf[cf[0, 0]] else full
            stem = os.path.join(d, "%s_%s" % (kind, shape))
            prng = np.random.default_rng(3)                        # a phase per element keeps the parity structure
            st_c = fermion.FermionState([[[a * np.exp(2j * np.pi * prng.uniform(size=a.shape)) for a in site] for site in r]
                                         for r in st.tensors], st.par, st.nf)
            np.save(stem + ".npy", st.extended_flat(st.D))
            np.save(stem + "_c.npy", st_c.extended_flat(st.D))
            np.save(stem + "_cfg.npy", st.ext_config(cfgs, fermion.ROW))
            np.save(stem + "_nf.npy", np.asarray(st.nf))


class _Log:
    """the outputs of a case in call order, with the BTen2 stack sizes after each call"""

    def __init__(self, ctx):
        self.ctx, self.out, self.sizes = ctx, [], []

    def add(self, label, *arrays):
        from peps_amd import capi
        self.out.append([label] + [np.ascontiguousarray(a).tobytes().hex() for a in arrays])
        self.sizes.append([self.ctx.bten2_stack_size(p) for p in (capi.LEFT, capi.DOWN, capi.RIGHT, capi.UP)])


def _run_slice(ctx, log, cfgs):
    from peps_amd import capi
    rows = cfgs.shape[1]
    ctx.generate_bmps_approach(capi.UP)
    for row in range(rows - 1):
        for mask in (3, 1, 2):
            log.add("row %d mask %d" % (row, mask), ctx.nnn_exchange_slice(row, mask))
        if row + 2 < rows:
            ctx.shift_bmps_window(capi.DOWN)


def _run_link(ctx, log, cfgs):
    from peps_amd import capi
    rows, cols = cfgs.shape[1:]
    passes = ((capi.HORIZONTAL, "row", rows, capi.UP, capi.DOWN, (15, 12, 3, 8, 4)), (capi.VERTICAL, "col", cols, capi.LEFT, capi.RIGHT, (12, 8, 4)))
    for orient, what, n, near, far, masks in passes:
        ctx.generate_bmps_approach(near)
        for s in range(n - 1):
            for mask in masks:
                log.add("%s %d mask %d" % (what, s, mask), ctx.link_exchange_slice(orient, s, mask))
            if s + 2 < n:
                ctx.shift_bmps_window(far)


def _run_hop(ctx, log, cfgs, nf):
    from peps_amd import capi
    rows, cols = cfgs.shape[1:]
    ctx.generate_bmps_approach(capi.UP)
    for row in range(rows - 1):
        ctx.init_bten(capi.LEFT, row)
        ctx.grow_full_bten(capi.RIGHT, row, 1, True)
        for mask in (3, 1, 2):
            psi, val = ctx.nnn_hop_slice_fermion(row, nf % 2, mask)
            log.add("row %d mask %d" % (row, mask), psi, val)
            log.add("row %d mask %d restored" % (row, mask), ctx.replace_plaquette_trace(row, cols - 2, None, 0, 0),
                    ctx.trace(row, 0, capi.HORIZONTAL))
        if row + 2 < rows:
            ctx.shift_bmps_window(capi.DOWN)


def _run_traces(ctx, log, cfgs):
    from peps_amd import capi
    L, r0, c0 = cfgs.shape[1], 1, 1
    cand = np.random.default_rng(7).integers(0, 2, size=(NW, 2, 2))
    for orient, name in ((capi.HORIZONTAL, "hor"), (capi.VERTICAL, "ver")):
        hor = orient == capi.HORIZONTAL
        near, far, num = (capi.LEFT, capi.RIGHT, r0) if hor else (capi.UP, capi.DOWN, c0)
        (ctx.grow_bmps_for_row if hor else ctx.grow_bmps_for_col)(num)
        ctx.grow_full_bten2(near, num, L - (c0 if hor else r0), True)
        ctx.grow_full_bten2(far, num, (c0 if hor else r0) + 2, True)
        for d in (capi.LEFTUP_TO_RIGHTDOWN, capi.LEFTDOWN_TO_RIGHTUP):
            log.add("nnn %s dir %d ncand 0" % (name, d), ctx.replace_nnn_trace(r0, c0, d, orient))
            log.add("nnn %s dir %d ncand 2" % (name, d), ctx.replace_nnn_trace(r0, c0, d, orient, cand))
        ctx.grow_full_bten2(far, num, (c0 if hor else r0) + 3, True)          # the sqrt5 block needs the far BTen2 one site further out
        for d in (capi.LEFTUP_TO_RIGHTDOWN, capi.LEFTDOWN_TO_RIGHTUP):
            log.add("sqrt5 %s dir %d ncand 0" % (name, d), ctx.replace_sqrt5_trace(r0, c0, d, orient))
            log.add("sqrt5 %s dir %d ncand 2" % (name, d), ctx.replace_sqrt5_trace(r0, c0, d, orient, cand))


def _run_sets(ctx, log, cfgs):
    """the sequence of tests/test_gpu_parity.py::test_plaquette_trace_second_bten2_set_and_slice_override"""
    from peps_amd import capi
    L, row, col = cfgs.shape[1], 1, 2
    rng = np.random.default_rng(3)
    ctx.generate_bmps_approach(capi.UP)
    ctx.shift_bmps_window(capi.DOWN)

    def chains():
        ctx.init_bten2(capi.LEFT, row)
        for _ in range(col):
            ctx.grow_bten2_step(capi.LEFT, row)
    ctx.grow_full_bten2(capi.RIGHT, row, 2, True)
    chains()
    log.add("sets 0 0 own", ctx.replace_plaquette_trace(row, col, None, 0, 0))
    new = cfgs.copy()
    new[:, row, :] = rng.integers(0, 2, size=(NW, L))
    new[:, row + 1, :] = rng.integers(0, 2, size=(NW, L))
    cand = np.stack([new[:, row, col], new[:, row + 1, col], new[:, row + 1, col + 1], new[:, row, col + 1]], axis=-1)
    log.add("sets 0 0 replaced", ctx.replace_plaquette_trace(row, col, np.stack([cand, cand[::-1]], axis=1), 0, 0))
    ctx.bten2_select_set(1)
    ctx.cfg_override_slice(capi.HORIZONTAL, row, new[:, row, :])
    ctx.grow_full_bten2(capi.RIGHT, row, 2, True)
    ctx.cfg_override_slice(capi.HORIZONTAL, row + 1, new[:, row + 1, :])
    chains()
    log.add("sets 1 1 under the override, own", ctx.replace_plaquette_trace(row, col, None, 1, 1))
    log.add("sets 1 1 under the override, replaced", ctx.replace_plaquette_trace(row, col, cand[:, None, :], 1, 1))
    log.add("sets 0 0 under the override", ctx.replace_plaquette_trace(row, col, None, 0, 0))
    ctx.cfg_override_slice(capi.HORIZONTAL, 0, None)
    log.add("sets 1 1 replaced", ctx.replace_plaquette_trace(row, col, cand[:, None, :], 1, 1))
    ctx.bten2_select_set(0)
    log.add("sets 0 0 own again", ctx.replace_plaquette_trace(row, col, None, 0, 0))


def worker(name, d):
    from peps_amd import capi
    family, stem, dt = CASES[name]
    flat = np.load(os.path.join(d, stem + ("_c" if dt == "c128" else "") + ".npy"))
    cfgs = np.load(os.path.join(d, stem + "_cfg.npy"))
    rows, cols = cfgs.shape[1:]
    if family == "hop":
        D, chi = HOP_SHAPES[stem.split("_")[1]][2:]
    else:
        D, chi = (3, 7) if family in ("slice", "link") else (3, 27) if family == "sets" else (3, 9)
    ctx = capi.Context(rows, cols, D, flat.shape[2], chi, dtype={"f32": capi.F32, "f64": capi.F64, "c128": capi.C128}[dt], max_walkers=NW)
    ctx.state_upload(flat)
    ctx.set_configs(cfgs)
    ctx.profile_enable(True)
    log = _Log(ctx)
    if family == "slice":
        _run_slice(ctx, log, cfgs)
    elif family == "link":
        _run_link(ctx, log, cfgs)
    elif family == "hop":
        _run_hop(ctx, log, cfgs, np.load(os.path.join(d, stem + "_nf.npy")))
    elif family == "traces":
        _run_traces(ctx, log, cfgs)
    else:
        _run_sets(ctx, log, cfgs)
    prof = ctx.profile_read()
    flags = ctx.walker_flags()
    ctx.close()
    print("RESULT " + json.dumps({
        "lib": capi.LIB_PATH, "outputs": log.out, "bten2_sizes": log.sizes, "flags": int(np.count_nonzero(flags)),
        "profile": {k: {"launches": v["launches"], "alg_flops": v["alg_flops"]} for k, v in prof.items()}}))


def _run(args, env, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT, **env), timeout=timeout)
    if r.returncode != 0:
        raise SystemExit("plaquette_ab: %s failed (exit %d):\n%s\n%s" % (args, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", help="the other build of libpepsgpu.so")
    ap.add_argument("--ref-name", default="", help="what the other build is, for the record (default: its path)")
    ap.add_argument("--lib", default=os.path.join(ROOT, "peps_amd", "lib", "libpepsgpu.so"), help="this tree's build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plaquette_closure_ab.json"))
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    ap.add_argument("--timeout", type=int, default=120, help="seconds per subprocess")
    ap.add_argument("--worker")
    ap.add_argument("--prep", action="store_true")
    ap.add_argument("--states")
    a = ap.parse_args()
    if a.prep:
        return prep(a.states)
    if a.worker:
        return worker(a.worker, a.states)
    if not a.ref:
        ap.error("--ref is required")
    libs = {"ref": os.path.abspath(a.ref), "tree": os.path.abspath(a.lib)}
    report = {"libs": {"ref": a.ref_name or os.path.relpath(libs["ref"], ROOT), "tree": os.path.relpath(libs["tree"], ROOT)}, "cases": {},
              "all_equal": False}
    if os.path.exists(a.out):
        report.update({k: v for k, v in json.load(open(a.out)).items() if k == "speed"})
    with tempfile.TemporaryDirectory() as states:
        _run(["--prep", "--states", states], {"PEPSGPU_LIB": libs["tree"]}, a.timeout)
        for name in CASES:
            if a.only not in name:
                continue
            res = {}
            for which, lib in libs.items():
                out = _run(["--worker", name, "--states", states], {"PEPSGPU_LIB": lib}, a.timeout)
                res[which] = json.loads([l for l in out.split("\n") if l.startswith("RESULT ")][0][7:])
                assert res[which]["lib"] == lib, res[which]["lib"]
            r, t = res["ref"], res["tree"]
            differing = [x[0] for x, y in zip(t["outputs"], r["outputs"]) if x != y]
            checks = {"output_bytes_equal": r["outputs"] == t["outputs"], "bten2_stack_sizes_equal": r["bten2_sizes"] == t["bten2_sizes"],
                      "profile_launches_and_alg_flops_equal": r["profile"] == t["profile"]}
            report["cases"][name] = {"checks": checks, "calls": len(t["outputs"]), "walkers_flagged": t["flags"],
                                     "nonzero_output_bytes": sum(len(h.strip("0")) > 0 for x in t["outputs"] for h in x[1:]),
                                     "launches": {k: v["launches"] for k, v in t["profile"].items() if v["launches"]}}
            print("%-36s %s  %d calls" % (name, "EQUAL " if all(checks.values()) else "DIFFER", len(t["outputs"])), flush=True)
            if not all(checks.values()):
                report["cases"][name].update({"differing_calls": differing, "ref_profile": r["profile"], "tree_profile": t["profile"],
                                              "ref_sizes": r["bten2_sizes"], "tree_sizes": t["bten2_sizes"]})
                json.dump(report, open(a.out, "w"), indent=1)
                raise SystemExit("plaquette_ab: case %s differs: %s" % (name, json.dumps(checks)))
    report["all_equal"] = True
    json.dump(report, open(a.out, "w"), indent=1)
    print("plaquette_ab: %d cases, all equal -> %s" % (len(report["cases"]), a.out))


if __name__ == "__main__":
    main()
