"""Are the wave slots full?  Per kernel and grid of a bench.py run: the mean number of resident waves per CU, from the SQ counters,
beside the most the kernel's registers, LDS and block size allow, from the compiler's resource report.

    python scripts/wave_slots_audit.py --trace DIR --pmc DIR --resources FILE [--min-ms 1.0] [--out FILE]

inputs, each of a run of its own (counters are never collected beside a tracing domain):
    --trace      output directory of `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --steps 2 --warmup 1`
    --pmc        output directory of `rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CU_CYCLES --output-format csv -d DIR -- python bench.py
                 --steps 2 --warmup 1`
    --resources  stderr of the library's hipcc line with `-Rpass-analysis=kernel-resource-usage` added

Reading of the counters (the assumptions of profiles/wave_slots_ab.md): SQ_WAVE_CYCLES counts quad-cycles summed over the waves,
SQ_BUSY_CU_CYCLES counts cycles summed over the CUs, so  resident = 4 * SQ_WAVE_CYCLES / SQ_BUSY_CU_CYCLES  is the mean number of
waves on a CU while it is busy.  `ghz_all_cus_busy` = SQ_BUSY_CU_CYCLES / (256 CUs * traced duration) is the check of that reading: it
comes out at the shader clock when every CU is busy for the whole launch, and below it when CUs stand idle (small grids, long tails).
Slots: waves per SIMD of the resource report * 4 SIMDs, in whole blocks, capped by 160 KB of LDS per CU.
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys

NCU = 256
LDS_PER_CU = 160 * 1024


def _grid(r):
    g = 1
    for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"):
        g *= int(r.get(k, 1) or 1)
    return g if "Grid_Size_X" in r else int(r.get("Grid_Size", 0) or 0)


def _wg(r):
    g = 1
    for k in ("Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z"):
        g *= int(r.get(k, 1) or 1)
    return g if "Workgroup_Size_X" in r else int(r.get("Workgroup_Size", 0) or 0)


def short_name(name):
    """`void ns::kernel<a, b>(args) [clone .kd]` -> `kernel<a, b>`"""
    s = name.strip()
    s = re.sub(r"\s*\[clone [^\]]*\]$", "", s)
    s = re.sub(r"\.kd$", "", s)
    if s.endswith(")"):                 # drop the argument list: the parenthesis that matches the last one
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            depth += (s[i] == ")") - (s[i] == "(")
            if depth == 0:
                s = s[:i]
                break
    s = re.sub(r"^void\s+", "", s)
    return re.sub(r"\bpepsgpu::", "", s).strip()


def read_trace(d):
    """(kernel, grid) -> dict(block, launches, us_median, us_mean, us_total)"""
    per = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            key = (short_name(r["Kernel_Name"]), _grid(r))
            per.setdefault(key, {"block": _wg(r), "us": []})["us"].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    for key, v in per.items():
        us = sorted(v["us"])
        out[key] = {"block": v["block"], "launches": len(us), "us_median": us[len(us) // 2], "us_mean": sum(us) / len(us), "us_total": sum(us)}
    return out


def read_pmc(d):
    """(kernel, grid) -> counter -> (sum, dispatches)"""
    per = {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            key = (short_name(r["Kernel_Name"]), _grid(r))
            c = per.setdefault(key, {}).setdefault(r["Counter_Name"], [0.0, 0])
            c[0] += float(r["Counter_Value"] or 0)
            c[1] += 1
    return per


def read_resources(path):
    """kernel -> dict(sgprs, vgprs, agprs, scratch, occupancy, lds) from the remarks of -Rpass-analysis=kernel-resource-usage"""
    fields = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
              "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds"}
    recs, cur = [], None
    for ln in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", ln)
        if m:
            cur = {"mangled": m.group(1)}
            recs.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (\d+) \[-Rpass-analysis", ln)
        if m and cur is not None and m.group(1) in fields:
            cur[fields[m.group(1)]] = int(m.group(2))
    names = [r["mangled"] for r in recs]
    tool = next((t for t in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt") if _which(t)), None)
    dem = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines() if tool and names else names
    return {short_name(n): r for n, r in zip(dem, recs)}


def _which(t):
    from shutil import which
    return os.path.exists(t) if os.path.isabs(t) else which(t) is not None


def slots_per_cu(res, block):
    """most waves of this kernel a CU holds: registers (occupancy of the report), whole blocks, LDS"""
    if not res or not res.get("occupancy") or not block:
        return None
    wpb = (block + 63) // 64
    blocks = (4 * res["occupancy"]) // wpb
    if res.get("lds"):
        blocks = min(blocks, LDS_PER_CU // res["lds"])
    return blocks * wpb


def audit(trace_dir, pmc_dir, resources, min_ms=1.0):
    tr, pm = read_trace(trace_dir), read_pmc(pmc_dir)
    rs = read_resources(resources) if resources else {}
    rows = []
    for key, t in tr.items():
        if t["us_total"] / 1e3 < min_ms:
            continue
        kern, grid = key
        c = pm.get(key, {})
        wave, busy = c.get("SQ_WAVE_CYCLES"), c.get("SQ_BUSY_CU_CYCLES")
        row = {"kernel": kern, "grid": grid, "block": t["block"], "launches": t["launches"], "us_median": t["us_median"],
               "us_mean": t["us_mean"], "ms_total": t["us_total"] / 1e3}
        res = rs.get(kern)
        if res:
            row.update({k: res.get(k, 0) for k in ("sgprs", "vgprs", "agprs", "scratch", "occupancy", "lds")})
        row["slots_per_cu"] = slots_per_cu(res, t["block"])
        if wave and busy and busy[0] > 0:
            row["SQ_WAVE_CYCLES_mean"] = wave[0] / wave[1]
            row["SQ_BUSY_CU_CYCLES_mean"] = busy[0] / busy[1]
            row["resident_waves_per_cu"] = 4.0 * wave[0] / busy[0]
            row["ghz_all_cus_busy"] = (busy[0] / busy[1]) / (NCU * t["us_mean"] * 1e3)
            if row["slots_per_cu"]:
                row["filled"] = row["resident_waves_per_cu"] / row["slots_per_cu"]
        rows.append(row)
    rows.sort(key=lambda r: -r["ms_total"])
    return rows


def table(rows):
    out = ["| kernel | grid | block | launches | median µs | ms in run | VGPRs | SGPRs | LDS | resident waves / CU | slots / CU | filled | GHz if all CUs busy |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    f = lambda v, p: "" if v is None else p % v   # noqa: E731
    for r in rows:
        out.append("| `%s` | %d | %d | %d | %.1f | %.1f | %s | %s | %s | %s | %s | %s | %s |" % (
            r["kernel"], r["grid"], r["block"], r["launches"], r["us_median"], r["ms_total"], f(r.get("vgprs"), "%d"), f(r.get("sgprs"), "%d"),
            f(r.get("lds"), "%d"), f(r.get("resident_waves_per_cu"), "%.1f"), f(r.get("slots_per_cu"), "%d"),
            f(None if r.get("filled") is None else 100 * r["filled"], "%.0f %%"), f(r.get("ghz_all_cus_busy"), "%.2f")))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", required=True)
    ap.add_argument("--pmc", required=True)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--min-ms", type=float, default=1.0, help="leave out (kernel, grid) pairs below this much time in the traced run")
    ap.add_argument("--out", default=None, help="JSON of the rows")
    a = ap.parse_args()
    rows = audit(a.trace, a.pmc, a.resources, a.min_ms)
    print(table(rows))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
