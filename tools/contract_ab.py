#!/usr/bin/env python3
"""Exact vs contracted arithmetic (wspr_set_arithmetic) on the headline workload: speed, interleaved.

configs[2] (8 192 segments x 10 signals, -10..-28 dB, resident in HBM) decoded by ONE wspr_decode_batch_device() call per
step on one lane, the two modes alternating step by step (exact, contracted, exact, ...), after one untimed step of each.
This is a single-call rate, not bench.py's `value` (which keeps twelve batches in flight and always runs the exact mode).
Then the same decode once per mode under `rocprofv3 --kernel-trace --stats`: every kernel's time, the fused
instantiation (template argument `true`) beside its exact twin (`false`).

  python tools/contract_ab.py [--nseg 8192] [--steps 6] [--out-dir profiles]   -> contracted_ab.json, contracted_ab.txt
"""
import argparse
import collections
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def workload(nseg):
    import torch
    import bench
    torch.cuda.set_device(0)
    I, Q, _ = bench.synth_batch_gpu(nseg, 20261016, torch.device("cuda", 0), 10, -10.0, -28.0, 0.3)
    return torch, I.contiguous(), Q.contiguous()


def run_steps(nseg, steps, modes):
    import rtlsdr_wsprd_amd as w
    torch, I, Q = workload(nseg)
    dec = w.BatchDecoder(nseg, max_results=16)
    w.sync_torch()
    times = collections.defaultdict(list)
    spots = {}
    for m in modes:                                         # untimed: first touch, clocks
        w.wspr_set_arithmetic(m)
        dec.decode_ptr(I.data_ptr(), Q.data_ptr(), I.shape[1], I.shape[1])
    for _ in range(steps):
        for m in modes:
            w.wspr_set_arithmetic(m)
            t0 = time.perf_counter()
            nres = dec.decode_ptr(I.data_ptr(), Q.data_ptr(), I.shape[1], I.shape[1])
            times[m].append(time.perf_counter() - t0)
            spots[m] = int(sum(nres))
    w.wspr_set_arithmetic(0)
    return times, spots


def kernel_table(trace_csvs):
    """kernel name (template arguments kept) -> (calls, total ms)."""
    tot = collections.defaultdict(lambda: [0, 0.0])
    for path in trace_csvs:
        for r in csv.DictReader(open(path)):
            name = r.get("Kernel_Name") or r.get("KernelName") or ""
            t = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
            tot[name][0] += 1
            tot[name][1] += t
    return tot


def short(name):
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    return name.split("(")[0].replace("wspr::", "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)     # one mode, one step (under rocprofv3)
    a = ap.parse_args()
    if a.child is not None:
        run_steps(a.nseg, 1, [a.child])
        return
    times, spots = run_steps(a.nseg, a.steps, [0, 1])
    res = {"workload": "configs[2]: %d segments x 10 signals, -10..-28 dB, resident; one wspr_decode_batch_device() call "
                       "per step, modes interleaved" % a.nseg, "steps_per_mode": a.steps, "modes": {}}
    for m, name in ((0, "exact"), (1, "contracted")):
        ts = sorted(times[m])
        res["modes"][name] = {"segments_per_s_median": a.nseg / ts[len(ts) // 2], "seconds_per_step": times[m],
                              "spots_last_step": spots[m]}
    res["contracted_over_exact"] = res["modes"]["contracted"]["segments_per_s_median"] / res["modes"]["exact"]["segments_per_s_median"]
    kern = {}
    for m in (0, 1):
        d = tempfile.mkdtemp(prefix="contract_ab_")
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                        sys.executable, os.path.abspath(__file__), "--nseg", str(a.nseg), "--child", str(m)],
                       check=True, timeout=600, stdout=subprocess.DEVNULL)
        for k, (calls, ms) in kernel_table(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)).items():
            kern[short(k)] = {"calls": calls, "ms": round(ms, 3)}
    pairs = []
    for k, v in sorted(kern.items()):
        if k.endswith("true>"):
            twin = k[:-5] + "false>"
            if twin in kern:
                pairs.append({"kernel": k[:-5].rstrip("<, ") , "exact_ms": kern[twin]["ms"], "contracted_ms": v["ms"],
                              "contracted_over_exact": round(v["ms"] / kern[twin]["ms"], 3) if kern[twin]["ms"] else None})
    res["kernels"] = kern
    res["fused_vs_exact_twin"] = pairs
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "contracted_ab.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = [res["workload"], "",
             "segments/s (median of %d steps): exact %.0f, contracted %.0f, ratio %.3f" % (
                 a.steps, res["modes"]["exact"]["segments_per_s_median"], res["modes"]["contracted"]["segments_per_s_median"],
                 res["contracted_over_exact"]), "",
             "%-44s %12s %15s %8s" % ("kernel (one step per mode)", "exact ms", "contracted ms", "ratio")]
    for p in pairs:
        lines.append("%-44s %12.3f %15.3f %8.3f" % (p["kernel"], p["exact_ms"], p["contracted_ms"], p["contracted_over_exact"] or 0))
    with open(os.path.join(a.out_dir, "contracted_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
