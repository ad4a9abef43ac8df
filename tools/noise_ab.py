#!/usr/bin/env python3
"""The band noise figures (K16) on an MI355X: what the kernel costs beside two yardsticks, and what the figures read.

  python tools/noise_ab.py [--nseg 2048] [--reps 9] [--out profiles/noise_figure.json]
                           [--bench-dumps PARENT_DIR THIS_DIR]

Cost, on --nseg full rows of the synthesiser's white noise resident in HBM, the three taking turns in one loop:
  K16   wspr_noise_batch_device(): a host clock around the call (it returns when its stream is done and the 32-byte
        records have arrived), and the kernel's own start and end stamps from a `rocprofv3 --kernel-trace` run of a child
        process (the library has no event hook for this stage, and the decode path's timing slots are not touched);
  copy  a device-to-device copy of the same rows, wspr_calib_copy16 of the lab library (its own HIP events);
  K1    the FFT bank on the same rows, wspr_bench_fft_sync of the lab library (HIP events; ms[0]), and fft_bank*_kernel in
        the same kernel trace.
K16 reads the bytes K1 reads and does half its transforms (hop 256 against 128): no longer than K1 is the goal.

Readings: the figures over 2 sigma^2 on device-generated white noise (the bias of "the quietest 30 %", re-measured; the CPU
test measures it on numpy's noise), and what ten strong signals per row (tests/noise_lib.py crowd_items()) do to each figure.
--bench-dumps: two directories written by `bench.py --dump-outputs` on the parent commit and on this one; recorded is
whether every file is byte-identical.  Nothing is asserted but that the records equal the checker's."""
import argparse
import csv
import ctypes as C
import filecmp
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rtlsdr_wsprd_amd as w  # noqa: E402

NS = 45000
SEED = 1600


def noise_rows(nseg, sigma, dev, stride, seed=SEED, items=None):
    dI = torch.zeros((nseg, stride), dtype=torch.float32, device=dev)
    dQ = torch.zeros((nseg, stride), dtype=torch.float32, device=dev)
    w.sync_torch()
    assert w.wspr_synth_batch_device(items or [], nseg, dI.data_ptr(), dQ.data_ptr(), noise_sigma=sigma, seed=seed) == 0
    return dI, dQ


def child(nseg):
    """Three calls of K16 and one timed pass set of K1 on the same rows, for the kernel trace."""
    import noise_lib as nl
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stride = int(w.lib().wspr_iq_stride())
    dI, dQ = noise_rows(nseg, float(np.float32(nl.SIGMA)), dev, stride)
    for _ in range(4):
        rc, _ = w.noise_batch_device(dI.data_ptr(), dQ.data_ptr(), nseg, NS, stride)
        assert rc == 0
    ms = (C.c_double * 8)()
    w.lab().wspr_bench_fft_sync(dI.data_ptr(), dQ.data_ptr(), nseg, NS, stride, 3, C.addressof(ms))


def kernel_times(nseg):
    """{kernel: [ms per launch]} of K16's and K1's kernels from a kernel trace of child()."""
    d = tempfile.mkdtemp(prefix="noise_ab_")
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
                    os.path.abspath(__file__), "--child", "--nseg", str(nseg)], check=True, timeout=400,
                   stdout=subprocess.DEVNULL)
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name") or r.get("KernelName") or ""
            for k in ("noise_kernel", "fft_bank_avg_kernel", "fft_bank_kernel"):
                if k in name:
                    out.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
                    break
    return out


def cost(a, dev, stride, nl):
    nseg = a.nseg
    sigma = float(np.float32(nl.SIGMA))
    dI, dQ = noise_rows(nseg, sigma, dev, stride)
    cI, cQ = torch.empty_like(dI), torch.empty_like(dQ)
    lab = w.lab()
    out = np.zeros(nseg, w.NOISE_DTYPE)
    nfloats = nseg * stride
    ms16, msk1 = C.c_double(0.0), (C.c_double * 8)()
    times = {"noise_call_ms": [], "copy_ms": [], "k1_ms": [], "k1_launches": []}
    for rep in range(a.reps + 2):                                # two warm-up rounds: code objects, contexts, tables
        torch.cuda.synchronize()
        t = time.perf_counter()
        rc, _ = w.noise_batch_device(dI.data_ptr(), dQ.data_ptr(), nseg, NS, stride, None, out)
        t_noise = (time.perf_counter() - t) * 1e3
        assert rc == 0
        lab.wspr_calib_copy16(dI.data_ptr(), cI.data_ptr(), nfloats, 1, 0, C.byref(ms16))      # one rail ...
        one = ms16.value
        lab.wspr_calib_copy16(dQ.data_ptr(), cQ.data_ptr(), nfloats, 1, 0, C.byref(ms16))      # ... and the other
        lab.wspr_bench_fft_sync(dI.data_ptr(), dQ.data_ptr(), nseg, NS, stride, 1, C.addressof(msk1))
        if rep >= 2:
            times["noise_call_ms"].append(t_noise)
            times["copy_ms"].append(one + ms16.value)
            times["k1_ms"].append(msk1[0])
            times["k1_launches"].append(msk1[3])
    # what the timed calls wrote is what the checker says (eight rows of them)
    hI, hQ = dI[:8, :NS].cpu().numpy(), dQ[:8, :NS].cpu().numpy()
    same = out[:8].tobytes() == nl.check_rows(hI, hQ, NS).tobytes()
    assert same
    trace = kernel_times(nseg)
    med = {k: float(np.median(v)) for k, v in times.items()}
    k16 = sorted(trace.get("noise_kernel", []))
    k1_trace = {k: float(np.median(v)) for k, v in trace.items() if k != "noise_kernel"}
    row_bytes = 2 * 4 * NS * nseg                                # both rails read once
    res = {
        "what": "noise_kernel_ms: the kernel's start-to-end stamps in a rocprofv3 kernel trace of a child process (median of "
                "its launches after the first); noise_call_ms: a host clock around the whole call; copy_ms and k1_ms: HIP "
                "events of the lab library's own hooks; all on the same rows, taking turns in one loop",
        "nseg": nseg, "samples": NS, "reps": a.reps, "records_equal_checker": bool(same),
        "noise_kernel_ms": float(np.median(k16[:-1] if len(k16) > 1 else k16)) if k16 else None,
        "noise_kernel_ms_all": trace.get("noise_kernel", []),
        "k1_kernels_in_trace_ms": k1_trace,
        "bytes_read_by_k16": row_bytes,
    }
    res.update(med)
    if res["noise_kernel_ms"]:
        res["noise_kernel_bytes_per_s"] = row_bytes / (res["noise_kernel_ms"] * 1e-3)
        res["noise_kernel_over_k1"] = res["noise_kernel_ms"] / med["k1_ms"]
        res["noise_kernel_over_copy"] = res["noise_kernel_ms"] / med["copy_ms"]
    res["noise_call_over_k1"] = med["noise_call_ms"] / med["k1_ms"]
    res.update({k + "_all": v for k, v in times.items()})
    # the white-noise readings of the same rows
    ref = 2.0 * sigma * sigma
    res["white_noise"] = {"sigma": sigma, "rows": nseg, "source": "wspr_synth_batch_device() noise, seed %d" % SEED}
    for f in nl.FIGURES:
        r = out[f].astype(np.float64) / ref
        res["white_noise"][f + "_over_2s2"] = {"mean": float(r.mean()), "sd": float(r.std(ddof=1)),
                                               "mean_db": float(10 * np.log10(r.mean()))}
    return res


def crowded(dev, stride, nl, nrows=64):
    sigma = 0.02
    clean_rows = noise_rows(nrows, sigma, dev, stride, seed=31)
    busy_rows = noise_rows(nrows, sigma, dev, stride, seed=31, items=nl.crowd_items(nrows, sigma))
    rc0, clean = w.noise_batch_device(clean_rows[0].data_ptr(), clean_rows[1].data_ptr(), nrows, NS, stride)
    rc1, busy = w.noise_batch_device(busy_rows[0].data_ptr(), busy_rows[1].data_ptr(), nrows, NS, stride)
    assert rc0 == 0 and rc1 == 0
    res = {"rows": nrows, "sigma": sigma, "scene": "tests/noise_lib.py crowd_items(): ten signals per row, +0 .. +9 dB in 2500 Hz, "
           "24 Hz apart, dt -1.0 .. +0.8 s, over the same noise as the clean rows", "shift_db": {}}
    for f in nl.FIGURES:
        s = 10.0 * np.log10(busy[f].astype(np.float64) / clean[f].astype(np.float64))
        res["shift_db"][f] = {"median": float(np.median(s)), "min": float(s.min()), "max": float(s.max())}
    return res


def compare_dumps(parent, this):
    names = sorted(os.listdir(parent))
    same = names == sorted(os.listdir(this)) and all(filecmp.cmp(os.path.join(parent, n), os.path.join(this, n), shallow=False)
                                                     for n in names)
    return {"files": names, "bytes": int(sum(os.path.getsize(os.path.join(this, n)) for n in os.listdir(this))),
            "spot_records_byte_identical_to_parent": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)      # under rocprofv3
    ap.add_argument("--nseg", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--bench-dumps", nargs=2, metavar=("PARENT_DIR", "THIS_DIR"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_figure.json"))
    a = ap.parse_args()
    if w.lib().wspr_device_ready() != 1:
        sys.exit("noise_ab: no usable HIP device (there is no CPU fallback)")
    if a.child:
        return child(a.nseg)
    import noise_lib as nl
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stride = int(w.lib().wspr_iq_stride())
    res = {"device": torch.cuda.get_device_name(0)}
    res["cost"] = cost(a, dev, stride, nl)
    print(json.dumps(res["cost"]), flush=True)
    res["crowded_band"] = crowded(dev, stride, nl)
    print(json.dumps(res["crowded_band"]), flush=True)
    stats = nl.white_noise_statistics()
    res["white_noise_cpu"] = {"rows": 64, "source": "numpy noise, tests/noise_lib.py white_rows(), through the serial checker",
                              **{f + "_over_2s2": {"mean": stats[f][0], "sd": stats[f][1]} for f in nl.FIGURES}}
    if a.bench_dumps:
        res["bench_py"] = compare_dumps(*a.bench_dumps)
        print(json.dumps(res["bench_py"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
