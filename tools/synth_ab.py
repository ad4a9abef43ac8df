#!/usr/bin/env python3
"""Speed of the device synthesiser (K8) on the configs[2] scene: 8 192 segments x 10 signals, noise, normalised.

Measured in one session on one device, wall time around synchronous calls:
  synth   one wspr_synth_batch_device() call (median of --reps after --warmup), list upload and kernels included;
  (a)     bench.py's synth_batch_gpu() making a scene of the same size (torch: parallel cumsum, scatter_add) -- how such a
          batch was produced before; the whole function, its host-side message work included (that of this tool's list is
          reported next to it);
  (b)     one exact-mode wspr_decode_batch_device() of the synthesised rows.
Requirements (the record states whether they hold): synth < (a), and synth < (b), so that a generate-and-decode loop is
decoder-bound.  Also the share of the fp64 vector rate the call reaches: 54 unfused double operations per transmission
sample (k8_synth.hip) against the DATA SHEET's 78.6 TFLOP/s, which counts a fused multiply-add as two -- 39.3 T
operations/s for code that may not fuse.  No measured fp64 figure exists for this part; no target is set.  The kernels' own times come from a separate
`rocprofv3 --kernel-trace` run of three more calls on the same list (a child process, after the timed ones).

    python tools/synth_ab.py [--segments 8192] [--out profiles/synth_ab.json]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np      # noqa: E402
import torch            # noqa: E402  (before the library: see tests/conftest.py)

import bench            # noqa: E402
import rtlsdr_wsprd_amd as w   # noqa: E402
import synth            # noqa: E402

NS = 45000
FP64_DATASHEET_TFLOPS = 78.6
OPS_PER_SAMPLE = 54


def scene(nseg, nsig, seed):
    """The configs[2] scene (bench.py synth_batch_gpu with n_signals = 10): frequency slots over +-100 Hz, SNR -10 .. -28 dB,
    t0 = 2 +- 0.3 s, every signal its own message."""
    rng = np.random.default_rng(seed)
    tx = np.zeros(nseg * nsig, w.SYNTH_TX_DTYPE)
    tx["seg"] = np.repeat(np.arange(nseg), nsig)
    tx["f0"] = (np.linspace(-100.0, 100.0, nsig)[None, :] + rng.uniform(-2.0, 2.0, (nseg, nsig))).ravel()
    tx["t0"] = (2.0 + rng.uniform(-0.3, 0.3, (nseg, nsig))).ravel()
    tx["amp"] = np.tile(10.0 ** (np.linspace(-10.0, -28.0, nsig) / 20.0), nseg)
    expected = []
    for k in range(nseg * nsig):
        m = synth.message_wide(int(rng.integers(0, 1 << 62)))
        tx["symbols"][k] = w.get_wspr_channel_symbols(m)[1]
        expected.append(synth.expected_text(m))
    return tx, [expected[s * nsig:(s + 1) * nsig] for s in range(nseg)]


def child(path, nseg):
    """Three calls on the saved list, for the kernel trace."""
    tx = np.load(path)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stride = int(w.lib().wspr_iq_stride())
    dI = torch.zeros(nseg, stride, device=dev)
    dQ = torch.zeros(nseg, stride, device=dev)
    w.sync_torch()
    sigma = float(np.float32(np.sqrt((375.0 / 2500.0) / 2.0)))
    for _ in range(3):
        assert w.wspr_synth_batch_device(tx, nseg, dI.data_ptr(), dQ.data_ptr(), 0, sigma, 4321, w.SYNTH_NORMALISE) == 0


def kernel_times(tx, nseg):
    """{kernel: [ms per launch]} of the synthesiser's kernels from a kernel trace of child()."""
    d = tempfile.mkdtemp(prefix="synth_ab_")
    path = os.path.join(d, "tx.npy")
    np.save(path, tx)
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
                    os.path.abspath(__file__), "--child", path, "--segments", str(nseg)], check=True, timeout=300,
                   stdout=subprocess.DEVNULL)
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name") or r.get("KernelName") or ""
            for k in ("synth_phase_kernel", "synth_fill_kernel", "normalise_kernel"):
                if k in name:
                    out.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)      # the saved list, three calls (under rocprofv3)
    ap.add_argument("--segments", type=int, default=8192)
    ap.add_argument("--signals", type=int, default=10)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth_ab.json"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.segments)
    assert w.lib().wspr_device_ready() == 1
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nseg, nsig = args.segments, args.signals
    stride = int(w.lib().wspr_iq_stride())
    sigma = float(np.float32(np.sqrt((375.0 / 2500.0) / 2.0)))

    t = time.perf_counter()
    tx, expected = scene(nseg, nsig, 4321)
    list_s = time.perf_counter() - t
    dI = torch.zeros(nseg, stride, device=dev)
    dQ = torch.zeros(nseg, stride, device=dev)
    w.sync_torch()
    times = []
    for r in range(args.warmup + args.reps):
        t = time.perf_counter()
        rc = w.wspr_synth_batch_device(tx, nseg, dI.data_ptr(), dQ.data_ptr(), 0, sigma, 4321, w.SYNTH_NORMALISE)
        times.append(time.perf_counter() - t)
        assert rc == 0
    synth_ms = [1e3 * x for x in times[args.warmup:]]

    dec = w.BatchDecoder(nseg, 32)
    dec_ms = []
    for r in range(1 + 5):
        t = time.perf_counter()
        dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)
        dec_ms.append(1e3 * (time.perf_counter() - t))
    dec_ms = dec_ms[1:]
    n_ok = sum(len(set(expected[s]) & {x.message.decode() for x in dec.spots(s)}) for s in range(nseg))
    n_false = sum(x.message.decode() not in expected[s] for s in range(nseg) for x in dec.spots(s))

    torch_ms = []
    for r in range(1 + 3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        bench.synth_batch_gpu(nseg, 4321 + r, dev, nsig, -10.0, -28.0, 0.3, wide=True)
        torch.cuda.synchronize()
        torch_ms.append(1e3 * (time.perf_counter() - t))
    torch_ms = torch_ms[1:]

    first = np.floor(tx["t0"].astype(np.float64) / (1 / 375.0)).astype(np.int64)
    in_row = int((np.minimum(first + 162 * 256, NS) - np.maximum(first, 0)).clip(0).sum())
    med = statistics.median(synth_ms)
    ops = in_row * OPS_PER_SAMPLE
    rate = ops / (med * 1e-3)
    try:
        kt = kernel_times(tx, nseg)
    except (OSError, subprocess.SubprocessError) as e:
        print("kernel trace not taken: %s" % e)
        kt = {}
    kern = {k: {"ms_median": statistics.median(v), "launches": len(v)} for k, v in kt.items()}
    if "synth_fill_kernel" in kern:
        kern["synth_fill_kernel"]["share_of_unfused_fp64_bound"] = \
            ops / (kern["synth_fill_kernel"]["ms_median"] * 1e-3) / (FP64_DATASHEET_TFLOPS * 0.5e12)
    rec = {
        "kernels_traced_separately": kern,
        "workload": "configs[2] scene: %d segments x %d signals, sigma %.4f per rail, normalised" % (nseg, nsig, sigma),
        "device": torch.cuda.get_device_name(0), "library": w.lib().wspr_mi355x_version().decode(),
        "synth_call_ms": {"median": med, "min": min(synth_ms), "max": max(synth_ms), "reps": len(synth_ms), "all": synth_ms},
        "synth_list_build_host_s": list_s,
        "a_bench_synth_batch_gpu_ms": {"median": statistics.median(torch_ms), "all": torch_ms},
        "b_exact_decode_ms": {"median": statistics.median(dec_ms), "all": dec_ms},
        "decoded_ok": "%d/%d" % (n_ok, nseg * nsig), "false_decodes": n_false,
        "faster_than_a": med < statistics.median(torch_ms), "below_b": med < statistics.median(dec_ms),
        "fp64": {"transmission_samples": in_row, "double_ops_per_sample": OPS_PER_SAMPLE, "double_ops": ops,
                 "reached_Tops_per_s": rate / 1e12,
                 "bound_source": "data sheet: %.1f TFLOP/s fp64 vector counting a fused multiply-add as two; "
                                 "unfused code issues at most half of it" % FP64_DATASHEET_TFLOPS,
                 "share_of_unfused_bound": rate / (FP64_DATASHEET_TFLOPS * 0.5e12),
                 "note": "whole call (list upload, phase kernel, fill, normalise) over the fill kernel's arithmetic: a lower bound of the kernel's own share"},
        "bytes_written": 2 * nseg * stride * 4,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: rec[k] for k in ("synth_call_ms", "a_bench_synth_batch_gpu_ms", "b_exact_decode_ms", "decoded_ok",
                                          "false_decodes", "faster_than_a", "below_b")}, default=lambda o: o))
    print("fp64: %.2f T double ops/s = %.1f %% of the unfused data-sheet bound" % (rate / 1e12, 100 * rec["fp64"]["share_of_unfused_bound"]))


if __name__ == "__main__":
    main()
