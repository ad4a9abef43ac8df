#!/usr/bin/env python3
"""Decode probability against Doppler spread, and what the fading channel (K13) costs.  MI355X.

The curve (profiles/fade_sensitivity.json).  tools/block_sensitivity.py's experiment through
wspr_synth_faded_batch_device(): per Doppler spread sigma in {0, 0.05, 0.1, 0.2, 0.5, 1.0} Hz (one Rayleigh path of gain
1; sigma = 0 is the constant carrier) and per SNR (default -30 .. -22 dB in 1 dB steps; the project's convention of
tests/synth.py: sigma^2 per rail = (375/2500)/2, amplitude 10^(SNR/20) -- the MEAN power under fading --, normalised to
a peak of 0.5): --segments segments (default 2 048), one synth.message_wide signal each, f0 uniform in +-100 Hz,
t0 = 2 +- 1 s, drift 0, generated on the device; the SAME rows are decoded with block detection off (maxblock 1), 2 and 3
under the default options.  Recorded per point and setting: decoded (the sent text is among the segment's spots) and
false (spots whose text was not sent).  The maxblock-1 decode runs with wspr_set_spread_estimate(1); per sigma the median
of w50 (and of w50 / sigma) over the decoded sent spots of all its SNR points is recorded.  Nothing is asserted.

The cost (profiles/fade_channel.json).  On one 2 048-segment scene (sigma = 0.2 Hz, -26 dB) three calls, alternating,
--reps times each after --warmup: the faded call, wspr_synth_batch_device() on the same list, and one decode of the
faded rows -- a host clock around calls that are complete on return (include/wspr_mi355x.h, stream contract).  Kernel
times come from a kernel trace of a child process in a run of its own.  Reported: the ratios faded / unfaded and faded /
decode, and the share of the fp64 vector rate without fused multiply-add that synth_fade_kernel reaches by the
definition's operation count (k13_fade.hip: 54 + 6 + 596 double operations per transmission sample of a one-path
diffuse channel), against half the data sheet's 78.6 TFLOP/s (tools/synth_ab.py states the convention).  Also, from the
CPU checker, synth_exp()'s largest distance from numpy.exp on 200 000 points of [-40, 0].

    python tools/fade_sensitivity.py [--segments 2048] [--skip-curve | --skip-cost]
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

import rtlsdr_wsprd_amd as w   # noqa: E402
import synth            # noqa: E402

NS = 45000
SIGLEN = 162 * 256
MAXBLOCKS = (1, 2, 3)
SIGMAS = (0.0, 0.05, 0.1, 0.2, 0.5, 1.0)
FP64_DATASHEET_TFLOPS = 78.6
OPS_UNFADED = 54                       # k8_synth.hip
OPS_FADED_ONE_DIFFUSE_PATH = 54 + 6 + 596   # k13_fade.hip: the unfaded sample, the complex product, one diffuse path
NOISE_SIGMA = float(np.float32(np.sqrt((375.0 / 2500.0) / 2.0)))


def messages(nseg, rng):
    sym = np.zeros((nseg, 162), np.uint8)
    expected = []
    for s in range(nseg):
        m = synth.message_wide(int(rng.integers(0, 1 << 62)))
        sym[s] = w.get_wspr_channel_symbols(m)[1]
        expected.append(synth.expected_text(m))
    return sym, expected


def scene(nseg, sym, rng, snr_db, sigma_hz):
    tx = np.zeros(nseg, w.SYNTH_TX_DTYPE)
    tx["seg"] = np.arange(nseg)
    tx["f0"] = rng.uniform(-100.0, 100.0, nseg)
    tx["t0"] = 2.0 + rng.uniform(-1.0, 1.0, nseg)
    tx["amp"] = 10.0 ** (snr_db / 20.0)
    tx["symbols"] = sym
    ch = np.zeros(nseg, w.SYNTH_CHANNEL_DTYPE)
    ch["path"]["gain"][:, 0] = 1.0
    ch["path"]["sigma"][:, 0] = sigma_hz
    return tx, ch


def curve(args, L, dev, stride):
    nseg = args.segments
    out_path = os.path.abspath(args.out_curve)
    rng = np.random.default_rng(args.seed)
    sym, expected = messages(nseg, rng)
    dI = torch.zeros(nseg, stride, device=dev)
    dQ = torch.zeros(nseg, stride, device=dev)
    w.sync_torch()
    dec = w.BatchDecoder(nseg, 16, w.default_options())
    per_sigma = []
    point = 0
    try:
        for sigma_hz in SIGMAS:
            rec_s = {"sigma_hz": sigma_hz, "points": []}
            w50 = []
            for snr in range(args.snr_lo, args.snr_hi + 1):
                tx, ch = scene(nseg, sym, rng, snr, sigma_hz)
                assert w.wspr_synth_faded_batch_device(tx, ch, nseg, dI.data_ptr(), dQ.data_ptr(), point * nseg, NOISE_SIGMA,
                                                       args.seed, w.SYNTH_NORMALISE) == 0
                point += 1
                rec = {"snr_db": snr, "segments": nseg}
                for mb in MAXBLOCKS:
                    w.set_block_detection(mb)
                    w.set_spread_estimate(1 if mb == 1 else 0)
                    dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)
                    texts = [[x.message.decode() for x in dec.spots(s)] for s in range(nseg)]
                    ok = sum(expected[s] in texts[s] for s in range(nseg))
                    false = sum(m != expected[s] for s in range(nseg) for m in texts[s])
                    rec["maxblock_%d" % mb] = {"decoded": ok, "share": ok / nseg, "false": false}
                    if mb == 1:
                        spr = w.last_spreads(nseg, 16)
                        assert spr is not None
                        for s in range(nseg):
                            if expected[s] in texts[s]:
                                r = spr[s, texts[s].index(expected[s])]
                                if r["valid"] == 1:
                                    w50.append(float(r["w50"]))
                print("sigma %.2f Hz SNR %4d dB: " % (sigma_hz, snr) + "   ".join(
                    "B%d %d/%d (%d false)" % (mb, rec["maxblock_%d" % mb]["decoded"], nseg, rec["maxblock_%d" % mb]["false"])
                    for mb in MAXBLOCKS), flush=True)
                rec_s["points"].append(rec)
            rec_s["w50"] = {"spots": len(w50), "median_hz": statistics.median(w50) if w50 else None,
                            "median_over_sigma": statistics.median(w50) / sigma_hz if w50 and sigma_hz > 0 else None}
            print("sigma %.2f Hz: median w50 %s Hz over %d decoded spots" % (sigma_hz, rec_s["w50"]["median_hz"], len(w50)), flush=True)
            per_sigma.append(rec_s)
            # the record as far as it has come: a run that is cut short still leaves its points
            write(out_path, {
                "what": "decode probability and false spots against Doppler spread (one Rayleigh path, Gaussian Doppler spectrum "
                        "of standard deviation sigma; sigma 0 = constant carrier) and SNR in 2500 Hz (mean power), block "
                        "detection off (maxblock 1) and on (2, 3); generated by wspr_synth_faded_batch_device() and decoded by "
                        "wspr_decode_batch_device() under the default options; w50: median of K11's figure over the decoded "
                        "sent spots of the maxblock-1 decodes; nothing asserted",
                "device": torch.cuda.get_device_name(0), "library": L.wspr_mi355x_version().decode(),
                "scene": {"segments_per_point": nseg, "sigma_per_rail": NOISE_SIGMA, "f0_hz": "uniform +-100",
                          "t0_s": "2 +- 1 uniform", "drift": 0, "normalised": True, "seed": args.seed,
                          "options": "npasses 2, subtraction 1, quickmode 0, usehashtable 0"},
                "maxblocks": list(MAXBLOCKS), "sigmas": per_sigma})
    finally:
        w.set_block_detection(1)
        w.set_spread_estimate(0)
    print(json.dumps({"written": os.path.relpath(out_path, ROOT), "sigmas": len(per_sigma)}))


def write(path, obj):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f, indent=1)
        f.write("\n")


def child(path, nseg):
    """Three faded and three unfaded calls on the saved lists, for the kernel trace."""
    d = np.load(path)
    tx, ch = d["tx"], d["ch"]
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stride = int(w.lib().wspr_iq_stride())
    dI = torch.zeros(nseg, stride, device=dev)
    dQ = torch.zeros(nseg, stride, device=dev)
    w.sync_torch()
    for _ in range(3):
        assert w.wspr_synth_faded_batch_device(tx, ch, nseg, dI.data_ptr(), dQ.data_ptr(), 0, NOISE_SIGMA, 4321, w.SYNTH_NORMALISE) == 0
        assert w.wspr_synth_batch_device(tx, nseg, dI.data_ptr(), dQ.data_ptr(), 0, NOISE_SIGMA, 4321, w.SYNTH_NORMALISE) == 0


def kernel_times(tx, ch, nseg):
    """{kernel: [ms per launch]} of the synthesiser's kernels from a kernel trace of child()."""
    d = tempfile.mkdtemp(prefix="fade_cost_")
    path = os.path.join(d, "scene.npz")
    np.savez(path, tx=tx, ch=ch)
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
                    os.path.abspath(__file__), "--child", path, "--segments", str(nseg)], check=True, timeout=300,
                   stdout=subprocess.DEVNULL)
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name") or r.get("KernelName") or ""
            for k in ("synth_phase_kernel", "synth_fill_kernel", "synth_fade_kernel", "normalise_kernel"):
                if k in name:
                    out.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    return out


def exp_distance():
    import fade_lib as fl
    x = np.linspace(-40.0, 0.0, 200000)
    got, want = fl.synth_exp(x), np.exp(x)
    return {"points": int(x.size), "interval": [-40.0, 0.0], "against": "numpy.exp",
            "largest_relative_error": float(np.max(np.abs(got - want) / want)),
            "largest_distance_ulp": float(np.max(np.abs(got - want) / np.spacing(want))), "bound_relative": 2.0 ** -40}


def cost(args, L, dev, stride):
    nseg = args.segments
    out_path = os.path.abspath(args.out_cost)
    rng = np.random.default_rng(args.seed + 1)
    sym, _ = messages(nseg, rng)
    tx, ch = scene(nseg, sym, rng, -26, 0.2)
    dI = torch.zeros(nseg, stride, device=dev)
    dQ = torch.zeros(nseg, stride, device=dev)
    w.sync_torch()
    dec = w.BatchDecoder(nseg, 16, w.default_options())

    def faded():
        assert w.wspr_synth_faded_batch_device(tx, ch, nseg, dI.data_ptr(), dQ.data_ptr(), 0, NOISE_SIGMA, 4321, w.SYNTH_NORMALISE) == 0

    def unfaded():
        assert w.wspr_synth_batch_device(tx, nseg, dI.data_ptr(), dQ.data_ptr(), 0, NOISE_SIGMA, 4321, w.SYNTH_NORMALISE) == 0

    def decode():
        dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)

    ms = {"faded": [], "unfaded": [], "decode": []}
    for r in range(args.warmup + args.reps):            # alternating; the decode always sees the faded rows
        for name, fn in (("unfaded", unfaded), ("faded", faded), ("decode", decode)):
            t = time.perf_counter()
            fn()
            dt = 1e3 * (time.perf_counter() - t)
            if r >= args.warmup:
                ms[name].append(dt)
    med = {k: statistics.median(v) for k, v in ms.items()}
    samples = nseg * SIGLEN                               # t0 = 2 +- 1 s: every frame lies inside its row
    bound = FP64_DATASHEET_TFLOPS * 0.5e12
    out = {
        "what": "cost of the synthesiser's fading channel (K13) on one scene of %d single-signal segments, one Rayleigh path of "
                "sigma 0.2 Hz, -26 dB: call times by a host clock around calls that are complete on return, alternating, "
                "median of %d after %d warm-up rounds; kernel times from a kernel trace of a child process" % (nseg, args.reps, args.warmup),
        "device": torch.cuda.get_device_name(0), "library": L.wspr_mi355x_version().decode(),
        "call_ms": {k: {"median": med[k], "min": min(v), "max": max(v), "all": v} for k, v in ms.items()},
        "faded_over_unfaded_call": med["faded"] / med["unfaded"], "faded_over_decode_call": med["faded"] / med["decode"],
        "generating_costs_more_than_decoding": med["faded"] > med["decode"],
        "operations": {"transmission_samples": samples, "per_sample_unfaded": OPS_UNFADED,
                       "per_sample_faded_one_diffuse_path": OPS_FADED_ONE_DIFFUSE_PATH,
                       "bound_tflops_unfused": bound * 1e-12,
                       "bound_source": "data sheet: %.1f TFLOP/s fp64 vector counting a fused multiply-add as two; unfused code "
                                       "issues at most half of it" % FP64_DATASHEET_TFLOPS},
        "synth_exp": exp_distance(),
    }
    out["operations"]["share_of_unfused_bound_faded_call"] = samples * OPS_FADED_ONE_DIFFUSE_PATH / (med["faded"] * 1e-3) / bound
    try:
        kt = kernel_times(tx, ch, nseg)
        kern = {k: {"ms_median": statistics.median(v), "launches": len(v)} for k, v in kt.items()}
        out["kernel_ms"] = kern
        if "synth_fade_kernel" in kern and "synth_fill_kernel" in kern:
            out["fade_over_fill_kernel"] = kern["synth_fade_kernel"]["ms_median"] / kern["synth_fill_kernel"]["ms_median"]
            out["operations"]["share_of_unfused_bound_fade_kernel"] = \
                samples * OPS_FADED_ONE_DIFFUSE_PATH / (kern["synth_fade_kernel"]["ms_median"] * 1e-3) / bound
            out["operations"]["share_of_unfused_bound_fill_kernel"] = \
                samples * OPS_UNFADED / (kern["synth_fill_kernel"]["ms_median"] * 1e-3) / bound
    except (subprocess.SubprocessError, OSError) as e:
        out["kernel_ms"] = "not measured: the kernel trace failed (%s)" % type(e).__name__
    write(out_path, out)
    print(json.dumps({k: out[k] for k in ("faded_over_unfaded_call", "faded_over_decode_call", "kernel_ms")}))
    print(json.dumps({"written": os.path.relpath(out_path, ROOT)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)      # the saved lists (under rocprofv3)
    ap.add_argument("--segments", type=int, default=2048)
    ap.add_argument("--snr-lo", type=int, default=-30)
    ap.add_argument("--snr-hi", type=int, default=-22)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-curve", action="store_true")
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--out-curve", default=os.path.join(ROOT, "profiles", "fade_sensitivity.json"))
    ap.add_argument("--out-cost", default=os.path.join(ROOT, "profiles", "fade_channel.json"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.segments)
    L = w.lib()
    assert L.wspr_device_ready() == 1
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stride = int(L.wspr_iq_stride())
    if not args.skip_cost:
        cost(args, L, dev, stride)
    if not args.skip_curve:
        curve(args, L, dev, stride)


if __name__ == "__main__":
    main()
