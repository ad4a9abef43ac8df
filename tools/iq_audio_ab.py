#!/usr/bin/env python3
"""IQ to audio (K18) on an MI355X: what a batch of rows costs against the audio front end (K12) going the other way, how
often normalised rows clip at the recommended gain, and what the loop K18 -> K12 does to the decoder.

  python tools/iq_audio_ab.py [--nseg 2048] [--reps 7] [--out profiles/iq_audio.json]

Cost, at 2 048 full rows (45 000 samples each, 1 440 000 samples of audio per record, 5.9 GB written):
wspr_iq_to_audio_batch_device(), wspr_audio_batch_device() on the records it wrote, and a device fill of the same bytes
(every sample written once: the memory floor) -- the three taking turns inside one loop, so that they see the same clocks.
Call times are a host clock around a call that ends in the library's own wait for its stream (torch's fill: around a device
synchronise).  Kernel times come from a kernel trace of a child process that makes the same calls, in a run of its own.
K12 does the same number of multiply-adds as K18 (at most 24 per audio sample after the exact zeros), so its kernel is the
yardstick: THE GOAL IS "NO SLOWER THAN K12".  Beside it: K18's share of the fp32 vector rate at 24 fused multiply-adds per
output (data sheet: 157.3 TFLOP/s counting a multiply-add as two).

Then, nothing asserted:
  clipping   the share of samples that clip at gain 32768 on normalised ten-signal scenes;
  loop       the decoded share of --nseg three-signal scenes at -26 and -29 dB, the rows decoded as they are and after
             K18 -> K12 (the same rows: the two differ by the loop alone);
  fading     K13 at -28 dB, one Rayleigh path of sigma 0.1 Hz, the rows decoded as they are (noise from K13) and through
             the audio path: K13 without noise -> K18 -> K17 (accumulate, noise only) -> K12."""
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

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rtlsdr_wsprd_amd as w  # noqa: E402
import synth                   # noqa: E402

NS = 45000
NSAMP = 32 * NS
FMA_PER_OUTPUT = 24
FP32_DATASHEET_TFLOPS = 157.3
NOISE_SIGMA = float(np.float32(np.sqrt((375.0 / 2500.0) / 2.0)))        # unit power in 2 500 Hz
AUDIO_SIGMA = 2000.0 * float(np.sqrt(2.4))                              # tests/audio_lib.py's noise in PCM units
SEED = 1800


def three_signal_scene(al, nseg, snr):
    tx = np.zeros(3 * nseg, w.SYNTH_TX_DTYPE)
    syms = [[w.get_wspr_channel_symbols(m)[1] for m in msgs] for msgs in al.SCENE_MESSAGES]
    for s in range(nseg):
        for j, (_, f0, t0) in enumerate(al.SIGNALS):
            r = tx[3 * s + j]
            r["seg"], r["f0"], r["t0"], r["amp"], r["drift"] = s, f0, t0, 10.0 ** (snr / 20.0), 0.0
            r["symbols"] = syms[s % 3][j]
    return tx


def ten_signal_scene(nseg, rng):
    tx = np.zeros(10 * nseg, w.SYNTH_TX_DTYPE)
    for s in range(nseg):
        for k, f0 in enumerate(np.linspace(-100, 100, 10) + rng.uniform(-2, 2, 10)):
            r = tx[10 * s + k]
            r["seg"], r["f0"], r["t0"], r["amp"], r["drift"] = s, f0, 2.0 + rng.uniform(-1, 1), 10 ** (-(10 + 2 * k) / 20.0), 0.0
            r["symbols"] = w.get_wspr_channel_symbols(synth.message_wide(int(rng.integers(0, 1 << 40))))[1]
    return tx


class Rows:
    def __init__(self, nseg, dev, stride):
        self.nseg, self.stride = nseg, stride
        self.dI = torch.zeros(nseg, stride, device=dev)
        self.dQ = torch.zeros(nseg, stride, device=dev)
        self.bI = torch.zeros(nseg, stride, device=dev)
        self.bQ = torch.zeros(nseg, stride, device=dev)
        self.pcm = torch.zeros((nseg, NSAMP), dtype=torch.int16, device=dev)
        self.count = np.zeros(nseg, np.int32)
        w.sync_torch()

    def up(self, gain=w.IQ_AUDIO_GAIN):
        assert w.iq_to_audio_batch_device(self.dI.data_ptr(), self.dQ.data_ptr(), self.nseg, NS, self.stride, self.pcm.data_ptr(),
                                          NSAMP, gain, self.count) == 0

    def down(self):
        assert w.audio_batch_device(self.pcm.data_ptr(), NSAMP, NSAMP, self.nseg, self.bI.data_ptr(), self.bQ.data_ptr(), 1) == 0


def child(nseg):
    """Three K18 and three K12 calls on a three-signal scene, for the kernel trace."""
    import audio_lib as al
    torch.cuda.set_device(0)
    r = Rows(nseg, torch.device("cuda", 0), int(w.lib().wspr_iq_stride()))
    assert w.wspr_synth_batch_device(three_signal_scene(al, nseg, -20.0), nseg, r.dI.data_ptr(), r.dQ.data_ptr(), 0, NOISE_SIGMA, SEED,
                                     w.SYNTH_NORMALISE) == 0
    for _ in range(3):
        r.up()
        r.down()


def kernel_times(nseg):
    """{kernel: [ms per launch]} of K18's and K12's kernels from a kernel trace of child()."""
    d = tempfile.mkdtemp(prefix="iq_audio_cost_")
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                    "--child", "--nseg", str(nseg)], check=True, timeout=300, stdout=subprocess.DEVNULL)
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Kernel_Name") or row.get("KernelName") or ""
            for k in ("iq_audio_kernel", "audio_front_kernel"):
                if k in name:
                    out.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    return out


def cost(a, r, al, iq, kt):
    nseg = r.nseg
    assert w.wspr_synth_batch_device(three_signal_scene(al, nseg, -20.0), nseg, r.dI.data_ptr(), r.dQ.data_ptr(), 0, NOISE_SIGMA, SEED,
                                     w.SYNTH_NORMALISE) == 0
    calls = {"fill_ms": lambda: (r.pcm.fill_(1), torch.cuda.synchronize()), "iq_to_audio_ms": r.up, "audio_front_ms": r.down}
    times = {k: [] for k in calls}
    for rep in range(a.reps + 2):                                # two warm-up rounds: code objects, contexts, scratch
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            if rep >= 2:
                times[name].append((time.perf_counter() - t) * 1e3)
    # what the timed call wrote is what the checker says (records 0 and the last)
    same = True
    for s in (0, nseg - 1):
        rc, want, n = iq.check_rows(r.dI[s, :NS].cpu().numpy(), r.dQ[s, :NS].cpu().numpy())
        same = same and rc == 0 and bool(np.array_equal(r.pcm[s].cpu().numpy(), want[0])) and int(n[0]) == int(r.count[s])
    med = {k: float(np.median(v)) for k, v in times.items()}
    nbytes = 2 * NSAMP * nseg
    res = {"what": "host clock around each call (it returns when its stream is done), the calls taking turns in one loop; kernel "
                   "times from a kernel trace of a child process making the same calls",
           "nseg": nseg, "samples": NS, "reps": a.reps, "records_and_counts_equal_checker": same, "output_bytes": nbytes,
           "clipped_samples": int(r.count.sum()),
           "iq_to_audio_over_audio_front_call": med["iq_to_audio_ms"] / med["audio_front_ms"],
           "iq_to_audio_over_fill_call": med["iq_to_audio_ms"] / med["fill_ms"], "fill_bytes_per_s": nbytes / (med["fill_ms"] * 1e-3)}
    res.update(med)
    res.update({k + "_all": v for k, v in times.items()})
    try:
        if isinstance(kt, str):
            raise OSError(kt)
        kern = {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "launches": len(v)} for k, v in kt.items()}
        res["kernel_ms"] = kern
        if "iq_audio_kernel" in kern and "audio_front_kernel" in kern:
            k18, k12 = kern["iq_audio_kernel"]["ms_median"], kern["audio_front_kernel"]["ms_median"]
            res["k18_over_k12_kernel"] = k18 / k12
            res["goal_no_slower_than_k12_met"] = bool(k18 <= k12)
            res["k18_kernel_over_fill_call"] = k18 / med["fill_ms"]
            res["k18_kernel_bytes_per_s"] = nbytes / (k18 * 1e-3)
            res["k18_share_of_fp32_fma_rate"] = (nseg * NSAMP * FMA_PER_OUTPUT * 2.0) / (k18 * 1e-3) / (FP32_DATASHEET_TFLOPS * 1e12)
            res["fp32_bound_source"] = "data sheet: %.1f TFLOP/s fp32 vector counting a fused multiply-add as two; %d multiply-adds " \
                                       "per output sample is the definition's maximum" % (FP32_DATASHEET_TFLOPS, FMA_PER_OUTPUT)
    except OSError as e:
        res["kernel_ms"] = "not measured: the kernel trace failed (%s)" % e
    return res


def clipping(r):
    nseg = r.nseg
    tx = ten_signal_scene(nseg, np.random.default_rng(SEED + 1))
    assert w.wspr_synth_batch_device(tx, nseg, r.dI.data_ptr(), r.dQ.data_ptr(), 0, NOISE_SIGMA, SEED + 1, w.SYNTH_NORMALISE) == 0
    r.up()
    c = r.count.astype(np.int64)
    return {"what": "normalised ten-signal scenes (-10 .. -28 dB) at gain 32768", "scenes": nseg, "samples": int(nseg) * NSAMP,
            "clipped_samples": int(c.sum()), "clipped_share": float(c.sum()) / (float(nseg) * NSAMP), "records_with_a_clipped_sample": int((c > 0).sum()),
            "most_in_one_record": int(c.max())}


def found_share(dec, nseg, expected):
    found = false = 0
    for s in range(nseg):
        texts = [x.message.decode().strip() for x in dec.spots(s)]
        found += sum(m in texts for m in expected[s])
        false += sum(m not in expected[s] for m in texts)
    return found, false


def loop(r, al):
    nseg = r.nseg
    dec = w.BatchDecoder(nseg, 32)
    expected = [[al.expected_text(m) for m in al.SCENE_MESSAGES[s % 3]] for s in range(nseg)]
    points = []
    for snr in (-26.0, -29.0):
        assert w.wspr_synth_batch_device(three_signal_scene(al, nseg, snr), nseg, r.dI.data_ptr(), r.dQ.data_ptr(), 0, NOISE_SIGMA,
                                         SEED + 2, w.SYNTH_NORMALISE) == 0
        dec.decode_ptr(r.dI.data_ptr(), r.dQ.data_ptr(), NS, r.stride)
        direct, direct_false = found_share(dec, nseg, expected)
        r.up()
        r.down()
        dec.decode_ptr(r.bI.data_ptr(), r.bQ.data_ptr(), NS, r.stride)
        through, through_false = found_share(dec, nseg, expected)
        n = 3.0 * nseg
        p = (direct + through) / (2.0 * n)
        row = {"snr_db": snr, "scenes": nseg, "sent": 3 * nseg, "direct_decoded": direct, "direct_share": direct / n, "direct_false": direct_false,
               "loop_decoded": through, "loop_share": through / n, "loop_false": through_false, "clipped_samples": int(r.count.sum()),
               "binomial_sd_of_a_share": float(np.sqrt(p * (1.0 - p) / n))}
        print(json.dumps(row), flush=True)
        points.append(row)
    return points


def fading(r):
    nseg = r.nseg
    rng = np.random.default_rng(SEED + 3)
    tx = np.zeros(nseg, w.SYNTH_TX_DTYPE)
    expected = []
    for s in range(nseg):
        m = synth.message_wide(int(rng.integers(0, 1 << 62)))
        tx[s]["symbols"] = w.get_wspr_channel_symbols(m)[1]
        expected.append([synth.expected_text(m)])
    tx["seg"], tx["f0"], tx["t0"], tx["amp"] = np.arange(nseg), rng.uniform(-100.0, 100.0, nseg), 2.0 + rng.uniform(-1.0, 1.0, nseg), 10.0 ** (-28.0 / 20.0)
    ch = np.zeros(nseg, w.SYNTH_CHANNEL_DTYPE)
    ch["path"]["gain"][:, 0] = 1.0
    ch["path"]["sigma"][:, 0] = 0.1
    dec = w.BatchDecoder(nseg, 16)
    assert w.wspr_synth_faded_batch_device(tx, ch, nseg, r.dI.data_ptr(), r.dQ.data_ptr(), 0, NOISE_SIGMA, SEED + 3, w.SYNTH_NORMALISE) == 0
    dec.decode_ptr(r.dI.data_ptr(), r.dQ.data_ptr(), NS, r.stride)
    direct, direct_false = found_share(dec, nseg, expected)
    # the audio path: the faded signal alone at 375 Hz, up at the gain that makes a phasor of amplitude 10^(snr/20) a cosine at
    # `snr` dB over K17's noise (w.audio_amp), the noise added at 12 kHz, down through K12
    assert w.wspr_synth_faded_batch_device(tx, ch, nseg, r.dI.data_ptr(), r.dQ.data_ptr(), 0, 0.0, SEED + 3, 0) == 0
    r.up(w.audio_amp(0.0, AUDIO_SIGMA))
    clipped_up = int(r.count.sum())
    assert w.synth_audio_batch_device([], nseg, NSAMP, r.pcm.data_ptr(), NSAMP, 0, AUDIO_SIGMA, SEED + 4, w.SYNTH_ACCUMULATE, r.count) == 0
    r.down()
    dec.decode_ptr(r.bI.data_ptr(), r.bQ.data_ptr(), NS, r.stride)
    audio, audio_false = found_share(dec, nseg, expected)
    p = (direct + audio) / (2.0 * nseg)
    return {"what": "K13, one Rayleigh path of sigma 0.1 Hz at -28 dB (mean power), one signal per segment: decoded as generated "
                    "(noise at 375 Hz from K13) and through K13 without noise -> K18 -> K17 (accumulate, noise only) -> K12",
            "segments": nseg, "direct_decoded": direct, "direct_share": direct / nseg, "direct_false": direct_false,
            "audio_decoded": audio, "audio_share": audio / nseg, "audio_false": audio_false, "k18_gain": w.audio_amp(0.0, AUDIO_SIGMA),
            "audio_noise_sigma": AUDIO_SIGMA, "clipped_by_k18": clipped_up, "clipped_by_k17": int(r.count.sum()),
            "binomial_sd_of_a_share": float(np.sqrt(p * (1.0 - p) / nseg))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)      # under rocprofv3
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iq_audio.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.nseg)
    kt = None
    if not a.skip_cost:              # the traced child first: this process has not opened the device yet
        try:
            kt = kernel_times(a.nseg)
        except (subprocess.SubprocessError, OSError) as e:
            kt = type(e).__name__
    if w.lib().wspr_device_ready() != 1:
        sys.exit("iq_audio_ab: no usable HIP device (there is no CPU fallback)")
    import audio_lib as al
    import iq_audio_lib as iq
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "library": w.lib().wspr_mi355x_version().decode()}
    r = Rows(a.nseg, torch.device("cuda", 0), int(w.lib().wspr_iq_stride()))
    if not a.skip_cost:
        res["cost"] = cost(a, r, al, iq, kt)
        print(json.dumps({k: v for k, v in res["cost"].items() if not k.endswith("_all")}), flush=True)
    res["clipping"] = clipping(r)
    print(json.dumps(res["clipping"]), flush=True)
    if not a.skip_decode:
        res["loop"] = loop(r, al)
        res["fading"] = fading(r)
        print(json.dumps(res["fading"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
