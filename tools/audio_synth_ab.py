#!/usr/bin/env python3
"""The 12 kHz audio scene synthesiser (K17) on an MI355X: what a batch of audio scenes costs, and a first decode-probability
figure through the audio path.

  python tools/audio_synth_ab.py [--nseg 2048] [--reps 7] [--out profiles/audio_synth.json]

Cost, at the size the audio front end was written for (2 048 records of 1 440 000 samples, three transmissions each, over
noise): wspr_synth_audio_batch_device() alone; a device fill of the same output bytes (the memory floor: every sample
written once); wspr_synth_batch_device() (K8) on the same scene at 375 Hz -- the three taking turns inside one loop, so that
they see the same clocks.  Every time is a host clock around a call that ends in the library's own wait for its stream
(torch's fill: around a device synchronise).  From the times come the shares of the fp64 vector rate for code that may not
fuse (half of the data sheet's figure, which counts a fused multiply-add as two) that the two calls reach by their
definitions' counts: 53 double operations per transmission sample for K17, 54 for K8.  K8's share in the same run is the
yardstick for K17's; no target is set.  One record of tests/audio_lib.py's audio_scene() on the host stands beside them.

Then the decoded share of the sent messages at two SNRs, K17 -> K12 -> decoder on --nseg scenes each, without a sample
leaving the device.  Nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rtlsdr_wsprd_amd as w  # noqa: E402

NSAMP = 1440000
NOUT = 45000
SIGLEN_AUDIO = 162 * 8192
SIGLEN_IQ = 162 * 256
OPS_K17, OPS_K8 = 53, 54                     # double operations per transmission sample (k17_audio_synth.hip, k8_synth.hip)
FP64_DATASHEET_TFLOPS = 78.6
SNRS = [-26.0, -29.0]
SEED = 8100


def scene_list(al, nseg, amp, first_of, siglen, nout):
    """(SYNTH_TX_DTYPE array, transmission samples inside the rows): audio_lib's three signals in every segment, the messages
    of its three scenes in turn."""
    tx = np.zeros(3 * nseg, w.SYNTH_TX_DTYPE)
    syms = [[w.get_wspr_channel_symbols(m)[1] for m in msgs] for msgs in al.SCENE_MESSAGES]
    inside = 0
    for s in range(nseg):
        for j, (_, f0, t0) in enumerate(al.SIGNALS):
            r = tx[3 * s + j]
            r["seg"], r["f0"], r["t0"], r["amp"], r["drift"] = s, f0, t0, amp, 0.0
            r["symbols"] = syms[s % 3][j]
            first = first_of(t0)
            inside += max(0, min(nout, first + siglen) - max(0, first))
    return tx, inside


def cost(a, dev, stride, al, asl):
    nseg = a.nseg
    sigma = asl.SIGMA
    tx_audio, in_audio = scene_list(al, nseg, w.audio_amp(-20.0, sigma), lambda t0: int(np.floor(float(np.float32(t0)) * 12000.0)),
                                    SIGLEN_AUDIO, NSAMP)
    # the same scene at 375 Hz: complex noise of unit power per 375 Hz, the signal at the same SNR in 2 500 Hz
    sigma_iq = float(np.sqrt(0.5))
    amp_iq = float(np.sqrt(375.0 / 2500.0) * 10.0 ** (-20.0 / 20.0))
    tx_iq, in_iq = scene_list(al, nseg, amp_iq, lambda t0: int(np.floor(float(np.float32(t0)) / (1 / 375.0))), SIGLEN_IQ, NOUT)
    d_pcm = torch.empty((nseg, NSAMP), dtype=torch.int16, device=dev)
    dI = torch.empty((nseg, stride), dtype=torch.float32, device=dev)
    dQ = torch.empty((nseg, stride), dtype=torch.float32, device=dev)
    count = np.zeros(nseg, np.int32)
    w.sync_torch()

    def check(rc):
        assert rc == 0, rc

    calls = {
        "fill_ms": lambda: (d_pcm.fill_(1), torch.cuda.synchronize()),
        "synth_iq_ms": lambda: check(w.wspr_synth_batch_device(tx_iq, nseg, dI.data_ptr(), dQ.data_ptr(), 0, sigma_iq, SEED, 0)),
        "synth_audio_ms": lambda: check(w.synth_audio_batch_device(tx_audio, nseg, NSAMP, d_pcm.data_ptr(), NSAMP, 0, sigma, SEED, 0,
                                                                   count)),
    }
    times = {k: [] for k in calls}
    for rep in range(a.reps + 2):                                # two warm-up rounds: code objects, contexts, scratch
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            if rep >= 2:
                times[name].append((time.perf_counter() - t) * 1e3)
    # what the timed call wrote is what the checker says (records 0, 1 and the last; the others differ in their noise alone)
    rows = d_pcm[[0, 1, nseg - 1]].cpu().numpy()
    same = True
    for r, s in enumerate((0, 1, nseg - 1)):
        items = [(0, float(x["f0"]), float(x["t0"]), float(x["amp"]), 0.0, x["symbols"]) for x in tx_audio[3 * s:3 * s + 3]]
        rc, want, n = asl.check_batch(items, 1, NSAMP, seg_index0=s, sigma=sigma, seed=SEED)
        same = same and rc == 0 and bool(np.array_equal(rows[r], want[0, :NSAMP])) and int(n[0]) == int(count[s])
    t = time.perf_counter()
    al.audio_scene(al.scene_items(0), 1)
    host_ms = (time.perf_counter() - t) * 1e3
    med = {k: float(np.median(v)) for k, v in times.items()}
    bound = FP64_DATASHEET_TFLOPS * 0.5e12
    nbytes = 2 * NSAMP * nseg
    res = {
        "what": "host clock around each call (it returns when its stream is done), the calls taking turns in one loop",
        "nseg": nseg, "nsamp": NSAMP, "transmissions_per_record": 3, "reps": a.reps, "noise_sigma": sigma,
        "records_and_counts_equal_checker": same, "clipped_samples": int(count.sum()),
        "output_bytes": nbytes,
        "synth_audio_bytes_per_s": nbytes / (med["synth_audio_ms"] * 1e-3), "fill_bytes_per_s": nbytes / (med["fill_ms"] * 1e-3),
        "synth_audio_over_fill": med["synth_audio_ms"] / med["fill_ms"],
        "records_per_s": nseg / (med["synth_audio_ms"] * 1e-3),
        "host_audio_scene_ms_per_record": host_ms,
        "host_audio_scene_over_synth_audio_per_record": host_ms / (med["synth_audio_ms"] / nseg),
        "fp64": {
            "bound_double_ops_per_s": bound,
            "bound_source": "data sheet: %.1f TFLOP/s fp64 vector counting a fused multiply-add as two; unfused code issues at "
                            "most half of it; no measured fp64 figure exists for this part" % FP64_DATASHEET_TFLOPS,
            "k17_transmission_samples": in_audio, "k17_double_ops_per_sample": OPS_K17,
            "k17_share_of_unfused_bound": in_audio * OPS_K17 / (med["synth_audio_ms"] * 1e-3) / bound,
            "k8_transmission_samples": in_iq, "k8_double_ops_per_sample": OPS_K8,
            "k8_share_of_unfused_bound": in_iq * OPS_K8 / (med["synth_iq_ms"] * 1e-3) / bound,
            "note": "whole calls (list upload, phase kernel, fill kernel, wait), not kernels alone; the noise draws (one per two "
                    "audio samples, one per IQ sample) are not counted on either side",
        },
    }
    res.update(med)
    res.update({k + "_all": v for k, v in times.items()})
    del d_pcm, dI, dQ
    return res


def decode_share(a, dev, stride, al, asl):
    n = a.nseg
    sigma = asl.SIGMA
    d_pcm = torch.empty((n, NSAMP), dtype=torch.int16, device=dev)
    dI = torch.empty((n, stride), dtype=torch.float32, device=dev)
    dQ = torch.empty((n, stride), dtype=torch.float32, device=dev)
    dec = w.BatchDecoder(n, 32)
    count = np.zeros(n, np.int32)
    w.sync_torch()
    points = []
    for snr in SNRS:
        tx, _ = scene_list(al, n, w.audio_amp(snr, sigma), lambda t0: 0, 0, 0)
        t = time.perf_counter()
        assert w.synth_audio_batch_device(tx, n, NSAMP, d_pcm.data_ptr(), NSAMP, 0, sigma, SEED + 1, 0, count) == 0
        t_synth = time.perf_counter()
        assert w.audio_batch_device(d_pcm.data_ptr(), NSAMP, NSAMP, n, dI.data_ptr(), dQ.data_ptr(), 1) == 0
        t_front = time.perf_counter()
        dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NOUT, stride)
        t_dec = time.perf_counter()
        found = false = 0
        for s in range(n):
            sent = [al.expected_text(m) for m in al.SCENE_MESSAGES[s % 3]]
            texts = [x.message.decode().strip() for x in dec.spots(s)]
            found += sum(m in texts for m in sent)
            false += sum(m not in sent for m in texts)
        row = {"snr_db": snr, "scenes": n, "sent": 3 * n, "decoded": found, "decoded_share": found / (3.0 * n), "false_spots": false,
               "clipped_samples": int(count.sum()), "synth_audio_ms": (t_synth - t) * 1e3, "front_end_ms": (t_front - t_synth) * 1e3,
               "decode_ms": (t_dec - t_front) * 1e3}
        print(json.dumps(row), flush=True)
        points.append(row)
    return points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_synth.json"))
    a = ap.parse_args()
    if w.lib().wspr_device_ready() != 1:
        sys.exit("audio_synth_ab: no usable HIP device (there is no CPU fallback)")
    import audio_lib as al
    import audio_synth_lib as asl
    dev = torch.device("cuda", 0)
    stride = int(w.lib().wspr_iq_stride())
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.skip_cost:
        res["cost"] = cost(a, dev, stride, al, asl)
        print(json.dumps(res["cost"]), flush=True)
        w.lib().wspr_release_buffers()
        torch.cuda.empty_cache()
    if not a.skip_decode:
        res["decode_share"] = decode_share(a, dev, stride, al, asl)
    # (the committed record also holds `checker_vs_numpy` and `bench_py`: the flip counts of tests/test_audio_synth_checker.py
    # and bench.py's spot records on this commit and on its parent, added by hand from those runs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
