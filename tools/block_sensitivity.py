#!/usr/bin/env python3
"""Decode probability against SNR with the noncoherent block-detection stage (wspr_set_block_detection).

tools/sensitivity.py's experiment with the stage off and on.  Per SNR point (default -34 .. -24 dB in 1 dB steps; the
project's convention of tests/synth.py: sigma^2 per rail = (375/2500)/2, amplitude 10^(SNR/20), normalised to a peak of
0.5): --segments segments (default 2 048), one synth.message_wide signal each, f0 uniform in +-100 Hz, t0 = 2 +- 1 s,
drift 0, generated on the device (K8); the SAME rows are decoded with maxblock 1 (off), 2 and 3 under the default decoder
options.  One more point holds noise only.  Recorded per point and setting: decoded (the sent text is among the
segment's spots), false (spots whose text was not sent), and from wspr_last_timings() the stage's milliseconds [32], the
vectors it sent to Fano [33] and its decodes at block size 2 [34] and 3 [35], beside the call's wall time.  Nothing is
asserted: it is a record.

    python tools/block_sensitivity.py [--segments 2048] [--out profiles/block_sensitivity.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np      # noqa: E402
import torch            # noqa: E402  (before the library: see tests/conftest.py)

import rtlsdr_wsprd_amd as w   # noqa: E402
import synth            # noqa: E402

NS = 45000
MAXBLOCKS = (1, 2, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=2048)
    ap.add_argument("--snr-lo", type=int, default=-34)
    ap.add_argument("--snr-hi", type=int, default=-24)
    ap.add_argument("--seed", type=int, default=20261018)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_sensitivity.json"))
    args = ap.parse_args()
    out_path = os.path.abspath(args.out)
    L = w.lib()
    assert L.wspr_device_ready() == 1
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nseg = args.segments
    stride = int(L.wspr_iq_stride())
    sigma = float(np.float32(np.sqrt((375.0 / 2500.0) / 2.0)))
    rng = np.random.default_rng(args.seed)
    dI = torch.zeros(nseg, stride, device=dev)
    dQ = torch.zeros(nseg, stride, device=dev)
    w.sync_torch()
    dec = w.BatchDecoder(nseg, 16, w.default_options())
    points = []
    try:
        snrs = list(range(args.snr_lo, args.snr_hi + 1)) + [None]      # None: the noise-only point
        for p, snr in enumerate(snrs):
            tx = np.zeros(nseg, w.SYNTH_TX_DTYPE)
            tx["seg"] = np.arange(nseg)
            tx["f0"] = rng.uniform(-100.0, 100.0, nseg)
            tx["t0"] = 2.0 + rng.uniform(-1.0, 1.0, nseg)
            tx["amp"] = 0.0 if snr is None else 10.0 ** (snr / 20.0)
            expected = []
            for s in range(nseg):
                m = synth.message_wide(int(rng.integers(0, 1 << 62)))
                tx["symbols"][s] = w.get_wspr_channel_symbols(m)[1]
                expected.append(synth.expected_text(m))
            assert w.wspr_synth_batch_device(tx, nseg, dI.data_ptr(), dQ.data_ptr(), p * nseg, sigma, args.seed,
                                             w.SYNTH_NORMALISE) == 0
            rec = {"snr_db": snr, "segments": nseg}
            if p == 0:
                dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)      # untimed: the first call sizes the work buffers
            for mb in MAXBLOCKS:
                w.set_block_detection(mb)
                t = time.perf_counter()
                dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)
                ms = 1e3 * (time.perf_counter() - t)
                tm = w.last_timings()
                texts = [[x.message.decode() for x in dec.spots(s)] for s in range(nseg)]
                ok = 0 if snr is None else sum(expected[s] in texts[s] for s in range(nseg))
                false = sum(m != expected[s] or snr is None for s in range(nseg) for m in texts[s])
                rec["maxblock_%d" % mb] = {
                    "decoded": ok, "share": ok / nseg, "false": false,
                    "block_ms": tm["block_ms"], "block_vectors": int(tm["block_vectors"]),
                    "block2_decodes": int(tm["block2_decodes"]), "block3_decodes": int(tm["block3_decodes"]),
                    "decode_ms": ms}
            w.set_block_detection(1)
            print("SNR %s dB: " % ("none" if snr is None else "%4d" % snr) + "   ".join(
                "B%d %d/%d (%d false, stage %.0f ms, %d vectors)" % (
                    mb, rec["maxblock_%d" % mb]["decoded"], nseg, rec["maxblock_%d" % mb]["false"],
                    rec["maxblock_%d" % mb]["block_ms"], rec["maxblock_%d" % mb]["block_vectors"]) for mb in MAXBLOCKS), flush=True)
            points.append(rec)
            # the record as far as it has come: a run that is cut short still leaves its points
            write(out_path, L, nseg, sigma, args.seed, points)
    finally:
        w.set_block_detection(1)
    print(json.dumps({"written": os.path.relpath(out_path, ROOT), "points": len(points)}))


def write(out_path, L, nseg, sigma, seed, points):
    out = {
        "what": "decode probability against SNR in 2500 Hz with the noncoherent block-detection stage off (maxblock 1) and "
                "on (2, 3), one signal per segment; generated by wspr_synth_batch_device() and decoded by "
                "wspr_decode_batch_device() under the default options; the last point is noise alone; nothing asserted",
        "device": torch.cuda.get_device_name(0), "library": L.wspr_mi355x_version().decode(),
        "scene": {"segments_per_point": nseg, "sigma_per_rail": sigma, "f0_hz": "uniform +-100", "t0_s": "2 +- 1 uniform",
                  "drift": 0, "normalised": True, "seed": seed, "options": "npasses 2, subtraction 1, quickmode 0, usehashtable 0"},
        "maxblocks": list(MAXBLOCKS),
        "points": points,
    }
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
