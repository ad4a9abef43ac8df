#!/usr/bin/env python3
"""Decode probability against SNR, generated (K8, wspr_synth_batch_device) and decoded on the device.

Per SNR point (default -34 .. -20 dB in 1 dB steps, the project's convention of tests/synth.py: sigma^2 per rail =
(375/2500)/2, amplitude 10^(SNR/20), normalised to a peak of 0.5): --segments segments (default 8 192), one
synth.message_wide signal each, f0 uniform in +-100 Hz, t0 = 2 +- 1 s, drift 0; the SAME rows are decoded in the exact
and in the contracted arithmetic (wspr_set_arithmetic).  Recorded per point and mode: the decoded share, the false
decodes (spots whose text was not sent), and how many segments' spot lists differ between the modes at all (any of
message, frequency, dt, SNR, drift, sync, cycles); per mode the linearly interpolated 50 % and 90 % points.  Nothing is asserted:
nobody has measured this curve before, the record is the deliverable.

One sanity line: the -20 dB point next to the decoded share of bench.py's configs[1] batch (its own torch generator,
1 024 x 1 signal at -20 dB -- what `bench.py --config 2 --full` reports as decoded_ok), decoded in the same session.

    python tools/sensitivity.py [--segments 8192] [--out profiles/sensitivity.json]
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

import bench            # noqa: E402
import rtlsdr_wsprd_amd as w   # noqa: E402
import synth            # noqa: E402

NS = 45000


def crossing(snrs, shares, level):
    """SNR at which the share first reaches `level`, linear between the two points around it (None if it never does)."""
    for k in range(1, len(snrs)):
        a, b = shares[k - 1], shares[k]
        if a < level <= b:
            return snrs[k - 1] + (level - a) / (b - a) * (snrs[k] - snrs[k - 1])
    return snrs[0] if shares and shares[0] >= level else None


def count(dec, expected, nseg):
    ok = sum(expected[s] in {x.message.decode() for x in dec.spots(s)} for s in range(nseg))
    false = sum(x.message.decode() != expected[s] for s in range(nseg) for x in dec.spots(s))
    return ok, false


def spot_lists(dec, nseg):
    return [[(x.message, x.freq, x.dt, x.snr, x.drift, x.sync, x.cycles, x.jitter) for x in dec.spots(s)] for s in range(nseg)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=8192)
    ap.add_argument("--snr-lo", type=int, default=-34)
    ap.add_argument("--snr-hi", type=int, default=-20)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensitivity.json"))
    args = ap.parse_args()
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
    dec = w.BatchDecoder(nseg, 16)
    snrs = list(range(args.snr_lo, args.snr_hi + 1))
    points = []
    for p, snr in enumerate(snrs):
        tx = np.zeros(nseg, w.SYNTH_TX_DTYPE)
        tx["seg"] = np.arange(nseg)
        tx["f0"] = rng.uniform(-100.0, 100.0, nseg)
        tx["t0"] = 2.0 + rng.uniform(-1.0, 1.0, nseg)
        tx["amp"] = 10.0 ** (snr / 20.0)
        expected = []
        for s in range(nseg):
            m = synth.message_wide(int(rng.integers(0, 1 << 62)))
            tx["symbols"][s] = w.get_wspr_channel_symbols(m)[1]
            expected.append(synth.expected_text(m))
        t = time.perf_counter()
        rc = w.wspr_synth_batch_device(tx, nseg, dI.data_ptr(), dQ.data_ptr(), p * nseg, sigma, args.seed, w.SYNTH_NORMALISE)
        gen_ms = 1e3 * (time.perf_counter() - t)
        assert rc == 0
        rec = {"snr_db": snr, "segments": nseg, "generate_ms": gen_ms}
        if p == 0:
            dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)      # untimed: the first call sizes the work buffers
        lists = {}
        for name, mode in (("exact", 0), ("contracted", 1)):
            w.wspr_set_arithmetic(mode)
            t = time.perf_counter()
            dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)
            ms = 1e3 * (time.perf_counter() - t)
            ok, false = count(dec, expected, nseg)
            rec[name] = {"decoded": ok, "share": ok / nseg, "false_decodes": false, "decode_ms": ms}
            lists[name] = spot_lists(dec, nseg)
        w.wspr_set_arithmetic(0)
        rec["segments_whose_spots_differ_between_modes"] = sum(a != b for a, b in zip(lists["exact"], lists["contracted"]))
        rec["segments_whose_messages_differ_between_modes"] = sum(
            sorted(t[0] for t in a) != sorted(t[0] for t in b) for a, b in zip(lists["exact"], lists["contracted"]))
        print("SNR %3d dB: exact %5d/%d (%d false)   contracted %5d/%d (%d false)   %d segments differ (%d in their messages)   "
              "generate %.1f ms, decode %.0f / %.0f ms"
              % (snr, rec["exact"]["decoded"], nseg, rec["exact"]["false_decodes"], rec["contracted"]["decoded"], nseg,
                 rec["contracted"]["false_decodes"], rec["segments_whose_spots_differ_between_modes"],
                 rec["segments_whose_messages_differ_between_modes"], gen_ms, rec["exact"]["decode_ms"],
                 rec["contracted"]["decode_ms"]), flush=True)
        points.append(rec)

    # sanity: bench.py's own configs[1] batch (torch generator) at -20 dB, decoded here and now
    bI, bQ, bexp = bench.synth_batch_gpu(1024, 1234, dev)
    bdec = w.BatchDecoder(1024, 16)
    bdec.decode(bI, bQ)
    b_ok = sum(bexp[s][0] in {x.message.decode() for x in bdec.spots(s)} for s in range(1024))
    last = points[-1]["exact"]["share"] if snrs[-1] == -20 else None
    out = {
        "what": "decode probability against SNR in 2500 Hz, one signal per segment, generated by wspr_synth_batch_device() "
                "and decoded by wspr_decode_batch_device() without the IQ visiting the host; nothing asserted",
        "device": torch.cuda.get_device_name(0), "library": L.wspr_mi355x_version().decode(),
        "scene": {"segments_per_point": nseg, "sigma_per_rail": sigma, "f0_hz": "uniform +-100", "t0_s": "2 +- 1 uniform",
                  "drift": 0, "messages": "synth.message_wide", "normalised": True, "seed": args.seed,
                  "options": "npasses 2, subtraction 1, quickmode 0, usehashtable 0"},
        "points": points,
        "snr_at_50_percent": {m: crossing(snrs, [q[m]["share"] for q in points], 0.5) for m in ("exact", "contracted")},
        "snr_at_90_percent": {m: crossing(snrs, [q[m]["share"] for q in points], 0.9) for m in ("exact", "contracted")},
        "sanity_minus_20_db": {"this_tool_exact_share": last, "bench_configs1_batch_decoded": "%d/1024" % b_ok,
                               "bench_configs1_share": b_ok / 1024.0,
                               "gap": None if last is None else abs(last - b_ok / 1024.0)},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("snr_at_50_percent", "snr_at_90_percent", "sanity_minus_20_db")}))


if __name__ == "__main__":
    main()
