#!/usr/bin/env python3
"""Decode probability against SNR with the ordered-statistics rescue stage (wspr_set_osd_depth) and a primed hash memory.

tools/sensitivity.py's experiment on a receiver that has heard its stations before: the scenes' type-1 messages are drawn
from 512 callsigns, all written to hashtable.txt through wspr_hash_commit() before every decode, and the rows are decoded
with usehashtable = 1.  Per SNR point (default -34 .. -26 dB in 1 dB steps; the project's convention of tests/synth.py:
sigma^2 per rail = (375/2500)/2, amplitude 10^(SNR/20), normalised to a peak of 0.5): --segments segments, one signal
each, f0 uniform in +-100 Hz, t0 = 2 +- 1 s, drift 0; the SAME rows are decoded at depth -1 (off), 1, 2 and 3.  One more
point holds noise only.  Recorded per point and depth: decoded (the sent text is among the segment's spots), false (spots
whose text was not sent), the spots the stage contributed (cycles == 0), and from wspr_last_timings() the stage's
milliseconds [26], the vectors it tried [27] and the results its gate accepted [28], beside the call's wall time.
Nothing is asserted: it is a record.

The working directory of the run is a scratch directory (hashtable.txt lives there), removed afterwards.

    python tools/osd_sensitivity.py [--segments 2048] [--out profiles/osd_sensitivity.json]
"""
import argparse
import ctypes as C
import json
import os
import shutil
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
DEPTHS = (-1, 1, 2, 3)
HASH_OP = np.dtype([("seg", "<i4"), ("slot", "<i4"), ("kind", "<i4"), ("call", "S13"), ("grid", "S5"), ("pad", "S2")])
assert HASH_OP.itemsize == 32


def prime(L, calls):
    """hashtable.txt of the working directory := exactly these calls (type-1 stores through wspr_hash_commit)."""
    if os.path.exists("hashtable.txt"):
        os.remove("hashtable.txt")
    ops = np.zeros(len(calls), HASH_OP)
    for k, c in enumerate(calls):
        ops[k] = (0, L.nhash(c.encode(), len(c), 146), 1, c.encode(), b"AA00", b"")
    L.wspr_hash_commit.argtypes = [C.c_void_p, C.c_int]
    assert L.wspr_hash_commit(ops.ctypes.data, len(calls)) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=2048)
    ap.add_argument("--snr-lo", type=int, default=-34)
    ap.add_argument("--snr-hi", type=int, default=-26)
    ap.add_argument("--calls", type=int, default=512)
    ap.add_argument("--seed", type=int, default=20261017)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "osd_sensitivity.json"))
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
    calls = []
    while len(calls) < args.calls:                         # distinct calls, distinct slots
        c = synth.message_wide(int(rng.integers(0, 1 << 62))).split()[0]
        if c not in calls and L.nhash(c.encode(), len(c), 146) not in {L.nhash(x.encode(), len(x), 146) for x in calls}:
            calls.append(c)
    dI = torch.zeros(nseg, stride, device=dev)
    dQ = torch.zeros(nseg, stride, device=dev)
    w.sync_torch()
    opt = w.default_options()
    opt.usehashtable = 1
    dec = w.BatchDecoder(nseg, 16, opt)
    scratch = tempfile.mkdtemp(prefix="osd_sensitivity_")
    cwd = os.getcwd()
    os.chdir(scratch)
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
                _, grid, pwr = synth.message_wide(int(rng.integers(0, 1 << 62))).split()
                m = "%s %s %s" % (calls[int(rng.integers(0, len(calls)))], grid, pwr)
                tx["symbols"][s] = w.get_wspr_channel_symbols(m)[1]
                expected.append(synth.expected_text(m))
            assert w.wspr_synth_batch_device(tx, nseg, dI.data_ptr(), dQ.data_ptr(), p * nseg, sigma, args.seed,
                                             w.SYNTH_NORMALISE) == 0
            rec = {"snr_db": snr, "segments": nseg}
            if p == 0:
                prime(L, calls)
                dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)      # untimed: the first call sizes the work buffers
            for depth in DEPTHS:
                prime(L, calls)
                w.set_osd_depth(depth)
                t = time.perf_counter()
                dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)
                ms = 1e3 * (time.perf_counter() - t)
                tm = w.last_timings()
                texts = [[x.message.decode() for x in dec.spots(s)] for s in range(nseg)]
                ok = 0 if snr is None else sum(expected[s] in texts[s] for s in range(nseg))
                false = sum(m != expected[s] or snr is None for s in range(nseg) for m in texts[s])
                rec["depth_%d" % depth] = {
                    "decoded": ok, "share": ok / nseg, "false": false,
                    "osd_spots": sum(x.cycles == 0 for s in range(nseg) for x in dec.spots(s)),
                    "osd_ms": tm["osd_ms"], "osd_vectors": int(tm["osd_vectors"]), "osd_accepted": int(tm["osd_spots"]),
                    "decode_ms": ms}
            w.set_osd_depth(-1)
            print("SNR %s dB: " % ("none" if snr is None else "%4d" % snr) + "   ".join(
                "d%d %d/%d (%d false, K9 %.1f ms for %d)" % (d, rec["depth_%d" % d]["decoded"], nseg, rec["depth_%d" % d]["false"],
                                                          rec["depth_%d" % d]["osd_ms"], rec["depth_%d" % d]["osd_vectors"])
                for d in DEPTHS), flush=True)
            points.append(rec)
    finally:
        w.set_osd_depth(-1)
        os.chdir(cwd)
        shutil.rmtree(scratch, ignore_errors=True)
    out = {
        "what": "decode probability against SNR in 2500 Hz with the ordered-statistics rescue stage, one signal per segment "
                "whose callsign is one of %d in a primed hashtable.txt; generated by wspr_synth_batch_device() and decoded "
                "by wspr_decode_batch_device() with usehashtable = 1; the last point is noise alone; nothing asserted"
                % len(calls),
        "device": torch.cuda.get_device_name(0), "library": L.wspr_mi355x_version().decode(),
        "scene": {"segments_per_point": nseg, "sigma_per_rail": sigma, "f0_hz": "uniform +-100", "t0_s": "2 +- 1 uniform",
                  "drift": 0, "calls": len(calls), "normalised": True, "seed": args.seed,
                  "options": "npasses 2, subtraction 1, quickmode 0, usehashtable 1"},
        "depths": list(DEPTHS),
        "points": points,
    }
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(out_path, ROOT), "points": len(points)}))


if __name__ == "__main__":
    main()
