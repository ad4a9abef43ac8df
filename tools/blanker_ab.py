#!/usr/bin/env python3
"""The impulse-noise blanker (K15) on an MI355X: what it costs and what it buys.

  python tools/blanker_ab.py [--nseg 2048] [--reps 7] [--scenes 256] [--out profiles/audio_blanker.json]

Cost, at the size the audio front end was written for (2 048 records of 1 440 000 samples, eight spiky scenes repeated):
wspr_audio_blank_batch_device() alone, a device-to-device copy of the same rows (it moves exactly the bytes K15 must move:
every sample read once and written once), wspr_audio_batch_device() (K12) alone on the same rows, and the fused call
wspr_audio_blanked_batch_device() against it -- the five taking turns inside one loop, so that they see the same clocks.
Every time is a host clock around a call that ends in the library's own wait for its stream (torch's copy: around a device
synchronise); the lab library's wspr_calib_copy16 (its own HIP events) over the same bytes stands beside the copy.

Benefit: the decoded share of the sent messages, blanker off and at (96, 4), on tests/blank_lib.py's spiky scenes (three
signals over noise, bursts of +-32767): --scenes scenes per point, burst rates 0, 10, 50, 200 per second of 3 samples and 50
per second of 30, signals at -20 and at -24 dB; the mean blanked share and the false spots of either path beside it.
SYNTHETIC SPIKES, not recorded static.  Nothing is asserted."""
import argparse
import concurrent.futures
import ctypes as C
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
POINTS = [(0, 3), (10, 3), (50, 3), (200, 3), (50, 30)]      # (bursts per second, samples per burst)
SNRS = [-20.0, -24.0]
SEED0 = 9100


def cost(a, dev, stride, al, bl):
    nseg = a.nseg
    distinct = np.stack([bl.dirty_scene(SEED0 + k, 50, 3) for k in range(8)])
    scenes = torch.from_numpy(distinct).to(dev)
    d_pcm = scenes[torch.arange(nseg, device=dev) % 8].contiguous()
    d_out = torch.empty_like(d_pcm)
    dI = torch.empty((nseg, stride), dtype=torch.float32, device=dev)
    dQ = torch.empty((nseg, stride), dtype=torch.float32, device=dev)
    count = np.zeros(nseg, np.int32)
    w.sync_torch()

    def check(rc):
        assert rc == 0, rc

    calls = {
        "blank_ms": lambda: check(w.audio_blank_batch_device(d_pcm.data_ptr(), NSAMP, NSAMP, nseg, bl.THR, bl.GUARD,
                                                             d_out.data_ptr(), NSAMP, count)),
        "copy_ms": lambda: (d_out.copy_(d_pcm), torch.cuda.synchronize()),
        "front_end_ms": lambda: check(w.audio_batch_device(d_pcm.data_ptr(), NSAMP, NSAMP, nseg, dI.data_ptr(), dQ.data_ptr(), 0)),
        "fused_ms": lambda: check(w.audio_blanked_batch_device(d_pcm.data_ptr(), NSAMP, NSAMP, nseg, bl.THR, bl.GUARD,
                                                               dI.data_ptr(), dQ.data_ptr(), 0, count)),
    }
    times = {k: [] for k in calls}
    for rep in range(a.reps + 2):                                # two warm-up rounds: code objects, contexts, scratch rows
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            if rep >= 2:
                times[name].append((time.perf_counter() - t) * 1e3)
    # what the timed calls wrote is what the checker says (the eight distinct records; the rest repeat them)
    calls["blank_ms"]()
    want, n = bl.check_rows(distinct, NSAMP, bl.THR, bl.GUARD)
    same = bool(np.array_equal(d_out[:8].cpu().numpy(), want) and count[:8].tolist() == n.tolist())
    nbytes = 2 * 2 * NSAMP * nseg                                # every sample read once and written once
    lab = w.lab()
    nfloats = (nbytes // 2 // 4) & ~3
    ms16 = C.c_double(0.0)
    for _ in range(2):
        lab.wspr_calib_copy16(d_pcm.data_ptr(), d_out.data_ptr(), nfloats, 5, 0, C.byref(ms16))
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {
        "what": "host clock around each call (it returns when its stream is done), the calls taking turns in one loop",
        "nseg": nseg, "nsamp": NSAMP, "reps": a.reps, "settings": [bl.THR, bl.GUARD],
        "rows_and_counts_equal_checker": same,
        "mean_blanked_share": float(count.mean() / NSAMP),
        "bytes_moved_by_blanker_or_copy": nbytes,
        "blank_bytes_per_s": nbytes / (med["blank_ms"] * 1e-3), "copy_bytes_per_s": nbytes / (med["copy_ms"] * 1e-3),
        "calib_copy16_ms": ms16.value,
        "blank_over_copy": med["blank_ms"] / med["copy_ms"], "blank_over_copy_target": 1.5,
        "blank_over_calib_copy16": med["blank_ms"] / ms16.value if ms16.value else None,
        "blank_over_front_end": med["blank_ms"] / med["front_end_ms"],
        "fused_over_front_end": med["fused_ms"] / med["front_end_ms"],
        "fused_minus_front_end_ms": med["fused_ms"] - med["front_end_ms"],
    }
    res.update(med)
    res.update({k + "_all": v for k, v in times.items()})
    return res


def benefit(a, dev, stride, al, bl):
    n = a.scenes
    dI = torch.empty((n, stride), dtype=torch.float32, device=dev)
    dQ = torch.empty((n, stride), dtype=torch.float32, device=dev)
    dec = w.BatchDecoder(n, 32)
    points = []
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        for snr in SNRS:
            sent = [al.expected_text(m) for m, _, _, _ in bl.dirty_items(snr)]
            for rate, blen in POINTS:
                recs = list(pool.map(lambda k: bl.dirty_scene(SEED0 + k, rate, blen, snr), range(n)))
                d_pcm = torch.from_numpy(np.stack(recs)).to(dev)
                count = np.zeros(n, np.int32)
                w.sync_torch()
                row = {"snr_db": snr, "bursts_per_s": rate, "burst_samples": blen, "scenes": n, "sent": 3 * n}
                for path in ("off", "on"):
                    if path == "on":
                        rc = w.audio_blanked_batch_device(d_pcm.data_ptr(), NSAMP, NSAMP, n, bl.THR, bl.GUARD, dI.data_ptr(),
                                                          dQ.data_ptr(), 1, count)
                    else:
                        rc = w.audio_batch_device(d_pcm.data_ptr(), NSAMP, NSAMP, n, dI.data_ptr(), dQ.data_ptr(), 1)
                    assert rc == 0, rc
                    dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NOUT, stride)
                    found = false = 0
                    for s in range(n):
                        texts = [x.message.decode().strip() for x in dec.spots(s)]
                        found += sum(t in texts for t in sent)
                        false += sum(t not in sent for t in texts)
                    row["decoded_" + path] = found
                    row["decoded_share_" + path] = found / (3.0 * n)
                    row["false_spots_" + path] = false
                row["mean_blanked_share"] = float(count.mean() / NSAMP)
                print(json.dumps(row), flush=True)
                points.append(row)
                del d_pcm
    return points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-benefit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_blanker.json"))
    a = ap.parse_args()
    if w.lib().wspr_device_ready() != 1:
        sys.exit("blanker_ab: no usable HIP device (there is no CPU fallback)")
    import audio_lib as al
    import blank_lib as bl
    dev = torch.device("cuda", 0)
    stride = int(w.lib().wspr_iq_stride())
    res = {"device": torch.cuda.get_device_name(0),
           "spikes": "synthetic (tests/blank_lib.py dirty_scene: bursts of +-32767), not recorded static"}
    if not a.skip_cost:
        res["cost"] = cost(a, dev, stride, al, bl)
        print(json.dumps(res["cost"]), flush=True)
        w.lib().wspr_release_buffers()
    if not a.skip_benefit:
        res["benefit"] = benefit(a, dev, stride, al, bl)
    # (the committed record also holds `bench_py`: bench.py's line and spot records on this commit and on its parent, added
    # by hand from runs of bench.py itself)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
