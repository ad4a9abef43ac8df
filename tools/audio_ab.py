#!/usr/bin/env python3
"""The audio front end (K12) at the size it was written for, on an MI355X: one call of wspr_audio_batch_device() over
2 048 records of 1 440 000 samples, next to a plain device copy and next to one decode of the rows it produced.

  python tools/audio_ab.py [--nseg 2048] [--reps 7] [--out profiles/audio_frontend.json]

Every time is a host clock around a call that ends in the library's own wait for its stream (the product library has no
event-timed form of the call; at 5.9 GB per call the wait's granularity is far below the call).  The kernel's traffic and
arithmetic are counted from the shapes: bytes = nseg * (2 * nsamp + 2 * 4 * stride), multiply-adds = nseg * n_out * 2 * 511
by the definition (the kernel skips the quarter whose tap is an exact zero; the definition's count is the one reported, the
executed count beside it).  The copy is the lab library's wspr_calib_copy (4 bytes per lane) and wspr_calib_copy16 (16 bytes
per lane, its own HIP events) over as many bytes as the front end moves.  Peak: 256 CUs x 4 SIMDs x 32 packed multiply-adds
per clock at 2.4 GHz = 78.6e12 multiply-adds per second."""
import argparse
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
PEAK_FMA_PER_S = 256 * 4 * 32 * 2.4e9


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_frontend.json"))
    a = ap.parse_args()
    if w.lib().wspr_device_ready() != 1:
        sys.exit("audio_ab: no usable HIP device (there is no CPU fallback)")
    import audio_lib as al
    dev = torch.device("cuda", 0)
    stride = int(w.lib().wspr_iq_stride())
    nseg = a.nseg
    # records: the three test scenes, repeated (three decodable signals per record)
    scenes = torch.from_numpy(np.stack([al.scene(k) for k in range(3)])).to(dev)
    d_pcm = scenes[torch.arange(nseg, device=dev) % 3].contiguous()
    dI = torch.empty((nseg, stride), dtype=torch.float32, device=dev)
    dQ = torch.empty((nseg, stride), dtype=torch.float32, device=dev)
    w.sync_torch()

    def audio(normalise):
        rc = w.audio_batch_device(d_pcm.data_ptr(), NSAMP, NSAMP, nseg, dI.data_ptr(), dQ.data_ptr(), normalise)
        assert rc == 0, rc

    audio(0); audio(1)                                                    # warm-up: code objects, the lane's context
    t_plain = timed(lambda: audio(0), a.reps)
    t_norm = timed(lambda: audio(1), a.reps)
    # the rows are what the checker says (three records suffice: the rest repeat them)
    got_i, got_q = dI[:3, :NOUT].cpu().numpy(), dQ[:3, :NOUT].cpu().numpy()
    same = all(np.array_equal(got_i[k].view(np.uint32), al.scene_rows(k, 1)[0].view(np.uint32)) and
               np.array_equal(got_q[k].view(np.uint32), al.scene_rows(k, 1)[1].view(np.uint32)) for k in range(3))

    nbytes = nseg * (2 * NSAMP + 2 * 4 * stride)
    fma_def = nseg * NOUT * 2 * 511
    fma_run = nseg * NOUT * (383 + 384)                                   # 511 less the 128 (I) and 127 (Q) exact zeros
    lab = w.lab()
    nfloats = (nbytes // 2 // 4) & ~3                                      # a copy reads and writes: half the bytes each way
    src = torch.empty(nfloats, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    w.sync_torch()
    iters = 5
    lab.wspr_calib_copy(src.data_ptr(), dst.data_ptr(), nfloats, 2)
    t_copy = [x / iters for x in timed(lambda: lab.wspr_calib_copy(src.data_ptr(), dst.data_ptr(), nfloats, iters), a.reps)]
    ms16 = C.c_double(0.0)
    lab.wspr_calib_copy16(src.data_ptr(), dst.data_ptr(), nfloats, iters, 0, C.byref(ms16))
    lab.wspr_calib_copy16(src.data_ptr(), dst.data_ptr(), nfloats, iters, 0, C.byref(ms16))
    del src, dst

    dec = w.BatchDecoder(nseg, 16)
    dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NOUT, stride)            # warm-up (the rows are decoded in place: refill)
    t_dec = []
    for _ in range(3):
        audio(1)
        t_dec += timed(lambda: dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NOUT, stride), 1)
    spots = dec.total_spots()

    med = lambda v: float(np.median(v))
    ms = med(t_plain)
    copy_rate = 2 * 4 * nfloats / (med(t_copy) * 1e-3)
    res = {
        "what": "wspr_audio_batch_device(), one call, host clock around the call (it returns when its stream is done)",
        "device": torch.cuda.get_device_name(0), "nseg": nseg, "nsamp": NSAMP, "reps": a.reps,
        "rows_equal_checker": bool(same),
        "audio_ms": ms, "audio_ms_all": t_plain, "audio_normalised_ms": med(t_norm), "audio_normalised_ms_all": t_norm,
        "bytes_moved": nbytes, "bytes_per_s": nbytes / (ms * 1e-3),
        "calib_copy_ms": med(t_copy), "calib_copy_bytes_per_s": copy_rate,
        "calib_copy16_ms": ms16.value, "calib_copy16_bytes_per_s": 2 * 4 * nfloats / (ms16.value * 1e-3) if ms16.value else None,
        "fraction_of_calib_copy_rate": nbytes / (ms * 1e-3) / copy_rate,
        "fma_by_definition": fma_def, "fma_executed": fma_run,
        "fma_per_s_by_definition": fma_def / (ms * 1e-3), "fma_per_s_executed": fma_run / (ms * 1e-3),
        "packed_fma_peak_per_s": PEAK_FMA_PER_S,
        "fraction_of_packed_fma_peak_by_definition": fma_def / (ms * 1e-3) / PEAK_FMA_PER_S,
        "fraction_of_packed_fma_peak_executed": fma_run / (ms * 1e-3) / PEAK_FMA_PER_S,
        "decode_ms": med(t_dec), "decode_ms_all": t_dec, "decode_spots": spots,
        "audio_over_decode": med(t_norm) / med(t_dec),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
