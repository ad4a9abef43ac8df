#!/usr/bin/env python3
"""The waterfall (K20) on an MI355X: what the kernel costs beside K16, K1 and a copy of the same rows.

  python tools/waterfall_ab.py [--nseg 2048] [--reps 7] [--out profiles/waterfall.json]
                               [--bench-dumps PARENT_DIR THIS_DIR] [--parent-k16-ms X]

On --nseg full rows of the synthesiser's white noise (K8) resident in HBM, six cases taking turns in one loop of ONE child
process under `rocprofv3 --kernel-trace` (no counters in that run); every figure is a kernel's own start-to-end stamp, the
median over the loop's rounds after two warm-up rounds:
  a  K20 alone: absolute mode, default columns (301), hop 256, tavg 1        waterfall_kernel
  b  the same at hop 128                                                     waterfall_kernel
  c  the default call (hop 128, floor mode): K16 + K20                       noise_kernel + waterfall_kernel
  d  K16's kernel: wspr_noise_batch_device()                                 noise_kernel
  e  K1: the FFT bank on the same rows (wspr_bench_fft_sync, lab library)    fft_bank*_kernel
  f  a device copy of the same rows (wspr_calib_copy16, lab library)         calib_copy16_kernel, both rails
The kernels of a round start in a fixed order, so the launches of one name, sorted by their start stamps, fall to the
cases in turn.  EXPECTATIONS, not facts, until this has run: (a) no longer than (d) -- the same 174 transforms per row on
the same bytes, 52 KB written instead of a ranking -- and (b) no more than twice (a).  What comes out is written down
either way.  A host clock around each call is recorded beside the stamps.
--bench-dumps: two directories written by `bench.py --dump-outputs` on the parent commit and on this one; recorded is
whether every file is byte-identical.  --parent-k16-ms: noise_kernel_ms of tools/noise_ab.py run on the parent commit in the
same session, recorded beside (d) (K16's transform moved into a header that K20 shares).
Nothing is asserted but that the images equal the checker's."""
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
SEED = 2000
SIGMA = 0.02
WARMUP = 2
CASES = {"a": dict(hop=256, ref_mode=0, ref=2 * SIGMA * SIGMA), "b": dict(hop=128, ref_mode=0, ref=2 * SIGMA * SIGMA), "c": None}


def noise_rows(nseg, dev, stride):
    dI = torch.zeros((nseg, stride), dtype=torch.float32, device=dev)
    dQ = torch.zeros((nseg, stride), dtype=torch.float32, device=dev)
    w.sync_torch()
    assert w.wspr_synth_batch_device([], nseg, dI.data_ptr(), dQ.data_ptr(), noise_sigma=SIGMA, seed=SEED) == 0
    return dI, dQ


def child(nseg, reps, out_path):
    """The six cases in turn, WARMUP + reps rounds; host-clock times of the calls and a check against the serial checker go to
    out_path."""
    import waterfall_lib as wl
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stride = int(w.lib().wspr_iq_stride())
    dI, dQ = noise_rows(nseg, dev, stride)
    cI, cQ = torch.empty_like(dI), torch.empty_like(dQ)
    lab = w.lab()
    ist = (348 * 301 + 15) & ~15
    d_img = torch.zeros((nseg, ist), dtype=torch.uint8, device=dev)
    nfloats = nseg * stride
    ms16, msk1 = C.c_double(0.0), (C.c_double * 8)()
    host = {k: [] for k in "abcd"}
    infos = {}
    same = {}
    for rep in range(WARMUP + reps):
        for case in "abc":
            torch.cuda.synchronize()
            t = time.perf_counter()
            rc, info = w.waterfall_batch_device(dI.data_ptr(), dQ.data_ptr(), nseg, NS, stride, d_img.data_ptr(), ist, CASES[case])
            host[case].append((time.perf_counter() - t) * 1e3)
            assert rc == 0
            infos[case] = info
            if rep == 0:                                             # what the timed calls write is what the checker says (4 rows)
                p = None if CASES[case] is None else wl.params(**CASES[case])
                want_img, want_info = wl.check_rows(dI[:4, :NS].cpu().numpy(), dQ[:4, :NS].cpu().numpy(), NS, p)
                got = d_img[:4].cpu().numpy()[:, :want_img[0].size].reshape(want_img.shape)
                same[case] = bool(np.array_equal(got, want_img) and info[:4].tobytes() == want_info.tobytes())
                assert same[case], case
        torch.cuda.synchronize()
        t = time.perf_counter()
        rc, _ = w.noise_batch_device(dI.data_ptr(), dQ.data_ptr(), nseg, NS, stride)
        host["d"].append((time.perf_counter() - t) * 1e3)
        assert rc == 0
        lab.wspr_bench_fft_sync(dI.data_ptr(), dQ.data_ptr(), nseg, NS, stride, 1, C.addressof(msk1))
        lab.wspr_calib_copy16(dI.data_ptr(), cI.data_ptr(), nfloats, 1, 0, C.byref(ms16))
        lab.wspr_calib_copy16(dQ.data_ptr(), cQ.data_ptr(), nfloats, 1, 0, C.byref(ms16))
    ref = infos["c"]["ref"].astype(np.float64) / (2 * SIGMA * SIGMA)
    with open(out_path, "w") as f:
        json.dump({"host_call_ms": {k: v[WARMUP:] for k, v in host.items()}, "images_equal_checker": same,
                   "floor_over_2s2": {"mean": float(ref.mean()), "sd": float(ref.std(ddof=1))},
                   "flags": sorted(set(int(x) for x in infos["c"]["flags"]))}, f)


def trace(nseg, reps):
    """({kernel: [(start, ms)] sorted by start}, what the child wrote) of one kernel-trace run of child()."""
    d = tempfile.mkdtemp(prefix="waterfall_ab_")
    side = os.path.join(d, "child.json")
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
                    os.path.abspath(__file__), "--child", side, "--nseg", str(nseg), "--reps", str(reps)], check=True,
                   timeout=900, stdout=subprocess.DEVNULL)
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name") or r.get("KernelName") or ""
            for k in ("waterfall_kernel", "noise_kernel", "fft_bank_avg_kernel", "fft_bank_kernel", "calib_copy16_kernel"):
                if k in name:
                    out.setdefault(k, []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6))
                    break
    return {k: sorted(v) for k, v in out.items()}, json.load(open(side))


def compare_dumps(parent, this):
    names = sorted(os.listdir(parent))
    same = names == sorted(os.listdir(this)) and all(filecmp.cmp(os.path.join(parent, n), os.path.join(this, n), shallow=False)
                                                     for n in names)
    return {"files": names, "bytes": int(sum(os.path.getsize(os.path.join(this, n)) for n in os.listdir(this))),
            "spot_records_byte_identical_to_parent": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="JSON", default=None, help=argparse.SUPPRESS)      # under rocprofv3
    ap.add_argument("--nseg", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bench-dumps", nargs=2, metavar=("PARENT_DIR", "THIS_DIR"), default=None)
    ap.add_argument("--parent-k16-ms", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "waterfall.json"))
    a = ap.parse_args()
    if w.lib().wspr_device_ready() != 1:
        sys.exit("waterfall_ab: no usable HIP device (there is no CPU fallback)")
    if a.child:
        return child(a.nseg, a.reps, a.child)
    t, side = trace(a.nseg, a.reps)
    rounds = WARMUP + a.reps
    wf = [ms for _, ms in t.get("waterfall_kernel", [])]
    k16 = [ms for _, ms in t.get("noise_kernel", [])]
    assert len(wf) == 3 * rounds and len(k16) == 2 * rounds, (len(wf), len(k16), rounds)
    med = lambda v: float(np.median(v))
    per = {"a_k20_hop256": wf[0::3][WARMUP:], "b_k20_hop128": wf[1::3][WARMUP:], "c_k20_of_default": wf[2::3][WARMUP:],
           "c_k16_of_default": k16[0::2][WARMUP:], "d_k16": k16[1::2][WARMUP:]}
    k1 = {k: [ms for _, ms in v] for k, v in t.items() if k.startswith("fft_bank")}
    copies = [ms for _, ms in t.get("calib_copy16_kernel", [])]
    # K1 is ONE launch of ONE kernel: the bank the library runs (the first name that appears), and of the launches of a round
    # (wspr_bench_fft_sync warms up before it times) the last, which is the timed one
    k1_name = next((k for k in ("fft_bank_avg_kernel", "fft_bank_kernel") if k in k1), None)
    per["e_k1"] = []
    if k1_name:
        v, n = k1[k1_name], len(k1[k1_name]) // rounds
        per["e_k1"] = [v[n * (i + 1) - 1] for i in range(rounds)][WARMUP:] if n else []
    per["f_copy_both_rails"] = [copies[2 * i] + copies[2 * i + 1] for i in range(len(copies) // 2)][WARMUP:]
    ms = {k: med(v) for k, v in per.items() if v}
    ms["c_default_call"] = ms["c_k16_of_default"] + ms["c_k20_of_default"]
    row_bytes = 2 * 4 * NS * a.nseg
    res = {
        "device": torch.cuda.get_device_name(0),
        "what": "kernel start-to-end stamps of ONE rocprofv3 --kernel-trace run of a child process (no counters), the cases "
                "taking turns in one loop; medians over the rounds after %d warm-up rounds; host_call_ms: a host clock around "
                "the whole call in the same run" % WARMUP,
        "nseg": a.nseg, "samples": NS, "reps": a.reps, "rows": "wspr_synth_batch_device() noise, sigma %g, seed %d" % (SIGMA, SEED),
        "kernel_ms": ms, "kernel_ms_all": per,
        "k1_kernel": k1_name, "k1_launches_in_trace": {k: len(v) for k, v in k1.items()},
        "bytes_read_per_pass": row_bytes, "bytes_written_by_k20": {"a": 174 * 301 * a.nseg, "b": 348 * 301 * a.nseg},
        "a_bytes_read_per_s": row_bytes / (ms["a_k20_hop256"] * 1e-3),
        "goal_a_no_longer_than_d": {"a_over_d": ms["a_k20_hop256"] / ms["d_k16"], "met": bool(ms["a_k20_hop256"] <= ms["d_k16"])},
        "goal_b_at_most_twice_a": {"b_over_a": ms["b_k20_hop128"] / ms["a_k20_hop256"],
                                   "met": bool(ms["b_k20_hop128"] <= 2.0 * ms["a_k20_hop256"])},
        "host_call_ms": {k: med(v) for k, v in side["host_call_ms"].items()},
        "images_equal_checker": side["images_equal_checker"], "floor_over_2s2": side["floor_over_2s2"], "flags_seen": side["flags"],
    }
    if "e_k1" in ms:
        res["a_over_k1"] = ms["a_k20_hop256"] / ms["e_k1"]
    if "f_copy_both_rails" in ms:
        res["a_over_copy"] = ms["a_k20_hop256"] / ms["f_copy_both_rails"]
    if a.parent_k16_ms is not None:
        res["k16_after_sharing_its_transform"] = {"parent_noise_kernel_ms": a.parent_k16_ms, "this_noise_kernel_ms": ms["d_k16"],
                                                  "this_over_parent": ms["d_k16"] / a.parent_k16_ms}
    if a.bench_dumps:
        res["bench_py"] = compare_dumps(*a.bench_dumps)
    print(json.dumps({k: res[k] for k in ("kernel_ms", "goal_a_no_longer_than_d", "goal_b_at_most_twice_a", "host_call_ms")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
