#!/usr/bin/env python3
"""The tunable multi-band front end (K21) on an MI355X: what it costs beside the parent commit's K0 and a copy of the same bytes.

  python tools/tune_ab.py --parent-lib PARENT/libwspr_mi355x.so [--nseg 16] [--reps 5] [--figures FILE.jsonl ...]
                          [--bench-dumps PARENT_DIR THIS_DIR] [--out profiles/tuner.json]

On --nseg full segments (576 000 000 bytes each: 127.5 + 10 LSB of Gaussian noise per rail, made on the device) seven cases
take turns in one loop of ONE child process under `rocprofv3 --kernel-trace` (no counters in that run); every figure is a
kernel's own start-to-end stamp, the median over the loop's rounds after one warm-up round:
  K21 with 1, 2, 4, 8 and 16 bands      tune_block_sums_kernel (one launch per four bands) + tune_comb_fir_kernel
  K0 through the PARENT commit's library (--parent-lib: libwspr_mi355x.so built from the parent commit, loaded beside this
     tree's; wspr_decimate_u8_batch_device on the same rows)       cic_block_sums_mfma_kernel + cic_comb_fir_kernel
  a device copy of the same bytes (wspr_calib_copy16, lab library) calib_copy16_kernel
The kernels of a round start in a fixed order, so the launches of one name, sorted by their start stamps, fall to the cases in
turn.  GOALS, reported met or NOT met whichever way they fall:
  one band takes no longer than 1.25 x the parent's K0;  four bands in one call take no longer than half of four one-band calls.
The band count at which the stage stops being memory-bound: a pass over the rows counts as memory-bound while it takes no longer
than 1.15 x the parent K0's pass over the same rows (K0 runs at 0.82 of HBM peak, profiles/r04_k0_alone.txt).
--figures: JSON-lines files written by the stage's tests under WSPR_TUNE_FIGURES (float64 distance, filter, spurs, end to end);
they are filed in the result as they are.  --bench-dumps: two directories written by `bench.py --dump-outputs` on the parent
commit and on this one; recorded is whether every file is byte-identical.
Nothing is asserted but that the rows of the timed calls equal the checker's on their first blocks."""
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

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rtlsdr_wsprd_amd as w  # noqa: E402

SEG_BYTES = 576000000
BANDS = (1, 2, 4, 8, 16)
WARMUP = 1
KERNELS = ("tune_block_sums_kernel", "tune_comb_fir_kernel", "cic_block_sums_mfma_kernel", "cic_comb_fir_kernel", "calib_copy16_kernel")


def noise_bytes(nseg, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(21)
    raw = torch.empty(nseg, SEG_BYTES, device=dev, dtype=torch.uint8)
    chunk = 64000000
    for s in range(nseg):
        for c0 in range(0, SEG_BYTES, chunk):
            raw[s, c0:c0 + chunk] = (127.5 + 10.0 * torch.randn(chunk, device=dev, generator=g)).round().clamp(1, 255).to(torch.uint8)
    return raw


def child(nseg, reps, parent_lib, out_path):
    import tune_lib as tl
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stride = int(w.lib().wspr_iq_stride())
    raw = noise_bytes(nseg, dev)
    copy = torch.empty_like(raw)
    dI = torch.zeros(nseg * 16, stride, device=dev)
    dQ = torch.zeros(nseg * 16, stride, device=dev)
    steps = [1 << 30] + [int(x) | 1 for x in np.random.default_rng(4).integers(0, 1 << 32, 15)]
    P = C.CDLL(parent_lib)
    P.wspr_decimate_u8_batch_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    assert not hasattr(P, "wspr_tune_step"), "--parent-lib is not the parent commit's library"
    lab = w.lab()
    ms = C.c_double(0.0)
    w.sync_torch()
    same = {}
    for rep in range(WARMUP + reps):
        for nb in BANDS:
            assert w.tune_u8_batch_device(raw.data_ptr(), SEG_BYTES, nseg, steps[:nb], dI.data_ptr(), dQ.data_ptr(), 0) == 0
            if rep == 0:                                            # what the timed calls write is what the checker says
                head = raw[nseg - 1, :40 * tl.BLOCK_BYTES].cpu().numpy()
                _, wI, wQ, _ = tl.check_rows(head, steps[:nb])
                r0 = (nseg - 1) * nb
                gI, gQ = dI[r0:r0 + nb, :40].cpu().numpy(), dQ[r0:r0 + nb, :40].cpu().numpy()
                same[nb] = bool(np.array_equal(gI.view(np.uint32), wI[:, :40].view(np.uint32)) and
                                np.array_equal(gQ.view(np.uint32), wQ[:, :40].view(np.uint32)))
                assert same[nb], nb
        assert P.wspr_decimate_u8_batch_device(raw.data_ptr(), SEG_BYTES, nseg, dI.data_ptr(), dQ.data_ptr(), 0) == 0
        assert lab.wspr_calib_copy16(raw.data_ptr(), copy.data_ptr(), nseg * SEG_BYTES // 4, 1, 0, C.byref(ms)) == 0
    with open(out_path, "w") as f:
        json.dump({"rows_equal_checker": same, "steps": steps}, f)


def trace(nseg, reps, parent_lib):
    d = tempfile.mkdtemp(prefix="tune_ab_")
    side = os.path.join(d, "child.json")
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                    "--child", side, "--nseg", str(nseg), "--reps", str(reps), "--parent-lib", parent_lib], check=True, timeout=1100,
                   stdout=subprocess.DEVNULL)
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name") or r.get("KernelName") or ""
            for k in KERNELS:
                if k in name:
                    out.setdefault(k, []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6))
                    break
    return {k: [ms for _, ms in sorted(v)] for k, v in out.items()}, json.load(open(side))


def compare_dumps(parent, this):
    names = sorted(os.listdir(parent))
    same = names == sorted(os.listdir(this)) and all(filecmp.cmp(os.path.join(parent, n), os.path.join(this, n), shallow=False)
                                                     for n in names)
    return {"files": names, "spot_records_byte_identical_to_parent": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="JSON", default=None, help=argparse.SUPPRESS)      # under rocprofv3
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--nseg", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--figures", nargs="*", default=[])
    ap.add_argument("--bench-dumps", nargs=2, metavar=("PARENT_DIR", "THIS_DIR"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tuner.json"))
    a = ap.parse_args()
    if w.lib().wspr_device_ready() != 1:
        sys.exit("tune_ab: no usable HIP device (there is no CPU fallback)")
    if a.child:
        return child(a.nseg, a.reps, a.parent_lib, a.child)
    t, side = trace(a.nseg, a.reps, os.path.abspath(a.parent_lib))
    rounds = WARMUP + a.reps
    passes = [(nb + 3) // 4 for nb in BANDS]
    pa, pb = t["tune_block_sums_kernel"], t["tune_comb_fir_kernel"]
    assert len(pa) == sum(passes) * rounds and len(pb) == len(BANDS) * rounds, (len(pa), len(pb), rounds)
    assert len(t["cic_block_sums_mfma_kernel"]) == rounds and len(t["calib_copy16_kernel"]) == rounds
    med = lambda v: float(np.median(v))
    k21 = {}
    for i, nb in enumerate(BANDS):
        at = sum(passes[:i])
        a_ms = [sum(pa[r * sum(passes) + at + j] for j in range(passes[i])) for r in range(WARMUP, rounds)]
        b_ms = [pb[r * len(BANDS) + i] for r in range(WARMUP, rounds)]
        k21[str(nb)] = {"block_sums_ms": med(a_ms), "passes": passes[i], "comb_fir_ms": med(b_ms), "total_ms": med(a_ms) + med(b_ms)}
    k0 = {"block_sums_ms": med(t["cic_block_sums_mfma_kernel"][WARMUP:]), "comb_fir_ms": med(t["cic_comb_fir_kernel"][WARMUP:])}
    k0["total_ms"] = k0["block_sums_ms"] + k0["comb_fir_ms"]
    copy_ms = med(t["calib_copy16_kernel"][WARMUP:])
    nbytes = a.nseg * SEG_BYTES
    one, four = k21["1"]["total_ms"], k21["4"]["total_ms"]
    bound = [nb for nb in BANDS if k21[str(nb)]["block_sums_ms"] / k21[str(nb)]["passes"] <= 1.15 * k0["block_sums_ms"]]
    res = {
        "device": torch.cuda.get_device_name(0),
        "what": "kernel start-to-end stamps of ONE rocprofv3 --kernel-trace run of a child process (no counters), the cases taking "
                "turns in one loop; medians over %d rounds after %d warm-up round(s); K0 through the parent commit's library" % (a.reps, WARMUP),
        "nseg": a.nseg, "bytes_per_seg": SEG_BYTES, "rows": "127.5 + 10 LSB of Gaussian noise per rail, no 0x00 byte",
        "k21_ms_by_bands": k21, "parent_k0_ms": k0, "copy_ms": copy_ms,
        "bytes_read_per_s": {"k21_1_band": nbytes / (k21["1"]["block_sums_ms"] * 1e-3), "k21_4_bands": nbytes / (k21["4"]["block_sums_ms"] * 1e-3),
                             "parent_k0": nbytes / (k0["block_sums_ms"] * 1e-3), "copy_read_plus_write": 2 * nbytes / (copy_ms * 1e-3)},
        "goal_one_band_within_1.25_of_parent_k0": {"ratio": one / k0["total_ms"], "met": bool(one <= 1.25 * k0["total_ms"])},
        "goal_four_bands_within_half_of_four_calls": {"ratio": four / (4 * one), "met": bool(four <= 0.5 * 4 * one)},
        "memory_bound": {"rule": "a pass takes no longer than 1.15 x the parent K0's pass over the same rows",
                         "band_counts_that_meet_it": bound,
                         "pass_ms_over_k0_pass_ms": {str(nb): k21[str(nb)]["block_sums_ms"] / k21[str(nb)]["passes"] / k0["block_sums_ms"] for nb in BANDS}},
        "rows_equal_checker": side["rows_equal_checker"], "steps": side["steps"],
    }
    for path in a.figures:
        for line in open(path):
            rec = json.loads(line)
            res.setdefault("figures", {}).setdefault(rec.pop("name"), []).append(rec)
    if a.bench_dumps:
        res["bench_py"] = compare_dumps(*a.bench_dumps)
    print(json.dumps({k: res[k] for k in ("k21_ms_by_bands", "parent_k0_ms", "copy_ms", "goal_one_band_within_1.25_of_parent_k0",
                                          "goal_four_bands_within_half_of_four_calls", "memory_bound")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
