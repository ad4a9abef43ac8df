#!/usr/bin/env python3
"""The spot-detail stage (wspr_set_spot_details, K19) on an MI355X: what it costs and what its figures read.

  python tools/spot_details_ab.py [--nseg 2048] [--reps 10] [--parent-lib PATH] [--out profiles/spot_details.json]
                                  [--bench-dumps PARENT_DIR THIS_DIR]

  call     wspr_decode_batch_device() on --nseg three-signal scenes at -20 dB resident in HBM (the scene of the other *_ab.py
           tools), a host clock around each call: the stage off, the stage on and -- with --parent-lib, the parent commit's
           libwspr_mi355x.so built elsewhere -- the parent's call, the three taking turns in one loop; median and range of
           --reps calls each after two warm-up rounds.  The spot records of the three are compared byte for byte.
  kernel   K19 alone for 2 048 and 65 536 jobs: the kernel's start and end stamps from a `rocprofv3 --kernel-trace` run of a
           child process, a host clock around wspr_spot_quality_batch_device() (which also carries the vectors up and the
           records down), and a device-to-device copy of the same bytes (wspr_calib_copy16 of the lab library, HIP events).
  figures  nhard and metric of TRUE spots (the message was sent in that segment) and of FALSE spots (it was not): the
           three-signal scene at -20 and at -29 dB, and the setting of tools/list_sensitivity.py that produced false spots --
           single signals at -30 dB whose own message is not listed while the same call and locator at another power is
           (zmin16 88 and 96).  The ordered-statistics settings of tools/osd_sensitivity.py are not run here.
--bench-dumps: two directories written by `bench.py --dump-outputs` on the parent commit and on this one; recorded is
whether every file is byte-identical.  Nothing is asserted but that the figures equal the checker's."""
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
import synth                   # noqa: E402

NS = 45000
NOISE_SIGMA = float(np.float32(np.sqrt((375.0 / 2500.0) / 2.0)))        # unit power in 2 500 Hz
SEED = 1900
K = 16


def three_signal_scene(al, nseg, snr):
    tx = np.zeros(3 * nseg, w.SYNTH_TX_DTYPE)
    syms = [[w.get_wspr_channel_symbols(m)[1] for m in msgs] for msgs in al.SCENE_MESSAGES]
    for s in range(nseg):
        for j, (_, f0, t0) in enumerate(al.SIGNALS):
            r = tx[3 * s + j]
            r["seg"], r["f0"], r["t0"], r["amp"], r["drift"] = s, f0, t0, 10.0 ** (snr / 20.0), 0.0
            r["symbols"] = syms[s % 3][j]
    return tx, [[synth.expected_text(m) for m in al.SCENE_MESSAGES[s % 3]] for s in range(nseg)]


class Call:
    """wspr_decode_batch_device() of one library on the resident rows, keeping the raw spot records."""
    def __init__(self, L, nseg, stride):
        self.L, self.nseg, self.stride = L, nseg, stride
        L.wspr_decode_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, w.decoder_options,
                                               C.c_void_p, C.c_int, C.c_void_p]
        L.wspr_decode_batch_device.restype = C.c_int
        self.out = (w.decoder_results * (nseg * K))()
        self.nres = (C.c_int * nseg)()
        self.opt = w.default_options()

    def __call__(self, dI, dQ):
        torch.cuda.synchronize()
        t = time.perf_counter()
        rc = self.L.wspr_decode_batch_device(dI.data_ptr(), dQ.data_ptr(), self.nseg, NS, self.stride, self.opt,
                                             C.addressof(self.out), K, C.addressof(self.nres))
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0
        return ms

    def records(self):
        return bytes(self.out), list(self.nres)

    def spots(self):
        return [[self.out[s * K + i] for i in range(self.nres[s])] for s in range(self.nseg)]


def spread_of(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [float(x) for x in v]}


def call_cost(a, dI, dQ, stride, al):
    nseg = a.nseg
    tx, _ = three_signal_scene(al, nseg, -20.0)
    assert w.wspr_synth_batch_device(tx, nseg, dI.data_ptr(), dQ.data_ptr(), 0, NOISE_SIGMA, SEED, w.SYNTH_NORMALISE) == 0
    sides = {"off": Call(w.lib(), nseg, stride), "on": Call(w.lib(), nseg, stride)}
    if a.parent_lib:
        sides = {"parent": Call(C.CDLL(os.path.abspath(a.parent_lib)), nseg, stride), **sides}
    times = {k: [] for k in sides}
    stage = {"spot_detail_ms": [], "spot_detail_jobs": []}
    for rep in range(a.reps + 2):                                # two warm-up rounds: code objects, contexts, buffers
        for name, call in sides.items():
            w.set_spot_details(1 if name == "on" else 0)
            ms = call(dI, dQ)
            w.set_spot_details(0)
            if rep >= 2:
                times[name].append(ms)
                if name == "on":
                    t = w.last_timings()
                    stage["spot_detail_ms"].append(t["spot_detail_ms"])
                    stage["spot_detail_jobs"].append(t["spot_detail_jobs"])
    rec = {k: c.records() for k, c in sides.items()}
    res = {"what": "host clock around wspr_decode_batch_device() on %d three-signal scenes at -20 dB resident in HBM (default "
                   "options: two passes, subtraction), the sides taking turns in one loop, %d calls each after two warm-up rounds; "
                   "parent = the parent commit's library loaded beside this one" % (nseg, a.reps),
           "nseg": nseg, "reps": a.reps, "spots": int(sum(rec["off"][1])),
           "call_ms": {k: spread_of(v) for k, v in times.items()},
           "spot_records_on_equal_off": rec["on"] == rec["off"],
           "stage_device_ms": spread_of(stage["spot_detail_ms"]), "stage_jobs": spread_of(stage["spot_detail_jobs"])}
    if a.parent_lib:
        res["spot_records_off_equal_parent"] = rec["off"] == rec["parent"]
        res["off_minus_parent_ms"] = res["call_ms"]["off"]["median"] - res["call_ms"]["parent"]["median"]
    off = times["off"]
    res["on_minus_off_ms"] = res["call_ms"]["on"]["median"] - res["call_ms"]["off"]["median"]
    res["off_scatter_ms"] = max(off) - min(off)
    res["on_within_off_scatter"] = bool(res["call_ms"]["on"]["median"] <= max(off))
    return res


def kernel_jobs(n):
    rng = np.random.default_rng(n)
    vec = rng.integers(0, 256, (n, 162), dtype=np.uint8)
    dec = np.zeros((n, 11), np.uint8)
    dec[:, :7] = rng.integers(0, 256, (n, 7), dtype=np.uint8)
    dec[:, 6] &= 0xC0
    return vec, dec


def child():
    for n in (2048, 65536):
        vec, dec = kernel_jobs(n)
        for _ in range(4):
            w.spot_quality_batch(vec, dec)


def kernel_cost(dev):
    import spotq_lib as sq
    d = tempfile.mkdtemp(prefix="spot_details_ab_")
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
                    os.path.abspath(__file__), "--child"], check=True, timeout=300, stdout=subprocess.DEVNULL)
    by_grid = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name") or r.get("KernelName") or ""
            if "spot_quality_kernel" in name:
                grid = int(r.get("Grid_Size") or r.get("Grid_Size_X") or 0)
                by_grid.setdefault(grid, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    lab = w.lab()
    res = {"what": "K19 alone: kernel_ms = start-to-end stamps of spot_quality_kernel in a rocprofv3 kernel trace of a child "
                   "process (its launches after the first); call_ms = a host clock around wspr_spot_quality_batch_device(), "
                   "vectors up and records down included; copy_ms = a device-to-device copy of the same n x 162 bytes (the lab "
                   "library's wspr_calib_copy16, HIP events)"}
    for n in (2048, 65536):
        vec, dec = kernel_jobs(n)
        got = sq.words(w.spot_quality_batch(vec, dec))
        same = bool(np.array_equal(got[:512], sq.check(vec[:512], dec[:512])))
        assert same
        call = []
        for rep in range(9):
            t = time.perf_counter()
            w.spot_quality_batch(vec, dec)
            if rep >= 2:
                call.append((time.perf_counter() - t) * 1e3)
        nfloats = n * 162 // 4
        src = torch.zeros(nfloats, device=dev)
        dst = torch.zeros(nfloats, device=dev)
        w.sync_torch()
        ms = C.c_double(0.0)
        copy = []
        for rep in range(9):
            lab.wspr_calib_copy16(src.data_ptr(), dst.data_ptr(), nfloats, 1, 0, C.byref(ms))
            if rep >= 2:
                copy.append(ms.value)
        kern = next((v for g, v in sorted(by_grid.items()) if g == 64 * n or g == 256 * ((n + 3) // 4)), [])
        res[str(n)] = {"records_equal_checker": same, "bytes_read": n * (162 + 11 + 4),
                       "kernel_ms": spread_of(kern[1:] if len(kern) > 1 else kern) if kern else None,
                       "call_ms": spread_of(call), "copy_ms": spread_of(copy)}
    res["kernel_trace_grids"] = {str(g): len(v) for g, v in by_grid.items()}
    return res


def quantiles(v):
    v = np.asarray(v)
    if v.size == 0:
        return None
    q = np.percentile(v, [0, 5, 25, 50, 75, 95, 100])
    return {"n": int(v.size), "min": float(q[0]), "p05": float(q[1]), "p25": float(q[2]), "median": float(q[3]), "p75": float(q[4]),
            "p95": float(q[5]), "max": float(q[6])}


def figures_of(call, dI, dQ, nseg, expected):
    """One call with the stage on: the records of true and of false spots, by stage."""
    w.set_spot_details(1)
    call(dI, dQ)
    w.set_spot_details(0)
    det = w.last_spot_details(nseg, K)
    assert det is not None
    rows = {"true": [], "false": []}
    for s, seg in enumerate(call.spots()):
        for i, sp in enumerate(seg):
            assert det[s, i]["valid"] == 1
            rows["true" if sp.message.decode() in expected[s] else "false"].append(det[s, i])
    out = {}
    for side, recs in rows.items():
        recs = np.array(recs, w.SPOT_DETAIL_DTYPE)
        out[side] = {"spots": int(recs.size), "nhard": quantiles(recs["nhard"]), "metric": quantiles(recs["metric"]),
                     "dist": quantiles(recs["dist"]),
                     "by_stage": {str(int(st)): int((recs["stage"] == st).sum()) for st in np.unique(recs["stage"])}}
        if side == "false":
            out[side]["records"] = [{k: int(r[k]) for k in ("nhard", "dist", "rsum", "v2", "metric", "pass", "stage", "cand")} for r in recs[:64]]
    return out


def figures(a, dI, dQ, stride, al):
    nseg = a.nseg
    call = Call(w.lib(), nseg, stride)
    res = {"what": "nhard, dist and metric of every spot of one call with the stage on; true = the spot's message was sent in that "
                   "segment, false = it was not"}
    for snr in (-20.0, -29.0):
        tx, expected = three_signal_scene(al, nseg, snr)
        assert w.wspr_synth_batch_device(tx, nseg, dI.data_ptr(), dQ.data_ptr(), 0, NOISE_SIGMA, SEED + 1, w.SYNTH_NORMALISE) == 0
        res["three_signals_%d_db" % snr] = figures_of(call, dI, dQ, nseg, expected)
    # tools/list_sensitivity.py, "power_-30": the sent message is not listed, the same call and locator at another power is
    rng = np.random.default_rng(20261019)
    pool = []
    while len(pool) < 512:
        m = synth.message_wide(int(rng.integers(0, 1 << 62)))
        if m.split()[0] not in {p.split()[0] for p in pool}:
            pool.append(m)
    sent, tx = [], np.zeros(nseg, w.SYNTH_TX_DTYPE)
    for s in range(nseg):
        c, g, p = pool[int(rng.integers(0, len(pool)))].split()
        other = synth.POWERS[(synth.POWERS.index(int(p)) + 1 + int(rng.integers(0, len(synth.POWERS) - 1))) % len(synth.POWERS)]
        sent.append([synth.expected_text("%s %s %d" % (c, g, other))])
        tx["seg"][s], tx["amp"][s] = s, 10.0 ** (-30.0 / 20.0)
        tx["symbols"][s] = w.get_wspr_channel_symbols("%s %s %d" % (c, g, other))[1]
    tx["f0"] = rng.uniform(-100.0, 100.0, nseg)
    tx["t0"] = 2.0 + rng.uniform(-1.0, 1.0, nseg)
    assert w.wspr_synth_batch_device(tx, nseg, dI.data_ptr(), dQ.data_ptr(), 0, NOISE_SIGMA, SEED + 2, w.SYNTH_NORMALISE) == 0
    for z in (88, 96):
        assert w.set_message_list(pool, z) == len(pool)
        res["neighbour_power_listed_-30_db_zmin16_%d" % z] = figures_of(call, dI, dQ, nseg, sent)
        w.set_message_list(None)
    return res


def compare_dumps(parent, this):
    names = sorted(os.listdir(parent))
    same = names == sorted(os.listdir(this)) and all(filecmp.cmp(os.path.join(parent, n), os.path.join(this, n), shallow=False)
                                                     for n in names)
    return {"files": names, "spot_records_byte_identical_to_parent": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)      # under rocprofv3
    ap.add_argument("--nseg", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-dumps", nargs=2, metavar=("PARENT_DIR", "THIS_DIR"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spot_details.json"))
    a = ap.parse_args()
    if w.lib().wspr_device_ready() != 1:
        sys.exit("spot_details_ab: no usable HIP device (there is no CPU fallback)")
    if a.child:
        return child()
    import audio_lib as al
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stride = int(w.lib().wspr_iq_stride())
    dI = torch.zeros(a.nseg, stride, device=dev)
    dQ = torch.zeros(a.nseg, stride, device=dev)
    w.sync_torch()
    res = {"device": torch.cuda.get_device_name(0)}

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    res["call"] = call_cost(a, dI, dQ, stride, al)
    print(json.dumps({k: v for k, v in res["call"].items() if k != "what"}), flush=True)
    flush()
    res["figures"] = figures(a, dI, dQ, stride, al)
    print(json.dumps({k: v for k, v in res["figures"].items() if k != "what"}), flush=True)
    flush()
    res["kernel"] = kernel_cost(dev)
    print(json.dumps(res["kernel"]), flush=True)
    if a.bench_dumps:
        res["bench_py"] = compare_dumps(*a.bench_dumps)
        print(json.dumps(res["bench_py"]), flush=True)
    flush()


if __name__ == "__main__":
    main()
