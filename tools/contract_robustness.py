#!/usr/bin/env python3
"""What does the contracted arithmetic (wspr_set_arithmetic(WSPR_ARITH_CONTRACTED)) change in the SPOTS?

The contracted mode is defined by its site list (include/wspr_mi355x.h); tests/test_gpu_contracted.py shows the device
equals the CONTRACT=1 checker (tests/helpers/contract_dsp.c) bit for bit.  This script decodes the same segments through
the CPU oracle (exact mode) and through that checker (contracted mode) and counts what changes, with the counters of
tools/fft_robustness.py:

  workloads   c1      BASELINE configs[1]: 1 024 segments x 1 signal at -20 dB
              c2      BASELINE configs[2]: 8 192 segments x 10 signals, -10..-28 dB
              scenes  3 000 randomised scenes of tests/test_gpu_parity.py

  python tools/contract_robustness.py [--workloads c1,c2,scenes] [--n-c1 1024] [--n-c2 8192] [--n-scenes 3000]
                                      [--threads N] [--out profiles/contracted_robustness.json] [--update EARLIER.json]

north_star tolerances: call/loc/pwr exact; SNR +-0.1 dB, dt +-10 ms, freq +-0.1 Hz.  CPU only (test infrastructure).
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import contract_lib as cl    # noqa: E402
import fft_robustness as fr  # noqa: E402
import oracle_lib as ol      # noqa: E402

NS = 45000


def decode_all(segs, threads, contracted):
    """Per segment: (spot records, pass-0 coarse candidate list (freq, shift, drift))."""
    def run(k):
        I, Q = segs[k]
        if contracted:
            spots, _, _, tr = cl.decode(1, I, Q, NS, trace=True)
        else:
            spots, _, _, tr = ol.decode(I, Q, NS, trace=True)
        cands = tuple((tr.cand_coarse[0][i].freq, tr.cand_coarse[0][i].shift, tr.cand_coarse[0][i].drift)
                      for i in range(tr.npk[0]))
        return [fr.spot_rec(s) for s in spots], cands
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(run, range(len(segs))))


def segments(wl, a):
    if wl == "c1":
        return fr.gen_c1(a.n_c1)
    if wl == "c2":
        with ThreadPoolExecutor(a.threads) as ex:
            return list(ex.map(fr.gen_c2_one, range(a.n_c2)))
    if wl == "scenes":
        return fr.gen_scenes(a.n_scenes)
    raise SystemExit("unknown workload " + wl)


def study(segs, threads):
    """compare() of tools/fft_robustness.py with the exact oracle as the base and the contracted checker as the variant."""
    base = decode_all(segs, threads, False)
    var = decode_all(segs, threads, True)
    r = fr.compare(base, var)
    r["spots_beyond_tolerance_fraction"] = r["spots_beyond_tolerance"] / max(1, r["spots_base"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c1,c2,scenes")
    ap.add_argument("--n-c1", type=int, default=1024)
    ap.add_argument("--n-c2", type=int, default=8192)
    ap.add_argument("--n-scenes", type=int, default=3000)
    ap.add_argument("--threads", type=int, default=len(os.sched_getaffinity(0)))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contracted_robustness.json"))
    ap.add_argument("--update", default=None,
                    help="start from this earlier result file and replace / add only the workloads run now")
    a = ap.parse_args()
    I0, Q0 = fr.gen_c1(1)[0]
    ol.decode(I0, Q0, NS)                        # static tables of both libraries initialised before the threads start
    cl.decode(1, I0, Q0, NS)
    result = {"base": "exact (CPU oracle, oracle/orc_dsp.c)",
              "variant": "contracted (tests/helpers/contract_dsp.c, CONTRACT=1)",
              "tolerances": fr.TOL, "workloads": {}}
    if a.update:
        with open(a.update) as f:
            result["workloads"].update(json.load(f)["workloads"])
    for wl in a.workloads.split(","):
        t0 = time.time()
        segs = segments(wl, a)
        block = study(segs, a.threads)
        block["seconds"] = round(time.time() - t0, 1)
        block["threads"] = a.threads
        result["workloads"][wl] = block
        print("%s: %s" % (wl, json.dumps(block)), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
