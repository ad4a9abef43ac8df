#!/usr/bin/env python3
"""CPU only: which single-signal scenes does the block-detection stage rescue?  How the seeds of
tests/test_block_checker.py's pinned walk and of tests/test_gpu_block.py's stage tests were chosen.

For every seed in [lo, hi): tests/synth.py make_segment(seed, snr_db=SNR) through the CPU oracle with its trace (one pass,
no subtraction); for every candidate the oracle visits, finds worth the jitter ladder and leaves undecoded, the stage's
rule over the serial checker and the oracle's Fano search (tests/block_lib.py walk(), exact arithmetic, maxblock 3).  One
line per seed: what Fano decoded, what was sent, and (candidate, block, jitter, cycles, text) of every walk that decoded;
then the totals.  QUICK=1 in the environment walks jitter 0 only.

    python tools/block_rescue_seeds.py -30 5000 5024
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import block_lib as bl                # noqa: E402
import oracle_lib as orc              # noqa: E402


def main():
    snr, lo, hi = float(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    quick = int(os.environ.get("QUICK", "0"))
    plain, rescued, false = [], [], []
    for seed in range(lo, hi):
        I, Q, sent = bl.weak_scene(seed, snr)
        spots, _, _, tr = orc.decode(I, Q, 45000, orc.default_options(npasses=1, subtraction=0), trace=True)
        res = []
        for p, j, freq, shift, drift in bl.undecoded_worth(tr):
            hit = bl.walk(0, I, Q, 45000, freq, shift, drift, quickmode=quick)
            if hit:
                res.append((j, hit[0], hit[1], hit[3], bl.unpack(hit[2])))
        fano = [s.message.decode() for s in spots]
        if sent in fano:
            plain.append(seed)
        elif any(r[4] == sent for r in res):
            rescued.append(seed)
        false += [(seed, r[4]) for r in res if r[4] != sent] + [(seed, m) for m in fano if m != sent]
        print(seed, "fano:", fano, "sent:", sent, "block:", res, flush=True)
    print("decoded by the plain ladder:", plain)
    print("added by the walk:", rescued)
    print("messages that were not sent:", false)


if __name__ == "__main__":
    main()
