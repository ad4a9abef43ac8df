#!/usr/bin/env python3
"""CPU only: which single-signal scenes does the ordered-statistics stage rescue?  How the seeds of
tests/test_gpu_osd.py's rescue and ordering tests were chosen.

For every seed in [lo, hi): tests/synth.py make_segment(seed, snr_db=SNR) through the CPU oracle with its trace; for every
candidate the oracle visits and leaves undecoded, that was worth a ladder and whose rung-0 vector passed the sync/rms
gate of wsprd.c:758, the serial checker (tests/helpers/osd_check.cpp) at depth 1 and 3 on the trace's rung-0 symbols,
then the "heard before" gate over a table holding synth.CALLS.  One line per seed: what Fano decoded, what was sent, and
(pass, candidate, depth, dist, nhard, order, text) of every accepted OSD result.

    python tools/osd_rescue_seeds.py -30 5000 5024
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                    # noqa: E402

import oracle_lib as orc              # noqa: E402
import osd_lib as ol                  # noqa: E402
import rtlsdr_wsprd_amd as w          # noqa: E402
import synth                          # noqa: E402


def text_of(data):
    h, l = C.create_string_buffer(32768 * 13), C.create_string_buffer(32768 * 5)
    msg = (C.c_byte * 12)(*[x - 256 if x > 127 else x for x in data], 0)
    out = [C.create_string_buffer(32) for _ in range(5)]
    w.lib().unpk_(msg, h, l, *out)
    return out[0].value.decode()


def main():
    snr, lo, hi = float(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    hashtab, loctab = np.zeros(32768 * 13, np.uint8), np.zeros(32768 * 5, np.uint8)
    for call in synth.CALLS:
        slot = w.lib().nhash(call.encode(), len(call), 146)
        hashtab[slot * 13:slot * 13 + len(call)] = np.frombuffer(call.encode(), np.uint8)
    symf = lambda m: orc.channel_symbols(m)[1]
    for seed in range(lo, hi):
        I, Q, truth = synth.make_segment(seed, symf, snr_db=snr)
        spots, _, _, tr = orc.decode(I, Q, 45000, orc.default_options(), trace=True)
        res = []
        for p in range(tr.passes_run):
            for j in range(tr.n_visited[p]):
                if tr.decoded[p][j] or tr.attempts[p][j] < 1:
                    continue
                if not (tr.first_sync2[p][j] > 0.12 and tr.first_rms[p][j] > 52.0 * (50 / 64.0)):
                    continue
                sym = np.array(tr.first_symbols[p][j], np.uint8)
                for depth in (1, 3):
                    data, dist, nh, order = ol.check(sym, depth)
                    d = np.array(data, np.uint8)
                    if ol.checker().osd_gate(d.ctypes.data, hashtab.ctypes.data, loctab.ctypes.data):
                        res.append((p, j, depth, dist, nh, order, text_of(data)))
        print(seed, "fano:", [s.message.decode() for s in spots], "sent:", synth.expected_text(truth[0][0]), "osd:", res, flush=True)


if __name__ == "__main__":
    main()
