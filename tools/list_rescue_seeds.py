#!/usr/bin/env python3
"""CPU only: which single-signal scenes does the list-decoding stage rescue?  The twin of tools/osd_rescue_seeds.py, and how
the floor of tests/test_gpu_list.py's stage test was chosen.

For every seed in [lo, hi): tests/synth.py make_segment(seed, snr_db=SNR) through the CPU oracle with its trace; for every
candidate the oracle visits and leaves undecoded and that was worth a ladder (attempts >= 1), the serial checker
(tests/helpers/list_check.c) on the trace's rung-0 symbols against the 7 600 messages synth.CALLS x GRIDS x POWERS, then
the gate at zmin16.  One line per seed: what Fano decoded, what was sent, and (pass, candidate, z, runner-up's z, text,
"gated" if the rung-0 vector also passed the sync/rms gate of wsprd.c:758 -- which the stage does NOT apply) of every
candidate with z >= 4; then the totals, over all candidates and over the gated subset.

    python tools/list_rescue_seeds.py -30 5000 5024 [zmin16 = 96]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                    # noqa: E402

import list_lib as ll                 # noqa: E402
import oracle_lib as orc              # noqa: E402
import synth                          # noqa: E402


def main():
    snr, lo, hi = float(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    zmin16 = int(sys.argv[4]) if len(sys.argv) > 4 else 96
    sym, msgs = ll.all_symbols(), ll.all_messages()
    symf = lambda m: orc.channel_symbols(m)[1]
    fano = failed = rescued = rescued_gated = wrong = 0
    zs = []
    for seed in range(lo, hi):
        I, Q, truth = synth.make_segment(seed, symf, snr_db=snr)
        sent = synth.expected_text(truth[0][0])
        spots, _, _, tr = orc.decode(I, Q, 45000, orc.default_options(), trace=True)
        where, vec = [], []
        for p in range(tr.passes_run):
            for j in range(tr.n_visited[p]):
                if tr.decoded[p][j] or tr.attempts[p][j] < 1:
                    continue
                where.append((p, j, bool(tr.first_sync2[p][j] > 0.12 and tr.first_rms[p][j] > 52.0 * (50 / 64.0))))
                vec.append(np.array(tr.first_symbols[p][j], np.uint8))
        res, hit, hit_gated = [], False, False
        if vec:
            for (p, j, gated), (idx, s, s2, v2) in zip(where, ll.check(sym, np.array(vec))):
                z, z2 = s / np.sqrt(v2), s2 / np.sqrt(v2)
                text = synth.expected_text(msgs[idx])
                if z >= 4.0:
                    res.append((p, j, round(float(z), 2), round(float(z2), 2), text, "gated" if gated else "-"))
                if ll.gate(s, v2, zmin16):
                    if text == sent:
                        hit, hit_gated = True, hit_gated or gated
                        zs.append(float(z))
                    else:
                        wrong += 1
        decoded = bool(spots)
        fano += decoded
        failed += not decoded
        rescued += (not decoded) and hit
        rescued_gated += (not decoded) and hit_gated
        print(seed, "fano:", [s.message.decode() for s in spots], "sent:", sent, "list:", res, flush=True)
    print("SNR %.0f dB, seeds %d..%d, zmin16 %d: Fano decodes %d / %d; of the %d Fano-failed scenes the list rule recovers the "
          "sent message in %d (%d on candidates that also pass the sync/rms gate), z %.2f .. %.2f; accepted entries that are "
          "NOT the sent message: %d" % (snr, lo, hi - 1, zmin16, fano, hi - lo, failed, rescued, rescued_gated,
                                        min(zs) if zs else 0.0, max(zs) if zs else 0.0, wrong))


if __name__ == "__main__":
    main()
