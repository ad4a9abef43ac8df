#!/usr/bin/env python3
"""Where the two tap tables of rtlsdr-wsprd_amd/csrc/kernels/audio_front.h come from (K12, the 12 kHz audio front end).

  h[k]  ~ sinc(2 * 187.5 * k / 12000) * kaiser(511, beta = 8)[k + 255],  k = -255 .. 255, scaled so that sum(h) = 1
  gI[k] = (float)( 2 h[k] c8[k mod 8]),   c8 = { 1, r, 0, -r, -1, -r,  0,  r}
  gQ[k] = (float)(-2 h[k] s8[k mod 8]),   s8 = { 0, r, 1,  r,  0, -r, -1, -r},   r = the double nearest sqrt(1/2)

all in double until the final rounding.  The committed bit patterns are the definition; this script documents them
(tests/test_audio_checker.py holds the header to this output within one float ulp: numpy's Bessel function may differ in
the last place between versions).

  python tools/gen_audio_taps.py            the design figures
  python tools/gen_audio_taps.py --tables   the two C tables as they stand in the header
"""
import sys

import numpy as np

K = 255
NTAPS = 2 * K + 1
RATE = 12000.0
DECIM = 32
CUTOFF_HZ = 187.5
BETA = 8.0


def prototype():
    """h[-255..255] in double, sum 1."""
    k = np.arange(-K, K + 1, dtype=np.float64)
    h = np.sinc(2.0 * CUTOFF_HZ * k / RATE) * np.kaiser(NTAPS, BETA)
    return h / h.sum()


def taps():
    """(gI, gQ) as float32 arrays of 511, index k + 255."""
    r = np.sqrt(0.5)
    c8 = np.array([1.0, r, 0.0, -r, -1.0, -r, 0.0, r])
    s8 = np.array([0.0, r, 1.0, r, 0.0, -r, -1.0, -r])
    k = np.arange(-K, K + 1)
    h = prototype()
    gi = (2.0 * h * c8[k % 8]).astype(np.float32)
    gq = (-2.0 * h * s8[k % 8]).astype(np.float32)
    gi[(k % 8 == 2) | (k % 8 == 6)] = 0.0          # +0.0f, not -0.0f: the stated exact zeros
    gq[(k % 8 == 0) | (k % 8 == 4)] = 0.0
    return gi, gq


def response_db(freqs_hz):
    """|H(f)| of the prototype in dB (the complex filter's response at 1500 + f), float64."""
    k = np.arange(-K, K + 1, dtype=np.float64)
    h = prototype()
    f = np.asarray(freqs_hz, dtype=np.float64)
    H = np.cos(2.0 * np.pi * np.outer(f, k) / RATE) @ h          # h is even: the response is real
    return 20.0 * np.log10(np.maximum(np.abs(H), 1e-300))


def c_table(name, g):
    bits = g.view(np.uint32)
    rows = ["    " + ", ".join("0x%08xu" % b for b in bits[i:i + 8]) for i in range(0, NTAPS, 8)]
    return "AUDIO_FRONT_TABLE uint32_t %s[AUDIO_FRONT_NTAPS] = {\n%s\n};" % (name, ",\n".join(rows))


def main():
    gi, gq = taps()
    if "--tables" in sys.argv:
        print(c_table("audio_front_gi_bits", gi))
        print(c_table("audio_front_gq_bits", gq))
        return
    p = response_db(np.arange(0.0, 110.0001, 0.25))
    w = response_db(np.arange(0.0, 150.0001, 0.25))
    s = response_db(np.arange(265.0, 6000.0001, 0.25))
    print("pass band |f| <= 110 Hz: %+.4f / %+.4f dB" % (p.max(), p.min()))
    print("|f| <= 150 Hz: %.2f dB at worst" % w.min())
    print("|f| >= 265 Hz: %.1f dB at most" % s.max())


if __name__ == "__main__":
    main()
