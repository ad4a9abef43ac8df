#!/usr/bin/env python3
"""Where rtlsdr-wsprd_amd/csrc/kernels/tune_tables.h comes from: the two rotor tables of the tunable front end (K21,
kernels/tune.h) and its scale, as integers and one float bit pattern.  Writes the header to stdout:

    python3 tools/gen_tune_tables.py > rtlsdr-wsprd_amd/csrc/kernels/tune_tables.h

  C[k] = round(16384 e^{2 pi i k / 256}),   F[k] = round(16384 e^{2 pi i k / 65536}),   k = 0 .. 255
(round: to nearest, computed with mpmath-free 50-digit decimals below so that no libm rounding enters a tie), and
  scale = float32(6401^2 / (800^2 * 8 * 16384)): what makes an in-band tone leave K21 with the amplitude K0 gives it
(K0's two integrators and combs have the gain 4 * 6401^2 on int8 samples, K21's 4 * 800^2 on 8-sample sums times 16384).
tests/test_tune_checker.py recomputes the tables with numpy's float64 and holds them equal to the committed ones.
"""
import struct
from decimal import Decimal, getcontext

getcontext().prec = 60
PI = Decimal("3.14159265358979323846264338327950288419716939937510582097494")


def _sincos(x):
    """(cos x, sin x) of a Decimal by their series after halving the argument into |x| < 0.01."""
    n = 0
    while abs(x) > Decimal("0.01"):
        x /= 2
        n += 1
    c, s, term_c, term_s = Decimal(1), x, Decimal(1), x
    for k in range(1, 30):
        term_c = -term_c * x * x / ((2 * k - 1) * (2 * k))
        term_s = -term_s * x * x / ((2 * k) * (2 * k + 1))
        c += term_c
        s += term_s
    for _ in range(n):
        c, s = c * c - s * s, 2 * c * s
    return c, s


def _round(x):
    return int((x + Decimal("0.5")).to_integral_value(rounding="ROUND_FLOOR"))


def table(turns):
    out = []
    for k in range(256):
        c, s = _sincos(2 * PI * k / turns)
        out.append((_round(16384 * c), _round(16384 * s)))
    return out


def scale_bits():
    exact = Decimal(6401 * 6401) / Decimal(800 * 800 * 8 * 16384)
    f = struct.unpack("<f", struct.pack("<f", float(exact)))[0]
    return struct.unpack("<I", struct.pack("<f", f))[0], f


def emit(name, tab):
    lines = ["static const int16_t %s[512] = {   /* re, im of entry k at [2k], [2k + 1] */" % name]
    for r in range(0, 256, 8):
        lines.append("    " + " ".join("%6d,%6d," % tab[k] for k in range(r, r + 8)))
    lines.append("};")
    return "\n".join(lines)


def main():
    bits, f = scale_bits()
    print("/* K21's rotor tables and scale (kernels/tune.h).  Written by tools/gen_tune_tables.py: do not edit. */")
    print("#pragma once")
    print("#include <stdint.h>")
    print("/* C[k] = round(16384 e^{2 pi i k / 256}) */")
    print(emit("kTuneC256", table(256)))
    print("/* F[k] = round(16384 e^{2 pi i k / 65536}) */")
    print(emit("kTuneF256", table(65536)))
    print("/* float32(6401^2 / (800^2 * 8 * 16384)) = %.9g */" % f)
    print("#define TUNE_SCALE_BITS 0x%08xu" % bits)


if __name__ == "__main__":
    main()
