// Arithmetic of the signal synthesiser (K8, wspr_synth*()), written once for the device and for a CPU.
//
// The synthesiser's contract (include/wspr_mi355x.h) is that a CPU can reproduce every sample it writes.  ocml's
// sin/cos/log are not glibc's, so nothing here calls a maths library: every function below is a fixed sequence of
// correctly rounded IEEE-754 operations (add, multiply, divide, sqrt, integer work) evaluated in the order written,
// compiled with -ffp-contract=off on both sides (no fused multiply-add anywhere), as fano_wave.h and phase_runs.h are.
//
//   synth_sincos()  double sine and cosine of the transmitter phase (|phi| reaches ~1e5 rad at +-150 Hz): Cody-Waite
//                   reduction by pi/2 in three 33-bit pieces and the degree-13 / degree-14 kernels of Sun's fdlibm
//                   (k_sin.c, k_cos.c, e_rem_pio2.c "medium size" path; public domain-style Sun licence), valid for
//                   |x| < 2^20 * pi/2.  Within one ulp of glibc's sin/cos, NOT equal to them: about 3 % of the double
//                   results differ in the last bit; after the rounding to float32 the contract asks for, no sample of
//                   the scenes of tests/test_synth_checker.py differs.
//   synth_noise()   one complex float32 Gaussian draw as a pure function of (seed, segment, sample): Philox-4x32-10
//                   (Salmon et al., SC'11) keyed by the seed, counter = (sample, 0, segment low, segment high), and the
//                   Box-Muller transform with the logarithm as an atanh series in double and the angle through
//                   glibc_sincosf.h.  synth_gauss() is the same draw for any first two counter words.
//   synth_exp()     double exponential on [-40, 0] (the fading channel's Gaussian pulse, fade.h): reduction by ln 2 in
//                   two pieces, the Taylor polynomial to degree 12, 2^k through the exponent bits.
//   synth_dphi()    phase increment of symbol i, the reference's statement rtlsdr_wsprd.c:753 plus the decoder's drift
//                   model (wsprd.c:156, 343).
#pragma once
#include <stdint.h>

#include "glibc_sincosf.h"

namespace wspr {

constexpr int kSynthNsym = 162;
constexpr int kSynthSps = 256;
constexpr int kSynthSigLen = kSynthNsym * kSynthSps;      // 41 472 samples of one transmission
constexpr int kSynthSamples = 45000;                       // samples of a segment row
constexpr double kSynthMaxHz = 1000.0;                     // |f0| + |drift|/2 beyond this is refused (the reduction's range)
constexpr int kSynthFlagAccumulate = 1;
constexpr int kSynthFlagNormalise = 2;

WSPR_HD uint64_t f64_bits(double d) {
    union { double d; uint64_t u; } v;
    v.d = d;
    return v.u;
}

// ---- double sincos --------------------------------------------------------------------------------------------------
WSPR_HD double synth_ksin(double x, double y) {            // fdlibm __kernel_sin(x, y, 1) on [-pi/4, pi/4], tail y
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double z = x * x;
    const double v = z * x;
    const double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
WSPR_HD double synth_kcos(double x, double y) {            // fdlibm __kernel_cos(x, y)
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = x * x;
    const double w = z * z;
    const double r = z * (C1 + z * (C2 + z * C3)) + (w * w) * (C4 + z * (C5 + z * C6));
    const double hz = 0.5 * z;
    const double u = 1.0 - hz;
    return u + (((1.0 - u) - hz) + (z * r - x * y));
}
WSPR_HD void synth_sincos(double x, double* sn, double* cs) {
    const double invpio2 = 6.36619772367581382433e-01;
    const double pio2_1 = 1.57079632673412561417e+00, pio2_1t = 6.07710050650619224932e-11;   // first 33 bits of pi/2, rest
    const double pio2_2 = 6.07710050630396597660e-11, pio2_2t = 2.02226624879595063154e-21;   // second 33 bits, rest
    const double pio2_3 = 2.02226624871116645580e-21, pio2_3t = 8.47842766036889956997e-32;   // third 33 bits, rest
    const double magic = 6755399441055744.0;               // 1.5 * 2^52: (t + magic) - magic = t rounded to an integer
    const double fn = (x * invpio2 + magic) - magic;
    const int n = (int)fn;
    double r = x - fn * pio2_1;                            // exact: fn < 2^20, pio2_1 has 33 bits
    double w = fn * pio2_1t;
    double y0 = r - w;
    const int ex = (int)((f64_bits(x) >> 52) & 0x7ff);
    if (ex - (int)((f64_bits(y0) >> 52) & 0x7ff) > 16) {   // cancellation: second piece
        double t = r;
        w = fn * pio2_2;
        r = t - w;
        w = fn * pio2_2t - ((t - r) - w);
        y0 = r - w;
        if (ex - (int)((f64_bits(y0) >> 52) & 0x7ff) > 49) {   // third piece (151 bits of pi/2 in all)
            t = r;
            w = fn * pio2_3;
            r = t - w;
            w = fn * pio2_3t - ((t - r) - w);
            y0 = r - w;
        }
    }
    const double y1 = (r - y0) - w;
    const double s = synth_ksin(y0, y1), c = synth_kcos(y0, y1);
    switch (n & 3) {
        case 0:  *sn = s;  *cs = c;  break;
        case 1:  *sn = c;  *cs = -s; break;
        case 2:  *sn = -s; *cs = -c; break;
        default: *sn = -c; *cs = s;  break;
    }
}

// ---- the transmitter's phase ----------------------------------------------------------------------------------------
// dphi of symbol i: 2.0 * M_PI * dt * ((f0 + fd_i) + ((double)symbol - 1.5) * df), all double, in that order
WSPR_HD double synth_dphi(float f0, float drift, int i, unsigned char symbol) {
    const double df = 375.0 / 256.0, dt = 1 / 375.0, two_pi = 2.0 * 3.14159265358979323846;
    const double fd = ((double)drift / 2.0) * ((double)i - 81.0) / 81.0;
    return two_pi * dt * (((double)f0 + fd) + ((double)symbol - 1.5) * df);
}
// output index of sample 0 of a transmission: floor(t0 / dt), clamped so that a far-away frame simply misses the row
WSPR_HD int synth_first_index(float t0) {
    const double dt = 1 / 375.0;
    const double q = __builtin_floor((double)t0 / dt);
    return q > 1.0e6 ? 1000000 : (q < -1.0e6 ? -1000000 : (int)q);
}

// ---- noise ----------------------------------------------------------------------------------------------------------
WSPR_HD void synth_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// natural logarithm of u in (0, 1]: u = m * 2^e with m in [sqrt(1/2), sqrt(2)), ln m = 2 atanh((m-1)/(m+1)) as its
// series to s^15 (|s| < 0.1716: the first term left out is below 3e-13 of the result's scale)
WSPR_HD double synth_log(double u) {
    const double ln2 = 6.93147180559945286227e-01;
    uint64_t b = f64_bits(u);
    int e = (int)((b >> 52) & 0x7ff) - 1023;
    b = (b & 0x000fffffffffffffull) | 0x3ff0000000000000ull;     // m in [1, 2)
    if ((b & 0x000fffffffffffffull) > 0x0006a09e667f3bccull) { b -= 0x0010000000000000ull; e += 1; }   // m > sqrt 2: halve
    union { uint64_t u; double d; } v;
    v.u = b;
    const double f = v.d - 1.0;
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double p = 1.0 / 3.0 + z * (1.0 / 5.0 + z * (1.0 / 7.0 + z * (1.0 / 9.0 + z * (1.0 / 11.0 + z * (1.0 / 13.0 + z * (1.0 / 15.0))))));
    return (double)e * ln2 + (2.0 * s + 2.0 * s * z * p);
}
// One complex float32 Gaussian draw for the Philox counter (c0, c1, segment low, segment high) under the seed's key:
// nI, nQ are N(0, sigma^2), independent.  Counter word 1 names the stream: 0 is the noise (synth_noise()), 1 + 2q + p the
// white impulses of path p of a segment's q-th transmission (fade.h).
WSPR_HD void synth_gauss(uint64_t seed, int64_t segment, uint32_t c0, uint32_t c1, float sigma, float* nI, float* nQ) {
    uint32_t r[4];
    synth_philox(c0, c1, (uint32_t)(uint64_t)segment, (uint32_t)((uint64_t)segment >> 32),
                 (uint32_t)seed, (uint32_t)(seed >> 32), r);
    // u in (0, 1] from 64 bits, theta in (0, 2 pi) from 32
    const double u = (((double)r[0] * 4294967296.0 + (double)r[1]) + 1.0) * 5.42101086242752217004e-20;   // 2^-64
    const double rad = __builtin_sqrt(-2.0 * synth_log(u));
    const float theta = (float)(((double)r[2] + 0.5) * 1.46291807926715968105e-09);                        // 2 pi / 2^32
    float sn, cs;
    glibc_sincosf_pair(theta, &sn, &cs);
    const float radf = (float)rad;
    *nI = (radf * cs) * sigma;
    *nQ = (radf * sn) * sigma;
}
// One complex draw for (seed, global segment, sample): nI, nQ are float32 N(0, sigma^2), independent.
WSPR_HD void synth_noise(uint64_t seed, int64_t segment, int sample, float sigma, float* nI, float* nQ) {
    synth_gauss(seed, segment, (uint32_t)sample, 0u, sigma, nI, nQ);
}

// ---- exponential ----------------------------------------------------------------------------------------------------
// exp(x) for -40 <= x <= 0 (the Gaussian pulse of the fading channel, fade.h): x = k ln 2 + r with k = x / ln 2 rounded
// to an integer and ln 2 in two pieces (the first has 32 bits, so k * ln2_hi is exact for |k| <= 58), |r| <= 0.3466;
// exp(r) as its Taylor polynomial to r^12 by Horner's rule (the first term left out is below 1.7e-16 of the result);
// the factor 2^k goes into the exponent bits (the result stays normal: exp(-40) = 2^-57.7).
WSPR_HD double synth_exp(double x) {
    const double invln2 = 1.44269504088896338700e+00;
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double magic = 6755399441055744.0;               // 1.5 * 2^52: (t + magic) - magic = t rounded to an integer
    const double fk = (x * invln2 + magic) - magic;
    const double r = (x - fk * ln2_hi) - fk * ln2_lo;
    double p = 1.0 / 479001600.0;
    p = 1.0 / 39916800.0 + r * p;
    p = 1.0 / 3628800.0 + r * p;
    p = 1.0 / 362880.0 + r * p;
    p = 1.0 / 40320.0 + r * p;
    p = 1.0 / 5040.0 + r * p;
    p = 1.0 / 720.0 + r * p;
    p = 1.0 / 120.0 + r * p;
    p = 1.0 / 24.0 + r * p;
    p = 1.0 / 6.0 + r * p;
    p = 0.5 + r * p;
    p = 1.0 + r * p;
    p = 1.0 + r * p;
    union { uint64_t u; double d; } v;
    v.d = p;
    v.u += (uint64_t)(int64_t)(int)fk << 52;               // k <= 0: the shift is on the unsigned value
    return v.d;
}

}  // namespace wspr
