// The HF fading channel of the signal synthesiser (K13, wspr_synth_faded*()), written once for the device and for a CPU.
// The definition is stated in full in include/wspr_mi355x.h ("fading channel"); tests/helpers/fade_check.cpp is its serial
// form.  Like synth_math.h: fixed sequences of IEEE-754 double operations, no maths library, -ffp-contract=off.
//
// A transmission's complex gain is G[n] = G_0[n] + G_1[n], n its own sample index.  A path is skipped (gain == 0), specular
// (sigma == 0: the constant gain) or diffuse (sigma > 0): white complex Gaussian impulses W[k], one every L samples,
// through a Gaussian pulse of standard deviation s samples -- sixteen terms per sample.  A non-zero shift rotates the
// path by w * n.  W[k] is a pure function of (seed, global segment S, ordinal q of the transmission in its segment,
// path p, k), so a realisation does not depend on how a job is split.
//
//   fade_path_setup()  the per-path constants from (gain, shift, sigma): evaluated on the HOST (wspr_capi_synth.hip) and in
//                      the checker, never on the device, so the device needs no double division or square root here
//   fade_draw()        W[k]
//   fade_sum()         the sixteen terms of one sample over W[kc-7 .. kc+8]
//   fade_rotate()      the shift
//   fade_apply()       step 3 of the synthesiser's contract with a gain
#pragma once
#include <stdint.h>

#include "synth_math.h"

#if defined(__HIPCC__)
#define WSPR_FADE_UNROLL _Pragma("unroll 2")   // two exponentials in flight; the sums stay in rising k
#else
#define WSPR_FADE_UNROLL
#endif

namespace wspr {

constexpr int kFadeTerms = 16;                 // k = kc-7 .. kc+8
constexpr int kFadeBelow = 7;
constexpr int kFadeKindSkipped = 0, kFadeKindSpecular = 1, kFadeKindDiffuse = 2;
constexpr float kFadeMinSigma = 0.001f, kFadeMaxSigma = 10.0f, kFadeMaxShift = 100.0f;

struct FadeTap { float re, im; };              // one W[k]
struct FadePath {                              // 32 bytes, derived from wspr_synth_path
    double beta;                               // diffuse: 1 / (2 s^2)
    double c;                                  // diffuse: gain / sqrt(2 s sqrt(pi) / L); specular: gain
    double w;                                  // rad per sample of the shift; used if shifted
    int32_t L;                                 // diffuse: spacing of the impulses, >= 4
    int16_t kind, shifted;
};
struct FadeChannel { FadePath path[2]; };      // 64 bytes, one per transmission

WSPR_HD FadePath fade_path_setup(float gain, float shift, float sigma) {
    FadePath p;
    p.beta = 0.0; p.c = (double)gain; p.w = 0.0; p.L = 1;
    p.kind = (int16_t)(gain == 0.0f ? kFadeKindSkipped : (sigma > 0.0f ? kFadeKindDiffuse : kFadeKindSpecular));
    p.shifted = (int16_t)(shift != 0.0f);
    if (p.kind == kFadeKindDiffuse) {
        const double s = 375.0 / ((2.0 * 1.4142135623730951 * 3.14159265358979323846) * (double)sigma);
        p.L = (int32_t)s;
        p.beta = 1.0 / (2.0 * s * s);
        p.c = (double)gain / __builtin_sqrt(2.0 * (s * 1.7724538509055159) / (double)p.L);
    }
    if (p.shifted) p.w = 2.0 * 3.14159265358979323846 * (1 / 375.0) * (double)shift;
    return p;
}

// W[k] of path p of the q-th transmission of global segment S: unit variance per rail
WSPR_HD FadeTap fade_draw(uint64_t seed, int64_t S, int q, int p, int k) {
    FadeTap t;
    synth_gauss(seed, S, (uint32_t)(k + 16), (uint32_t)(1 + 2 * q + p), 1.0f, &t.re, &t.im);
    return t;
}

// c * sum over the sixteen impulses W[0 .. 15] = W[kc-7 .. kc+8] around sample n, kc = n / L; d0 = n - (kc-7) * L
template <class Taps>
WSPR_HD void fade_sum(Taps W, int d0, int L, double beta, double c, double* re, double* im) {
    double sr = 0.0, si = 0.0;
    int d = d0;
    WSPR_FADE_UNROLL
    for (int j = 0; j < kFadeTerms; ++j) {
        const FadeTap t = W[j];
        const double e = synth_exp(-((double)d * (double)d) * beta);
        sr += (double)t.re * e;
        si += (double)t.im * e;
        d -= L;
    }
    *re = c * sr;
    *im = c * si;
}

WSPR_HD void fade_rotate(double w, int n, double* re, double* im) {
    double ss, cc;
    synth_sincos(w * (double)n, &ss, &cc);
    const double a = *re, b = *im;
    *re = a * cc - b * ss;
    *im = a * ss + b * cc;
}

// x = (float)((double)x + amp * (the transmitter's phasor (cs, sn) times G)), both rails
WSPR_HD void fade_apply(double amp, double sn, double cs, double gre, double gim, float* xi, float* xq) {
    *xi = (float)((double)*xi + amp * (cs * gre - sn * gim));
    *xq = (float)((double)*xq + amp * (sn * gre + cs * gim));
}

}  // namespace wspr
