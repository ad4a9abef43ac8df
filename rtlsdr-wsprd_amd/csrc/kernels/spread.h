// The Doppler-spread figure of a decoded spot (K11, wspr_spread_batch(), wspr_set_spread_estimate()), written once for the
// device and for a CPU.  There is no reference behaviour to match: the definition is this project's own, stated here and
// repeated in include/wspr_mi355x.h; tests/helpers/spread_check.c is its serial form over the functions of this header.
//
// For one job (seg, f0, shift, drift, symbols[162]) over a row of np samples:
//   1. Phase.   phi is the synthesiser's serial recurrence (synth_math.h, include/wspr_mi355x.h at wspr_synth_tx): phi =
//               0.0, and for symbol i, sample j: use phi, then phi += dphi_i, dphi_i = synth_dphi(f0, drift, i, symbols[i]).
//               The recurrence is run as written (checkpoints plus a walk), never replaced by a prefix sum.
//               (sn, cs) = synth_sincos(phi).
//   2. Wipe.    n = 256 i + j, k = shift + n:  zr = (double)I[k]*cs + (double)Q[k]*sn,  zi = (double)Q[k]*cs - (double)I[k]*sn,
//               unfused doubles; a sample with k < 0 or k >= np counts as I = Q = 0 (zr = zi = 0).
//   3. Blocks.  y[b], b = 0 .. 1295 = the sum of z over samples 32b .. 32b+31, each rail in double, in sample order from
//               0.0, rounded once to float.
//   4. Spectrum.  y zero-padded to 2 048 points; complex float32 radix-2 decimation-in-frequency FFT, stages 0 .. 10 of
//               spread_butterfly() below, no fused multiply-add; twiddles (float)cos(2 pi m/2048), (float)(-sin(2 pi m/2048))
//               from the host libm in double (spread_twiddles()).  P[j] = re*re + im*im in float, separately rounded; j is
//               the bin's signed index -1024 .. 1023, bin j lies at j * kDelta Hz, kDelta = 375/32/2048.
//   5. Width.   In double, and THE ORDER OF ADDITIONS IS PART OF THE DEFINITION: bins are taken in chunks of 16 consecutive
//               j, a chunk is summed serially from 0.0 in rising j, chunk totals are accumulated serially in rising chunk
//               order.  Noise floor nz = (the 40 chunks covering 640 <= |j| <= 959, negative side first: chunk c < 20
//               starts at j = -959 + 16c, chunk 20 + c at 640 + 16c) / 640.  Signal region j = -512 .. 511, 64 chunks,
//               Q[j] = (double)P[j] - nz, tot = the accumulated total of the 64 chunk totals.  For q = 0.25, 0.5, 0.75: the
//               first chunk whose running total reaches q*tot, inside it the first bin whose running sum (the chunk's
//               start value plus the serial partial sum) reaches it, f_q = (j - 0.5 + (q*tot - C_before) / Q[j]) * kDelta.
//               w50 = (float)(f_75 - f_25), f50 = (float)f_50, ratio = (float)(max P[j] of the signal region / nz).
//               valid = 1 if nz > 0, tot > 0, the three crossings exist and every number involved is finite; else
//               valid = 0 and the three floats are 0.
// wspr_set_arithmetic() does not touch any of this: it is a measurement, not part of the reference's arithmetic.
#pragma once
#include <stdint.h>

#include "synth_math.h"

#include <math.h>

namespace wspr {
namespace spread {

constexpr int kBlockLen = 32;                              // samples per block sum
constexpr int kBlocks = kSynthSigLen / kBlockLen;          // 1 296
constexpr int kFft = 2048, kStages = 11, kTwiddles = kFft / 2;
constexpr int kChunk = 16, kNoiseChunks = 40, kSignalChunks = 64;
constexpr int kNoiseLo = 640, kNoiseHi = 959, kSignalLo = -512;
constexpr int kShiftClamp = 1 << 20;                       // a shift beyond it lies off the row just the same
constexpr double kDelta = 375.0 / 32.0 / 2048.0;           // Hz per bin, 0.005722...

struct Result {
    float w50, f50, ratio;
    int32_t valid;
};

// tw[2m], tw[2m+1] = the real and imaginary part of exp(-2 pi i m / 2048), m = 0 .. 1023, from the host libm
#if defined(__HIPCC__)
__host__
#endif
static inline void spread_twiddles(float* tw) {
    for (int m = 0; m < kTwiddles; ++m) {
        const double a = 2.0 * 3.14159265358979323846 * (double)m / 2048.0;
        tw[2 * m] = (float)cos(a);
        tw[2 * m + 1] = (float)(-sin(a));
    }
}

WSPR_HD int clamp_shift(int shift) { return shift < -kShiftClamp ? -kShiftClamp : (shift > kShiftClamp ? kShiftClamp : shift); }

// One block sum: the 32 wiped samples from xi / xq (stride 1; the row's samples, 0.0f where the row has none), the phase
// at the block's first sample.  Returns the phase after the block.
WSPR_HD double spread_block(const float* xi, const float* xq, double phi, double dphi, float* yr, float* yi) {
    double sr = 0.0, si = 0.0;
    for (int s = 0; s < kBlockLen; ++s) {
        double sn, cs;
        synth_sincos(phi, &sn, &cs);
        const double a = (double)xi[s], b = (double)xq[s];
        const double zr = a * cs + b * sn;
        const double zi = b * cs - a * sn;
        sr += zr;
        si += zi;
        phi += dphi;
    }
    *yr = (float)sr;
    *yi = (float)si;
    return phi;
}

// Butterfly t (0 .. 1023) of stage `stage` (0 .. 10) of the in-place decimation-in-frequency transform: natural order
// in, bit-reversed order out.  The butterflies of a stage are independent; a stage needs the one before it complete.
WSPR_HD void spread_butterfly(float* re, float* im, const float* tw, int stage, int t) {
    const int half = (kFft / 2) >> stage;
    const int k = t & (half - 1);
    const int i = ((t - k) << 1) + k;
    const int m = k << stage;
    const float wr = tw[2 * m], wi = tw[2 * m + 1];
    const float ar = re[i], ai = im[i], br = re[i + half], bi = im[i + half];
    const float dr = ar - br, di = ai - bi;
    re[i] = ar + br;
    im[i] = ai + bi;
    re[i + half] = dr * wr - di * wi;
    im[i + half] = dr * wi + di * wr;
}

// where bin j (-1024 .. 1023) lies after the transform
WSPR_HD int spread_slot(int j) {
    unsigned u = (unsigned)j & (unsigned)(kFft - 1);
    u = ((u & 0x5555u) << 1) | ((u >> 1) & 0x5555u);
    u = ((u & 0x3333u) << 2) | ((u >> 2) & 0x3333u);
    u = ((u & 0x0f0fu) << 4) | ((u >> 4) & 0x0f0fu);
    u = ((u & 0x00ffu) << 8) | ((u >> 8) & 0x00ffu);
    return (int)(u >> 5);                                  // 16 reversed bits -> the 11 that count
}
WSPR_HD float spread_power(const float* re, const float* im, int j) {
    const int p = spread_slot(j);
    const float a = re[p], b = im[p];
    const float aa = a * a, bb = b * b;
    return aa + bb;
}

WSPR_HD int noise_chunk_start(int c) { return c < kNoiseChunks / 2 ? -kNoiseHi + kChunk * c : kNoiseLo + kChunk * (c - kNoiseChunks / 2); }
WSPR_HD double spread_noise_chunk(const float* re, const float* im, int c) {
    const int j0 = noise_chunk_start(c);
    double s = 0.0;
    for (int k = 0; k < kChunk; ++k) s += (double)spread_power(re, im, j0 + k);
    return s;
}
WSPR_HD double spread_noise_floor(const double* chunks) {
    double s = 0.0;
    for (int c = 0; c < kNoiseChunks; ++c) s += chunks[c];
    return s / 640.0;
}
// total of signal chunk c (bins -512 + 16c ...) and the largest power in it
WSPR_HD double spread_signal_chunk(const float* re, const float* im, int c, double nz, float* maxp) {
    const int j0 = kSignalLo + kChunk * c;
    double s = 0.0;
    float mx = 0.0f;
    for (int k = 0; k < kChunk; ++k) {
        const float p = spread_power(re, im, j0 + k);
        if (p > mx) mx = p;
        s += (double)p - nz;
    }
    *maxp = mx;
    return s;
}

WSPR_HD bool spread_finite(double v) { return ((f64_bits(v) >> 52) & 0x7ff) != 0x7ff; }

// the crossing of q*tot; false if there is none
WSPR_HD bool spread_crossing(const float* re, const float* im, const double* sig, double nz, double target, double* f) {
    double run = 0.0;
    for (int c = 0; c < kSignalChunks; ++c) {
        const double after = run + sig[c];
        if (after >= target) {
            const int j0 = kSignalLo + kChunk * c;
            double part = 0.0;
            for (int k = 0; k < kChunk; ++k) {
                const double before = run + part;
                const double qj = (double)spread_power(re, im, j0 + k) - nz;
                part += qj;
                if (run + part >= target) {
                    *f = ((double)(j0 + k) - 0.5 + (target - before) / qj) * kDelta;
                    return true;
                }
            }
            return false;                                  // (a NaN in the chunk: the comparisons above all fail)
        }
        run = after;
    }
    return false;
}

// sig: the 64 signal chunk totals, maxp: the 64 chunk maxima
WSPR_HD Result spread_width(const float* re, const float* im, const double* sig, const float* maxp, double nz) {
    Result r;
    r.w50 = 0.0f; r.f50 = 0.0f; r.ratio = 0.0f; r.valid = 0;
    double tot = 0.0;
    float mx = 0.0f;
    for (int c = 0; c < kSignalChunks; ++c) {
        tot += sig[c];
        if (maxp[c] > mx) mx = maxp[c];
    }
    if (!(nz > 0.0) || !(tot > 0.0) || !spread_finite(nz) || !spread_finite(tot)) return r;
    double f25 = 0.0, f50 = 0.0, f75 = 0.0;
    if (!spread_crossing(re, im, sig, nz, 0.25 * tot, &f25)) return r;
    if (!spread_crossing(re, im, sig, nz, 0.5 * tot, &f50)) return r;
    if (!spread_crossing(re, im, sig, nz, 0.75 * tot, &f75)) return r;
    const double ratio = (double)mx / nz;
    if (!spread_finite(f25) || !spread_finite(f50) || !spread_finite(f75) || !spread_finite(ratio)) return r;
    const float w = (float)(f75 - f25), fm = (float)f50, rt = (float)ratio;
    if (!spread_finite((double)w) || !spread_finite((double)fm) || !spread_finite((double)rt)) return r;
    r.w50 = w; r.f50 = fm; r.ratio = rt; r.valid = 1;
    return r;
}

}  // namespace spread
}  // namespace wspr
