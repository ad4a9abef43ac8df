// The band noise figures of one segment (K16, wspr_noise_batch_device(), wspr_noise()): THE DEFINITION, written once for
// the kernel (k16_noise.hip) and for a CPU; tests/helpers/noise_check.c is its serial form over the functions of this
// header, and include/wspr_mi355x.h repeats it.  There is no reference behaviour to match (the reference's noise_level,
// wsprd.c:590-616, is internal, taken on a smoothed +-150 Hz spectrum, and only enters the SNR): the definition is this
// project's own, after the two figures wsprdaemon-style receiver farms log per two-minute slot and band.
//
// For one row of np samples (0 .. 45 000) of I and Q at 375 samples per second:
//   0. Guard.    If any I[k] or Q[k] with k < np has exponent bits 0xff (an integer test on the bit pattern: NaN, +Inf, -Inf),
//                every float of the result is 0 and flags = kNonFinite alone; nframes is still reported.  Everything below
//                therefore sees finite input only.
//   1. Gap figure (the "RMS" one).  Block b = samples 16b .. 16b+15 (42.7 ms, the stand-in for sox's 50 ms trough window).
//                p[b] = (float)(S / 16.0), S the double sum, in sample order from 0.0, of (double)I*(double)I +
//                (double)Q*(double)Q, unfused.  A window is a block range [b0, b1), 0 <= b0 <= b1 <= 2812, clipped to the
//                blocks that lie wholly inside [0, np): [b0, min(b1, np / 16)).  mean = (float)(the double sum of
//                (double)p[b] in rising b from 0.0 / (double)count); trough = the minimum p[b]: m = p[b0], then
//                "if (p < m) m = p" in rising b.  A window that is empty (after clipping as well) gives 0 for both and
//                leaves its flag bit clear.  The two windows (pre, post) are arguments, not state.
//   2. Spectrum figure (the "FFT" one).  Frames of 512 samples at hop 256: nframes = np >= 512 ? (np - 512)/256 + 1 : 0
//                (174 for a full row); frame f holds the samples 256f .. 256f+511.
//                Window w[n] = (float)(0.5 - 0.5*cos(2 pi n/512)), twiddles (float)cos(2 pi m/512), (float)(-sin(2 pi m/512)),
//                m = 0 .. 255, both from the host libm in double (noise_tables()).
//                x[n] = (I[256f+n]*w[n], Q[256f+n]*w[n]) as float products; the 512-point complex float32 radix-2
//                decimation-in-frequency transform, stages 0 .. 8 of noise_butterfly() below (the statements of
//                spread_butterfly(), spread.h), no fused multiply-add.  P_f[j] = re*re + im*im in float, separately
//                rounded; j is the signed bin -256 .. 255, bin j lies at j * 375/512 Hz.
//                A[j], the double sum of (double)P_f[j] over the frames, and THE ORDER OF ITS ADDITIONS IS PART OF THE
//                DEFINITION: four partial sums, S_c[j] (c = 0 .. 3) = the sum from 0.0 over the frames f = c, c+4, c+8, ...
//                below nframes in rising f; A[j] = ((S_0[j] + S_1[j]) + S_2[j]) + S_3[j].  (Four waves of the kernel take
//                one class of frames each.)
//                a[j] = (float)(A[j] / (double)nframes / W2), W2 = the double sum of (double)w[n]*(double)w[n] in rising n
//                from 0.0.  With this scaling white noise of per-rail variance s^2 gives E a[j] = 2 s^2: the scale of
//                the gap figure.
//                The 443 bins j = -221 .. 221 (+-161.9 Hz: the 1338 .. 1662 Hz of the audio world) are ranked by their
//                uint32 bit pattern (finite and >= +0: that order is the numeric one), ties go to the lower j.
//                fft_floor = (float)(the double sum of the 132 lowest, in rank order from 0.0 / 132.0): the quietest 30 %.
//                fft_p30 = the value of rank 132.  nframes == 0 gives 0 for both and leaves the flag bit clear.
//   Flags        bit 0 pre window used, bit 1 post window used, bit 2 spectrum used, bit 3 kNonFinite.
// All powers are linear, per complex sample, relative to the row's own scale: UNCALIBRATED, and meaningless in absolute
// terms on a row that was normalised to a peak of 0.5.  wspr_set_arithmetic() does not touch any of this: it is a
// measurement, not part of the reference's arithmetic.
#pragma once
#include <stdint.h>

#include "glibc_sincosf.h"   // WSPR_HD, f32_bits()

#include <math.h>

namespace wspr {
namespace noise {

constexpr int kMaxSamples = 45000;
constexpr int kBlockLen = 16;                              // samples per block of the gap figure
constexpr int kBlocks = kMaxSamples / kBlockLen;           // 2 812
constexpr int kFft = 512, kStages = 9, kTwiddles = kFft / 2, kFrameHop = 256;
constexpr int kClasses = 4;                                // partial sums of A[j]: frames f with f % 4 == c
constexpr int kBandHalf = 221, kBand = 2 * kBandHalf + 1;  // the 443 ranked bins
constexpr int kLowest = 132;                               // the quietest 30 % of 443
constexpr int kTableFloats = 2 * kTwiddles + kFft;         // twiddles, then the window
constexpr int kPreUsed = 1, kPostUsed = 2, kSpectrumUsed = 4, kNonFinite = 8;

// The default windows.  wsprdaemon measures 0.25-0.75 s and 113-118 s of a wav file whose transmissions start 1 s into
// the record; in this library's rows a transmission with dt = 0 starts at 2.0 s (wspr_selftest() places a signal of dt = 0
// at sample 2.0 * 375 = 750, "dt = t0 - 2.0"), one second later.  So the windows move by one second: blocks 6 .. 41
// (0.256 .. 1.792 s, all before the 2.0 s at which the earliest on-time transmission starts) and 2672 .. 2789 (114.005 ..
// 119.040 s: a transmission of 110.6 s that started at 2.0 s, or up to a second late, has ended by 113.6 s).
constexpr int kPreB0 = 6, kPreB1 = 42, kPostB0 = 2672, kPostB1 = 2790;

struct Windows {
    int32_t pre_b0, pre_b1, post_b0, post_b1;
};
struct Result {
    float pre_mean, pre_trough, post_mean, post_trough, fft_floor, fft_p30;
    int32_t nframes, flags;
};

WSPR_HD bool windows_ok(int b0, int b1) { return 0 <= b0 && b0 <= b1 && b1 <= kBlocks; }
WSPR_HD int frames_of(int np) { return np >= kFft ? (np - kFft) / kFrameHop + 1 : 0; }
WSPR_HD int whole_blocks(int np) { return np / kBlockLen; }
WSPR_HD bool non_finite(float v) { return ((f32_bits(v) >> 23) & 0xffu) == 0xffu; }

// table[2m], table[2m+1] = the real and imaginary part of exp(-2 pi i m / 512), m = 0 .. 255; table[512 + n] = w[n];
// returns W2.  From the host libm.
#if defined(__HIPCC__)
__host__
#endif
static inline double noise_tables(float* table) {
    for (int m = 0; m < kTwiddles; ++m) {
        const double a = 2.0 * 3.14159265358979323846 * (double)m / 512.0;
        table[2 * m] = (float)cos(a);
        table[2 * m + 1] = (float)(-sin(a));
    }
    double w2 = 0.0;
    for (int n = 0; n < kFft; ++n) {
        const float w = (float)(0.5 - 0.5 * cos(2.0 * 3.14159265358979323846 * (double)n / 512.0));
        table[2 * kTwiddles + n] = w;
        const double ww = (double)w * (double)w;
        w2 += ww;
    }
    return w2;
}

// p[b] of one block: 16 samples of each rail, stride 1
WSPR_HD float block_power(const float* xi, const float* xq) {
    double s = 0.0;
    for (int k = 0; k < kBlockLen; ++k) {
        const double a = (double)xi[k], b = (double)xq[k];
        const double aa = a * a, bb = b * b;
        const double e = aa + bb;
        s += e;
    }
    return (float)(s / 16.0);
}

// mean and trough of the window [b0, b1) over p[]; false (and zeros) if it is empty
WSPR_HD bool window_figures(const float* p, int b0, int b1, float* mean, float* trough) {
    *mean = 0.0f;
    *trough = 0.0f;
    if (b1 <= b0) return false;
    double s = 0.0;
    float m = p[b0];
    for (int b = b0; b < b1; ++b) {
        const float v = p[b];
        s += (double)v;
        if (v < m) m = v;
    }
    *mean = (float)(s / (double)(b1 - b0));
    *trough = m;
    return true;
}

// Butterfly t (0 .. 255) of stage `stage` (0 .. 8) of the in-place decimation-in-frequency transform: natural order in,
// bit-reversed order out.  The butterflies of a stage are independent; a stage needs the one before it complete.
// The butterfly on values, (a, b) -> (a + b, (a - b) w): THE statements, for a transform that keeps its points in registers
// (the kernel) and for one that keeps them in an array (noise_butterfly() below).
WSPR_HD void butterfly_values(float* ar, float* ai, float* br, float* bi, float wr, float wi) {
    const float dr = *ar - *br, di = *ai - *bi;
    *ar = *ar + *br;
    *ai = *ai + *bi;
    *br = dr * wr - di * wi;
    *bi = dr * wi + di * wr;
}
WSPR_HD void noise_butterfly(float* re, float* im, const float* tw, int stage, int t) {
    const int half = (kFft / 2) >> stage;
    const int k = t & (half - 1);
    const int i = ((t - k) << 1) + k;
    const int m = k << stage;
    butterfly_values(&re[i], &im[i], &re[i + half], &im[i + half], tw[2 * m], tw[2 * m + 1]);
}

// the signed bin (-256 .. 255) that slot p (0 .. 511) of the transform's output holds: nine bits reversed
WSPR_HD int bin_of_slot(int p) {
    unsigned u = (unsigned)p & 0x1ffu;
    u = ((u & 0x5555u) << 1) | ((u >> 1) & 0x5555u);
    u = ((u & 0x3333u) << 2) | ((u >> 2) & 0x3333u);
    u = ((u & 0x0f0fu) << 4) | ((u >> 4) & 0x0f0fu);
    u = ((u & 0x00ffu) << 8) | ((u >> 8) & 0x00ffu);
    u >>= 7;                                               // 16 reversed bits -> the 9 that count
    return u < 256u ? (int)u : (int)u - kFft;
}
WSPR_HD float slot_power(float re, float im) {
    const float aa = re * re, bb = im * im;
    return aa + bb;
}
// A[j] of the four partial sums, and a[j]
WSPR_HD double join_classes(double s0, double s1, double s2, double s3) { return ((s0 + s1) + s2) + s3; }
WSPR_HD float bin_level(double a, int nframes, double w2) { return (float)(a / (double)nframes / w2); }

// the rank of entry i among the kBand bit patterns v[]: the entries that precede it (ties: the lower index first)
WSPR_HD int band_rank(const uint32_t* v, int i) {
    const uint32_t mine = v[i];
    int r = 0;
    for (int k = 0; k < kBand; ++k) r += (v[k] < mine || (v[k] == mine && k < i)) ? 1 : 0;
    return r;
}
// sorted: the kBand bit patterns in rank order
WSPR_HD float band_floor(const uint32_t* sorted) {
    double s = 0.0;
    for (int k = 0; k < kLowest; ++k) {
        union { uint32_t u; float f; } v;
        v.u = sorted[k];
        s += (double)v.f;
    }
    return (float)(s / 132.0);
}

}  // namespace noise
}  // namespace wspr
