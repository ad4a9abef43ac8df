/* K18, IQ to audio: THE DEFINITION, shared by the kernel (k18_iq_audio.hip) and by the serial checker
 * (tests/helpers/iq_audio_check.c).  Plain C.  The decoder's 375 Hz IQ rows back to the 16-bit records at 12 000 Hz with the
 * band at 1 500 Hz that K12 (audio_front.h), K15, wsprd and a sound card take.  It is the transpose of K12 over K12's own
 * two tap tables (audio_front_gi_bits, audio_front_gq_bits): no table of its own.  The reference has no audio output; this
 * arithmetic is the project's own and wspr_set_arithmetic() does not touch it.
 *
 * Input   I[0 .. np), Q[0 .. np): float at 375 Hz, np <= 45 000; any bit pattern (non-finite values included).
 * Output  pcm[0 .. 32 np): signed 16-bit mono at 12 000 Hz, and the number of clipped samples of the record.
 *
 * Output sample n:
 *   acc = +0.0f
 *   for every m with 0 <= m < np and |n - 32 m| <= 255, IN RISING m, with k = n - 32 m:
 *       acc = fmaf(gI[k], I[m], acc)        unless k = 2, 6 (mod 8)
 *       acc = fmaf(gQ[k], Q[m], acc)        unless k = 0, 4 (mod 8)
 *   y = 16.0f * acc
 *   p = (double)y * (double)gain
 *   p is NaN:   the sample is 0 and counts as clipped
 *   otherwise:  p > 32767.0 gives 32767, p < -32768.0 gives -32768, and either counts as clipped; else the sample is
 *               (p + 6755399441055744.0) - 6755399441055744.0 -- nearest, ties to even: pcm_quantise() of pcm_quantise.h,
 *               which K17's audio_synth_quantise() is as well.
 * fmaf is the single rounding rule of the chain and nothing else is fused or reordered (-ffp-contract=off on both sides).
 *
 * THE SKIPPED STEPS ARE PART OF THE DEFINITION.  gI[k] for k = 2, 6 (mod 8) and gQ[k] for k = 0, 4 (mod 8) are +0.0f
 * (audio_front.h).  K12 may skip them because its input is finite; here I[m] may be Inf or NaN, fmaf(+0, Inf, acc) is NaN,
 * and so a step on a stated zero is NOT PART OF THE CHAIN.  As 32 m = 0 (mod 8), k = n (mod 8): output n takes the I rail
 * alone for n = 0, 4 (mod 8), the Q rail alone for n = 2, 6 (mod 8) and both for odd n.  At most 16 values of m and 24
 * multiply-adds per output.
 *
 * Scale and timing.  The taps carry K12's factor 2 and every 32nd tap of h sums to 1/32 of its DC gain 1, so the factor 16
 * makes a phasor A e^{+j 2 pi f m / 375} leave as the cosine A cos(2 pi (1500 + f) n / 12000): +f in the decoder's convention is
 * audio at 1500 + f Hz, and K18 followed by K12 is the identity inside the search band (K12's pass-band ripple, twice, and
 * the 16-bit rounding).  gain = 32768 is the inverse of K12's 2^-15.  Output n = 32 m is centred on input m: no delay is
 * added in either direction.
 *
 * IQ_AUDIO_TILE is the kernel's outputs per workgroup (64 inputs and a halo of 8 on each side): the lengths worth testing
 * sit around its multiples. */
#ifndef WSPR_IQ_AUDIO_H
#define WSPR_IQ_AUDIO_H
#include <stdint.h>

#include "audio_front.h"
#include "pcm_quantise.h"

#define IQ_AUDIO_INTERP      AUDIO_FRONT_DECIM      /* output samples per input sample */
#define IQ_AUDIO_MAX_SAMPLES AUDIO_FRONT_MAX_OUT    /* inputs of a row: 45 000 */
#define IQ_AUDIO_TILE        2048                   /* outputs per workgroup of k18_iq_audio.hip */
#if defined(__HIPCC__) || defined(__CUDACC__)
#define IQ_AUDIO_HD __host__ __device__ static inline
#else
#define IQ_AUDIO_HD static inline
#endif
#ifdef __cplusplus
#define IQ_AUDIO_CONSTEXPR constexpr                /* the kernel checks its choice of rails at compile time */
#else
#define IQ_AUDIO_CONSTEXPR
#endif

/* is the step on tap k (-255 .. 255) of rail 0 = I, 1 = Q outside the chain?  (k & 7 is k mod 8, non-negative) */
IQ_AUDIO_CONSTEXPR IQ_AUDIO_HD int iq_audio_skipped(int rail, int k) {
    return rail ? ((k & 7) == 0 || (k & 7) == 4) : ((k & 7) == 2 || (k & 7) == 6);
}

/* the last three lines of the definition; *clipped is incremented for a sample that leaves the 16-bit range or is NaN */
IQ_AUDIO_HD int16_t iq_audio_quantise(double p, int *clipped) {
    if (p != p) { ++*clipped; return (int16_t)0; }
    return pcm_quantise(p, clipped);
}
IQ_AUDIO_HD int16_t iq_audio_sample(float acc, float gain, int *clipped) {
    const float y = 16.0f * acc;
    const double p = (double)y * (double)gain;
    return iq_audio_quantise(p, clipped);
}

#if !defined(__HIPCC__) && !defined(__CUDACC__)
#include <math.h>
/* the chain of output n (0 .. 32 np - 1) of one row, serially: the checker's, and anybody's who wants one sample */
static inline float iq_audio_chain(const float *I, const float *Q, int np, long n) {
    float acc = 0.0f;
    const long b = n / IQ_AUDIO_INTERP;
    for (long m = b - 8; m <= b + 8; ++m) {
        const long k = n - IQ_AUDIO_INTERP * m;
        if (m < 0 || m >= np || k < -AUDIO_FRONT_K || k > AUDIO_FRONT_K) continue;
        if (!iq_audio_skipped(0, (int)k)) acc = fmaf(audio_front_tap(0, (int)k), I[m], acc);
        if (!iq_audio_skipped(1, (int)k)) acc = fmaf(audio_front_tap(1, (int)k), Q[m], acc);
    }
    return acc;
}
#endif
#endif
