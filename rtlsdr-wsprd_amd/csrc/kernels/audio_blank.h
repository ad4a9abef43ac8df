/* K15, the impulse-noise blanker of the audio front end: THE DEFINITION, shared by the kernel (k15_blank.hip) and by the
 * serial checker (tests/helpers/blank_check.c).  Plain C, integer arithmetic only: there is no rounding to agree on, the
 * kernel and the checker are equal bit for bit by construction.  It acts on the 12 kHz samples, BEFORE the narrow filter
 * of K12 (audio_front.h) smears a spike of a few samples over 43 ms of the 375 Hz IQ.
 *
 * Input   pcm[0 .. nsamp): signed 16-bit, nsamp <= 1 440 000.   a[n] = |pcm[n]| as an int (-32768 gives 32768).
 * Blocks  block b holds the samples 8192 b .. min(8192 (b + 1), nsamp) - 1 (8192 samples = one WSPR symbol at 12 kHz);
 *         c_b is its sample count, the last block may be short.
 * Level   L_b = the LOWER MEDIAN of the block's a[]: the element of 0-based rank (c_b - 1) / 2 in non-decreasing order,
 *         over the block's own samples inside the record only.
 * Rule    for n in block b:  out[n] = 0  if  L_b > 0  and some n' with max(0, n - G) <= n' <= min(nsamp - 1, n + G) has
 *         16 a[n'] > thr16 L_b  (strict, in int32: the largest product is 2^27);  otherwise out[n] = pcm[n].
 *         thr16 = 16 .. 4096 is the threshold in sixteenths of the level, G = guard = 0 .. 64 samples.
 *         THE LEVEL IS THAT OF THE OUTPUT SAMPLE'S BLOCK: a neighbour n' in the next or the previous block is judged by
 *         L_b too (so a workgroup that owns a block and a halo of G samples needs nothing from its neighbours; at a block
 *         edge the rule is asymmetric, and the tests pin that).  A block with L_b == 0 (digital silence) is copied.
 * Count   n_blanked = the number of n of the record for which the condition held, whatever pcm[n] was.
 * Padding the columns nsamp .. roundup8(nsamp) - 1 of the output row are written 0; what lies behind is left alone. */
#ifndef WSPR_AUDIO_BLANK_H
#define WSPR_AUDIO_BLANK_H
#include <stdint.h>

#define AUDIO_BLANK_BLOCK     8192        /* samples per block */
#define AUDIO_BLANK_THR_MIN   16
#define AUDIO_BLANK_THR_MAX   4096
#define AUDIO_BLANK_GUARD_MAX 64
#if defined(__HIPCC__)
#define AUDIO_BLANK_FN __host__ __device__ static inline      /* the kernel calls them as well */
#else
#define AUDIO_BLANK_FN static inline
#endif

AUDIO_BLANK_FN int audio_blank_abs(int16_t x) { return x < 0 ? -(int)x : (int)x; }
AUDIO_BLANK_FN int audio_blank_nblocks(int nsamp) { return (nsamp + AUDIO_BLANK_BLOCK - 1) / AUDIO_BLANK_BLOCK; }
/* samples of block b inside the record */
AUDIO_BLANK_FN int audio_blank_count(int nsamp, int b) {
    const int left = nsamp - b * AUDIO_BLANK_BLOCK;
    return left < AUDIO_BLANK_BLOCK ? left : AUDIO_BLANK_BLOCK;
}
AUDIO_BLANK_FN int audio_blank_rank(int count) { return (count - 1) / 2; }
/* does a sample of magnitude a trip the blanker of a block whose level is `level`? */
AUDIO_BLANK_FN int audio_blank_hit(int a, int thr16, int level) { return level > 0 && 16 * a > thr16 * level; }
AUDIO_BLANK_FN int audio_blank_settings_ok(int thr16, int guard) {
    return thr16 >= AUDIO_BLANK_THR_MIN && thr16 <= AUDIO_BLANK_THR_MAX && guard >= 0 && guard <= AUDIO_BLANK_GUARD_MAX;
}
#endif
