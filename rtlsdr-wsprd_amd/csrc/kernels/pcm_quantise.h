/* A double to a signed 16-bit PCM sample, for K17 (audio_synth.h) and K18 (iq_audio.h) and their serial checkers.  Plain C.
 *   acc > 32767.0 gives 32767, acc < -32768.0 gives -32768, and either counts as clipped; otherwise the sample is
 *   (acc + 6755399441055744.0) - 6755399441055744.0 -- nearest, ties to even.
 * acc is not NaN: a caller whose values may be NaN decides what that means first (K18 does). */
#ifndef WSPR_PCM_QUANTISE_H
#define WSPR_PCM_QUANTISE_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCM_QUANTISE_HD __host__ __device__ static inline
#else
#define PCM_QUANTISE_HD static inline
#endif

/* *clipped is incremented for a sample that leaves the 16-bit range */
PCM_QUANTISE_HD int16_t pcm_quantise(double acc, int *clipped) {
    const double magic = 6755399441055744.0;               /* 1.5 * 2^52: (t + magic) - magic = t rounded to an integer, ties to even */
    if (acc > 32767.0) { ++*clipped; return (int16_t)32767; }
    if (acc < -32768.0) { ++*clipped; return (int16_t)-32768; }
    return (int16_t)(int)((acc + magic) - magic);
}
#endif
