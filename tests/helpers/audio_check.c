/* The contract of wspr_audio_batch_device() in serial C: the definition of
 * rtlsdr-wsprd_amd/csrc/kernels/audio_front.h, statement by statement.  TEST INFRASTRUCTURE ONLY.
 * Built on demand by tests/audio_lib.py with -ffp-contract=off: the only fused operations are the fmaf() calls. */
#include <math.h>
#include <stddef.h>
#include "audio_front.h"

int audio_check_tile(void) { return AUDIO_FRONT_TILE; }
void audio_check_taps(float *gi, float *gq) {
    for (int k = -AUDIO_FRONT_K; k <= AUDIO_FRONT_K; ++k) {
        gi[k + AUDIO_FRONT_K] = audio_front_tap(0, k);
        gq[k + AUDIO_FRONT_K] = audio_front_tap(1, k);
    }
}

/* nseg records (row s at pcm + s * pcm_stride) into rows of out_stride floats, the whole row written; normalise != 0: then
 * the receiver's scaling to a peak of 0.5 over the first 45000 columns of both rails (rtlsdr_wsprd.c:290-305).
 * Returns 0, -1 for bad arguments, -2 for nsamp > 1 440 000. */
int audio_check_rows(const int16_t *pcm, size_t pcm_stride, int nsamp, int nseg, float *I, float *Q, size_t out_stride,
                     int normalise) {
    if (nsamp > AUDIO_FRONT_MAX_SAMPLES) return -2;
    if (nsamp < 0 || nseg < 0 || pcm_stride < (size_t)nsamp || out_stride < AUDIO_FRONT_MAX_OUT) return -1;
    const int n_out = audio_front_n_out(nsamp);
    for (int s = 0; s < nseg; ++s) {
        const int16_t *p = pcm + (size_t)s * pcm_stride;
        float *ri = I + (size_t)s * out_stride, *rq = Q + (size_t)s * out_stride;
        for (size_t m = 0; m < out_stride; ++m) {
            float ai = 0.0f, aq = 0.0f;
            if ((int)m < n_out && m < AUDIO_FRONT_MAX_OUT)
                for (int k = -AUDIO_FRONT_K; k <= AUDIO_FRONT_K; ++k) {
                    const long n = 32L * (long)m + k;
                    const float x = (n >= 0 && n < nsamp) ? (float)p[n] * 0x1p-15f : 0.0f;
                    ai = fmaf(audio_front_tap(0, k), x, ai);
                    aq = fmaf(audio_front_tap(1, k), x, aq);
                }
            ri[m] = ai;
            rq[m] = aq;
        }
        if (normalise) {
            float peak = 1e-24f;
            for (int i = 0; i < AUDIO_FRONT_MAX_OUT; ++i) {
                const float a = fabsf(ri[i]), b = fabsf(rq[i]);
                if (a > peak) peak = a;
                if (b > peak) peak = b;
            }
            const float scale = (float)(0.5 / (double)peak);
            for (int i = 0; i < AUDIO_FRONT_MAX_OUT; ++i) { ri[i] *= scale; rq[i] *= scale; }
        }
    }
    return 0;
}
