/* The contract of wspr_iq_to_audio_batch_device() in serial C: the definition of
 * rtlsdr-wsprd_amd/csrc/kernels/iq_audio.h, statement by statement.  TEST INFRASTRUCTURE ONLY.
 * Built on demand by tests/iq_audio_lib.py with -ffp-contract=off: the only fused operations are the fmaf() calls.  With
 * -DIQ_AUDIO_CHECK_MAIN it is a stand-alone program that runs the checker over rows of every length around a block and a
 * tile, in buffers exactly as large as the contract allows, for a run under -fsanitize=address,undefined: the first and the
 * last eight inputs of a row are where an off-by-one would live. */
#include <math.h>
#include <stddef.h>
#include "iq_audio.h"

int iq_audio_check_tile(void) { return IQ_AUDIO_TILE; }

/* the quantiser alone, on given values of p */
void iq_audio_check_quantise(const double *p, int n, int16_t *out, int *clipped) {
    int c = 0;
    for (int i = 0; i < n; ++i) out[i] = iq_audio_quantise(p[i], &c);
    *clipped = c;
}

/* nseg rows (row s at I + s * stride, Q + s * stride) of np samples into records of pcm_stride samples: columns
 * 0 .. 32 np - 1 written, the rest left alone; n_clipped (nseg, may be NULL) = clipped samples per record.
 * Returns 0, -1 for bad arguments, -2 for np > 45 000. */
int iq_audio_check_rows(const float *I, const float *Q, int nseg, int np, size_t stride, float gain, int16_t *pcm,
                        size_t pcm_stride, int *n_clipped) {
    if (nseg < 0 || np < 0) return -1;
    if (np > IQ_AUDIO_MAX_SAMPLES) return -2;
    if (!isfinite(gain)) return -1;
    if (nseg > 0 && (stride < (size_t)np || pcm_stride < (size_t)IQ_AUDIO_INTERP * (size_t)np)) return -1;
    for (int s = 0; s < nseg; ++s) {
        const float *ri = I + (size_t)s * stride, *rq = Q + (size_t)s * stride;
        int16_t *o = pcm + (size_t)s * pcm_stride;
        int clipped = 0;
        for (long n = 0; n < (long)IQ_AUDIO_INTERP * np; ++n) o[n] = iq_audio_sample(iq_audio_chain(ri, rq, np, n), gain, &clipped);
        if (n_clipped) n_clipped[s] = clipped;
    }
    return 0;
}

#ifdef IQ_AUDIO_CHECK_MAIN
#include <stdio.h>
#include <stdlib.h>
int main(void) {
    static const int lengths[] = {0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 131, 1000};
    unsigned long long state = 0x9E3779B97F4A7C15ull;
    long total = 0, nonzero = 0;
    for (size_t li = 0; li < sizeof lengths / sizeof lengths[0]; ++li) {
        const int np = lengths[li], nseg = 2;
        const size_t stride = ((size_t)np + 3) & ~(size_t)3, pcm_stride = 32 * (size_t)np + 8;
        /* the last row ends at np, the last record at 32 np: one element more read or written is out of bounds */
        const size_t n_in = ((size_t)nseg - 1) * stride + (size_t)np, n_out = ((size_t)nseg - 1) * pcm_stride + 32 * (size_t)np;
        float *I = malloc(n_in * sizeof *I + 1), *Q = malloc(n_in * sizeof *Q + 1);
        int16_t *pcm = malloc(n_out * sizeof *pcm + 1);
        int count[2] = {-1, -1};
        if (!I || !Q || !pcm) return 2;
        for (size_t i = 0; i < n_in; ++i) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            I[i] = (float)((double)(state >> 40) / 16777216.0 - 0.5);
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            Q[i] = (float)((double)(state >> 40) / 16777216.0 - 0.5);
        }
        if (np > 4) { I[3] = INFINITY; Q[np - 1] = NAN; I[np - 2] = 1e30f; Q[0] = 1e-42f; }
        if (iq_audio_check_rows(I, Q, nseg, np, stride, 40000.0f, pcm, pcm_stride, count) != 0) return 3;
        for (int s = 0; s < nseg; ++s) {
            if (count[s] < 0 || count[s] > 32 * np) return 4;
            total += count[s];
            for (long n = 0; n < 32L * np; ++n) nonzero += pcm[(size_t)s * pcm_stride + n] != 0;
        }
        free(I);
        free(Q);
        free(pcm);
    }
    printf("iq_audio_check: ok, %ld samples clipped, %ld not zero\n", total, nonzero);
    return 0;
}
#endif
