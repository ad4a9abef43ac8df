// The audio scene synthesiser's contract (include/wspr_mi355x.h, "12 kHz audio scene synthesiser") in plain serial C++ over
// the shared headers audio_synth.h and synth_math.h: what wspr_synth_audio_batch_device() must write, sample for sample,
// and the counts it must report.  TEST INFRASTRUCTURE ONLY -- built on demand by tests/audio_synth_lib.py with
// -ffp-contract=off; the product never links it.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "audio_synth.h"

struct synth_tx {                   // wspr_synth_tx
    int32_t seg;
    float f0, t0, amp, drift;
    unsigned char symbols[162];
    unsigned char pad[2];
};
static_assert(sizeof(synth_tx) == 184, "wspr_synth_tx is 184 bytes");

using namespace wspr;

extern "C" {

// rows: nseg rows of `stride` samples; columns [0, nsamp) are written, and without the accumulate flag the columns up to
// roundup8(nsamp) are zeroed (where the row holds them); n_clipped: nseg ints, may be null
int audio_synth_check_batch(const synth_tx* tx, int ntx, int nseg, int seg_index0, int nsamp, float sigma, uint64_t seed,
                            int flags, int16_t* pcm, size_t stride, int* n_clipped) {
    if (ntx < 0 || nseg < 0 || nsamp < 0) return -1;
    if (nsamp > kAudioSynthMaxSamples) return -2;
    if (!isfinite(sigma) || sigma < 0.0f || (double)sigma > kAudioSynthMaxLevel || (flags & ~kSynthFlagAccumulate)) return -1;
    if (nseg > 0 && stride < (size_t)nsamp) return -1;
    for (int t = 0; t < ntx; ++t) {
        const synth_tx& x = tx[t];
        if (x.seg < 0 || x.seg >= nseg || (t > 0 && x.seg < tx[t - 1].seg)) return -1;
        if (!isfinite(x.f0) || !isfinite(x.t0) || !isfinite(x.amp) || !isfinite(x.drift)) return -1;
        if (fabs((double)x.amp) > kAudioSynthMaxLevel) return -1;
        if (fabs((double)x.f0) + fabs((double)x.drift) / 2.0 > kAudioSynthMaxHz) return -1;
        for (int i = 0; i < 162; ++i) if (x.symbols[i] > 3) return -1;
    }
    std::vector<double> acc((size_t)nsamp);
    std::vector<double> P(kSynthNsym), dphi(kSynthNsym);
    int t = 0;
    for (int seg = 0; seg < nseg; ++seg) {
        int16_t* row = pcm + (size_t)seg * stride;
        for (int k = 0; k < nsamp; ++k) acc[k] = (flags & kSynthFlagAccumulate) ? (double)row[k] : 0.0;
        if (sigma > 0.0f)
            for (int k = 0; k < nsamp; ++k) {
                float a, b;
                synth_gauss(seed, (int64_t)seg_index0 + seg, (uint32_t)(k >> 1), kAudioSynthNoiseStream, sigma, &a, &b);
                acc[k] = acc[k] + (double)((k & 1) ? b : a);
            }
        for (; t < ntx && tx[t].seg == seg; ++t) {
            const synth_tx& x = tx[t];
            const long first = audio_synth_first(x.t0);
            const double amp = (double)x.amp;
            audio_synth_phases(x.f0, x.drift, x.symbols, P.data(), dphi.data(), 1);
            for (int i = 0; i < kSynthNsym; ++i)
                for (int j = 0; j < kAudioSynthSps; ++j) {
                    const long k = first + (long)kAudioSynthSps * i + j;
                    if (k < 0 || k >= nsamp) continue;
                    const double phi = P[i] + (double)j * dphi[i];
                    double sn, cs;
                    synth_sincos(phi, &sn, &cs);
                    acc[k] = acc[k] + amp * cs;
                }
        }
        int clipped = 0;
        for (int k = 0; k < nsamp; ++k) row[k] = audio_synth_quantise(acc[k], &clipped);
        if (!(flags & kSynthFlagAccumulate))
            for (size_t k = (size_t)nsamp; k < (((size_t)nsamp + 7) & ~(size_t)7) && k < stride; ++k) row[k] = 0;
        if (n_clipped) n_clipped[seg] = clipped;
    }
    return 0;
}

// the quantiser alone, on given accumulator values
void audio_synth_check_quantise(const double* acc, int n, int16_t* out, int* clipped) {
    int c = 0;
    for (int i = 0; i < n; ++i) out[i] = audio_synth_quantise(acc[i], &c);
    *clipped = c;
}

int audio_synth_check_first(float t0) { return audio_synth_first(t0); }

// the noise draw of the sample pair m of global segment S
void audio_synth_check_gauss(uint64_t seed, long long S, uint32_t m, float sigma, float* a, float* b) {
    synth_gauss(seed, (int64_t)S, m, kAudioSynthNoiseStream, sigma, a, b);
}

}  // extern "C"

#ifdef AUDIO_SYNTH_CHECK_MAIN
// The checker as a stand-alone program for a sanitizer run: a short record with a frame hanging off both ends.
int main() {
    synth_tx tx[2] = {};
    for (int q = 0; q < 2; ++q) {
        tx[q].seg = q; tx[q].f0 = 21.7f; tx[q].t0 = q ? 0.9f : -109.9f; tx[q].amp = 30000.0f; tx[q].drift = 3.0f;
        for (int i = 0; i < 162; ++i) tx[q].symbols[i] = (unsigned char)((i * 7 + q) & 3);
    }
    const int nsamp = 12345;
    std::vector<int16_t> pcm(2 * 12352, 7);
    int clipped[2] = {-1, -1};
    const int rc = audio_synth_check_batch(tx, 2, 2, 5, nsamp, 3000.0f, 42, 1, pcm.data(), 12352, clipped);
    printf("%d %d %d\n", rc, clipped[0], clipped[1]);
    return rc;
}
#endif
