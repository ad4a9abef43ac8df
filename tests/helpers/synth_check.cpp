// The synthesiser's contract (include/wspr_mi355x.h, "signal synthesiser") in plain serial C++ over the shared maths
// header: what wspr_synth_batch_device() must write, sample for sample.  TEST INFRASTRUCTURE ONLY -- built on demand by
// tests/synth_lib.py with -ffp-contract=off; the product never links it.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "synth_math.h"

struct synth_tx {                   // wspr_synth_tx
    int32_t seg;
    float f0, t0, amp, drift;
    unsigned char symbols[162];
    unsigned char pad[2];
};
static_assert(sizeof(synth_tx) == 184, "wspr_synth_tx is 184 bytes");

using namespace wspr;

extern "C" {

// rows: nseg rows of `stride` floats; only columns [0, 45000) are touched
int synth_check_batch(const synth_tx* tx, int ntx, int nseg, int seg_index0, float sigma, uint64_t seed, int flags,
                      float* I, float* Q, size_t stride) {
    if (ntx < 0 || nseg < 0 || !isfinite(sigma) || (flags & ~3)) return -1;
    for (int t = 0; t < ntx; ++t) {
        const synth_tx& x = tx[t];
        if (x.seg < 0 || x.seg >= nseg || (t > 0 && x.seg < tx[t - 1].seg)) return -1;
        if (!isfinite(x.f0) || !isfinite(x.t0) || !isfinite(x.amp) || !isfinite(x.drift)) return -1;
        if (fabs((double)x.f0) + fabs((double)x.drift) / 2.0 > kSynthMaxHz) return -1;
        for (int i = 0; i < 162; ++i) if (x.symbols[i] > 3) return -1;
    }
    int t = 0;
    for (int seg = 0; seg < nseg; ++seg) {
        float* xi = I + (size_t)seg * stride;
        float* xq = Q + (size_t)seg * stride;
        if (!(flags & kSynthFlagAccumulate)) for (int k = 0; k < kSynthSamples; ++k) { xi[k] = 0.0f; xq[k] = 0.0f; }
        if (sigma > 0.0f)
            for (int k = 0; k < kSynthSamples; ++k) {
                float nI, nQ;
                synth_noise(seed, (int64_t)seg_index0 + seg, k, sigma, &nI, &nQ);
                xi[k] = (float)((double)xi[k] + (double)nI);
                xq[k] = (float)((double)xq[k] + (double)nQ);
            }
        for (; t < ntx && tx[t].seg == seg; ++t) {
            const synth_tx& x = tx[t];
            const int first = synth_first_index(x.t0);
            const double amp = (double)x.amp;
            double phi = 0.0;
            for (int i = 0; i < 162; ++i) {
                const double dphi = synth_dphi(x.f0, x.drift, i, x.symbols[i]);
                for (int j = 0; j < 256; ++j) {
                    const long k = (long)first + 256 * i + j;
                    if (k >= 0 && k < kSynthSamples) {
                        double sn, cs;
                        synth_sincos(phi, &sn, &cs);
                        xi[k] = (float)((double)xi[k] + amp * cs);
                        xq[k] = (float)((double)xq[k] + amp * sn);
                    }
                    phi += dphi;
                }
            }
        }
        if (flags & kSynthFlagNormalise) {                    // rtlsdr_wsprd.c:290-305
            float peak = 1e-24f;
            for (int k = 0; k < kSynthSamples; ++k) {
                const float a = fabsf(xi[k]), b = fabsf(xq[k]);
                if (a > peak) peak = a;
                if (b > peak) peak = b;
            }
            const float scale = (float)(0.5 / (double)peak);
            for (int k = 0; k < kSynthSamples; ++k) { xi[k] = xi[k] * scale; xq[k] = xq[k] * scale; }
        }
    }
    return 0;
}

void synth_check_sincos(const double* x, int n, double* sn, double* cs) {
    for (int i = 0; i < n; ++i) synth_sincos(x[i], &sn[i], &cs[i]);
}

double synth_check_log(double u) { return synth_log(u); }

}  // extern "C"
