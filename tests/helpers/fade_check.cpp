// The fading channel's contract (include/wspr_mi355x.h, "fading channel") in plain serial C++ over the shared headers
// fade.h / synth_math.h: what wspr_synth_faded_batch_device() must write, sample for sample; the gain G[n] alone; and
// synth_exp().  TEST INFRASTRUCTURE ONLY -- built on demand by tests/fade_lib.py with -ffp-contract=off; the product
// never links it.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "fade.h"

struct synth_tx {                   // wspr_synth_tx
    int32_t seg;
    float f0, t0, amp, drift;
    unsigned char symbols[162];
    unsigned char pad[2];
};
static_assert(sizeof(synth_tx) == 184, "wspr_synth_tx is 184 bytes");
struct synth_path { float gain, shift, sigma; };       // wspr_synth_path
struct synth_channel { synth_path path[2]; };          // wspr_synth_channel
static_assert(sizeof(synth_channel) == 24, "wspr_synth_channel is 24 bytes");

using namespace wspr;

static bool channel_ok(const synth_channel& c) {
    for (int p = 0; p < 2; ++p) {
        const synth_path& a = c.path[p];
        if (!isfinite(a.gain) || !isfinite(a.shift) || !isfinite(a.sigma)) return false;
        if (a.sigma != 0.0f && !(a.sigma >= kFadeMinSigma && a.sigma <= kFadeMaxSigma)) return false;
        if (fabsf(a.shift) > kFadeMaxShift) return false;
    }
    return true;
}
static FadeChannel setup(const synth_channel& c) {
    FadeChannel f;
    for (int p = 0; p < 2; ++p) f.path[p] = fade_path_setup(c.path[p].gain, c.path[p].shift, c.path[p].sigma);
    return f;
}

// G[n] of one transmission, serially.  The sixteen impulses of a path are drawn again only when kc = n / L moves: the
// same draws, so the same bits, as drawing all sixteen at every sample.
struct Gain {
    uint64_t seed; int64_t S; int q; FadeChannel f;
    int kc[2] = {-1, -1};
    FadeTap W[2][kFadeTerms];
    Gain(uint64_t seed_, int64_t S_, int q_, const FadeChannel& f_) : seed(seed_), S(S_), q(q_), f(f_) {}
    void at(int n, double* re, double* im) {
        double gr = 0.0, gi = 0.0;
        for (int p = 0; p < 2; ++p) {
            const FadePath& pa = f.path[p];
            if (pa.kind == kFadeKindSkipped) continue;
            double a = pa.c, b = 0.0;
            if (pa.kind == kFadeKindDiffuse) {
                const int k = n / pa.L;
                if (k != kc[p]) {
                    for (int j = 0; j < kFadeTerms; ++j) W[p][j] = fade_draw(seed, S, q, p, k - kFadeBelow + j);
                    kc[p] = k;
                }
                fade_sum((const FadeTap*)W[p], n - (k - kFadeBelow) * pa.L, pa.L, pa.beta, pa.c, &a, &b);
            }
            if (pa.shifted) fade_rotate(pa.w, n, &a, &b);
            gr += a;
            gi += b;
        }
        *re = gr;
        *im = gi;
    }
};

extern "C" {

// rows: nseg rows of `stride` floats; only columns [0, 45000) are touched.  ch == NULL: every channel is the identity by
// the UNFADED statement x + amp * cos(phi) (the unfaded call).
int fade_check_batch(const synth_tx* tx, const synth_channel* ch, int ntx, int nseg, int seg_index0, float sigma,
                     uint64_t seed, int flags, float* I, float* Q, size_t stride) {
    if (ntx < 0 || nseg < 0 || !isfinite(sigma) || (flags & ~3)) return -1;
    for (int t = 0; t < ntx; ++t) {
        const synth_tx& x = tx[t];
        if (x.seg < 0 || x.seg >= nseg || (t > 0 && x.seg < tx[t - 1].seg)) return -1;
        if (!isfinite(x.f0) || !isfinite(x.t0) || !isfinite(x.amp) || !isfinite(x.drift)) return -1;
        if (fabs((double)x.f0) + fabs((double)x.drift) / 2.0 > kSynthMaxHz) return -1;
        for (int i = 0; i < 162; ++i) if (x.symbols[i] > 3) return -1;
        if (ch && !channel_ok(ch[t])) return -1;
    }
    int t = 0;
    for (int seg = 0; seg < nseg; ++seg) {
        float* xi = I + (size_t)seg * stride;
        float* xq = Q + (size_t)seg * stride;
        const int64_t S = (int64_t)seg_index0 + seg;
        if (!(flags & kSynthFlagAccumulate)) for (int k = 0; k < kSynthSamples; ++k) { xi[k] = 0.0f; xq[k] = 0.0f; }
        if (sigma > 0.0f)
            for (int k = 0; k < kSynthSamples; ++k) {
                float nI, nQ;
                synth_noise(seed, S, k, sigma, &nI, &nQ);
                xi[k] = (float)((double)xi[k] + (double)nI);
                xq[k] = (float)((double)xq[k] + (double)nQ);
            }
        for (int q = 0; t < ntx && tx[t].seg == seg; ++t, ++q) {
            const synth_tx& x = tx[t];
            const int first = synth_first_index(x.t0);
            const double amp = (double)x.amp;
            Gain g(seed, S, q, ch ? setup(ch[t]) : FadeChannel());
            double phi = 0.0;
            for (int i = 0; i < 162; ++i) {
                const double dphi = synth_dphi(x.f0, x.drift, i, x.symbols[i]);
                for (int j = 0; j < 256; ++j) {
                    const int n = 256 * i + j;
                    const long k = (long)first + n;
                    if (k >= 0 && k < kSynthSamples) {
                        double sn, cs;
                        synth_sincos(phi, &sn, &cs);
                        if (ch) {
                            double gre, gim;
                            g.at(n, &gre, &gim);
                            fade_apply(amp, sn, cs, gre, gim, &xi[k], &xq[k]);
                        } else {
                            xi[k] = (float)((double)xi[k] + amp * cs);
                            xq[k] = (float)((double)xq[k] + amp * sn);
                        }
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

// G[n] for n = n0 .. n0 + count - 1 of the q-th transmission of global segment S
int fade_check_gain(uint64_t seed, int64_t S, int q, const synth_channel* ch, int n0, int count, double* re, double* im) {
    if (!ch || !channel_ok(*ch) || q < 0 || n0 < 0 || count < 0 || (long)n0 + count > kSynthSigLen) return -1;
    Gain g(seed, S, q, setup(*ch));
    for (int i = 0; i < count; ++i) g.at(n0 + i, &re[i], &im[i]);
    return 0;
}

void fade_check_exp(const double* x, int n, double* out) {
    for (int i = 0; i < n; ++i) out[i] = synth_exp(x[i]);
}

void fade_check_noise(uint64_t seed, int64_t segment, int sample0, int count, float sigma, float* nI, float* nQ) {
    for (int i = 0; i < count; ++i) synth_noise(seed, segment, sample0 + i, sigma, &nI[i], &nQ[i]);
}

}  // extern "C"
