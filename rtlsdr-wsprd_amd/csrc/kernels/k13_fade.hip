// K13: the signal synthesiser with an HF fading channel per transmission (wspr_synth_faded*(), include/wspr_mi355x.h,
// "fading channel"; the definition's arithmetic is fade.h, tests/helpers/fade_check.cpp its serial form).
//
// K8's shape (k8_synth.hip): synth_phase_kernel's checkpoints are reused as they are (launch_synth_phase());
//   synth_fade_kernel   workgroup = (segment, tile of 4 096 samples), a thread owns 16 consecutive samples of both rails in
//                       registers, draws their noise, and for each transmission of the segment in list order multiplies
//                       the transmitter's phasor by the gain G[n] before it is added.  One 16-byte store per four
//                       samples, no atomics.
// A diffuse path's gain is sixteen white impulses W[k] through a Gaussian pulse.  The impulses a tile needs -- k from
// (first sample)/L - 7 to (last sample)/L + 8, at most 4 096/L + 16 <= 1 040 at L = 4 -- are drawn ONCE per workgroup into
// LDS (both paths: 16 640 B), one Philox + Box-Muller each instead of sixteen per sample; the samples then walk their
// sixteen terms from there.  The transmission loop and both barriers are uniform over the workgroup: a thread whose 16
// samples miss the frame still takes part in the staging.
// The bound is the fp64 vector rate without fused multiply-add.  Per transmission sample a diffuse path costs sixteen
// terms of 37 double operations (2 for the argument, 31 in synth_exp(): 7 reduction, 24 polynomial; 4 for the two sums),
// 2 for the scale and 2 to add the path: 596.  The complex product costs 6 more than the unfaded sample's 54, a shifted
// path 55 + 6 (its own sincos and the rotation).
#include <hip/hip_runtime.h>

#include "fade.h"
#include "wspr_device.h"

namespace wspr {

static_assert(sizeof(FadeChannel) == 64, "FadeChannel is 64 bytes");

namespace {
constexpr int kPerThread = 16;
constexpr int kTile = 256 * kPerThread;                   // 4 096 samples; 11 tiles cover a row of kIqStride floats
constexpr int kMaxTaps = kTile / 4 + kFadeTerms;          // 1 040: L >= 4 (sigma <= 10 Hz, refused above that)
static_assert(kIqStride % kTile == 0, "tiles must cover the row exactly");

__global__ __launch_bounds__(256)
void synth_fade_kernel(const SynthTx* __restrict__ tx, const FadeChannel* __restrict__ ch, int ntx,
                       const int* __restrict__ seg_off, const int* __restrict__ first, const double* __restrict__ ckpt,
                       long long seg_index0, float sigma, unsigned long long seed, int accumulate, int seg_base,
                       float* __restrict__ dI, float* __restrict__ dQ) {
    __shared__ FadeTap taps[2][kMaxTaps];
    const int seg = seg_base + blockIdx.y;
    const int tile0 = blockIdx.x * kTile;
    const int base = tile0 + threadIdx.x * kPerThread;                  // < kIqStride by the grid
    float4* __restrict__ pi = reinterpret_cast<float4*>(dI + (size_t)seg * kIqStride + base);
    float4* __restrict__ pq = reinterpret_cast<float4*>(dQ + (size_t)seg * kIqStride + base);
    float xi[kPerThread], xq[kPerThread];
#pragma unroll
    for (int v = 0; v < kPerThread / 4; ++v) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (accumulate) { a = pi[v]; b = pq[v]; }
        xi[4 * v] = a.x; xi[4 * v + 1] = a.y; xi[4 * v + 2] = a.z; xi[4 * v + 3] = a.w;
        xq[4 * v] = b.x; xq[4 * v + 1] = b.y; xq[4 * v + 2] = b.z; xq[4 * v + 3] = b.w;
    }
    if (sigma > 0.0f) {
#pragma unroll
        for (int s = 0; s < kPerThread; ++s) {
            if (base + s < kMaxSamples) {
                float nI, nQ;
                synth_noise(seed, seg_index0 + seg, base + s, sigma, &nI, &nQ);
                xi[s] = (float)((double)xi[s] + (double)nI);
                xq[s] = (float)((double)xq[s] + (double)nQ);
            }
        }
    }
    const int t_begin = seg_off[seg], t_end = seg_off[seg + 1];
    for (int t = t_begin; t < t_end; ++t) {                             // uniform over the workgroup
        const int f = first[t];
        int blo = tile0 - f, bhi = tile0 - f + (kTile - 1);             // the tile in the transmission's own samples
        if (bhi < 0 || blo >= kSigLen) continue;
        blo = blo < 0 ? 0 : blo;
        bhi = bhi > kSigLen - 1 ? kSigLen - 1 : bhi;
        const FadeChannel* __restrict__ c = ch + t;
        int klo[2] = {0, 0};
        __syncthreads();                                                // the previous transmission's impulses are done with
        for (int p = 0; p < 2; ++p) {
            if (c->path[p].kind != kFadeKindDiffuse) continue;
            const int L = c->path[p].L;
            klo[p] = blo / L - kFadeBelow;
            int count = bhi / L + (kFadeTerms - kFadeBelow) - klo[p];   // last k is bhi / L + 8
            count = count > kMaxTaps ? kMaxTaps : count;                // (never: L >= 4)
            for (int i = threadIdx.x; i < count; i += 256) taps[p][i] = fade_draw(seed, seg_index0 + seg, t - t_begin, p, klo[p] + i);
        }
        __syncthreads();
        const int n0 = base - f;                           // the transmission's sample index at this thread's first output
        if (n0 + kPerThread <= 0 || n0 >= kSigLen) continue;
        const SynthTx* __restrict__ me = tx + t;
        const float f0 = me->f0, drift = me->drift;
        const double amp = (double)me->amp;
        const int nlo = n0 < 0 ? 0 : n0;
        const int ck = nlo / kSynthCkptEvery;
        double phi = ckpt[(size_t)ck * ntx + t];
        double dphi = synth_dphi(f0, drift, nlo >> 8, me->symbols[nlo >> 8]);
        for (int m = ck * kSynthCkptEvery; m < nlo; ++m) phi += dphi;   // same symbol: 64 divides 256
#pragma unroll
        for (int s = 0; s < kPerThread; ++s) {
            const int n = n0 + s;
            if (n >= 0 && n < kSigLen && base + s < kMaxSamples) {
                if ((n & (kSps - 1)) == 0) dphi = synth_dphi(f0, drift, n >> 8, me->symbols[n >> 8]);
                double sn, cs;
                synth_sincos(phi, &sn, &cs);
                double gr = 0.0, gi = 0.0;
#pragma unroll 1
                for (int p = 0; p < 2; ++p) {
                    const int kind = c->path[p].kind;
                    if (kind == kFadeKindSkipped) continue;
                    double a = c->path[p].c, b = 0.0;
                    if (kind == kFadeKindDiffuse) {
                        const int L = c->path[p].L;
                        const int kc = n / L;
                        int j0 = kc - kFadeBelow - klo[p];              // 0 .. count - 16 by the staging above
                        j0 = j0 < 0 ? 0 : (j0 > kMaxTaps - kFadeTerms ? kMaxTaps - kFadeTerms : j0);
                        fade_sum(&taps[p][j0], n - (kc - kFadeBelow) * L, L, c->path[p].beta, a, &a, &b);
                    }
                    if (c->path[p].shifted) fade_rotate(c->path[p].w, n, &a, &b);
                    gr += a;
                    gi += b;
                }
                fade_apply(amp, sn, cs, gr, gi, &xi[s], &xq[s]);
                phi += dphi;
            }
        }
    }
#pragma unroll
    for (int v = 0; v < kPerThread / 4; ++v) {
        pi[v] = make_float4(xi[4 * v], xi[4 * v + 1], xi[4 * v + 2], xi[4 * v + 3]);
        pq[v] = make_float4(xq[4 * v], xq[4 * v + 1], xq[4 * v + 2], xq[4 * v + 3]);
    }
}
}  // namespace

void launch_synth_faded(const SynthTx* tx, const FadeChannel* ch, int ntx, const int* seg_off, int nseg, long long seg_index0,
                        float sigma, unsigned long long seed, int accumulate, double* ckpt, int* first, float* dI, float* dQ,
                        hipStream_t st) {
    if (nseg <= 0) return;
    launch_synth_phase(tx, ntx, ckpt, first, st);
    for (int s0 = 0; s0 < nseg; s0 += 32768)               // grid.y is limited to 65 535
        hipLaunchKernelGGL(synth_fade_kernel, dim3(kIqStride / kTile, nseg - s0 < 32768 ? nseg - s0 : 32768), dim3(256), 0, st,
                           tx, ch, ntx, seg_off, first, ckpt, seg_index0, sigma, seed, accumulate, s0, dI, dQ);
}

}  // namespace wspr
