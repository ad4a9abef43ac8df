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
#include "synth_tile.h"

namespace wspr {

static_assert(sizeof(FadeChannel) == 64, "FadeChannel is 64 bytes");

namespace {
constexpr int kPerThread = kSynthPerThread, kTile = kSynthTile;   // 16 samples per thread, tiles of 4 096 (synth_tile.h)
constexpr int kMaxTaps = kTile / 4 + kFadeTerms;          // 1 040: L >= 4 (sigma <= 10 Hz, refused above that)

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
    synth_tile_load(pi, pq, accumulate, xi, xq);
    synth_tile_noise(seed, seg_index0 + seg, base, sigma, xi, xq);
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
        double dphi;
        double phi = synth_phase_at(me, ckpt, ntx, t, nlo, &dphi);
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
    synth_tile_store(pi, pq, xi, xq);
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
