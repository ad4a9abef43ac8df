// What the two fill kernels of the signal synthesiser share (K8's synth_fill_kernel, k8_synth.hip; K13's
// synth_fade_kernel, k13_fade.hip): the tile, and steps 1, 2 and the store of the contract stated in k8_synth.hip, over
// the 16 samples of both rails a thread keeps in registers.  Free functions over plain arrays on purpose: as members of
// a struct with the per-sample loop handed in as a lambda, the same code cost K13 scratch memory.  The per-sample loops
// stay written out in their kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "synth_math.h"
#include "wspr_device.h"

namespace wspr {

constexpr int kSynthPerThread = 16;
constexpr int kSynthTile = 256 * kSynthPerThread;         // 4 096 samples; 11 tiles cover a row of kIqStride floats
static_assert(kIqStride % kSynthTile == 0, "tiles must cover the row exactly");

// step 1: zero, or the row's values (accumulate)
__device__ __forceinline__ void synth_tile_load(const float4* __restrict__ pi, const float4* __restrict__ pq, int accumulate,
                                                float (&xi)[kSynthPerThread], float (&xq)[kSynthPerThread]) {
#pragma unroll
    for (int v = 0; v < kSynthPerThread / 4; ++v) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (accumulate) { a = pi[v]; b = pq[v]; }
        xi[4 * v] = a.x; xi[4 * v + 1] = a.y; xi[4 * v + 2] = a.z; xi[4 * v + 3] = a.w;
        xq[4 * v] = b.x; xq[4 * v + 1] = b.y; xq[4 * v + 2] = b.z; xq[4 * v + 3] = b.w;
    }
}

// step 2: the noise draw of every sample of the row (base = the thread's first sample, S = the global segment)
__device__ __forceinline__ void synth_tile_noise(unsigned long long seed, long long S, int base, float sigma,
                                                 float (&xi)[kSynthPerThread], float (&xq)[kSynthPerThread]) {
    if (sigma > 0.0f) {
#pragma unroll
        for (int s = 0; s < kSynthPerThread; ++s) {
            if (base + s < kMaxSamples) {
                float nI, nQ;
                synth_noise(seed, S, base + s, sigma, &nI, &nQ);
                xi[s] = (float)((double)xi[s] + (double)nI);
                xq[s] = (float)((double)xq[s] + (double)nQ);
            }
        }
    }
}

// every output sample is stored once, with 16-byte stores
__device__ __forceinline__ void synth_tile_store(float4* __restrict__ pi, float4* __restrict__ pq,
                                                 const float (&xi)[kSynthPerThread], const float (&xq)[kSynthPerThread]) {
#pragma unroll
    for (int v = 0; v < kSynthPerThread / 4; ++v) {
        pi[v] = make_float4(xi[4 * v], xi[4 * v + 1], xi[4 * v + 2], xi[4 * v + 3]);
        pq[v] = make_float4(xq[4 * v], xq[4 * v + 1], xq[4 * v + 2], xq[4 * v + 3]);
    }
}

// phi at sample nlo (0 .. kSigLen - 1) of transmission t: the checkpoint below it (layout [checkpoint][transmission]), then at
// most 63 of the recurrence's adds -- all within one symbol, as 64 divides 256.  *dphi = the increment of that symbol.
__device__ __forceinline__ double synth_phase_at(const SynthTx* __restrict__ me, const double* __restrict__ ckpt, int ntx, int t,
                                                 int nlo, double* dphi) {
    const int c = nlo / kSynthCkptEvery;
    double phi = ckpt[(size_t)c * ntx + t];
    const double d = synth_dphi(me->f0, me->drift, nlo >> 8, me->symbols[nlo >> 8]);
    for (int m = c * kSynthCkptEvery; m < nlo; ++m) phi += d;
    *dphi = d;
    return phi;
}

}  // namespace wspr
