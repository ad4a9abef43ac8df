// K8: the signal synthesiser (wspr_synth*(), include/wspr_mi355x.h) -- the reference's self-test generator
// (decoderSelfTest() / whiteGaussianNoise(), rtlsdr_wsprd.c:706-760) for batches of scenes resident in HBM.
//
// Per output sample x of a rail, in this order (the contract; tests/helpers/synth_check.cpp is its serial form):
//   x = 0 or the row's value (accumulate);  x = (float)((double)x + (double)n) with n the sample's noise draw;
//   for every transmission of the segment in list order  x = (float)((double)x + (double)amp * cos(phi))  (sin for Q).
// phi is the reference's SERIAL double recurrence (phi = 0; use; phi += dphi_i; 41 472 times): a parallel prefix sum
// moves phases by a few ulp and changes float samples, so the recurrence itself is run:
//   synth_phase_kernel  one lane per transmission walks the 41 472 dependent adds and writes phi at every 64th sample
//                       (648 checkpoints = 5 184 B per transmission, layout [checkpoint][transmission]); transmissions
//                       are independent, so the kernel's time is one lane's chain whatever the batch;
//   synth_fill_kernel   workgroup = (segment, tile of 4 096 samples), a thread owns 16 consecutive samples of both rails
//                       in registers: draws their noise, then for each transmission of the segment walks at most 63
//                       adds from the checkpoint below its first sample and one add per sample from there, evaluating
//                       synth_sincos() (synth_math.h) at each.  Every output sample is stored once, with 16-byte
//                       stores; no atomics, so the result is deterministic by construction.
// The bound is the fp64 vector rate: one transmission sample costs 54 double operations, none fused (9 reduction,
// 18 sine kernel, 22 cosine kernel, 4 for the two rails, 1 phase add) and four float/double conversions.
#include <hip/hip_runtime.h>

#include "synth_tile.h"

namespace wspr {

static_assert(kSynthSamples == kMaxSamples && kSynthSigLen == kSigLen, "synth_math.h and wspr_device.h disagree");

namespace {
constexpr int kCkptEvery = kSynthCkptEvery;               // 64
constexpr int kCkptPerTx = kSigLen / kCkptEvery;          // 648
constexpr int kPerThread = kSynthPerThread, kTile = kSynthTile;   // 16 samples per thread, tiles of 4 096 (synth_tile.h)

__global__ __launch_bounds__(64)
void synth_phase_kernel(const SynthTx* __restrict__ tx, int ntx, double* __restrict__ ckpt, int* __restrict__ first) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= ntx) return;
    const SynthTx* __restrict__ me = tx + t;
    const float f0 = me->f0, drift = me->drift;
    first[t] = synth_first_index(me->t0);
    double phi = 0.0;
    for (int i = 0; i < kNSymD; ++i) {
        const double dphi = synth_dphi(f0, drift, i, me->symbols[i]);
        for (int q = 0; q < kSps / kCkptEvery; ++q) {
            ckpt[(size_t)(i * (kSps / kCkptEvery) + q) * ntx + t] = phi;
            for (int j = 0; j < kCkptEvery; ++j) phi += dphi;
        }
    }
}

__global__ __launch_bounds__(256)
void synth_fill_kernel(const SynthTx* __restrict__ tx, int ntx, const int* __restrict__ seg_off,
                       const int* __restrict__ first, const double* __restrict__ ckpt, long long seg_index0,
                       float sigma, unsigned long long seed, int accumulate, int seg_base, float* __restrict__ dI,
                       float* __restrict__ dQ) {
    const int seg = seg_base + blockIdx.y;
    const int base = (blockIdx.x * 256 + threadIdx.x) * kPerThread;     // < kIqStride by the grid
    float4* __restrict__ pi = reinterpret_cast<float4*>(dI + (size_t)seg * kIqStride + base);
    float4* __restrict__ pq = reinterpret_cast<float4*>(dQ + (size_t)seg * kIqStride + base);
    float xi[kPerThread], xq[kPerThread];
    synth_tile_load(pi, pq, accumulate, xi, xq);
    synth_tile_noise(seed, seg_index0 + seg, base, sigma, xi, xq);
    const int t_end = seg_off[seg + 1];
    for (int t = seg_off[seg]; t < t_end; ++t) {
        const int n0 = base - first[t];                    // the transmission's sample index at this thread's first output
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
                xi[s] = (float)((double)xi[s] + amp * cs);
                xq[s] = (float)((double)xq[s] + amp * sn);
                phi += dphi;
            }
        }
    }
    synth_tile_store(pi, pq, xi, xq);
}
}  // namespace

size_t synth_checkpoint_doubles(int ntx) { return (size_t)kCkptPerTx * (size_t)(ntx > 0 ? ntx : 0); }

// the phase checkpoints [checkpoint][transmission] and first indices alone: K13 (k13_fade.hip) fills from the same ones
void launch_synth_phase(const SynthTx* tx, int ntx, double* ckpt, int* first, hipStream_t st) {
    if (ntx > 0)
        hipLaunchKernelGGL(synth_phase_kernel, dim3((ntx + 63) / 64), dim3(64), 0, st, tx, ntx, ckpt, first);
}

void launch_synth(const SynthTx* tx, int ntx, const int* seg_off, int nseg, long long seg_index0, float sigma,
                  unsigned long long seed, int accumulate, double* ckpt, int* first, float* dI, float* dQ,
                  hipStream_t st) {
    if (nseg <= 0) return;
    launch_synth_phase(tx, ntx, ckpt, first, st);
    for (int s0 = 0; s0 < nseg; s0 += 32768)               // grid.y is limited to 65 535
        hipLaunchKernelGGL(synth_fill_kernel, dim3(kIqStride / kTile, nseg - s0 < 32768 ? nseg - s0 : 32768), dim3(256), 0, st,
                           tx, ntx, seg_off, first, ckpt, seg_index0, sigma, seed, accumulate, s0, dI, dQ);
}

}  // namespace wspr
