// K11: the Doppler-spread figure of a decoded spot (wspr_spread_batch(), wspr_set_spread_estimate(); the definition in
// spread.h, tests/helpers/spread_check.c its serial form).  Per job -- a row, (f0, shift, drift) and the 162 channel
// symbols of the message it carries -- the modulation is wiped off with the synthesiser's exact double phase, the result
// is summed over blocks of 32 samples, and the spectrum of the 1 296 block sums gives the width that holds the middle half
// of the carrier's power.
//   spread_phase_kernel  K8's synth_phase_kernel over the job list: one lane per job walks the 41 472 dependent adds and
//                        writes phi at every 64th sample (layout [checkpoint][job], 5 184 B per job).
//   spread_kernel        one workgroup of 256 threads per job.  Six rounds of 256 blocks: the round's 8 192 samples of both
//                        rails come in with aligned 16-byte loads (a float4 never leaves the row: rows are kIqStride
//                        floats, 256-byte aligned) and are staged in LDS with a pitch of 33 floats, so that a thread that
//                        owns one whole block reads it without bank conflicts; the thread walks 0 or 32 adds from the
//                        checkpoint below its block and forms the block's two sums in registers.  The 2 048-point
//                        transform runs in the staging area (16 KB of it), four butterflies per thread and stage; lanes
//                        0-39 and 0-63 sum one chunk of 16 bins each, lane 0 accumulates the chunk totals and searches
//                        the crossings.  Four words per job leave with one 16-byte vector store; neither z, y nor P
//                        reaches HBM.  No atomics, no inline assembly; every job is independent: deterministic.
// The bound is the fp64 vector rate, as for K8's fill kernel: 58 double operations per sample, none fused.
#include <hip/hip_runtime.h>

#include "spread.h"
#include "wspr_device.h"

namespace wspr {

static_assert(kSynthSamples == kMaxSamples && kSynthSigLen == kSigLen, "synth_math.h and wspr_device.h disagree");

namespace {
constexpr int kCkptEvery = 64;
constexpr int kCkptPerJob = kSigLen / kCkptEvery;         // 648
constexpr int kRound = 256;                               // blocks per round = threads
constexpr int kRounds = (spread::kBlocks + kRound - 1) / kRound;   // 6
constexpr int kPitch = spread::kBlockLen + 1;             // floats between two blocks in the staging area
constexpr int kStageFloats = 2 * kRound * kPitch;         // 16 896
constexpr int kYFloats = 2 * spread::kBlocks;             // 2 592: the block sums, later the chunk totals
static_assert(kStageFloats >= 2 * spread::kFft, "the transform runs in the staging area");
static_assert(kYFloats * 4 >= (spread::kNoiseChunks + spread::kSignalChunks) * 8 + spread::kSignalChunks * 4, "chunk totals fit");
static_assert(kIqStride % 4 == 0 && (kStageFloats * 4) % 8 == 0, "16-byte loads stay in the row; doubles are aligned");

__global__ __launch_bounds__(64)
void spread_phase_kernel(const SubJob* __restrict__ jobs, int n, double* __restrict__ ckpt) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const SubJob* __restrict__ me = jobs + t;
    const float f0 = me->f0, drift = me->drift;
    double phi = 0.0;
    for (int i = 0; i < kNSymD; ++i) {
        const double dphi = synth_dphi(f0, drift, i, me->sym[i]);
        for (int q = 0; q < kSps / kCkptEvery; ++q) {
            ckpt[(size_t)(i * (kSps / kCkptEvery) + q) * n + t] = phi;
            for (int j = 0; j < kCkptEvery; ++j) phi += dphi;
        }
    }
}

__global__ __launch_bounds__(256)
void spread_kernel(const float* __restrict__ dI, const float* __restrict__ dQ, int samples, const SubJob* __restrict__ jobs,
                   int n, const double* __restrict__ ckpt, const float* __restrict__ tw, uint4* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[kStageFloats + kYFloats];
    float* const sI = lds;
    float* const sQ = lds + kRound * kPitch;
    float* const yr = lds + kStageFloats;
    float* const yi = yr + spread::kBlocks;
    const int job = blockIdx.x, tid = threadIdx.x;
    const SubJob* __restrict__ me = jobs + job;
    const float f0 = me->f0, drift = me->drift;
    const int shift = spread::clamp_shift(me->shift);
    const float* __restrict__ rowI = dI + (size_t)me->seg * kIqStride;
    const float* __restrict__ rowQ = dQ + (size_t)me->seg * kIqStride;

    for (int r = 0; r < kRounds; ++r) {
        const int nb = spread::kBlocks - r * kRound < kRound ? spread::kBlocks - r * kRound : kRound;   // blocks of this round
        const int k0 = shift + r * kRound * spread::kBlockLen;            // row index of the round's first sample
        const int a0 = k0 & ~3;                                           // ... rounded down to a 16-byte boundary
        if (r) __syncthreads();                                           // the round before has been read
        for (int v = tid; v < nb * (spread::kBlockLen / 4) + 1; v += 256) {
            const int a = a0 + 4 * v;
            float4 xi = make_float4(0.f, 0.f, 0.f, 0.f), xq = xi;
            if (a >= 0 && a < samples) {                                  // samples <= kMaxSamples < kIqStride, a % 4 == 0
                xi = *reinterpret_cast<const float4*>(rowI + a);
                xq = *reinterpret_cast<const float4*>(rowQ + a);
            }
            const float ei[4] = {xi.x, xi.y, xi.z, xi.w}, eq[4] = {xq.x, xq.y, xq.z, xq.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int o = a + e - k0;
                if (o >= 0 && o < nb * spread::kBlockLen) {
                    const bool in = a + e < samples;                      // (a + e >= 0 wherever something was loaded)
                    sI[(o >> 5) * kPitch + (o & 31)] = in ? ei[e] : 0.0f;
                    sQ[(o >> 5) * kPitch + (o & 31)] = in ? eq[e] : 0.0f;
                }
            }
        }
        __syncthreads();
        const int b = r * kRound + tid;
        if (b < spread::kBlocks) {
            const int sym = b >> 3;                                       // 8 blocks per symbol
            const double dphi = synth_dphi(f0, drift, sym, me->sym[sym]);
            double phi = ckpt[(size_t)(b >> 1) * n + job];
            if (b & 1) for (int j = 0; j < spread::kBlockLen; ++j) phi += dphi;
            float sr, si;
            spread::spread_block(sI + tid * kPitch, sQ + tid * kPitch, phi, dphi, &sr, &si);
            yr[b] = sr;
            yi[b] = si;
        }
    }
    __syncthreads();
    float* const re = lds;
    float* const im = lds + spread::kFft;
    for (int p = tid; p < spread::kFft; p += 256) {
        re[p] = p < spread::kBlocks ? yr[p] : 0.0f;
        im[p] = p < spread::kBlocks ? yi[p] : 0.0f;
    }
    __syncthreads();
    for (int st = 0; st < spread::kStages; ++st) {
#pragma unroll
        for (int q = 0; q < spread::kTwiddles / 256; ++q) spread::spread_butterfly(re, im, tw, st, tid + 256 * q);
        __syncthreads();
    }
    double* const noise = reinterpret_cast<double*>(lds + kStageFloats);
    double* const sig = noise + spread::kNoiseChunks;
    float* const maxp = reinterpret_cast<float*>(sig + spread::kSignalChunks);
    if (tid < spread::kNoiseChunks) noise[tid] = spread::spread_noise_chunk(re, im, tid);
    __syncthreads();
    const double nz = spread::spread_noise_floor(noise);
    if (tid < spread::kSignalChunks) {
        float mx;
        sig[tid] = spread::spread_signal_chunk(re, im, tid, nz, &mx);
        maxp[tid] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        const spread::Result res = spread::spread_width(re, im, sig, maxp, nz);
        out[job] = make_uint4(__float_as_uint(res.w50), __float_as_uint(res.f50), __float_as_uint(res.ratio), (unsigned)res.valid);
    }
}
}  // namespace

size_t spread_checkpoint_doubles(int n) { return (size_t)kCkptPerJob * (size_t)(n > 0 ? n : 0); }

void launch_spread(const float* dI, const float* dQ, int samples, const SubJob* jobs, int n, double* ckpt, const float* tw,
                   void* out, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(spread_phase_kernel, dim3((n + 63) / 64), dim3(64), 0, st, jobs, n, ckpt);
    hipLaunchKernelGGL(spread_kernel, dim3(n), dim3(256), 0, st, dI, dQ, samples, jobs, n, ckpt, tw, static_cast<uint4*>(out));
}

}  // namespace wspr
