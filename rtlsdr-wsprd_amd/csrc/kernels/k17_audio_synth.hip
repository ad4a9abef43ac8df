// K17: the 12 kHz audio scene synthesiser (wspr_synth_audio*(), include/wspr_mi355x.h) -- message, f0, t0, level and
// drift to the 16-bit records K12 and K15 take, for batches of scenes resident in HBM.  The definition is audio_synth.h;
// tests/helpers/audio_synth_check.cpp is its serial form, and the rows and counts here are the checker's bit for bit.
//
//   audio_synth_phase_kernel  one lane per transmission walks the 162 dependent adds and writes P_i and dphi_i
//                             (2 x 162 doubles per transmission, layout [symbol][transmission]) and the first index.
//   audio_synth_fill_kernel   workgroup = (record, tile of 2 048 samples); a thread owns 8 consecutive samples as doubles
//                             in registers: loads them (accumulate) with one 16-byte load, draws their noise (one Philox
//                             draw per two samples), then for each transmission of the record evaluates synth_sincos() at
//                             phi = P_i + j dphi_i -- no chain inside a thread, so its samples may straddle a symbol
//                             boundary or either end of the frame --, quantises and stores 16 bytes.  Clipped samples are
//                             summed over the wavefront by ballots and added to the record's counter with one vector
//                             atomic per wavefront that has any: integer counts, so the result does not depend on the order.
// The bound is the fp64 vector rate: one transmission sample costs 53 double operations, none fused (2 phase, 9 reduction,
// 18 sine kernel, 22 cosine kernel, 2 accumulate) and an int-to-double conversion.
#include <hip/hip_runtime.h>

#include "audio_synth.h"
#include "wspr_device.h"

namespace wspr {

static_assert(kSynthNsym == kNSymD, "synth_math.h and wspr_device.h disagree");

namespace {
constexpr int kPerThread = 8;                             // one 16-byte vector of int16
constexpr int kThreads = 256;
constexpr int kTile = kAudioSynthTile;
static_assert(kTile == kThreads * kPerThread, "a workgroup covers a tile");

__global__ __launch_bounds__(64)
void audio_synth_phase_kernel(const SynthTx* __restrict__ tx, int ntx, double* __restrict__ phase, int* __restrict__ first) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= ntx) return;
    const SynthTx* __restrict__ me = tx + t;
    first[t] = audio_synth_first(me->t0);
    audio_synth_phases(me->f0, me->drift, me->symbols, phase + t, phase + (size_t)kNSymD * ntx + t, ntx);
}

__global__ __launch_bounds__(kThreads)
void audio_synth_fill_kernel(const SynthTx* __restrict__ tx, int ntx, const int* __restrict__ seg_off,
                             const int* __restrict__ first, const double* __restrict__ phase, long long seg_index0, int nsamp,
                             float sigma, unsigned long long seed, int accumulate, int seg_base, int16_t* __restrict__ pcm,
                             size_t pcm_stride, int* __restrict__ n_clipped) {
    const int seg = seg_base + blockIdx.y;
    const int base = (blockIdx.x * kThreads + threadIdx.x) * kPerThread;
    // a chunk that starts below nsamp ends inside the row: the stride is a multiple of 8 that is >= nsamp.  No lane
    // leaves early: the ballots below want the whole wavefront.
    const bool active = base < nsamp;
    uint4* __restrict__ out = reinterpret_cast<uint4*>(pcm + (size_t)seg * pcm_stride + (active ? base : 0));
    uint32_t raw[4] = {0u, 0u, 0u, 0u};
    if (active && accumulate) { const uint4 v = *out; raw[0] = v.x; raw[1] = v.y; raw[2] = v.z; raw[3] = v.w; }
    double acc[kPerThread];
#pragma unroll
    for (int s = 0; s < kPerThread; ++s) acc[s] = (double)(int)(short)(raw[s >> 1] >> (16 * (s & 1)));
    if (active && sigma > 0.0f) {
#pragma unroll
        for (int m = 0; m < kPerThread / 2; ++m) {
            if (base + 2 * m < nsamp) {
                float a, b;
                synth_gauss(seed, seg_index0 + seg, (uint32_t)((base >> 1) + m), kAudioSynthNoiseStream, sigma, &a, &b);
                acc[2 * m] = acc[2 * m] + (double)a;
                acc[2 * m + 1] = acc[2 * m + 1] + (double)b;        // (outside the record: never stored)
            }
        }
    }
    const int t_end = active ? seg_off[seg + 1] : 0;
    for (int t = active ? seg_off[seg] : 0; t < t_end; ++t) {
        const int n0 = base - first[t];                    // the transmission's sample index at this thread's first output
        if (n0 + kPerThread <= 0 || n0 >= kAudioSynthSigLen) continue;
        const double amp = (double)tx[t].amp;
        int cur = -1;
        double P = 0.0, dphi = 0.0;
#pragma unroll
        for (int s = 0; s < kPerThread; ++s) {
            const int n = n0 + s;
            if (n >= 0 && n < kAudioSynthSigLen && base + s < nsamp) {
                const int i = n >> 13;
                if (i != cur) {
                    cur = i;
                    P = phase[(size_t)i * ntx + t];
                    dphi = phase[(size_t)(kNSymD + i) * ntx + t];
                }
                const double phi = P + (double)(n & (kAudioSynthSps - 1)) * dphi;
                double sn, cs;
                synth_sincos(phi, &sn, &cs);
                acc[s] = acc[s] + amp * cs;
            }
        }
    }
    int clipped = 0;
    if (active) {
        uint32_t w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            uint32_t lo = accumulate ? raw[e] & 0xffffu : 0u, hi = accumulate ? raw[e] >> 16 : 0u;   // from nsamp on: kept, or zero
            if (base + 2 * e < nsamp) lo = (uint32_t)(uint16_t)audio_synth_quantise(acc[2 * e], &clipped);
            if (base + 2 * e + 1 < nsamp) hi = (uint32_t)(uint16_t)audio_synth_quantise(acc[2 * e + 1], &clipped);
            w[e] = lo | (hi << 16);
        }
        *out = make_uint4(w[0], w[1], w[2], w[3]);
    }
    // the wavefront's sum of a per-lane count <= 8
    uint32_t sum = 0;
#pragma unroll
    for (int bit = 0; bit < 4; ++bit) sum += (uint32_t)__popcll(__ballot((clipped >> bit) & 1)) << bit;
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(n_clipped + seg, (int)sum);
}
}  // namespace

size_t audio_synth_phase_doubles(int ntx) { return (size_t)2 * kNSymD * (size_t)(ntx > 0 ? ntx : 0); }

void launch_audio_synth(const SynthTx* tx, int ntx, const int* seg_off, int nseg, long long seg_index0, int nsamp, float sigma,
                        unsigned long long seed, int accumulate, double* phase, int* first, int16_t* pcm, size_t pcm_stride,
                        int* n_clipped, hipStream_t st) {
    if (nseg <= 0 || nsamp <= 0) return;
    if (ntx > 0)
        hipLaunchKernelGGL(audio_synth_phase_kernel, dim3((ntx + 63) / 64), dim3(64), 0, st, tx, ntx, phase, first);
    const int ntiles = (nsamp + kTile - 1) / kTile;          // 704 at the most
    for (int s0 = 0; s0 < nseg; s0 += 32768)               // grid.y is limited to 65 535
        hipLaunchKernelGGL(audio_synth_fill_kernel, dim3(ntiles, nseg - s0 < 32768 ? nseg - s0 : 32768), dim3(kThreads), 0, st,
                           tx, ntx, seg_off, first, phase, seg_index0, nsamp, sigma, seed, accumulate, s0, pcm, pcm_stride,
                           n_clipped);
}

}  // namespace wspr
