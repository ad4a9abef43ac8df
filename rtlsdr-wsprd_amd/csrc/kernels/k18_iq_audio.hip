// K18, IQ to audio: the decoder's 375 Hz IQ rows -> 16-bit PCM at 12 000 Hz with the WSPR band at 1 500 Hz, the records K12
// and K15 take.  The definition (the order of the at most 24 fused multiply-adds per output, the steps that are not part of
// the chain, the quantiser) is iq_audio.h; the serial checker tests/helpers/iq_audio_check.c is the contract, and the rows
// and counts here are the checker's bit for bit.  Every multiply-add is an explicit fma in the definition's order.
//
// Shape.  A workgroup of four wavefronts owns IQ_AUDIO_TILE = 2 048 consecutive outputs of one row: the 64 blocks of 32
// outputs that are centred on the inputs b0 .. b0 + 63.  Lane t of EVERY wavefront owns block b0 + t; wavefront q owns the
// outputs 8 q .. 8 q + 7 of each block, so a thread makes 8 consecutive samples, one 16-byte vector.
//   input   Output 32 b + p draws on the inputs b - 7 .. b + 8 (b + 8 only for p >= 1: tap -256 does not exist).  The tile's
//           64 + 2 x 8 inputs are staged once as {I, Q} pairs; a lane walks its 16 pairs in rising m with one 8-byte LDS read
//           each, consecutive lanes reading consecutive pairs.
//   taps    The tap of a step depends on (p, b - m) alone, and p is the wavefront's: a scalar operand, from a constant table
//           arranged [q][step][12] in the order the six packed multiply-adds of a step take them (the table's values are
//           known at compile time and the unrolled walk carries them as literals).
//   chains  n = p (mod 8) decides the rails of an output (iq_audio.h): outputs 0 and 4 of a thread take I alone, 2 and 6 take
//           Q alone, the odd ones both, I first.  Two outputs share one v_pk_fma_f32: {0, 2} and {4, 6} against {I, Q},
//           {1, 3} and {5, 7} against {I, I} and then against {Q, Q} -- twelve multiply-adds per step and thread, and each
//           output's own order is the definition's.
//   edges   A step whose m lies outside [0, np) is not part of the chain (the input may be non-finite: multiplying a staged
//           zero would not do).  Only the tiles at either end of a row have such steps; they run the same walk with a select
//           behind every multiply-add, every other tile runs it bare.
//   output  The four wavefronts' vectors of a block are 16 bytes apart in the record: they meet in LDS and leave as one
//           contiguous 4 KB run, thread t storing bytes 16 t .. 16 t + 15 of the tile.
//   counts  Clipped samples are summed over the wavefront by ballots and added to the row's counter with one vector atomic
//           per wavefront that has any, as in K17.
#include <hip/hip_runtime.h>

#include "iq_audio.h"
#include "wspr_device.h"

namespace wspr {
namespace {
typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int kTile = IQ_AUDIO_TILE;                  // outputs per workgroup
constexpr int kBlocks = kTile / IQ_AUDIO_INTERP;      // 64: inputs a tile is centred on, one per lane
constexpr int kHalo = 8;                              // inputs staged on each side (7 and 8 are used; 8 keeps the loads aligned)
constexpr int kStage = kBlocks + 2 * kHalo;           // 80 staged inputs per rail
constexpr int kThreads = 256;
constexpr int kSteps = 16;                            // step i of block b is input m = b - 7 + i
static_assert(kBlocks == 64 && kThreads == 4 * kBlocks, "a lane per block, a wavefront per quarter of a block");
static_assert(kMaxSamples == IQ_AUDIO_MAX_SAMPLES, "the decoder's row");

// g[q][i][.]: the taps k = 32 (7 - i) + 8 q + e of step i for the outputs e of wavefront q, in the order of use:
//   0 gI e=0   1 gQ e=2   2 gI e=4   3 gQ e=6   4..7 gI e=1,3,5,7   8..11 gQ e=1,3,5,7
// (k = -256, q = 0, e = 0, i = 15, does not exist: the entry is zero and never used)
struct TapTable { float g[4][kSteps][12]; };
constexpr float tap_at(int rail, int k) {
    const bool in = k >= -AUDIO_FRONT_K && k <= AUDIO_FRONT_K;
    return __builtin_bit_cast(float, in ? (rail ? audio_front_gq_bits : audio_front_gi_bits)[k + AUDIO_FRONT_K] : 0u);
}
constexpr TapTable make_taps() {
    TapTable t{};
    for (int q = 0; q < 4; ++q)
        for (int i = 0; i < kSteps; ++i) {
            const int k0 = 32 * (7 - i) + 8 * q;
            float* g = t.g[q][i];
            g[0] = tap_at(0, k0);     g[1] = tap_at(1, k0 + 2); g[2] = tap_at(0, k0 + 4); g[3] = tap_at(1, k0 + 6);
            for (int h = 0; h < 4; ++h) { g[4 + h] = tap_at(0, k0 + 2 * h + 1); g[8 + h] = tap_at(1, k0 + 2 * h + 1); }
        }
    return t;
}
__constant__ TapTable c_taps = make_taps();

// the rails of the eight outputs are what iq_audio.h says they are
constexpr bool rails_ok() {
    for (int e = 0; e < 8; ++e) {
        const bool wantI = e != 2 && e != 6, wantQ = e != 0 && e != 4;
        for (int k = e - 256; k <= AUDIO_FRONT_K; k += 8)
            if (k >= -AUDIO_FRONT_K && (iq_audio_skipped(0, k) == wantI || iq_audio_skipped(1, k) == wantQ)) return false;
    }
    return true;
}
static_assert(rails_ok(), "the kernel's choice of rails per output is not the definition's");

__device__ __forceinline__ f2 pk_fma(float g0, float g1, f2 x, f2 a) {
    const f2 g = {g0, g1};
    return __builtin_elementwise_fma(g, x, a);
}

// The walk of one thread: a[0] = outputs {0, 2}, a[1] = {4, 6}, a[2] = {1, 3}, a[3] = {5, 7}.  in: the staged pair of the
// thread's step 0.  EDGE: m = m0 + i outside [0, np) leaves the chains alone.
template <int QQ, bool EDGE>
__device__ __forceinline__ void walk(f2 (&a)[4], const f2* __restrict__ in, int m0, int np) {
#pragma unroll
    for (int i = 0; i < kSteps; ++i) {
        const float* __restrict__ g = c_taps.g[QQ][i];
        const f2 x = in[i];
        const f2 xi = {x.x, x.x}, xq = {x.y, x.y};
        f2 r0 = a[0];
        if (QQ == 0 && i == kSteps - 1) r0.y = __builtin_fmaf(g[1], x.y, r0.y);      // output 0 of the block: no tap -256
        else r0 = pk_fma(g[0], g[1], x, r0);
        f2 r1 = pk_fma(g[2], g[3], x, a[1]);
        f2 r2 = pk_fma(g[4], g[5], xi, a[2]);
        f2 r3 = pk_fma(g[6], g[7], xi, a[3]);
        r2 = pk_fma(g[8], g[9], xq, r2);
        r3 = pk_fma(g[10], g[11], xq, r3);
        if (EDGE) {
            const int m = m0 + i;
            const bool ok = m >= 0 && m < np;
            a[0] = ok ? r0 : a[0]; a[1] = ok ? r1 : a[1]; a[2] = ok ? r2 : a[2]; a[3] = ok ? r3 : a[3];
        } else {
            a[0] = r0; a[1] = r1; a[2] = r2; a[3] = r3;
        }
    }
}

template <int QQ>
__device__ __forceinline__ void walk_tile(f2 (&a)[4], const f2* __restrict__ in, bool edge, int m0, int np) {
    if (edge) walk<QQ, true>(a, in, m0, np);
    else walk<QQ, false>(a, in, m0, np);
}

__global__ __launch_bounds__(kThreads)
void iq_audio_kernel(const float* __restrict__ dI, const float* __restrict__ dQ, size_t stride, int np, float gain,
                     int seg_base, int16_t* __restrict__ pcm, size_t pcm_stride, int* __restrict__ n_clipped) {
    __shared__ f2 in[kStage];                                  // {I, Q} of the inputs b0 - 8 .. b0 + 71
    __shared__ uint4 out[kThreads];                            // the tile's 2 048 samples in output order
    const int tid = threadIdx.x, lane = tid & 63;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t seg = (size_t)seg_base + blockIdx.y;
    const int b0 = blockIdx.x * kBlocks;                       // below np: the grid has ceil(np / 64) tiles
    // staging: 20 chunks of four inputs per rail.  b0 - 8 is a multiple of 4, the rows are 16-byte aligned and the stride a
    // multiple of 4: a chunk inside [0, np) is one aligned load; one that straddles either end is read input by input, so
    // that nothing at or behind np is read.
    if (tid < 2 * (kStage / 4)) {
        const int rail = tid >= kStage / 4, c = tid - rail * (kStage / 4);
        const int m0 = b0 - kHalo + 4 * c;
        const float* __restrict__ row = (rail ? dQ : dI) + seg * stride;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (m0 >= 0 && m0 + 3 < np) {
            const float4 t = *reinterpret_cast<const float4*>(row + m0);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (m0 + e >= 0 && m0 + e < np) v[e] = row[m0 + e];
        }
        float* __restrict__ dst = reinterpret_cast<float*>(in) + 2 * (4 * c) + rail;
        dst[0] = v[0]; dst[2] = v[1]; dst[4] = v[2]; dst[6] = v[3];
    }
    __syncthreads();
    const int b = b0 + lane;
    const bool edge = b0 < 7 || b0 + kBlocks + 8 > np;         // the tile has a step outside [0, np): the same for all of it
    f2 a[4] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
    const f2* __restrict__ mine = in + lane + 1;               // input b - 7 is staged at lane + 1
    if (q == 0) walk_tile<0>(a, mine, edge, b - 7, np);
    else if (q == 1) walk_tile<1>(a, mine, edge, b - 7, np);
    else if (q == 2) walk_tile<2>(a, mine, edge, b - 7, np);
    else walk_tile<3>(a, mine, edge, b - 7, np);
    // a block at or behind np (the last tile of a row) is neither stored nor counted; no lane leaves early: the barrier and
    // the ballots below want the whole wavefront
    const bool active = b < np;
    const float r[8] = {a[0].x, a[2].x, a[0].y, a[2].y, a[1].x, a[3].x, a[1].y, a[3].y};
    int clipped = 0;
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t lo = (uint16_t)iq_audio_sample(r[2 * e], gain, &clipped);
        const uint32_t hi = (uint16_t)iq_audio_sample(r[2 * e + 1], gain, &clipped);
        w[e] = lo | (hi << 16);
    }
    if (!active) clipped = 0;
    out[4 * lane + q] = make_uint4(w[0], w[1], w[2], w[3]);
    __syncthreads();
    const int n = blockIdx.x * kTile + 8 * tid;                // 32 np is a multiple of 8: a vector lies inside the record or outside
    if (n < IQ_AUDIO_INTERP * np) *reinterpret_cast<uint4*>(pcm + seg * pcm_stride + n) = out[tid];
    // the wavefront's sum of a per-lane count <= 8
    uint32_t sum = 0;
#pragma unroll
    for (int bit = 0; bit < 4; ++bit) sum += (uint32_t)__popcll(__ballot((clipped >> bit) & 1)) << bit;
    if (lane == 0 && sum) atomicAdd(n_clipped + seg, (int)sum);
}
}  // namespace

void launch_iq_audio(const float* dI, const float* dQ, size_t stride, int samples, int nseg, float gain, int16_t* pcm,
                     size_t pcm_stride, int* n_clipped, hipStream_t st) {
    if (nseg <= 0 || samples <= 0) return;
    const int ntiles = (samples + kBlocks - 1) / kBlocks;       // 704 at the most
    for (int s0 = 0; s0 < nseg; s0 += 32768)                   // grid.y is limited to 65 535
        hipLaunchKernelGGL(iq_audio_kernel, dim3(ntiles, nseg - s0 < 32768 ? nseg - s0 : 32768), dim3(kThreads), 0, st, dI, dQ,
                           stride, samples, gain, s0, pcm, pcm_stride, n_clipped);
}

}  // namespace wspr
