// K12, the 12 kHz audio front end: 16-bit PCM with the WSPR band at 1 500 Hz -> the decoder's 375 Hz IQ rows.
// The definition (taps, order of the 511 fused multiply-adds per rail and output) is audio_front.h; the serial checker
// tests/helpers/audio_check.c is the contract.  Every multiply-add here is an explicit fma in the definition's order.
//
// Shape.  A workgroup of two wavefronts owns AUDIO_FRONT_TILE = 512 consecutive outputs of one record: wavefront 0 the
// I rail, wavefront 1 the Q rail, lane t the 8 consecutive outputs 8t .. 8t+7 of the tile.  The lane walks the 735 input
// samples its outputs touch in rising order (so every output sees its own taps in rising k) and applies each sample to the
// up to 8 outputs whose window holds it: one word of LDS feeds up to 16 multiply-adds, and a lane keeps 8 independent
// chains going, as four packed ones.
//   input   The tile's 66 x 256 samples (a halo of 256 on each side) come from HBM as aligned 16-byte loads and are staged
//           POLYPHASE: sample S0 + 256 c + ph sits at [ph][c], so the lanes of a wavefront, whose samples are 256 apart,
//           read consecutive words.  The samples stay 16-bit in LDS, two neighbouring phases to a word -- as floats the
//           tile would take 74 KB and leave one wavefront per SIMD; at 35 KB four workgroups share a CU -- and are
//           converted as they are used; the factor 2^-15 is folded into the taps (an exact scaling: the products, hence
//           the fused results, are the definition's).  Row r of the image is rotated by r / 32 columns: the staging
//           stores of a half-wave then fall on 32 different banks (pitch 69, odd).
//   taps    The tap a step needs is the same for every lane: it comes from constant memory through the scalar cache,
//           transposed ([phase][row of 32 taps]) so that the 8 taps of a step are one 32-byte scalar load.
//   zeros   gI[k] is +0 for k = 2, 6 (mod 8), gQ[k] for k = 0, 4 (mod 8): those steps are skipped (audio_front.h says why
//           that changes nothing).  x = 0 outside [0, nsamp) comes from the staging guard, never from a neighbouring row
//           or the padding of the stride.
#include "audio_front.h"
#include "wspr_device.h"

namespace wspr {
namespace {
typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int kTile = AUDIO_FRONT_TILE;              // outputs per workgroup
constexpr int kPerLane = 8;                          // consecutive outputs per lane
constexpr int kPoly = AUDIO_FRONT_DECIM * kPerLane;  // 256: the lanes' samples are this far apart
constexpr int kCols = 64 + 2;                        // columns of 256 samples in a tile: 64 lanes and the halo
constexpr int kChunks = kCols * kPoly / 8;           // 16-byte loads per tile
constexpr int kPitch = 69;                           // words per image row: kCols + the largest rotation (3), odd
constexpr int kRows = kPoly / 2;                     // two phases to a word
constexpr int kTilesPerRow = kIqStride / kTile;
static_assert(kTile == 64 * kPerLane && kIqStride % kTile == 0, "tiles cover an output row exactly");
static_assert(kMaxSamples == AUDIO_FRONT_MAX_OUT, "the decoder's row");

// g[rail][p][jj] = 2^-15 * tap(32 * (jj - 15) + p), zero outside -255 .. 255: block b of a lane's walk needs, for its output
// 7 - e, the tap 32 * (b - 15 + e) + p -- entries b .. b + 7 of row p.
struct TapTable { float g[2][32][32]; };
constexpr TapTable make_taps() {
    TapTable t{};
    for (int rail = 0; rail < 2; ++rail)
        for (int p = 0; p < 32; ++p)
            for (int jj = 0; jj < 32; ++jj) {
                const int k = 32 * (jj - 15) + p;
                const bool in = k >= -AUDIO_FRONT_K && k <= AUDIO_FRONT_K;
                const uint32_t bits = in ? (rail ? audio_front_gq_bits : audio_front_gi_bits)[k + AUDIO_FRONT_K] : 0u;
                t.g[rail][p][jj] = __builtin_bit_cast(float, bits) * 0x1p-15f;
            }
    return t;
}
__constant__ TapTable c_taps = make_taps();

constexpr bool skipped(int rail, int p) { return rail == 0 ? (p % 8 == 2 || p % 8 == 6) : (p % 8 == 0 || p % 8 == 4); }

// one sample into the chains LO <= e < HI (e = 7 - output index): pairs as one packed fma
template <int LO, int HI>
__device__ __forceinline__ void step(f2 (&a)[4], const float* __restrict__ g, float x) {
#pragma unroll
    for (int pr = 0; pr < 4; ++pr) {
        const bool in0 = 2 * pr >= LO && 2 * pr < HI, in1 = 2 * pr + 1 >= LO && 2 * pr + 1 < HI;
        if (in0 && in1) {
            const f2 gg = {g[2 * pr], g[2 * pr + 1]}, xx = {x, x};
            a[pr] = __builtin_elementwise_fma(gg, xx, a[pr]);
        } else if (in0) {
            a[pr].x = __builtin_fmaf(g[2 * pr], x, a[pr].x);
        } else if (in1) {
            a[pr].y = __builtin_fmaf(g[2 * pr + 1], x, a[pr].y);
        }
    }
}

// block `blk` of the walk: samples 32 blk .. 32 blk + 31 of the lane's 736; `img` = the image at the lane's column
template <int RAIL, int LO, int HI>
__device__ __forceinline__ void walk_block(f2 (&a)[4], const uint32_t* __restrict__ img, int blk) {
    const uint32_t* __restrict__ src = img + (16 * (blk & 7)) * kPitch + (blk >> 3) + ((blk & 7) >> 1);
    const float* __restrict__ taps = &c_taps.g[RAIL][0][blk];
#pragma unroll
    for (int pp = 0; pp < 16; ++pp) {
        if (skipped(RAIL, 2 * pp) && skipped(RAIL, 2 * pp + 1)) continue;
        const uint32_t w = src[pp * kPitch];
        if (!skipped(RAIL, 2 * pp)) step<LO, HI>(a, taps + (2 * pp) * 32, (float)(int)(short)(w & 0xffffu));
        if (!skipped(RAIL, 2 * pp + 1)) step<LO, HI>(a, taps + (2 * pp + 1) * 32, (float)((int)w >> 16));
    }
}

template <int RAIL, int B>
__device__ __forceinline__ void walk_edge(f2 (&a)[4], const uint32_t* __restrict__ img) {
    walk_block<RAIL, (7 - B > 0 ? 7 - B : 0), (23 - B < 8 ? 23 - B : 8)>(a, img, B);
}

template <int RAIL>
__device__ __forceinline__ void walk(f2 (&a)[4], const uint32_t* __restrict__ img) {
    walk_edge<RAIL, 0>(a, img); walk_edge<RAIL, 1>(a, img); walk_edge<RAIL, 2>(a, img); walk_edge<RAIL, 3>(a, img);
    walk_edge<RAIL, 4>(a, img); walk_edge<RAIL, 5>(a, img); walk_edge<RAIL, 6>(a, img);
#pragma unroll 1
    for (int blk = 7; blk < 16; ++blk) walk_block<RAIL, 0, 8>(a, img, blk);       // every output's window holds these
    walk_edge<RAIL, 16>(a, img); walk_edge<RAIL, 17>(a, img); walk_edge<RAIL, 18>(a, img); walk_edge<RAIL, 19>(a, img);
    walk_edge<RAIL, 20>(a, img); walk_edge<RAIL, 21>(a, img); walk_edge<RAIL, 22>(a, img);
}

__global__ __launch_bounds__(128)
void audio_front_kernel(const int16_t* __restrict__ pcm, size_t pcm_stride, int nsamp, int n_out,
                        float* __restrict__ dI, float* __restrict__ dQ) {
    __shared__ uint32_t img[kRows * kPitch];
    const int tid = threadIdx.x, lane = tid & 63;
    const int rail = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x % kTilesPerRow;
    const size_t seg = blockIdx.x / kTilesPerRow;
    const int m0 = tile * kTile;
    float4* __restrict__ out = reinterpret_cast<float4*>((rail ? dQ : dI) + seg * kIqStride + m0 + kPerLane * lane);
    if (m0 >= n_out) {                                       // the row's tail: zeros up to the stride
        out[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        out[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    // staging: chunk i = samples S0 + 8 i .. + 7, S0 = 32 m0 - 256 (a multiple of 8: the loads are aligned, and a chunk
    // that starts below nsamp ends inside the row, pcm_stride being a multiple of 8 that is >= nsamp)
    const int16_t* __restrict__ row = pcm + seg * pcm_stride;
    const long s0 = 32L * m0 - kPoly;
    for (int i = tid; i < kChunks; i += 128) {
        const long n0 = s0 + 8L * i;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (n0 >= 0 && n0 < nsamp) {
            v = *reinterpret_cast<const uint4*>(row + n0);
            const long left = nsamp - n0;                   // samples of the chunk inside the record
            if (left < 8) {
                uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = 2 * e + 1 < left ? w[e] : (2 * e < left ? (w[e] & 0xffffu) : 0u);
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        const int ph = (8 * i) & (kPoly - 1), col = (8 * i) / kPoly;
        uint32_t* __restrict__ dst = img + (ph >> 1) * kPitch + col + (ph >> 6);
        dst[0] = v.x; dst[kPitch] = v.y; dst[2 * kPitch] = v.z; dst[3 * kPitch] = v.w;
    }
    __syncthreads();
    f2 a[4] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
    if (rail == 0) walk<0>(a, img + lane);
    else walk<1>(a, img + lane);
    // chain e belongs to output 7 - e
    const int m = m0 + kPerLane * lane;
    float r[8] = {a[3].y, a[3].x, a[2].y, a[2].x, a[1].y, a[1].x, a[0].y, a[0].x};
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = m + j < n_out ? r[j] : 0.0f;
    out[0] = make_float4(r[0], r[1], r[2], r[3]);
    out[1] = make_float4(r[4], r[5], r[6], r[7]);
}
}  // namespace

void audio_front_taps(float* gi511, float* gq511) {
    for (int k = -AUDIO_FRONT_K; k <= AUDIO_FRONT_K; ++k) {
        gi511[k + AUDIO_FRONT_K] = audio_front_tap(0, k);
        gq511[k + AUDIO_FRONT_K] = audio_front_tap(1, k);
    }
}

void launch_audio_front(const int16_t* pcm, size_t pcm_stride, int nsamp, int nseg, float* dI, float* dQ, hipStream_t st) {
    if (nseg <= 0) return;
    const int n_out = audio_front_n_out(nsamp);
    // 88 tiles per row on x: 2^31 / 88 rows per launch is beyond any memory
    hipLaunchKernelGGL(audio_front_kernel, dim3((unsigned)nseg * kTilesPerRow), dim3(128), 0, st, pcm, pcm_stride, nsamp,
                       n_out, dI, dQ);
}

}  // namespace wspr
