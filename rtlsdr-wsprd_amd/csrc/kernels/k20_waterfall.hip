// K20: the waterfall of a segment (wspr_waterfall_batch_device(), wspr_waterfall(); the definition in waterfall.h over
// noise.h, tests/helpers/waterfall_check.c its serial form): K16's frame powers kept frame by frame, tavg of them summed
// into an image row, every power turned into a byte by a table of thresholds.
//   waterfall_kernel  grid (tiles of image rows) x segments, 256 threads (four waves).  A tile is R = max(1, 16 / tavg)
//                 image rows, at most 16 frames.  The workgroup stages the tile's samples once into LDS with aligned
//                 16-byte loads, (R tavg - 1) hop + 512 of each rail: the first lies at a multiple of hop and the last
//                 belongs to a complete frame, so nothing at or behind `samples` is read.  Wave w takes the image rows
//                 w, w + 4, ... of the tile: for each it transforms the row's tavg frames in rising f with the in-register
//                 scheme of noise_fft.h, keeps the eight double sums of the output slots 8l + e in registers, runs the
//                 exponent test on what it reads, turns each sum into a level (eight steps through the 255 thresholds in
//                 LDS) and puts the byte of column bin_of_slot() - j0 into an LDS tile [R][ncols].  A tile is ONE
//                 contiguous byte range of the image, [r0 ncols, (r0 + R) ncols), and the image base is 16-byte aligned:
//                 the LDS tile starts at the range's own offset mod 16, the head and the tail of the range are stored
//                 byte by byte and the middle with 16-byte vector stores.
//                 The info record is zeroed before the launch; tile 0 writes ref, nframes and nrows, and every flag bit is
//                 an integer atomicOr, so order cannot matter.  In floor mode the reference is read from K16's record of
//                 the same row, which the same stream wrote before.
// No other atomics, no inline assembly: deterministic.  LDS 63.8 KB (34 KB of samples, 17.8 KB of exchange, 8 KB of tile,
// 2 KB of thresholds, 2 KB of twiddles): two workgroups per CU.
#include <hip/hip_runtime.h>

#include "noise_fft.h"
#include "waterfall.h"
#include "wspr_device.h"

namespace wspr {

static_assert(sizeof(waterfall::Params) == 32 && sizeof(waterfall::Info) == 16, "the public records");

namespace {
constexpr int kThreads = 256, kWaves = 4;
constexpr int kTileFrames = 16;                                            // frames a tile holds at most
constexpr int kTileSamples = (kTileFrames - 1) * 256 + noise::kFft;        // ... and samples of each rail
constexpr int kTileBytes = kTileFrames * noise::kFft;                      // R * ncols at most
static_assert(kTileFrames >= waterfall::kMaxAvg && kTileSamples % 4 == 0, "a tile holds one image row at least");
using noise_fft::kExch;

__host__ __device__ constexpr int rows_per_tile(int tavg) { return kTileFrames / tavg > 1 ? kTileFrames / tavg : 1; }

__global__ __launch_bounds__(kThreads)
void waterfall_kernel(const float* __restrict__ dI, const float* __restrict__ dQ, int np, size_t stride,
                      const float* __restrict__ table, double w2, waterfall::Params p, const double* __restrict__ levels,
                      const noise::Result* __restrict__ floors, uint8_t* __restrict__ img, size_t img_stride,
                      waterfall::Info* __restrict__ info) {
    __shared__ __attribute__((aligned(16))) float smp[2 * kTileSamples];
    __shared__ __attribute__((aligned(16))) float2 exch[kWaves * kExch];
    __shared__ __attribute__((aligned(16))) double thr[waterfall::kLevels];
    __shared__ __attribute__((aligned(16))) float tab[2 * noise::kTwiddles];
    __shared__ __attribute__((aligned(16))) uint8_t tile[kTileBytes + 16];
    float* const smpI = smp;
    float* const smpQ = smp + kTileSamples;
    const int seg = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int hop = p.hop, tavg = p.tavg, ncols = waterfall::cols_of(p.j0, p.j1);
    const int nframes = waterfall::frames_of(np, hop), nrows = nframes / tavg;
    const int R = rows_per_tile(tavg);
    const int r0 = (int)blockIdx.x * R;
    const int rows = nrows - r0 < R ? nrows - r0 : R;                      // image rows of this tile

    float ref = p.ref;
    bool has_ref = true;
    int ref_flags = 0;
    if (p.ref_mode == waterfall::kRefFloor) {
        const noise::Result rec = floors[seg];
        has_ref = waterfall::floor_ref(rec.fft_p30, rec.flags, &ref);
        if (!has_ref) ref_flags = waterfall::kNoRef | (rec.flags & noise::kNonFinite ? waterfall::kNonFinite : 0);
    }
    int* const flags = &info[seg].flags;
    if (blockIdx.x == 0 && tid == 0) {
        info[seg].ref = ref;
        info[seg].nframes = nframes;
        info[seg].nrows = nrows;
        const int f = (nrows > 0 ? waterfall::kWritten : 0) | ref_flags;
        if (f) atomicOr(flags, f);
    }
    if (rows <= 0) return;

    const int total = rows * ncols;                                       // bytes of the tile
    const int g0 = r0 * ncols;                                            // ... and where they lie in the image
    const int off = g0 & 15;
    uint8_t* const mytile = tile + off;                                   // the same offset mod 16 as in the image

    if (has_ref) {
        for (int i = tid; i < 2 * noise::kTwiddles; i += kThreads) tab[i] = table[i];
        for (int i = tid; i < waterfall::kLevels; i += kThreads) thr[i] = levels[i];
        const float* __restrict__ rowI = dI + (size_t)seg * stride;
        const float* __restrict__ rowQ = dQ + (size_t)seg * stride;
        const int s0 = hop * (r0 * tavg);
        const int ns = (rows * tavg - 1) * hop + noise::kFft;             // <= kTileSamples, a multiple of 4, s0 + ns <= np
        for (int v = 4 * tid; v < ns; v += 4 * kThreads) {
            *reinterpret_cast<float4*>(smpI + v) = noise_fft::load_vec(rowI, s0 + v, np);
            *reinterpret_cast<float4*>(smpQ + v) = noise_fft::load_vec(rowQ, s0 + v, np);
        }
    } else {
        for (int i = tid; i < total; i += kThreads) mytile[i] = 0;
    }
    __syncthreads();

    if (has_ref) {
        float2* const mine = exch + wave * kExch;
        const float2* const tw = reinterpret_cast<const float2*>(tab);    // tw[m] = exp(-2 pi i m / 512)
        const int lo = lane & 7, hi = lane >> 3;
        float hann[8];                                                    // the window at the points l + 64e
#pragma unroll
        for (int e = 0; e < 8; ++e) hann[e] = table[2 * noise::kTwiddles + lane + 64 * e];
        const noise_fft::LastTwiddles last = noise_fft::last_twiddles(table);
        const int rounds = (rows + kWaves - 1) / kWaves;
        for (int q = 0; q < rounds; ++q) {
            const int rr = kWaves * q + wave;                             // this wave's image row of the tile
            const bool active = rr < rows;
            double acc[8];                                                // the sums of the output slots 8l + e
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.0;
            unsigned bad = 0;
            for (int k = 0; k < tavg; ++k) {
                float2 x[8];
                if (active) {                                             // stages 0-2 on the points l + 64e
                    const int base = (rr * tavg + k) * hop + lane;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float vi = smpI[base + 64 * e], vq = smpQ[base + 64 * e];
                        bad |= (noise::non_finite(vi) || noise::non_finite(vq)) ? 1u : 0u;
                        x[e] = make_float2(vi * hann[e], vq * hann[e]);
                    }
                    noise_fft::pass_a(x, tw, lane);
                    noise_fft::store_a(mine, x, lane);
                }
                __syncthreads();
                if (active) {                                             // stages 3-5 on the points lo + 64 hi + 8e
                    noise_fft::load_b(x, mine, lo, hi);
                    noise_fft::pass_b(x, tw, lo);
                }
                __syncthreads();                                          // every lane has read what it needs of the first layout
                if (active) noise_fft::store_b(mine, x, lo, hi);
                __syncthreads();
                if (active) {                                             // stages 6-8 on the points 8l + e: the output slots
                    noise_fft::load_c(x, mine, lane);
                    noise_fft::pass_c(x, last);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += (double)noise::slot_power(x[e].x, x[e].y);
                }
                __syncthreads();                                          // ... and of the second, before the next frame
            }
            if (active) {
                const bool white = __any((int)bad) != 0;                  // the row guard: the wave has read every sample of the row
                if (white && lane == 0) atomicOr(flags, waterfall::kNonFinite);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int c = noise::bin_of_slot(8 * lane + e) - p.j0;
                    if (c >= 0 && c < ncols) {
                        const float m = waterfall::pixel_power(acc[e], tavg, w2);
                        const int level = waterfall::level_of(waterfall::level_ratio(m, ref), thr);
                        mytile[rr * ncols + c] = (uint8_t)(white ? 255 : level);
                    }
                }
            }
        }
        __syncthreads();
    }

    uint8_t* const dst = img + (size_t)seg * img_stride + (size_t)g0;     // dst and mytile: the same address mod 16
    const int head = ((16 - off) & 15) < total ? ((16 - off) & 15) : total;
    const int nvec = (total - head) >> 4;
    const int tail0 = head + 16 * nvec;
    if (tid < head) dst[tid] = mytile[tid];
    for (int v = tid; v < nvec; v += kThreads)
        *reinterpret_cast<uint4*>(dst + head + 16 * v) = *reinterpret_cast<const uint4*>(mytile + head + 16 * v);
    if (tid < total - tail0) dst[tail0 + tid] = mytile[tail0 + tid];
}
}  // namespace

// info: nseg zeroed records on the device; floors: K16's records of the same rows (floor mode) or null
void launch_waterfall(const float* dI, const float* dQ, int samples, size_t stride, int nseg, const float* table, double w2,
                      const waterfall::Params& p, const double* levels, const noise::Result* floors, uint8_t* img,
                      size_t img_stride, waterfall::Info* info, hipStream_t st) {
    const int nrows = waterfall::rows_of(samples, p.hop, p.tavg), R = rows_per_tile(p.tavg);
    const int tiles = nrows > 0 ? (nrows + R - 1) / R : 1;               // (no image row: tile 0 still writes the info record)
    for (int s0 = 0; s0 < nseg; s0 += 65535) {
        const int n = nseg - s0 < 65535 ? nseg - s0 : 65535;
        hipLaunchKernelGGL(waterfall_kernel, dim3(tiles, n), dim3(kThreads), 0, st, dI + (size_t)s0 * stride,
                           dQ + (size_t)s0 * stride, samples, stride, table, w2, p, levels, floors ? floors + s0 : nullptr,
                           img + (size_t)s0 * img_stride, img_stride, info + s0);
    }
}

}  // namespace wspr
