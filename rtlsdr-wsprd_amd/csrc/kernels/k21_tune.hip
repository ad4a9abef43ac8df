// K21 -- tunable multi-band front end: one pass over a 2.4 Msps unsigned-8-bit capture, up to 16 bands out, each a
// 375.000 Hz float32 IQ row the decoder takes as it stands.  The definition is tune.h (serial C: tests/helpers/tune_check.c).
// Everything up to the block sums is integer arithmetic, so the order of the sums is free; the float tail has one order.
//
//   pass A (the hot one): block sums.  sums[seg][band][block] = {S_re, S_im, W_re, W_im} (int64) of the block's 800 mixed
//     vectors.  A WAVE owns a block (800 vectors of 16 bytes: twelve rounds of 64 without a bounds test and one of 32), as
//     K0's whole-segment kernel does; a workgroup is four consecutive blocks.  A block therefore reduces wave-wide and needs
//     no step across waves: LDS holds the two 256-entry rotor tables only.  Loads are aligned 16-byte non-temporal ones, four
//     in flight per lane; every loaded vector is unpacked once (bytes to unsigned 16-bit pairs) and used for every band of
//     the tile before the next is touched.  Per band and vector: sixteen packed 16-bit dot products for z (H_k and the -128
//     bias are wave-uniform kernel arguments, i.e. scalar registers), two table reads and two dot products for the vector's
//     rotor, four 32 x 32 -> 64-bit multiply-adds for y, two more for W.
//     BAND TILE: 4, by registers.  Per band a lane keeps S (2 x int32: 13 vectors of |y| < 2^27) and W (2 x int64) = 6
//     registers, its H_k in 19 scalar registers, next to 16 registers of loads in flight and 8 of unpacked samples; the
//     compiler's counts are 80 / 109 / 143 / 93 VGPRs for 1 / 2 / 3 / 4 bands, no scratch: four bands still leave a SIMD
//     five waves, and eight would not fit the scalar registers.  More bands than 4: one more launch per four bands, each a
//     pass over the rows.  Measured: memory-bound with one band only.
//   pass B: combs + scale + FIR per (segment, band) row from the block sums, K0's cic_comb_fir_kernel in int64:
//     d_b = 800 (S_{b-1} + 2 S_{b-2} + S_{b-3}) + W_b + W_{b-1} - W_{b-2} - W_{b-3}; the two running sums of the definition
//     never have to be formed (tune.h).  The whole row is written: zeros from n_out on.
// Plain vector stores only.  Rows: 16-byte aligned, bytes_per_seg a multiple of 16; a block that counts lies inside the row.
#include "wspr_device.h"
#include "tune.h"

#pragma clang fp contract(off)

namespace wspr {
namespace {

constexpr int kTuneTile = 4;                                   // bands per pass over the row
constexpr int kWavesPerGroup = 4;                              // blocks per workgroup

struct TuneTile { tune_band b[kTuneTile]; };
struct TuneTaps { float t[33]; };

typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef short s2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int dot2(unsigned a, unsigned b, int c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s2, a), __builtin_bit_cast(s2, b), c, false);
}
__device__ __forceinline__ long long wave_sum64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int NT>
__global__ __launch_bounds__(64 * kWavesPerGroup)
void tune_block_sums_kernel(const uint8_t* __restrict__ raw, size_t bytes_per_seg, int nblk, int nbands, int band0,
                            const TuneTile tile, long long* __restrict__ sums) {
    __shared__ unsigned ldsC[256];                             // (cr, ci) as two int16
    __shared__ uint2 ldsF[256];                                // (fr, -fi) and (fi, fr)
    {
        const int k = threadIdx.x;                             // 256 threads, 256 entries
        const int cr = kTuneC256[2 * k], ci = kTuneC256[2 * k + 1], fr = kTuneF256[2 * k], fi = kTuneF256[2 * k + 1];
        ldsC[k] = ((unsigned)cr & 0xffffu) | ((unsigned)ci << 16);
        ldsF[k] = make_uint2(((unsigned)fr & 0xffffu) | ((unsigned)(-fi) << 16), ((unsigned)fi & 0xffffu) | ((unsigned)fr << 16));
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int seg = blockIdx.y;
    const int blk = blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6);
    if (blk >= nblk) return;                                   // wave-uniform, behind the only barrier
    const u4* __restrict__ vec = reinterpret_cast<const u4*>(raw + (size_t)seg * bytes_per_seg) + (size_t)blk * TUNE_R;
    const unsigned v0 = (unsigned)blk * (unsigned)TUNE_R;      // the block's first vector in the row

    int sre[NT], sim[NT];
    long long wre[NT], wim[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { sre[t] = sim[t] = 0; wre[t] = wim[t] = 0; }

    // one vector, r = its place in the block
    auto vector = [&](const u4 q, const int r) {
        const unsigned d[4] = {q.x, q.y, q.z, q.w};
        unsigned p[8];                                         // sample k as (u_I, u_Q) in two 16-bit halves
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p[2 * j] = (d[j] & 0xffu) | ((d[j] & 0xff00u) << 8);
            p[2 * j + 1] = ((d[j] >> 16) & 0xffu) | ((d[j] >> 8) & 0xff0000u);
        }
        const unsigned n8 = 8u * (v0 + (unsigned)r);           // 8 v mod 2^32
        const int wgt = TUNE_R - r;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const tune_band& b = tile.b[t];
            tune_c32 z = {b.bias_re, b.bias_im};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                z.re = dot2(p[k], b.h_re[k], z.re);
                z.im = dot2(p[k], b.h_im[k], z.im);
            }
            const unsigned P = n8 * b.step;
            const unsigned c = ldsC[tune_hi(P)];
            const uint2 f = ldsF[tune_lo(P)];
            tune_c32 rot;
            rot.re = (dot2(c, f.x, 0) + 8192) >> 14;
            rot.im = (dot2(c, f.y, 0) + 8192) >> 14;
            const tune_c32 y = tune_mix(z, rot);
            sre[t] += y.re;
            sim[t] += y.im;
            wre[t] += (long long)wgt * y.re;
            wim[t] += (long long)wgt * y.im;
        }
    };

    const u4* __restrict__ p0 = vec + lane;
#pragma unroll 1
    for (int g = 0; g < 12; g += 4) {                          // 768 vectors, no bounds test
        u4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = __builtin_nontemporal_load(p0 + 64 * (g + u));
#pragma unroll
        for (int u = 0; u < 4; ++u) vector(q[u], 64 * (g + u) + lane);
    }
    if (lane < TUNE_R - 768) vector(__builtin_nontemporal_load(p0 + 768), 768 + lane);   // the last 32

    long long* __restrict__ out = sums + (((size_t)seg * nbands + band0) * (size_t)nblk + blk) * 4;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const long long a = wave_sum64(sre[t]), b = wave_sum64(sim[t]), c = wave_sum64(wre[t]), e = wave_sum64(wim[t]);
        if (lane == 0) {
            long long* o = out + (size_t)t * nblk * 4;
            o[0] = a; o[1] = b; o[2] = c; o[3] = e;
        }
    }
}

// One workgroup: 256 outputs of one (segment, band) row.  Row s * nbands + b of dI / dQ.
__global__ __launch_bounds__(256)
void tune_comb_fir_kernel(const long long* __restrict__ sums, int nblk, const TuneTaps taps, float* __restrict__ dI,
                          float* __restrict__ dQ, int* __restrict__ n_out) {
    __shared__ long long sb[256 + 32 + 3][4];                  // block sums of blocks m0-35 .. m0+255
    __shared__ float x[2][256 + 32];                           // x_b of blocks m0-32 .. m0+255
    const int row = blockIdx.y, tid = threadIdx.x, m0 = blockIdx.x * 256;
    if (blockIdx.x == 0 && tid == 0 && n_out) n_out[row] = nblk;
    const long long* __restrict__ s = sums + (size_t)row * nblk * 4;
    for (int e = tid; e < (256 + 35) * 4; e += 256) {
        const int b = m0 - 35 + (e >> 2);
        sb[e >> 2][e & 3] = (b >= 0 && b < nblk) ? s[(size_t)b * 4 + (e & 3)] : 0;
    }
    __syncthreads();
    for (int e = tid; e < 256 + 32; e += 256) {                // d of block m0 - 32 + e = sums index e + 3
        const bool live = (m0 - 32 + e) >= 0;                  // before the start the history holds 0.0f
#pragma unroll
        for (int rail = 0; rail < 2; ++rail) {
            const long long d = (long long)TUNE_R * (sb[e + 2][rail] + 2 * sb[e + 1][rail] + sb[e][rail]) +
                                sb[e + 3][2 + rail] + sb[e + 2][2 + rail] - sb[e + 1][2 + rail] - sb[e][2 + rail];
            x[rail][e] = live ? tune_to_float(d) : 0.0f;
        }
    }
    __syncthreads();
    const int m = m0 + tid;
    if (m >= kIqStride) return;
#pragma unroll
    for (int rail = 0; rail < 2; ++rail) {
        float acc = 0.0f;
        for (int j = 0; j < 33; ++j) {
            const float p = x[rail][tid + j] * taps.t[j];
            acc += p;
        }
        (rail == 0 ? dI : dQ)[(size_t)row * kIqStride + m] = (m < nblk) ? acc : 0.0f;
    }
}

// rows without a whole block: zeros
__global__ __launch_bounds__(256)
void tune_zero_rows_kernel(float* __restrict__ dI, float* __restrict__ dQ, size_t n, int* __restrict__ n_out, int nrows) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { dI[i] = 0.0f; dQ[i] = 0.0f; }
    if (i < (size_t)nrows && n_out) n_out[i] = 0;
}

}  // namespace

int tune_band_tile() { return kTuneTile; }

size_t tune_scratch_bytes(size_t bytes_per_seg, int nseg, int nbands) {
    return (size_t)nseg * nbands * (size_t)tune_n_out(bytes_per_seg / 2) * 4 * sizeof(long long);
}

void launch_tune(const uint8_t* raw, size_t bytes_per_seg, int nseg, const uint32_t* steps, int nbands, float* dI, float* dQ,
                 int* n_out, long long* scratch, hipStream_t st) {
    if (nseg <= 0 || nbands <= 0) return;
    const int nrows = nseg * nbands;
    const int nblk = tune_n_out(bytes_per_seg / 2);
    if (nblk == 0) {
        const size_t n = (size_t)nrows * kIqStride;
        hipLaunchKernelGGL(tune_zero_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dI, dQ, n, n_out, nrows);
        return;
    }
    const dim3 grid((nblk + kWavesPerGroup - 1) / kWavesPerGroup, nseg), wg(64 * kWavesPerGroup);
    for (int band0 = 0; band0 < nbands; band0 += kTuneTile) {
        const int nt = nbands - band0 < kTuneTile ? nbands - band0 : kTuneTile;
        TuneTile tile{};
        for (int t = 0; t < nt; ++t) tune_band_setup(steps[band0 + t], &tile.b[t]);
        switch (nt) {
            case 1: hipLaunchKernelGGL(tune_block_sums_kernel<1>, grid, wg, 0, st, raw, bytes_per_seg, nblk, nbands, band0, tile, scratch); break;
            case 2: hipLaunchKernelGGL(tune_block_sums_kernel<2>, grid, wg, 0, st, raw, bytes_per_seg, nblk, nbands, band0, tile, scratch); break;
            case 3: hipLaunchKernelGGL(tune_block_sums_kernel<3>, grid, wg, 0, st, raw, bytes_per_seg, nblk, nbands, band0, tile, scratch); break;
            default: hipLaunchKernelGGL(tune_block_sums_kernel<4>, grid, wg, 0, st, raw, bytes_per_seg, nblk, nbands, band0, tile, scratch); break;
        }
    }
    TuneTaps taps;
    int r = 0;
    front_end_constants(taps.t, &r);
    hipLaunchKernelGGL(tune_comb_fir_kernel, dim3((kIqStride + 255) / 256, nrows), dim3(256), 0, st, scratch, nblk, taps, dI, dQ, n_out);
}

}  // namespace wspr
