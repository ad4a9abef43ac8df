// K10 -- noncoherent block detection: the soft-symbol vectors of block sizes 1, 2 and 3 of one hypothesis.
//
// The definition is in blockdemod.h (there is no reference code for this stage; tests/helpers/block_check.c is the serial
// statement the kernel is held to, byte for byte, in both arithmetic modes).
//
// Mapping: one workgroup per hypothesis (segment, freq, shift, drift), in three phases that never leave the CU.
//   tone sums   lane = symbol (162 of 192 lanes), exactly demod_kernel's loop (k4_demod.hip): the four tone phasors as
//               float recurrences, the 256-sample matched-filter sums serially in the reference's order, samples through
//               a [162][32 + 1] LDS tile.  The sums are KEPT as (is, qs) and the recurrence takes one more step for the
//               phase advance (cf, sf); both go to LDS, 64 B per symbol, with the mode-2 amplitudes beside them.
//   combine     lane = block, for B = 1, 2, 3 in turn (162, 81, 54 lanes): 2^B sequences of B complex multiply-adds
//               (blockdemod::combine), the soft values to LDS.
//   fold        lanes 0..2 take the normalisation sums of B = 1..3 in symbol order (SoftNorm, as demod_metric_kernel),
//               lane 64 -- another wave -- folds the mode-2 sync metric; then lane = symbol quantises, the bytes leave
//               with vector stores and lanes 0..2 sum the squares for the rms (small integers: exact in any order).
// Nothing but the 3 x 162 bytes, three rms values and the sync leaves the workgroup: the complex sums (223 KB per
// candidate over a 43-rung ladder) never reach HBM.
// Bound: fp32 VALU in the tone sums (16 mul/add pairs per sample and lane, the same 1.33 MFLOP per hypothesis as mode 2);
// the combine adds 162 x (1 + 2 + 8/3 ...) < 3 % to it.  No MFMA (separately rounded chains), no atomics, no inline assembly.
#include "wspr_device.h"
#include "arith.h"
#include "glibc_sincosf.h"
#include "demod_math.h"
#include "blockdemod.h"

#pragma clang fp contract(off)

namespace wspr {
namespace {

using blockdemod::ToneSum;

constexpr int kBlkThreads = 192;
constexpr int kBlkChunk = 32;
constexpr int kBlkPerThread = kNSymD * kBlkChunk / kBlkThreads;     // 27 samples staged per thread and chunk
static_assert(kNSymD * kBlkChunk % kBlkThreads == 0, "chunk must split evenly over the workgroup");
static_assert(kNSymD % 2 == 0 && kNSymD % 3 == 0, "blocks of 2 and 3 tile the frame");

// soft values of the blocks of size B, lane = block
template <int B, bool kFma>
__device__ __forceinline__ void combine_blocks(const ToneSum (*ts)[4], const unsigned char* __restrict__ pr3,
                                               float* __restrict__ fs) {
    const int blk = threadIdx.x;
    if (blk >= kNSymD / B) return;
    const int i0 = blk * B;
    float p[1 << B];
    blockdemod::combine<B, kFma>([&](int ib, int b) { return ts[i0 + ib][pr3[i0 + ib] + 2 * b]; }, p);
#pragma unroll
    for (int ib = 0; ib < B; ++ib) fs[i0 + ib] = blockdemod::soft_value<B>(p, ib);
}

template <bool kFma>
__global__ __launch_bounds__(kBlkThreads)
void block_demod_kernel(const float* __restrict__ dI, const float* __restrict__ dQ, int np,
                        const BlockHyp* __restrict__ hyps, int nhyp, const unsigned char* __restrict__ pr3,
                        unsigned char* __restrict__ sym_out, float* __restrict__ rms_out, float* __restrict__ sync_out) {
    using A = Arith<kFma>;
    __shared__ float2 tile[kNSymD][kBlkChunk + 1];
    __shared__ ToneSum ts[kNSymD][4];
    __shared__ float pw[kNSymD][4];
    __shared__ float fs[blockdemod::kMaxBlock][kNSymD];
    __shared__ unsigned char qb[blockdemod::kMaxBlock][kNSymD];
    __shared__ float fac[blockdemod::kMaxBlock];
    const int h = blockIdx.x;
    if (h >= nhyp) return;
    const BlockHyp hy = hyps[h];
    const int lag = hy.shift;
    const double f0 = hy.freq;

    // ---- tone sums: demod_kernel's loop, lane = symbol ----------------------------------------------------------------
    const int i = threadIdx.x, tid = threadIdx.x;
    const float* __restrict__ xi = dI + (size_t)hy.seg * kIqStride;
    const float* __restrict__ xq = dQ + (size_t)hy.seg * kIqStride;
    float cd[4], sd[4], c[4], s[4], ai[4], aq[4];
    if (i < kNSymD) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float dphi = tone_dphi(f0, hy.drift, i, t);
            cd[t] = glibc_cosf(dphi);
            sd[t] = glibc_sinf(dphi);
            c[t] = 1.0f; s[t] = 0.0f; ai[t] = 0.0f; aq[t] = 0.0f;
        }
    }
    float2 nxt[kBlkPerThread];
    auto fetch = [&](int ch) {
#pragma unroll
        for (int u = 0; u < kBlkPerThread; ++u) {
            const int e = u * kBlkThreads + tid, row = e >> 5, col = e & (kBlkChunk - 1);
            const long long k = (long long)lag + kSps * row + kBlkChunk * ch + col;
            const bool ok = (k > 0) && (k < np);                         // wsprd.c:199; nothing outside the row is read
            nxt[u] = ok ? make_float2(xi[k], xq[k]) : make_float2(0.0f, 0.0f);
        }
    };
    fetch(0);
    for (int ch = 0; ch < kSps / kBlkChunk; ++ch) {
        __syncthreads();                                             // the previous chunk has been consumed
#pragma unroll
        for (int u = 0; u < kBlkPerThread; ++u) {
            const int e = u * kBlkThreads + tid;
            tile[e >> 5][e & (kBlkChunk - 1)] = nxt[u];
        }
        __syncthreads();
        if (ch + 1 < kSps / kBlkChunk) fetch(ch + 1);
        if (i < kNSymD) {
            const long long base = (long long)lag + kSps * i + kBlkChunk * ch;
#pragma unroll 4
            for (int jj = 0; jj < kBlkChunk; ++jj) {
                const long long k = base + jj;
                if (kBlkChunk * ch + jj > 0) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) phasor_step<kFma>(c[t], s[t], cd[t], sd[t]);
                }
                if (k > 0 && k < np) {
                    const float2 xy = tile[i][jj];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {       // ai = (ai + x*c) + y*s ; aq = (aq - x*s) + y*c (wsprd.c:200-207)
                        ai[t] = A::mad(xy.y, s[t], A::mad(xy.x, c[t], ai[t]));
                        aq[t] = A::mad(xy.y, c[t], A::nmad(xy.x, s[t], aq[t]));
                    }
                }
            }
        }
    }
    if (i < kNSymD) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            pw[i][t] = sqrtf(A::mma(ai[t], ai[t], aq[t], aq[t]));
            phasor_step<kFma>(c[t], s[t], cd[t], sd[t]);             // one step past the table's last entry: the advance
            ts[i][t] = ToneSum{ai[t], aq[t], c[t], s[t]};
        }
    }
    __syncthreads();

    // ---- combine: lane = block ----------------------------------------------------------------------------------------
    combine_blocks<1, kFma>(ts, pr3, fs[0]);
    combine_blocks<2, kFma>(ts, pr3, fs[1]);
    combine_blocks<3, kFma>(ts, pr3, fs[2]);
    __syncthreads();

    // ---- fold in symbol order: the three normalisations, and the hypothesis' mode-2 sync (the gate reads it) ----------
    if (tid < blockdemod::kMaxBlock) {
        SoftNorm norm;
        for (int k = 0; k < kNSymD; ++k) norm.add(fs[tid][k]);
        fac[tid] = norm.fac<kFma>();
    } else if (tid == 64) {
        const float ss = sync_metric([&](int k) { return make_float4(pw[k][0], pw[k][1], pw[k][2], pw[k][3]); }, pr3);
        sync_out[h] = (ss > -1e30f) ? ss : -1e30f;
    }
    __syncthreads();
    if (i < kNSymD) {
#pragma unroll
        for (int b = 0; b < blockdemod::kMaxBlock; ++b) {
            const unsigned char q = soft_quantise(fs[b][i], fac[b], kSymFac);
            qb[b][i] = q;
            sym_out[((size_t)h * blockdemod::kMaxBlock + b) * kNSymD + i] = q;
        }
    }
    __syncthreads();
    if (tid < blockdemod::kMaxBlock) {
        float sq = 0.0f;
        for (int k = 0; k < kNSymD; ++k) sq += soft_square(qb[tid][k]);
        rms_out[(size_t)h * blockdemod::kMaxBlock + tid] = sqrtf(sq / 162.0f);
    }
}

}  // namespace

void launch_block_demod(const float* dI, const float* dQ, int samples, const BlockHyp* hyps, int nhyp,
                        unsigned char* sym_out, float* rms_out, float* sync_out, const DeviceTables& t, hipStream_t st,
                        int arith) {
    if (nhyp <= 0) return;
    auto k = arith ? block_demod_kernel<true> : block_demod_kernel<false>;
    hipLaunchKernelGGL(k, dim3(nhyp), dim3(kBlkThreads), 0, st, dI, dQ, samples, hyps, nhyp, t.sync, sym_out, rms_out,
                       sync_out);
}

}  // namespace wspr
