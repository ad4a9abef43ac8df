// K16: the band noise figures of a segment (wspr_noise_batch_device(), wspr_noise(); the definition in noise.h,
// tests/helpers/noise_check.c its serial form).  Two figures per row: the mean and the trough of the power in two gaps
// before and after the transmissions, and the mean of the quietest 30 % of the averaged spectrum of the +-162 Hz band.
//   noise_kernel  one workgroup of 256 threads (four waves) per segment, 44 rounds of 1 024 samples for a full row.
//                 Every sample is read from HBM once: a thread loads one aligned 16-byte vector of each rail per round
//                 (the row's last, partial vector element by element: nothing behind np is touched), a round ahead of
//                 its use, tests the exponent bits and puts it into a ring of 2 048 samples per rail in LDS.  The ring
//                 serves the 50 % overlap of the frames: round r transforms the frames 4r-1 .. 4r+2, one per wave.
//                 A lane holds eight points of its wave's frame in registers and runs three of the nine stages on them
//                 (twelve butterflies, noise.h's statements on values); between the three passes the points change
//                 lanes through the wave's own 4.5 KB of LDS, in two padded layouts that keep the 8-byte accesses off
//                 each other's banks: points l + 64e (stages 0-2), (l & 7) + 64 (l >> 3) + 8e (stages 3-5), 8l + e
//                 (stages 6-8); that choreography is noise_fft.h, shared with K20.  The windowed points come straight from the ring, the window in registers; the last
//                 pass leaves output slot 8l + e in lane l, which keeps that slot's double sum in a register across all
//                 rounds; wave w so forms the partial sum S_c of noise.h for c = (w + 3) % 4, in rising frame order.
//                 Wave 0 forms the block powers of the round's 64 blocks that lie in a window from the same ring (one
//                 lane per block: the sum is serial), 16-byte LDS reads.  At the end the partial sums are joined in the
//                 fixed order, the 443 bins rank themselves by counting (443 broadcast reads each, no data-dependent
//                 loop), three lanes finish the three figures and one writes the 32-byte record with two 16-byte vector
//                 stores.
// No atomics, no inline assembly, every segment independent: deterministic.  LDS 47.7 KB: three workgroups per CU.
#include <hip/hip_runtime.h>

#include "noise.h"
#include "noise_fft.h"
#include "wspr_device.h"

namespace wspr {

static_assert(noise::kMaxSamples == kMaxSamples, "noise.h and wspr_device.h disagree");
static_assert(sizeof(noise::Result) == 32 && sizeof(noise::Windows) == 16, "the record is 32 bytes");

namespace {
constexpr int kThreads = 256;
constexpr int kRound = 1024;                               // samples per round = 4 hops = 64 blocks
constexpr int kRing = 2048;                                // samples of each rail the ring holds
constexpr int kBlocksPerRound = kRound / noise::kBlockLen;
static_assert(kRound == 4 * kThreads && kRound == noise::kClasses * noise::kFrameHop && kBlocksPerRound == 64, "one vector per thread, one frame per wave, one block per lane of wave 0");
static_assert(kRing >= kRound + noise::kFft + noise::kFrameHop && (kRing & (kRing - 1)) == 0, "the ring holds the round, the frame that began before it, and what the next round writes");
static_assert(2 * kRing * 4 == noise::kClasses * noise::kFft * 8, "the partial sums take the ring's place");
using noise_fft::kExch;                                    // the transform, its exchange layouts and the row loads: noise_fft.h
using noise_fft::load_vec;
using noise_fft::vec_non_finite;
static_assert(noise::kClasses * kExch * 8 >= 2 * noise::kFft * 4, "the band and the band in rank order fit into the four areas");

__global__ __launch_bounds__(kThreads)
void noise_kernel(const float* __restrict__ dI, const float* __restrict__ dQ, int np, size_t stride,
                  const float* __restrict__ table, double w2, noise::Windows win, uint4* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float ring[2 * kRing];                       // later: the four partial sums
    __shared__ __attribute__((aligned(16))) float2 exch[noise::kClasses * kExch];       // later: the band, and the band in rank order
    __shared__ float pw[noise::kBlocks];
    __shared__ __attribute__((aligned(16))) float tab[2 * noise::kTwiddles];       // the twiddles; the window lives in registers
    __shared__ uint32_t res[8];
    float* const ringI = ring;
    float* const ringQ = ring + kRing;
    const int seg = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* __restrict__ rowI = dI + (size_t)seg * stride;
    const float* __restrict__ rowQ = dQ + (size_t)seg * stride;
    const int nframes = noise::frames_of(np), nblk = noise::whole_blocks(np);
    const int pre0 = win.pre_b0, pre1 = win.pre_b1 < nblk ? win.pre_b1 : nblk;
    const int post0 = win.post_b0, post1 = win.post_b1 < nblk ? win.post_b1 : nblk;
    const int rounds = (np + kRound - 1) / kRound;
    float2* const mine = exch + wave * kExch;
    const float2* const tw = reinterpret_cast<const float2*>(tab);        // tw[m] = exp(-2 pi i m / 512)
    const int lo = lane & 7, hi = lane >> 3;

    for (int i = tid; i < 2 * noise::kTwiddles; i += kThreads) tab[i] = table[i];
    float hann[8];                                                        // the window at the points l + 64e
    double acc[8];                                                        // the sums of the output slots 8l + e
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        hann[e] = table[2 * noise::kTwiddles + lane + 64 * e];
        acc[e] = 0.0;
    }
    const noise_fft::LastTwiddles last = noise_fft::last_twiddles(table);
    unsigned bad = 0;
    float4 nxtI = load_vec(rowI, 4 * tid, np), nxtQ = load_vec(rowQ, 4 * tid, np);

    for (int r = 0; r < rounds; ++r) {
        // (the slots written held samples that this round and the later ones no longer need; the reads of round r - 1 lie
        // before its barriers)
        const int slot = (r * kRound + 4 * tid) & (kRing - 1);
        *reinterpret_cast<float4*>(ringI + slot) = nxtI;
        *reinterpret_cast<float4*>(ringQ + slot) = nxtQ;
        bad |= vec_non_finite(nxtI) | vec_non_finite(nxtQ);
        if (r + 1 < rounds) {
            nxtI = load_vec(rowI, (r + 1) * kRound + 4 * tid, np);
            nxtQ = load_vec(rowQ, (r + 1) * kRound + 4 * tid, np);
        }
        __syncthreads();
        const int f = 4 * r - 1 + wave;                                   // the frame that ends in this round's quarter `wave`
        const bool active = f >= 0 && f < nframes;
        float2 x[8];
        if (active) {                                                     // stages 0-2 on the points l + 64e
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int s = (f * noise::kFrameHop + lane + 64 * e) & (kRing - 1);
                x[e] = make_float2(ringI[s] * hann[e], ringQ[s] * hann[e]);
            }
            noise_fft::pass_a(x, tw, lane);
            noise_fft::store_a(mine, x, lane);
        }
        if (wave == 0) {
            const int b = r * kBlocksPerRound + lane;
            if (b < nblk && ((b >= pre0 && b < pre1) || (b >= post0 && b < post1))) {
                const int s = (b * noise::kBlockLen) & (kRing - 1);
                float xi[noise::kBlockLen], xq[noise::kBlockLen];
#pragma unroll
                for (int k = 0; k < noise::kBlockLen / 4; ++k) {
                    const float4 vi = *reinterpret_cast<const float4*>(ringI + s + 4 * k);
                    const float4 vq = *reinterpret_cast<const float4*>(ringQ + s + 4 * k);
                    xi[4 * k] = vi.x; xi[4 * k + 1] = vi.y; xi[4 * k + 2] = vi.z; xi[4 * k + 3] = vi.w;
                    xq[4 * k] = vq.x; xq[4 * k + 1] = vq.y; xq[4 * k + 2] = vq.z; xq[4 * k + 3] = vq.w;
                }
                pw[b] = noise::block_power(xi, xq);
            }
        }
        __syncthreads();
        if (active) {                                                     // stages 3-5 on the points lo + 64 hi + 8e
            noise_fft::load_b(x, mine, lo, hi);
            noise_fft::pass_b(x, tw, lo);
        }
        __syncthreads();                                                  // every lane has read what it needs of the first layout
        if (active) {
            noise_fft::store_b(mine, x, lo, hi);
        }
        __syncthreads();
        if (active) {                                                     // stages 6-8 on the points 8l + e: the output slots
            noise_fft::load_c(x, mine, lane);
            noise_fft::pass_c(x, last);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (double)noise::slot_power(x[e].x, x[e].y);
        }
    }
    __syncthreads();
    double* const part = reinterpret_cast<double*>(ring);                 // [class][slot]
    const int cls = (wave + 3) & 3;                                       // f = 4r - 1 + wave
#pragma unroll
    for (int e = 0; e < 8; ++e) part[cls * noise::kFft + 8 * lane + e] = acc[e];
    const int any_bad = __syncthreads_or((int)bad);
    uint32_t* const band = reinterpret_cast<uint32_t*>(exch);
    uint32_t* const ranked = band + noise::kFft;
    for (int p = tid; p < noise::kFft; p += kThreads) {
        const int j = noise::bin_of_slot(p);
        if (j >= -noise::kBandHalf && j <= noise::kBandHalf) {
            const double a = noise::join_classes(part[p], part[noise::kFft + p], part[2 * noise::kFft + p], part[3 * noise::kFft + p]);
            band[j + noise::kBandHalf] = nframes > 0 ? f32_bits(noise::bin_level(a, nframes, w2)) : 0u;
        }
    }
    __syncthreads();
    for (int i = tid; i < noise::kBand; i += kThreads) ranked[noise::band_rank(band, i)] = band[i];
    __syncthreads();
    if (tid == 0) {
        res[4] = f32_bits(noise::band_floor(ranked));
        res[5] = ranked[noise::kLowest];
    }
    if (tid == 64 || tid == 128) {
        float mean, trough;
        const bool post = tid == 128;
        const bool used = noise::window_figures(pw, post ? post0 : pre0, post ? post1 : pre1, &mean, &trough);
        res[post ? 2 : 0] = f32_bits(mean);
        res[post ? 3 : 1] = f32_bits(trough);
        res[post ? 7 : 6] = used ? 1u : 0u;
    }
    __syncthreads();
    if (tid == 0) {
        uint4 first = make_uint4(res[0], res[1], res[2], res[3]);
        uint4 second = make_uint4(res[4], res[5], (uint32_t)nframes,
                              (res[6] ? noise::kPreUsed : 0) | (res[7] ? noise::kPostUsed : 0) | (nframes > 0 ? noise::kSpectrumUsed : 0));
        if (any_bad) {
            first = make_uint4(0u, 0u, 0u, 0u);
            second = make_uint4(0u, 0u, (uint32_t)nframes, (uint32_t)noise::kNonFinite);
        }
        out[2 * (size_t)seg] = first;
        out[2 * (size_t)seg + 1] = second;
    }
}
}  // namespace

void launch_noise(const float* dI, const float* dQ, int samples, size_t stride, int nseg, const float* table, double w2,
                  const noise::Windows& win, void* out, hipStream_t st) {
    if (nseg <= 0) return;
    hipLaunchKernelGGL(noise_kernel, dim3(nseg), dim3(kThreads), 0, st, dI, dQ, samples, stride, table, w2, win,
                       static_cast<uint4*>(out));
}

}  // namespace wspr
