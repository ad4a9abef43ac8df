// K15, the impulse-noise blanker in front of K12: 16-bit PCM rows -> 16-bit PCM rows with the spikes (and a guard of G
// samples around each) set to zero.  The definition is audio_blank.h; the serial checker tests/helpers/blank_check.c is the
// contract.  Integer arithmetic only: the rows and the counts are the checker's bit for bit.
//
// Shape.  One workgroup of four wavefronts per (record, block of 8192 samples).  Every input byte comes from HBM once, as
// aligned 16-byte loads, and STAYS IN REGISTERS until it is stored: lane t holds the four chunks (8 samples each)
// t, t + 256, t + 512, t + 768 of the block, the lanes 0 .. 15 one chunk of the halo (64 samples on each side) besides.  LDS
// carries one bit per sample and a word per wavefront, nothing else.
//   median  exact, by a 16-step bitwise search for the largest x with count(a < x) <= rank.  x = 32768 is asked first, on
//           its own (a == 32768 only for pcm == -32768); the other 15 steps run on 15-bit values kept two to a word under a
//           guard bit each, word = (a | 0x8000) twice: one 32-bit subtraction of (x, x) leaves the guard bit of a half set
//           iff a >= x, and a population count of the two guard bits adds them up -- three instructions for two samples.
//           A lane's count (<= 32) is summed over the wavefront with six ballots, over the workgroup through one LDS word per
//           wavefront (two sets that take turns: one barrier per step).  Slots outside the record count as 32767: never
//           below any x, so the rank among the block's own samples is untouched.
//   hits    16 a > thr16 L  <=>  a > q = (thr16 L) >> 4.  Each lane writes one byte of hit bits per chunk to LDS, the halo's
//           chunks included (judged by THIS block's level, as the definition says).  In a full block with q < 32767 the
//           bits come from the search image by the same subtraction (min(a, 32767) >= q + 1); the record's last block,
//           the halo and the thresholds that only 32768 or nothing exceeds take the samples themselves.  Zero outside
//           [0, nsamp) comes from the staging guard below, never from a neighbouring row or the padding of the stride.
//   guard   lane t dilates the bits of samples 32 t .. 32 t + 31: the 160 bits around them are smeared upwards by 2 G in
//           at most 8 doubling steps and read G bits higher.  The result goes back through LDS to the lanes that hold the
//           samples, which store 16 bytes per chunk.
//   count   one vector atomic add per workgroup into the record's counter (an integer: the order does not matter).
#include "audio_blank.h"
#include "wspr_device.h"

namespace wspr {
namespace {
constexpr int kBlock = AUDIO_BLANK_BLOCK;
constexpr int kThreads = 256;
constexpr int kChunks = kBlock / 8;                  // 16-byte chunks of a block
constexpr int kPerLane = kChunks / kThreads;         // 4
constexpr int kHalo = AUDIO_BLANK_GUARD_MAX;         // samples staged on each side of the block
constexpr int kHaloChunks = kHalo / 8;               // 8
constexpr int kHitBytes = kChunks + 2 * kHaloChunks; // one byte of hit bits per staged chunk
constexpr uint32_t kGuardBits = 0x80008000u;
static_assert(kPerLane * kThreads == kChunks && kHalo % 8 == 0 && kHitBytes % 4 == 0, "chunks tile the block and the halo");
static_assert(kBlock / 32 == kThreads, "one lane per word of the dilated mask");
static_assert(2 * kHaloChunks <= 64, "the halo is staged by lanes of the first wavefront");

// chunk at sample n0 (a multiple of 8) of a row: zero outside [0, nsamp).  A chunk that starts below nsamp ends inside
// the row, because the stride is a multiple of 8 that is >= nsamp.
// In two halves, so that a lane's loads are all in flight before the first is looked at: a chunk outside the record is
// loaded from sample 0 of the row instead (nsamp >= 1 here, so that chunk exists) and masked away afterwards.
__device__ __forceinline__ uint4 load_chunk(const int16_t* __restrict__ row, long n0, int nsamp) {
    return *reinterpret_cast<const uint4*>(row + (n0 >= 0 && n0 < nsamp ? n0 : 0));
}
__device__ __forceinline__ uint4 guard_chunk(uint4 v, long n0, int nsamp) {
    const int left = n0 >= 0 && n0 < nsamp ? (int)min(8L, nsamp - n0) : 0;     // samples of the chunk inside the record
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = 2 * e + 1 < left ? w[e] : (2 * e < left ? (w[e] & 0xffffu) : 0u);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ int abs16(uint32_t half) { const int x = (int)(short)half; return x < 0 ? -x : x; }

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
typedef short ss2 __attribute__((ext_vector_type(2)));
// |lo| and |hi| of a word of two samples as two unsigned halves: max(x, -x) with the negation wrapping, so -32768 gives 0x8000
__device__ __forceinline__ uint32_t abs_pair(uint32_t w) {
    const us2 u = __builtin_bit_cast(us2, w), n = (us2)(0) - u;
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(ss2, u), __builtin_bit_cast(ss2, n)));
}
// both halves limited to 32767
__device__ __forceinline__ uint32_t clip_pair(uint32_t a) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(us2, a), (us2)(0x7fff)));
}

// the 8 hit bits of a chunk from its search image (word e = samples 2 e, 2 e + 1 under their guard bits): bit i = a'[i] >= x,
// xx = (x, x), 1 <= x <= 32767.  The subtraction leaves a half's guard bit set iff a' >= x; the shifts put the low halves'
// guard bits at bits 0, 2, 4, 6 and the high halves' at 16, 18, 20, 22.
__device__ __forceinline__ uint32_t hit_bits_image(const uint32_t (&img)[4], uint32_t xx) {
    const uint32_t d = (((img[0] - xx) & kGuardBits) >> 15) | (((img[1] - xx) & kGuardBits) >> 13) |
                       (((img[2] - xx) & kGuardBits) >> 11) | (((img[3] - xx) & kGuardBits) >> 9);
    return (d | (d >> 15)) & 0xffu;
}

// the 8 hit bits of a chunk: bit e = a[e] > q
__device__ __forceinline__ uint32_t hit_bits(uint4 v, int q) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t bits = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        bits |= (abs16(w[e] & 0xffffu) > q ? 1u : 0u) << (2 * e);
        bits |= (abs16(w[e] >> 16) > q ? 1u : 0u) << (2 * e + 1);
    }
    return bits;
}

// w |= w << (32 WS + bs) on the 160-bit number w[0] (low) .. w[4], 0 <= bs < 32
template <int WS>
__device__ __forceinline__ void shl_or(uint32_t (&w)[5], int bs) {
#pragma unroll
    for (int k = 4; k >= WS; --k) {                     // falling: w[k - WS] and w[k - WS - 1] are still the old words
        const uint32_t hi = w[k - WS], lo = k - WS - 1 >= 0 ? w[k - WS - 1] : 0u;
        w[k] |= (uint32_t)((((uint64_t)hi << 32) | lo) >> (32 - bs));
    }
}

// bit j of w becomes the OR of the bits j - len .. j (len <= 128, the same in every lane): doubling steps
__device__ __forceinline__ void smear_up(uint32_t (&w)[5], int len) {
    for (int done = 0; done < len;) {
        const int s = min(done + 1, len - done);        // after it the bits j - (done + s) .. j are covered; s <= 64
        switch (s >> 5) {
            case 0: shl_or<0>(w, s & 31); break;
            case 1: shl_or<1>(w, s & 31); break;
            default: shl_or<2>(w, s & 31); break;
        }
        done += s;
    }
}

__global__ __launch_bounds__(kThreads)
void audio_blank_kernel(const int16_t* __restrict__ pcm, size_t pcm_stride, int nsamp, int nblk, int thr16, int guard,
                        int16_t* __restrict__ out, size_t out_stride, int* __restrict__ n_blanked) {
    __shared__ uint32_t hits[kHitBytes / 4];            // bit 8 c + e: sample e of staged chunk c (the halo in front first)
    __shared__ uint32_t mask[kThreads];                 // bit i of word t: block sample 32 t + i is blanked
    __shared__ uint32_t wave_sum[2][kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x % nblk;
    const size_t seg = blockIdx.x / nblk;
    const int16_t* __restrict__ row = pcm + seg * pcm_stride;
    const long base = (long)b * kBlock;                 // the block's first sample
    const int count = min(kBlock, nsamp - (int)base);   // c_b >= 1: the grid holds only blocks that start inside the record

    // ---- staging: the samples into registers, and the search's 15-bit image of them
    uint4 raw[kPerLane];
    uint32_t img[kPerLane][4];
    int n_top = 0;                                      // own samples with a == 32768
    const long halo_n0 = tid < kHaloChunks ? base - kHalo + 8 * tid : base + kBlock + 8 * (tid - kHaloChunks);
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) raw[j] = load_chunk(row, base + 8 * (tid + kThreads * j), nsamp);
    uint4 halo = make_uint4(0u, 0u, 0u, 0u);
    if (tid < 2 * kHaloChunks) halo = guard_chunk(load_chunk(row, halo_n0, nsamp), halo_n0, nsamp);
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const int off = 8 * (tid + kThreads * j);       // the chunk's first sample within the block
        raw[j] = guard_chunk(raw[j], base + off, nsamp);
        const uint32_t w[4] = {raw[j].x, raw[j].y, raw[j].z, raw[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {                   // two samples at a time, packed 16-bit arithmetic
            const uint32_t a = abs_pair(w[e]);
            n_top += __popc(a & kGuardBits);            // a half is 0x8000 only for -32768 (outside the record it is 0)
            img[j][e] = clip_pair(a) | kGuardBits;
        }
        if (off + 8 > count) {                          // the block's last chunks: slots outside the record read 32767
#pragma unroll
            for (int e = 0; e < 4; ++e)
                img[j][e] |= (off + 2 * e >= count ? 0xffffu : 0u) | (off + 2 * e + 1 >= count ? 0xffff0000u : 0u);
        }
    }

    // the sum over the workgroup of a per-lane value < 64; `turn` alternates between consecutive calls
    auto block_sum = [&](uint32_t v, int turn) {
        uint32_t s = 0;
#pragma unroll
        for (int bit = 0; bit < 6; ++bit) s += (uint32_t)__popcll(__ballot((v >> bit) & 1u)) << bit;
        if (lane == 0) wave_sum[turn][wave] = s;
        __syncthreads();
        return wave_sum[turn][0] + wave_sum[turn][1] + wave_sum[turn][2] + wave_sum[turn][3];
    };

    // ---- the lower median: the largest x in 0 .. 32768 with count(a < x) <= rank
    const int rank = audio_blank_rank(count);
    int level = 0;
    if (count - (int)block_sum((uint32_t)n_top, 0) <= rank) {
        level = 32768;                                  // more than half of the block is -32768
    } else {
#pragma unroll 1
        for (int bit = 14; bit >= 0; --bit) {
            const uint32_t x = (uint32_t)(level | (1 << bit)), xx = x | (x << 16);
            uint32_t ge = 0;                            // slots with a >= x, those outside the record included
#pragma unroll
            for (int j = 0; j < kPerLane; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) ge += (uint32_t)__popc((img[j][e] - xx) & kGuardBits);
            const int below = kBlock - (int)block_sum(ge, (bit & 1) ^ 1);      // bit 14 takes turn 1, after turn 0 above
            if (below <= rank) level = (int)x;
        }
    }

    // ---- hits, one byte per staged chunk
    uint8_t* __restrict__ hit_bytes = reinterpret_cast<uint8_t*>(hits);
    const int q = level > 0 ? (thr16 * level) >> 4 : 32768;     // a > 32768 never holds: a silent block has no hits
    if (count == kBlock && q < 32767) {                 // a full block: a > q <=> min(a, 32767) >= q + 1, from the image
        const uint32_t xx = (uint32_t)(q + 1) * 0x10001u;
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) hit_bytes[kHaloChunks + tid + kThreads * j] = (uint8_t)hit_bits_image(img[j], xx);
    } else {                                            // the record's last block (its image has 32767 outside the record),
#pragma unroll                                          // or a threshold that only 32768 exceeds, or none
        for (int j = 0; j < kPerLane; ++j) hit_bytes[kHaloChunks + tid + kThreads * j] = (uint8_t)hit_bits(raw[j], q);
    }
    if (tid < 2 * kHaloChunks) hit_bytes[tid < kHaloChunks ? tid : kChunks + tid] = (uint8_t)hit_bits(halo, q);
    __syncthreads();

    // ---- the guard: block sample 32 t + i is bit 64 + 32 t + i of `hits`, bit 64 + i of the five words from word t on
    uint32_t w[5] = {hits[tid], hits[tid + 1], hits[tid + 2], hits[tid + 3], hits[tid + 4]};
    smear_up(w, 2 * guard);
    const int first = kHalo + guard;                    // bit 64 + i + G of the smeared number: the OR of 64 + i - G .. 64 + i + G
    const int fw = first >> 5;                          // 2, 3 or 4
    const uint32_t lo = fw == 2 ? w[2] : (fw == 3 ? w[3] : w[4]), hi = fw == 2 ? w[3] : (fw == 3 ? w[4] : 0u);
    uint32_t m = (uint32_t)((((uint64_t)hi << 32) | lo) >> (first & 31));
    const int inside = count - 32 * tid;                // samples of this word inside the record
    m = inside >= 32 ? m : (inside > 0 ? m & ((1u << inside) - 1u) : 0u);
    mask[tid] = m;
    const uint32_t blanked = block_sum((uint32_t)__popc(m), 0);     // (barrier: `mask` is complete as well)
    if (tid == 0 && blanked) atomicAdd(n_blanked + seg, (int)blanked);

    // ---- the output: every chunk that starts below roundup8(nsamp), zeros from nsamp on (the staging guard's)
    const uint8_t* __restrict__ mask_bytes = reinterpret_cast<const uint8_t*>(mask);
    int16_t* __restrict__ orow = out + seg * out_stride;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const int c = tid + kThreads * j;
        if (8 * c >= count) continue;
        const uint32_t mb = mask_bytes[c];
        uint32_t v[4] = {raw[j].x, raw[j].y, raw[j].z, raw[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
            v[e] &= ((mb >> (2 * e)) & 1u ? 0u : 0xffffu) | ((mb >> (2 * e + 1)) & 1u ? 0u : 0xffff0000u);
        *reinterpret_cast<uint4*>(orow + base + 8 * c) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}
}  // namespace

void launch_audio_blank(const int16_t* pcm, size_t pcm_stride, int nsamp, int nseg, int thr16, int guard, int16_t* out,
                        size_t out_stride, int* n_blanked, hipStream_t st) {
    const int nblk = audio_blank_nblocks(nsamp);
    if (nseg <= 0 || nblk <= 0) return;
    // 176 blocks per row at the most on x: 2^31 / 176 rows per launch is beyond any memory
    hipLaunchKernelGGL(audio_blank_kernel, dim3((unsigned)nseg * (unsigned)nblk), dim3(kThreads), 0, st, pcm, pcm_stride, nsamp,
                       nblk, thr16, guard, out, out_stride, n_blanked);
}

}  // namespace wspr
