// K9 -- ordered-statistics decoding on the device, one wavefront per soft-symbol vector.
//
// The definition is in osd.h (there is no reference code for this stage; tests/helpers/osd_check.cpp is the serial
// statement the kernel is held to, field for field).  Per vector:
//   order      every lane ranks its (at most three) positions by counting the positions that precede them
//   basis      lane j holds row j of G (7 words: 162 code bits + 50 message bits) in registers.  Walking the positions
//              most reliable first, the lanes whose row is still free and has the position's bit set answer one 64-bit
//              ballot; the lowest of them becomes the pivot, its row is read out lane-to-scalar (v_readlane: no LDS on
//              the broadcast) and every other row with the bit set takes the XOR.  50 pivots later the rows are G~.
//   trials     G~ goes to LDS by pivot number, 7 words per row: lanes that read different rows hit different banks
//              (7 is odd).  Lane 0 tries c_0, lanes 0..49 the single rows, and the 1 225 pairs (a, b) are dealt round
//              robin; a lane forms c_0 ^ G~[a] ^ G~[b] once and, at depth 3, walks c = b+1..49 with ONE row XOR per
//              trial (nested subsets).  A trial's cost is 48 and + popcount over the 8 bit-planes of r, which are
//              wave-uniform (ballots) and live in scalar registers.
//   winner     the packed key (D, |T|, T) of osd.h, minimum across the lanes by butterfly
// Integer work throughout: ~100 VALU operations per trial, 326 trials per lane at depth 3.
#include "wspr_device.h"
#include "osd.h"

namespace wspr {
namespace {

using namespace osd;

__device__ __forceinline__ int lanes_below_mask(unsigned long long mask) {   // popcount(mask & lanes below me)
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(64)
void osd_kernel(const unsigned char* __restrict__ symbols, const int* __restrict__ offsets, int n, int depth,
                const uint32_t* __restrict__ gen, unsigned char* __restrict__ data, unsigned* __restrict__ dist,
                unsigned* __restrict__ nhard, unsigned* __restrict__ order_out) {
    __shared__ unsigned char symd[kNSymD];                  // deinterleaved soft symbols
    __shared__ unsigned char rel[192];                      // r by position (0 beyond 161)
    __shared__ unsigned char ord[192];                      // position by rank
    __shared__ unsigned char pivpos[64];                    // p_k
    __shared__ uint32_t rows[kK * kRowWords];               // G~ by pivot number
    __shared__ unsigned short pairs[kPairs];                // (a << 8) | b, lexicographic
    const int lane = threadIdx.x;
    const int v = blockIdx.x;
    if (v >= n) return;

    // ---- deinterleave (as K6w: the p-th bit-reversed counter value below 162) ------------------------------------
    {
        const unsigned char* __restrict__ sym = symbols + (size_t)offsets[v] * kNSymD;
        int base = 0;
        for (int c = 0; c < 4; ++c) {
            const int i = 64 * c + lane;
            const int j = (int)(__brev((unsigned)i) >> 24);
            const bool valid = j < kNSymD;
            const unsigned long long m = __ballot(valid);
            if (valid) symd[base + lanes_below_mask(m)] = sym[j];
            base += __popcll(m);
        }
    }
    if (lane < kK - 1)                                       // the pair list (depth >= 2)
        for (int b = lane + 1, q = pair_base(lane); b < kK; ++b, ++q) pairs[q] = (unsigned short)((lane << 8) | b);
    __syncthreads();

    // ---- decisions, reliabilities and their bit-planes (wave-uniform) ---------------------------------------------
    uint32_t plane[kPlanes][kCodeWords], hw[kCodeWords];
    int myr[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int i = 64 * c + lane;
        const bool valid = i < kN;
        const int s = valid ? (int)symd[i] : 0;
        const int r = valid ? reliab(s) : 0;
        myr[c] = r;
        rel[i] = (unsigned char)r;
        const unsigned long long hm = __ballot(valid && hard(s));
        hw[2 * c] = (uint32_t)hm; hw[2 * c + 1] = (uint32_t)(hm >> 32);
#pragma unroll
        for (int b = 0; b < kPlanes; ++b) {
            const unsigned long long pm = __ballot((r >> b) & 1);
            plane[b][2 * c] = (uint32_t)pm; plane[b][2 * c + 1] = (uint32_t)(pm >> 32);
        }
    }
    __syncthreads();

    // ---- order: rank = number of positions that come first --------------------------------------------------------
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int i = 64 * c + lane;
        if (i < kN) {
            int rank = 0;
            for (int j = 0; j < kN; ++j) {
                const int rj = rel[j];
                rank += (rj > myr[c] || (rj == myr[c] && j < i)) ? 1 : 0;
            }
            ord[rank] = (unsigned char)i;
        }
    }
    __syncthreads();

    // ---- most reliable basis: Gauss-Jordan, one row per lane -----------------------------------------------------
    uint32_t w[kRowWords];
#pragma unroll
    for (int k = 0; k < kRowWords; ++k) w[k] = lane < kK ? gen[lane * kRowWords + k] : 0u;
    bool used = lane >= kK;
    int mypiv = -1, npiv = 0;
    for (int t = 0; t < kN && npiv < kK; ++t) {
        const int p = __builtin_amdgcn_readfirstlane((int)ord[t]);
        const int pw_ = p >> 5;
        uint32_t x = w[0];
#pragma unroll
        for (int k = 1; k < kCodeWords; ++k) x = pw_ == k ? w[k] : x;
        const bool bit = (x >> (p & 31)) & 1u;
        const unsigned long long m = __ballot(bit && !used);
        if (m == 0ull) continue;                             // the column depends on the ones already kept
        const int pl = __builtin_ctzll(m);
        uint32_t pr[kRowWords];
#pragma unroll
        for (int k = 0; k < kRowWords; ++k) pr[k] = (uint32_t)__builtin_amdgcn_readlane((int)w[k], pl);
        if (bit && lane != pl) {
#pragma unroll
            for (int k = 0; k < kRowWords; ++k) w[k] ^= pr[k];
        }
        if (lane == pl) { used = true; mypiv = npiv; pivpos[npiv] = (unsigned char)p; }
        ++npiv;
    }
    if (mypiv >= 0) {
#pragma unroll
        for (int k = 0; k < kRowWords; ++k) rows[mypiv * kRowWords + k] = w[k];
    }
    __syncthreads();

    // ---- c_0: the rows whose pivot position holds a hard 1 ---------------------------------------------------------
    uint32_t c0[kRowWords];
    {
        const bool take = mypiv >= 0 && symd[pivpos[mypiv >= 0 ? mypiv : 0]] >= 128;
#pragma unroll
        for (int k = 0; k < kRowWords; ++k) {
            uint32_t x = take ? w[k] : 0u;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) x ^= (uint32_t)__shfl_xor((int)x, m, 64);
            c0[k] = x;
        }
    }
    uint32_t e0[kCodeWords];                                 // c_0 XOR h over the code words
#pragma unroll
    for (int k = 0; k < kCodeWords; ++k) e0[k] = c0[k] ^ hw[k];

    // ---- trials ----------------------------------------------------------------------------------------------------
    uint64_t best = ~0ull;
    if (lane == 0) best = pack_key(cost(e0, plane), 0u, 0u, 0u, 0u);
    if (depth >= 1 && lane < kK) {
        uint32_t e[kCodeWords];
#pragma unroll
        for (int k = 0; k < kCodeWords; ++k) e[k] = e0[k] ^ rows[lane * kRowWords + k];
        const uint64_t key = pack_key(cost(e, plane), 1u, (unsigned)lane, 0u, 0u);
        best = key < best ? key : best;
    }
    if (depth >= 2)
        for (int q = lane; q < kPairs; q += 64) {
            const unsigned ab = pairs[q], a = ab >> 8, b = ab & 255u;
            uint32_t e2[kCodeWords];
#pragma unroll
            for (int k = 0; k < kCodeWords; ++k) e2[k] = e0[k] ^ rows[a * kRowWords + k] ^ rows[b * kRowWords + k];
            uint64_t key = pack_key(cost(e2, plane), 2u, a, b, 0u);
            best = key < best ? key : best;
            if (depth >= 3)
                for (unsigned c = b + 1; c < (unsigned)kK; ++c) {
                    uint32_t e3[kCodeWords];
#pragma unroll
                    for (int k = 0; k < kCodeWords; ++k) e3[k] = e2[k] ^ rows[c * kRowWords + k];
                    key = pack_key(cost(e3, plane), 3u, a, b, c);
                    best = key < best ? key : best;
                }
        }
    best = wave_min_u64(best);

    // ---- the winner once more (wave-uniform), for its message and its Hamming distance ----------------------------
    const unsigned ordw = key_order(best);
    uint32_t win[kRowWords];
#pragma unroll
    for (int k = 0; k < kRowWords; ++k) {
        uint32_t x = c0[k];
        if (ordw >= 1) x ^= rows[key_elem(best, 0) * kRowWords + k];
        if (ordw >= 2) x ^= rows[key_elem(best, 1) * kRowWords + k];
        if (ordw >= 3) x ^= rows[key_elem(best, 2) * kRowWords + k];
        win[k] = x;
    }
    uint32_t ew[kCodeWords];
#pragma unroll
    for (int k = 0; k < kCodeWords; ++k) ew[k] = win[k] ^ hw[k];
    unsigned mine = 0;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
        const unsigned bv = message_byte(win, k);
        mine = lane == k ? bv : mine;
    }
    if (lane < 11) data[(size_t)v * 11 + lane] = (unsigned char)mine;
    if (lane == 0) {
        dist[v] = key_dist(best);
        nhard[v] = hamming(ew);
        order_out[v] = ordw;
    }
}

}  // namespace

void launch_osd(const unsigned char* symbols, const int* offsets, int n, int depth, const uint32_t* gen,
                unsigned char* data, unsigned* dist, unsigned* nhard, unsigned* order, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(osd_kernel, dim3(n), dim3(64), 0, st, symbols, offsets, n, depth, gen, data, dist, nhard, order);
}

}  // namespace wspr
