// K14 -- list decoding against known messages on the device: N soft-symbol vectors x M listed code words.
//
// The definition is in listmatch.h (there is no reference code for this stage; tests/helpers/list_check.c is the serial
// statement the kernel is held to, field for field).  One workgroup of 256 threads takes a tile of kVecTile vectors
// and walks the WHOLE list once for it:
//   vectors    a[i] = s[i] - 128 as int8, padded from 162 to 192 with zeros, in LDS word-major ([word][vector]), so that
//              the kVecTile words a step needs are one wave-uniform (broadcast) read
//   list       int8 chips, word-major (word k of entry m at table[k * mpad + m]): thread t takes entries t, t + 256, ...,
//              and the 64 lanes of a wave read 64 consecutive words -- the list is read once per vector tile, coalesced
//   score      48 v_dot4_i32_i8 per (entry, vector): exact, S = 2 * sum + B_m
//   winner     every thread keeps the two best packed keys (score, inverted index) per vector; two best of a union =
//              the two best among the parts' two best, so the butterfly over the lanes and the merge over the four waves
//              reproduce the tie rule and `second` exactly wherever winner and runner-up sit
// Expected load is small (about one vector per weak segment), so nothing here is tuned beyond that.
#include "wspr_device.h"
#include "listmatch.h"

namespace wspr {
namespace {

using namespace listmatch;

constexpr int kVecTile = 8, kThreads = 256, kWaves = kThreads / 64;

__device__ __forceinline__ int64_t shfl_xor_i64(int64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)v >> 32), m, 64);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__global__ __launch_bounds__(kThreads)
void list_match_kernel(const unsigned char* __restrict__ symbols, const int* __restrict__ offsets, int n,
                       const int* __restrict__ table, const int* __restrict__ bias, int m, int mpad,
                       ListMatch* __restrict__ out) {
    __shared__ int vec[kWords][kVecTile];                   // four int8 a[i] per word; zero beyond position 161 / vector n-1
    __shared__ int v2[kVecTile];
    __shared__ int64_t wbest[kWaves][kVecTile], wsecond[kWaves][kVecTile];
    const int tid = threadIdx.x, v0 = blockIdx.x * kVecTile;
    if (v0 >= n) return;

    for (int idx = tid; idx < kWords * kVecTile; idx += kThreads) {
        const int k = idx / kVecTile, v = idx % kVecTile;
        unsigned word = 0u;
        if (v0 + v < n) {
            const unsigned char* __restrict__ s = symbols + (size_t)offsets[v0 + v] * kN;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int i = 4 * k + b;
                const int a = i < kN ? centred((int)s[i]) : 0;
                word |= ((unsigned)a & 0xFFu) << (8 * b);
            }
        }
        vec[k][v] = (int)word;
    }
    if (tid < kVecTile) {                                    // V = sum of v[i]^2
        int acc = 0;
        if (v0 + tid < n) {
            const unsigned char* __restrict__ s = symbols + (size_t)offsets[v0 + tid] * kN;
            for (int i = 0; i < kN; ++i) { const int x = value((int)s[i]); acc += x * x; }
        }
        v2[tid] = acc;
    }
    __syncthreads();

    Top2 top[kVecTile];
#pragma unroll
    for (int v = 0; v < kVecTile; ++v) top[v] = Top2{kNoKey, kNoKey};
    for (int e = tid; e < m; e += kThreads) {                // e < m <= mpad: every read lies inside the table
        int acc[kVecTile];
#pragma unroll
        for (int v = 0; v < kVecTile; ++v) acc[v] = 0;
#pragma unroll 8
        for (int k = 0; k < kWords; ++k) {
            const int c = table[(size_t)k * mpad + e];
#pragma unroll
            for (int v = 0; v < kVecTile; ++v) acc[v] = __builtin_amdgcn_sdot4(c, vec[k][v], acc[v], false);
        }
        const int b = bias[e];
#pragma unroll
        for (int v = 0; v < kVecTile; ++v) top2_add(top[v], pack_key(2 * acc[v] + b, (uint32_t)e));
    }

    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int v = 0; v < kVecTile; ++v) {
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int64_t ob = shfl_xor_i64(top[v].best, s), os = shfl_xor_i64(top[v].second, s);
            top2_merge(top[v], ob, os);
        }
        if (lane == 0) { wbest[wave][v] = top[v].best; wsecond[wave][v] = top[v].second; }
    }
    __syncthreads();
    if (tid < kVecTile && v0 + tid < n) {
        Top2 t{wbest[0][tid], wsecond[0][tid]};
        for (int w = 1; w < kWaves; ++w) top2_merge(t, wbest[w][tid], wsecond[w][tid]);
        ListMatch r;
        r.index = (int32_t)key_index(t.best);
        r.score = key_score(t.best);
        r.second = key_score(t.second);
        r.v2 = v2[tid];
        out[v0 + tid] = r;
    }
}

}  // namespace

void launch_list_match(const unsigned char* symbols, const int* offsets, int n, const int* table, const int* bias, int m,
                       ListMatch* out, hipStream_t st) {
    if (n <= 0 || m <= 0) return;
    hipLaunchKernelGGL(list_match_kernel, dim3((n + kVecTile - 1) / kVecTile), dim3(kThreads), 0, st, symbols, offsets, n,
                       table, bias, m, padded(m), out);
}

}  // namespace wspr
