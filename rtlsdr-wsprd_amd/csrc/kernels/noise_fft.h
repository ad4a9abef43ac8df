// The 512-point frame transform of noise.h as one wave runs it (K16's noise_kernel and K20's waterfall_kernel): stated
// once.  A lane holds eight points of its wave's frame in registers and runs three of the nine stages on them (twelve
// butterflies, noise.h's statements on values); between the three passes the points change lanes through the wave's own
// exchange area of kExch complex points in LDS, in two padded layouts that keep the 8-byte accesses off each other's
// banks: points l + 64e (stages 0-2), (l & 7) + 64 (l >> 3) + 8e (stages 3-5), 8l + e (stages 6-8: the output slots, whose
// bins are noise::bin_of_slot()).  The caller places its barriers: store_a | load_b; load_b | store_b (every lane has read
// what it needs of the first layout); store_b | load_c.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "noise.h"

namespace wspr {
namespace noise_fft {

constexpr int kExch = 568;                                 // complex points of one wave's exchange area
// where point i lies between the first and the second pass, and between the second and the third
__device__ __forceinline__ int pos_a(int i) { return i + 8 * (i >> 6); }
__device__ __forceinline__ int pos_b(int i) { return (i & 7) * 65 + (i >> 3); }
static_assert(noise::kFft - 1 + 8 * 7 < kExch && 7 * 65 + 63 < kExch, "both layouts fit");

// butterfly of the points a and b of x[] with twiddle w
__device__ __forceinline__ void bfly(float2* x, int a, int b, float2 w) {
    noise::butterfly_values(&x[a].x, &x[a].y, &x[b].x, &x[b].y, w.x, w.y);
}

// one 16-byte vector of a row at sample a (a % 4 == 0); what lies at or behind np reads as 0 and is not touched
__device__ __forceinline__ float4 load_vec(const float* __restrict__ row, int a, int np) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a + 4 <= np) {
        v = *reinterpret_cast<const float4*>(row + a);
    } else {
        if (a < np) v.x = row[a];
        if (a + 1 < np) v.y = row[a + 1];
        if (a + 2 < np) v.z = row[a + 2];
    }
    return v;
}
__device__ __forceinline__ unsigned vec_non_finite(const float4& v) {
    return (noise::non_finite(v.x) || noise::non_finite(v.y) || noise::non_finite(v.z) || noise::non_finite(v.w)) ? 1u : 0u;
}

// the twiddles of the last pass are the same in every lane
struct LastTwiddles {
    float2 w0, w64, w128, w192;
};
__device__ __forceinline__ LastTwiddles last_twiddles(const float* __restrict__ table) {
    LastTwiddles t;
    t.w0 = make_float2(table[0], table[1]);
    t.w64 = make_float2(table[128], table[129]);
    t.w128 = make_float2(table[256], table[257]);
    t.w192 = make_float2(table[384], table[385]);
    return t;
}

// stages 0-2 on the points l + 64e; tw[m] = exp(-2 pi i m / 512)
__device__ __forceinline__ void pass_a(float2* x, const float2* tw, int lane) {
#pragma unroll
    for (int e = 0; e < 4; ++e) bfly(x, e, e + 4, tw[lane + 64 * e]);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const float2 w = tw[(lane + 64 * e) << 1];
        bfly(x, e, e + 2, w);
        bfly(x, e + 4, e + 6, w);
    }
    {
        const float2 w = tw[lane << 2];
#pragma unroll
        for (int e = 0; e < 8; e += 2) bfly(x, e, e + 1, w);
    }
}
__device__ __forceinline__ void store_a(float2* mine, const float2* x, int lane) {
#pragma unroll
    for (int e = 0; e < 8; ++e) mine[pos_a(lane + 64 * e)] = x[e];
}
// stages 3-5 on the points lo + 64 hi + 8e (lo = lane & 7, hi = lane >> 3)
__device__ __forceinline__ void load_b(float2* x, const float2* mine, int lo, int hi) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = mine[pos_a(lo + 64 * hi + 8 * e)];
}
__device__ __forceinline__ void pass_b(float2* x, const float2* tw, int lo) {
#pragma unroll
    for (int e = 0; e < 4; ++e) bfly(x, e, e + 4, tw[(lo + 8 * e) << 3]);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const float2 w = tw[(lo + 8 * e) << 4];
        bfly(x, e, e + 2, w);
        bfly(x, e + 4, e + 6, w);
    }
    {
        const float2 w = tw[lo << 5];
#pragma unroll
        for (int e = 0; e < 8; e += 2) bfly(x, e, e + 1, w);
    }
}
__device__ __forceinline__ void store_b(float2* mine, const float2* x, int lo, int hi) {
#pragma unroll
    for (int e = 0; e < 8; ++e) mine[pos_b(lo + 64 * hi + 8 * e)] = x[e];
}
// stages 6-8 on the points 8l + e: the output slots
__device__ __forceinline__ void load_c(float2* x, const float2* mine, int lane) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = mine[pos_b(8 * lane + e)];
}
__device__ __forceinline__ void pass_c(float2* x, const LastTwiddles& t) {
    bfly(x, 0, 4, t.w0); bfly(x, 1, 5, t.w64); bfly(x, 2, 6, t.w128); bfly(x, 3, 7, t.w192);
    bfly(x, 0, 2, t.w0); bfly(x, 4, 6, t.w0); bfly(x, 1, 3, t.w128); bfly(x, 5, 7, t.w128);
#pragma unroll
    for (int e = 0; e < 8; e += 2) bfly(x, e, e + 1, t.w0);
}

}  // namespace noise_fft
}  // namespace wspr
