// Arithmetic policy (wspr_set_arithmetic): every contraction site of wsprd.c, in K1, K4 and K7, is written ONCE, through
// Arith<kFma>, and every kernel that evaluates such a site is a template on kFma.
//   kFma = false  the exact mode: separately rounded multiplies and adds, the reference's arithmetic as x86-64 SSE
//                 evaluates it.
//   kFma = true   the contracted mode: each site as clang's -ffp-contract=on fuses it in wsprd.c, the LEFT product of a
//                 sum into the fma (a*b + c*d -> fma(a, b, c*d); (acc + x*c) + y*s -> fma(y, s, fma(x, c, acc));
//                 acc - x*s -> fma(-x, s, acc)).  Per-lane accumulation order stays the reference's loop order.
// The v2f overloads are the packed forms (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 on a register pair): each half is
// an ordinary IEEE operation, so a packed site rounds exactly like two scalar ones.
// CPU twin: tests/helpers/contract_dsp.c states the same sites through the macros MAD, NMAD, MMA and MMS
// (CONTRACT=0/1); its table maps every wsprd.c line to its form.
// The sources are built with -ffp-contract=off (build.sh): the only fusions are the ones spelled here.
#pragma once

#pragma clang fp contract(off)

namespace wspr {

typedef float v2f __attribute__((ext_vector_type(2)));      // one VGPR pair: operands of the packed fp32 instructions

__device__ __forceinline__ float fused(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ v2f fused(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }

// T is float or v2f (the two overloads of fused())
template <bool kFma>
struct Arith {
    template <class T> static __device__ __forceinline__ T mad(T a, T b, T c) {           // a*b + c
        if constexpr (kFma) return fused(a, b, c); else return a * b + c;
    }
    template <class T> static __device__ __forceinline__ T nmad(T a, T b, T c) {          // c - a*b
        if constexpr (kFma) return fused(-a, b, c); else return c - a * b;
    }
    template <class T> static __device__ __forceinline__ T mma(T a, T b, T c, T d) {      // a*b + c*d
        if constexpr (kFma) return fused(a, b, c * d); else return a * b + c * d;
    }
    template <class T> static __device__ __forceinline__ T mms(T a, T b, T c, T d) {      // a*b - c*d
        if constexpr (kFma) return fused(a, b, -(c * d)); else return a * b - c * d;
    }
    // N independent sites with a common factor, acc[r] = a*b[r] + acc[r] (the taps of K7's FIR).  The exact arm is
    // hand-scheduled: the N products are formed before the N sums, so that dependent packed instructions sit apart.
    template <int N, class T> static __device__ __forceinline__ void mad_each(T a, const T (&b)[N], T (&acc)[N]) {
        if constexpr (kFma) {
#pragma unroll
            for (int r = 0; r < N; ++r) acc[r] = fused(a, b[r], acc[r]);
        } else {
            T p[N];
#pragma unroll
            for (int r = 0; r < N; ++r) p[r] = a * b[r];
#pragma unroll
            for (int r = 0; r < N; ++r) acc[r] = acc[r] + p[r];
        }
    }
};

}  // namespace wspr
