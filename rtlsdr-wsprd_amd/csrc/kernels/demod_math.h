// The pieces every kernel of K4 (k4_demod.hip) and K10 (k10_blockdemod.hip) shares: the tone phasors of
// sync_and_demodulate() (wsprd.c:158-187), its sync metric (:209-218) and its soft symbols (:219-225, :243-256).
// Each contraction site goes through Arith<kFma> (arith.h).  Device code only.
#pragma once
#include "wspr_device.h"
#include "arith.h"
#include "glibc_sincosf.h"

#pragma clang fp contract(off)

namespace wspr {
namespace {

constexpr double kTwoPiDt = 2.0 * 3.14159265358979323846 * 1.0 / 375.0;   // TWOPIDT
constexpr double kDf05 = 375.0 / 256.0 * 0.5;
constexpr double kDf15 = 375.0 / 256.0 * 1.5;

// f0 = *freq + ifreq * fstep, wsprd.c:151
template <bool kFma>
__device__ __forceinline__ float hyp_freq(float freq, int ifreq, float fstep) {
    return Arith<kFma>::mad((float)ifreq, fstep, freq);
}

// Phase step of one tone of one symbol (wsprd.c:158-177): the symbol's frequency on the drift line, in float as the
// reference keeps it, then the tone's offset in double.  f0 is the reference's float, widened (exactly) by the call.
__device__ __forceinline__ float tone_dphi(double f0, float drift, int sym, int tone) {
    const float fp = (float)(f0 + ((double)drift / 2.0) * (double)((float)sym - 81.0f) / (double)81.0f);
    const double off = (tone == 0) ? -kDf15 : (tone == 1) ? -kDf05 : (tone == 2) ? kDf05 : kDf15;
    return (float)(kTwoPiDt * ((double)fp + off));
}

// One step of the phasor recurrence (wsprd.c:180-187): c' = c*cd - s*sd, s' = c*sd + s*cd; T = float or v2f
template <bool kFma, class T>
__device__ __forceinline__ void phasor_step(T& c, T& s, T cd, T sd) {
    const T cn = Arith<kFma>::mms(c, cd, s, sd);
    s = Arith<kFma>::mma(c, sd, s, cd);
    c = cn;
}

// One tone's table: 256 steps of the recurrence from (1, 0) into t[256][8] = (cos of tones 0..3, sin of tones 0..3)
template <bool kFma>
__device__ __forceinline__ void build_phasor_table(float dphi, int tone, float* __restrict__ t) {
    const float cd = glibc_cosf(dphi), sd = glibc_sinf(dphi);
    float c = 1.0f, s = 0.0f;
    for (int j = 0; j < kSps; ++j) {
        if (j > 0) phasor_step<kFma>(c, s, cd, sd);
        t[8 * j + tone] = c;
        t[8 * j + 4 + tone] = s;
    }
}

// Sync metric of one hypothesis (wsprd.c:209-218): the 162 symbols' tone amplitudes amp(k) folded in symbol order
template <class Amp>
__device__ __forceinline__ float sync_metric(Amp amp, const unsigned char* __restrict__ pr3) {
    float ss = 0.0f, totp = 0.0f;
    for (int k = 0; k < kNSymD; ++k) {
        const float4 p = amp(k);
        totp = totp + p.x + p.y + p.z + p.w;
        const float cmet = (p.y + p.w) - (p.x + p.z);
        ss = pr3[k] ? ss + cmet : ss - cmet;
    }
    return ss / totp;
}

// Soft symbols, wsprd.c:219-225 and :243-256.  fsymb of one symbol from its amplitudes and its sync bit:
__device__ __forceinline__ float soft_f(const float4 p, unsigned char sync_bit) { return sync_bit ? p.w - p.y : p.z - p.x; }
// their mean and mean square, in symbol order, and the normalisation fac = sqrt(f2sum - fsum*fsum):
struct SoftNorm {
    float fsum = 0.0f, f2sum = 0.0f;
    __device__ __forceinline__ void add(float f) {
        fsum += f / 162.0f;
        const float ff = f * f;
        f2sum += ff / 162.0f;
    }
    template <bool kFma>
    __device__ __forceinline__ float fac() const { return sqrtf(Arith<kFma>::nmad(fsum, fsum, f2sum)); }
};
// symfac * fsymb[i] / fac (wsprd.c:250, int -> float), clamped to -128 .. 127, offset by 128; NaN -> 0
__device__ __forceinline__ unsigned char soft_quantise(float f, float fac, float symfac) {
    float v = symfac * f / fac;
    if (v > 127.0f) v = 127.0f;
    if (v < -128.0f) v = -128.0f;
    const float w = v + 128.0f;
    return (w == w) ? (unsigned char)(int)w : (unsigned char)0;
}
// a quantised symbol's term of the rms (a small integer squared: the sum is exact in any order)
__device__ __forceinline__ float soft_square(unsigned char b) {
    const float y = (float)b - 128.0f;
    return y * y;
}
constexpr float kSymFac = 50.0f;      // the symfac of every caller but the exported sync_and_demodulate()

}  // namespace
}  // namespace wspr
