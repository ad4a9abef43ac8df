// Noncoherent block detection of the WSPR soft symbols: the definition.
//
// Soft symbols formed from the best COHERENT combination of the tone correlations over B consecutive symbols, instead of
// from single-symbol amplitudes.  There is no reference code for it (the reference predates wsprd's -B); what follows
// IS the contract, shaped after WSJT-X's noncoherent_sequence_detection().  tests/helpers/block_check.c states it once
// more in serial C (CONTRACT=0/1), and the kernel (k10_blockdemod.hip) is held to that checker bit for bit.
//
// For one hypothesis (f, shift, drift) and block size B in {1, 2, 3} (162 = 2*81 = 3*54):
//   tone sums    is[t][i], qs[t][i], symbol i, tone t: the eight accumulators of wsprd.c:200-207 at k = shift + 256 i + j
//                under the reference's guard k > 0 && k < np, with the phasor tables of wsprd.c:158-187 (tone_dphi(),
//                glibc_sinf/cosf, the float recurrence), in the reference's order, in the call's arithmetic mode.
//                sqrt(is^2 + qs^2) is the p[t] of sync_and_demodulate() mode 2.
//   advance      (cf, sf)[t][i], the phase tone t gains over symbol i: the table's recurrence taken one step past its
//                last entry, (c[255], s[255]) through phasor_step() once more.
//   combine      for each block of B symbols from i0 and each of the 2^B bit sequences j (the bit of the block's first
//                symbol is the most significant): xi = xq = 0, cm = 1, sm = 0; for ib = 0 .. B-1, with b that symbol's bit
//                and (is, qs, cf, sf) those of tone t = pr3[i0 + ib] + 2 b of symbol i0 + ib:
//                    xi  = xi + is*cm + qs*sm;
//                    xq  = xq + qs*cm - is*sm;
//                    cmp = cf*cm - sf*sm;
//                    smp = sf*cm + cf*sm;
//                    cm  = cmp;  sm = smp;
//                then p[j] = sqrt(xi*xi + xq*xq), the correctly rounded root of the mode-2 amplitudes.
//                Exact mode: every operation separately rounded, left to right.  Contracted mode: clang's rule (arith.h)
//                on these statements as written:
//                    xi  = mad(qs, sm, mad(is, cm, xi));         (xi + is*cm) + qs*sm
//                    xq  = nmad(is, sm, mad(qs, cm, xq));        (xq + qs*cm) - is*sm
//                    cmp = mms(cf, cm, sf, sm);   smp = mma(sf, cm, cf, sm);   p[j] = sqrt(mma(xi, xi, xq, xq))
//   soft value   of symbol i0 + ib: fsymb = xm1 - xm0, xm1 the maximum of p[j] over the sequences whose bit for that
//                symbol is 1, xm0 over those whose bit is 0; both start from 0.0f and take a p[j] only if p[j] > xm.
//   bytes        as sync_and_demodulate() mode 2: SoftNorm over fsymb in symbol order, soft_quantise() with symfac 50
//                (NaN -> 0), rms = sqrt(sum((byte - 128)^2) / 162).
// At B = 1 and on finite input this is mode 2's vector bit for bit in both modes: 0 + is*1 + qs*0 = is, max(0, p) = p
// and the soft value is pr3 ? p3 - p1 : p2 - p0.  That identity pins the definition to the compiled reference.
#pragma once
#include "arith.h"

#pragma clang fp contract(off)

namespace wspr {
namespace blockdemod {

constexpr int kMaxBlock = 3;

// one tone of one symbol as the combine reads it
struct ToneSum { float is, qs, cf, sf; };

// The 2^B amplitudes p[j] of one block; tone(ib, b) returns the ToneSum of the block's symbol ib under bit b.
template <int B, bool kFma, class Tone>
__device__ __forceinline__ void combine(Tone tone, float (&p)[1 << B]) {
    using A = Arith<kFma>;
#pragma unroll
    for (int j = 0; j < (1 << B); ++j) {
        float xi = 0.0f, xq = 0.0f, cm = 1.0f, sm = 0.0f;
#pragma unroll
        for (int ib = 0; ib < B; ++ib) {
            const ToneSum t = tone(ib, (j >> (B - 1 - ib)) & 1);
            xi = A::mad(t.qs, sm, A::mad(t.is, cm, xi));
            xq = A::nmad(t.is, sm, A::mad(t.qs, cm, xq));
            const float cmp = A::mms(t.cf, cm, t.sf, sm);
            const float smp = A::mma(t.sf, cm, t.cf, sm);
            cm = cmp; sm = smp;
        }
        p[j] = sqrtf(A::mma(xi, xi, xq, xq));
    }
}

// fsymb of the block's symbol ib from the 2^B amplitudes
template <int B>
__device__ __forceinline__ float soft_value(const float (&p)[1 << B], int ib) {
    float xm1 = 0.0f, xm0 = 0.0f;
#pragma unroll
    for (int j = 0; j < (1 << B); ++j) {
        if ((j >> (B - 1 - ib)) & 1) { if (p[j] > xm1) xm1 = p[j]; }
        else                         { if (p[j] > xm0) xm0 = p[j]; }
    }
    return xm1 - xm0;
}

}  // namespace blockdemod
}  // namespace wspr
