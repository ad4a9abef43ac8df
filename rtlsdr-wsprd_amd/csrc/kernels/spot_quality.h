// Decode-quality figures of one spot: the definition, shared by host and device.
//
// How well did the soft-symbol vector that decoded agree with the code word it decoded to?  There is no reference code for
// these figures (the reference reports only its 80-byte decoder_results); what follows IS the contract,
// tests/helpers/spot_quality_check.c states it once more in serial C, and the kernel (k19_spot_quality.hip) is held to
// that checker field for field -- everything here is integer.
//
//   job       162 soft symbols s[i] in transmission (interleaved) order, as the Fano search, the ordered-statistics and the
//             list stage take them, and decdata[11] as fano() leaves it
//   code word c[i] in {0, 1}, i = 0 .. 161 in transmission order: message bit j (0 .. 49) is bit 7 - (j & 7) of
//             decdata[j >> 3]; bits 50 .. 80 are the zero tail whatever decdata holds there; the encoder's state after bit
//             j is state_j = sum of bit[j - t] << t, t = 0 .. 31; coder output 2j = parity(state_j & 0xf2d05351), 2j + 1 =
//             parity(state_j & 0xe4613c47) (fano.c:51-52); coder output k is sent at transmission position at[k], the k-th
//             bit-reversed 8-bit counter value below 162 (wsprsim_utils.c:144-161).  c[i] = coder output where[i], where
//             where[at[k]] = k: the data bits of encode() + interleave() of the 50 message bits.  It is the code word, not a
//             re-encoding of the unpacked text: it exists for every decode and needs no hash memory
//   h, v, r   h[i] = (s[i] >= 128), v[i] = 2 s[i] - 255 (odd, never 0), r[i] = |v[i]|: the ordered-statistics and the list
//             stage's own conventions (osd.h, listmatch.h)
//   nhard     the number of i with h[i] != c[i]
//   dist      the sum of r[i] over those i         (the ordered-statistics cost D of that code word)
//   rsum      the sum of r[i] over all i           (rsum - 2 dist = the list stage's score S of that code word)
//   v2        the sum of v[i]^2                    (the list stage's V; at most 10 534 050)
//   metric    the sum over i of mettab[c[i]][s[i]], int32, mettab = wspr_fano_metric_table(): for a vector on which fano()
//             succeeded this is its *metric (gamma at the last node = the sum of the 81 branch metrics of the decoded path;
//             fano() hands it out as unsigned int: the same word, gamma can be negative)
//
// mettab[1][s] = mettab[0][255 - s] (wsprd.c:471-472), so the kernel reads row 0 alone: the 256 shorts the Fano wave uses.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define WSPR_SQ_HD __host__ __device__ __forceinline__
#else
#define WSPR_SQ_HD static inline
#endif

namespace wspr {
namespace spotq {

constexpr int kN = 162, kMsgBits = 50;
constexpr uint32_t kPoly1 = 0xf2d05351u, kPoly2 = 0xe4613c47u;

// the five figures of one job, in the order the public header's wspr_spot_quality declares them (20 bytes)
struct Figures {
    int32_t nhard, dist, rsum, v2, metric;
};

WSPR_SQ_HD unsigned parity32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (unsigned)__popc(v) & 1u;
#else
    return (unsigned)__builtin_popcount(v) & 1u;
#endif
}

// the 50 message bits of decdata, bit 0 the most significant of the 50
WSPR_SQ_HD uint64_t message_bits(const unsigned char* decdata) {
    uint64_t m = 0;
    for (int k = 0; k < 7; ++k) m = (m << 8) | decdata[k];
    return m >> 6;
}
// the encoder's state after bit j (0 .. 80) of the message followed by its zero tail
WSPR_SQ_HD uint32_t coder_state(uint64_t m, int j) {
    return j < kMsgBits ? (uint32_t)(m >> (kMsgBits - 1 - j)) : (uint32_t)(m << (j - (kMsgBits - 1)));
}
// coder output k (0 .. 161)
WSPR_SQ_HD unsigned code_bit(uint64_t m, int k) { return parity32(coder_state(m, k >> 1) & ((k & 1) ? kPoly2 : kPoly1)); }

WSPR_SQ_HD int value(int s) { return 2 * s - 255; }

}  // namespace spotq
}  // namespace wspr
