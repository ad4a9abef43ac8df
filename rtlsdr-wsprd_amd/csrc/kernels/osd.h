// Ordered-statistics decoding (OSD) of the WSPR code: the definition, shared by host and device.
//
// A second chance for a soft-symbol vector on which the Fano search failed.  There is no reference code for it (the
// reference predates wsprd's -o); what follows IS the contract, tests/helpers/osd_check.cpp states it once more in
// serial C++, and the kernel (k9_osd.hip) is held to that checker bit for bit -- everything here is integer.
//
//   input     162 soft symbols s[i], deinterleaved (as the Fano search takes them)
//   code      row j (0..49) of G = the first 162 outputs of the convolutional encoder for the message with only
//             message bit j set (MSB first, bits 50..87 zero); each row carries its 50-bit message alongside
//   decisions h[i] = (s[i] >= 128),  reliabilities r[i] = |2 s[i] - 255|   (odd, 1..255, never zero)
//   order     positions by r descending, ties to the lower index
//   basis     walking the positions in that order, a position is kept if its column of G is linearly independent of
//             the columns kept so far, until 50 are kept: p_0 .. p_49.  G~ = the generator of the same code with
//             G~[k][p_m] = (k == m)
//   trials    c_0 = XOR of G~[k] over k with h[p_k] = 1;  for every T in {0..49} with |T| <= depth,
//             c_T = c_0 XOR (XOR of G~[k] over k in T),  D(T) = sum of r[i] where c_T[i] != h[i]
//   winner    smallest D, then smaller |T|, then the lexicographically smaller ascending tuple T
//   output    the winner's message as the Fano decoder leaves decdata (11 bytes, bits 50.. zero), dist = D,
//             nhard = positions where the winner differs from h, order = |T|
// depth 0..3: 1, 51, 1 276, 20 876 trials.
//
// Layout.  A row is 7 words: bit b of the row is bit (b & 31) of word (b >> 5); bits 0..161 are the code word, bit
// 162 + j is message bit j, bits 212..223 are zero.  The reliabilities are held as 8 bit-planes over the same 6 code
// words (plane[b] has bit i set when bit b of r[i] is set; nothing set at or beyond bit 162), so that the cost of a
// trial is 48 and + popcount, and a row's message bits never count.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define WSPR_OSD_HD __host__ __device__ __forceinline__
#else
#define WSPR_OSD_HD static inline
#endif

namespace wspr {
namespace osd {

constexpr int kN = 162, kK = 50, kRowWords = 7, kCodeWords = 6, kPlanes = 8, kMaxDepth = 3;
constexpr int kPairs = kK * (kK - 1) / 2;                    // 1 225 subsets of size two
constexpr uint32_t kLastCodeMask = (1u << (kN - 32 * (kCodeWords - 1))) - 1u;   // code bits of word 5: bits 160, 161

WSPR_OSD_HD int hard(int s)   { return s >= 128 ? 1 : 0; }
WSPR_OSD_HD int reliab(int s) { const int v = 2 * s - 255; return v < 0 ? -v : v; }
WSPR_OSD_HD int trials(int depth) {                          // subsets of {0..49} with at most `depth` elements
    return depth <= 0 ? 1 : depth == 1 ? 51 : depth == 2 ? 1276 : 20876;
}

WSPR_OSD_HD unsigned popc32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (unsigned)__popc(v);
#else
    return (unsigned)__builtin_popcount(v);
#endif
}

WSPR_OSD_HD unsigned row_bit(const uint32_t* w, int b) { return (w[b >> 5] >> (b & 31)) & 1u; }
WSPR_OSD_HD void row_set(uint32_t* w, int b) { w[b >> 5] |= 1u << (b & 31); }

// row j of G from the encoder's 162 output bits (bytes 0/1) for the message with only bit j set
WSPR_OSD_HD void pack_generator_row(const unsigned char* code162, int j, uint32_t* w) {
    for (int k = 0; k < kRowWords; ++k) w[k] = 0u;
    for (int i = 0; i < kN; ++i) if (code162[i] & 1u) row_set(w, i);
    row_set(w, kN + j);
}

// D of the definition for e = c XOR h over the 6 code words (whatever e holds beyond bit 161 does not count: the
// planes are empty there)
WSPR_OSD_HD unsigned cost(const uint32_t* e, const uint32_t (*plane)[kCodeWords]) {
    unsigned d = 0;
    for (int b = 0; b < kPlanes; ++b) {
        unsigned c = 0;
        for (int k = 0; k < kCodeWords; ++k) c += popc32(e[k] & plane[b][k]);
        d += c << b;
    }
    return d;
}
WSPR_OSD_HD unsigned hamming(const uint32_t* e) {            // positions 0..161 where e is set
    unsigned c = 0;
    for (int k = 0; k < kCodeWords - 1; ++k) c += popc32(e[k]);
    return c + popc32(e[kCodeWords - 1] & kLastCodeMask);
}

// The winner's rule as one unsigned comparison: D (<= 162 * 255 < 2^16), then |T|, then the ascending tuple (a, b, c)
// with the absent elements zero (tuples are only compared at equal |T|).  Smaller key wins.
WSPR_OSD_HD uint64_t pack_key(unsigned d, unsigned order, unsigned a, unsigned b, unsigned c) {
    return ((uint64_t)d << 32) | ((uint64_t)order << 24) | (a << 12) | (b << 6) | c;
}
WSPR_OSD_HD unsigned key_dist(uint64_t k)  { return (unsigned)(k >> 32); }
WSPR_OSD_HD unsigned key_order(uint64_t k) { return (unsigned)(k >> 24) & 3u; }
WSPR_OSD_HD unsigned key_elem(uint64_t k, int i) { return (unsigned)(k >> (12 - 6 * i)) & 63u; }

// The row's 50 message bits as the Fano decoder leaves decdata: byte k = message bits 8k .. 8k+7, first in the MSB
WSPR_OSD_HD unsigned message_byte(const uint32_t* w, int k) {
    unsigned v = 0;
    for (int j = 0; j < 8; ++j) {
        const int m = 8 * k + j;
        v = (v << 1) | (m < kK ? row_bit(w, kN + m) : 0u);
    }
    return v;
}

// first index of the pairs (a, a+1..49) in the list of all pairs in lexicographic order
WSPR_OSD_HD int pair_base(int a) { return a * (kK - 1) - a * (a - 1) / 2; }

}  // namespace osd
}  // namespace wspr
