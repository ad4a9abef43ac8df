// List decoding against known messages: the definition, shared by host and device.
//
// A second chance for a soft-symbol vector on which every Fano attempt failed, when the caller knows which messages to
// expect (the texts a receiver decoded in the last hours: beacons repeat their 50 bits slot after slot).  Correlating
// the vector with the code word of every listed message and taking the best is maximum-likelihood decoding over that
// list.  There is no reference code for it; what follows IS the contract, tests/helpers/list_check.c states it once more
// in serial C, and the kernel (k14_list.hip) is held to that checker bit for bit -- everything here is integer.
//
//   entry     a message text that channel_symbols() encodes on an empty hash memory and whose 11-byte decdata (as the Fano
//             decoder leaves it) unpacks, on an empty hash memory and without a hash look-up, to a canonical text that
//             encodes to the same 162 symbols: message types 1 and 2.  It is held as
//                 c[i] = 2 * (symbols[i] >> 1) - 1   in {-1, +1},   i = 0 .. 161, TRANSMISSION (interleaved) order
//             -- nothing is deinterleaved anywhere in this stage.
//   vector    162 soft symbols s[i] in transmission order, as the Fano and OSD entry points take them;
//                 v[i] = 2 s[i] - 255   (odd, never 0; |v[i]| is the reliability r[i] of osd.h)
//   score     S(m) = sum over i of c_m[i] * v[i], an int32 in [-41 310, 41 310].  With R = sum |v[i]| and D the OSD cost
//             of that code word (osd.h: the sum of r over the positions where it differs from the hard decisions),
//             S = R - 2 D: the list's best entry is its entry of least OSD cost.
//             In int8 arithmetic: a[i] = s[i] - 128 in [-128, 127], S = 2 * sum c[i] a[i] + B_m, B_m = sum c_m[i].
//   winner    the largest S, ties to the LOWER list index.  second = the largest S among all other entries (INT32_MIN for
//             a list of one).  V = sum v[i]^2 <= 162 * 255^2 = 10 534 050.
//   gate      accepted iff S1 > 0 and 256 * S1^2 >= zmin16^2 * V, in int64: z = S1 / sqrt(V) >= zmin16 / 16.  By Cauchy-
//             Schwarz |S1| <= R <= sqrt(162 V), so z never exceeds sqrt(162) = 12.73 and zmin16 is 1 .. 203.
//
// Layout on the device.  K is padded from 162 to 192 with zeros (48 words of four int8) in both operands, and the table
// is stored word-major: word k of entry m at table[k * mpad + m], mpad = the entry count rounded up to kEntryAlign, the
// entries beyond the list all zero.  Consecutive lanes then read consecutive words.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define WSPR_LIST_HD __host__ __device__ __forceinline__
#else
#define WSPR_LIST_HD static inline
#endif

namespace wspr {
namespace listmatch {

constexpr int kN = 162, kKPad = 192, kWords = kKPad / 4, kEntryAlign = 64;
constexpr int kMaxEntries = 65536;                           // WSPR_LIST_MAX of the public header
constexpr int kZminLo = 1, kZminHi = 203;                    // 16 * sqrt(162) = 203.6
constexpr int32_t kNoSecond = INT32_MIN;

WSPR_LIST_HD int chip(int symbol)  { return 2 * (symbol >> 1) - 1; }     // c[i] of a channel symbol 0..3
WSPR_LIST_HD int value(int s)      { return 2 * s - 255; }               // v[i] of a soft symbol
WSPR_LIST_HD int centred(int s)    { return s - 128; }                   // a[i]
WSPR_LIST_HD int padded(int m)     { return (m + kEntryAlign - 1) / kEntryAlign * kEntryAlign; }

WSPR_LIST_HD bool gate(int32_t s1, int32_t v2, int zmin16) {
    return s1 > 0 && 256ll * (int64_t)s1 * (int64_t)s1 >= (int64_t)zmin16 * (int64_t)zmin16 * (int64_t)v2;
}

// The winner's rule as one signed comparison: the score, then the INVERTED index, so that the larger key is the better
// entry and the lower index wins a tie.  The two best keys of a set are its winner and the holder of `second`.
WSPR_LIST_HD int64_t pack_key(int32_t score, uint32_t index) {
    return (int64_t)(((uint64_t)(uint32_t)score << 32) | (uint64_t)(0xFFFFFFFFu - index));
}
WSPR_LIST_HD int32_t key_score(int64_t k)  { return (int32_t)(k >> 32); }
WSPR_LIST_HD uint32_t key_index(int64_t k) { return 0xFFFFFFFFu - (uint32_t)k; }
constexpr int64_t kNoKey = INT64_MIN;                        // below every real key; its score reads as kNoSecond

struct Top2 { int64_t best, second; };
WSPR_LIST_HD void top2_add(Top2& t, int64_t k) {
    const int64_t lo = k < t.best ? k : t.best;
    t.best = k < t.best ? t.best : k;
    t.second = lo < t.second ? t.second : lo;
}
WSPR_LIST_HD void top2_merge(Top2& t, int64_t ob, int64_t os) {         // the two best of the union of two sets
    const int64_t lo = ob < t.best ? ob : t.best, s2 = os < t.second ? t.second : os;
    t.best = ob < t.best ? t.best : ob;
    t.second = lo < s2 ? s2 : lo;
}

}  // namespace listmatch
}  // namespace wspr
