// Test helper: the ordered-statistics decoder as the kernel k9_osd.hip computes it, emulated on the host lane by lane
// with the packed half of csrc/kernels/osd.h -- 7-word rows (pack_generator_row, row_bit), the 8 bit-planes of the
// reliabilities and cost(), hamming(), the rank sort by counting, one generator row per "lane" with the lowest free lane
// as the pivot, the pair list (pair_base) dealt round robin over 64 lanes with nested depth-3 subsets, pack_key /
// key_dist / key_order / key_elem and message_byte().  Only the cross-lane intrinsics (ballot, readlane, the shuffle
// butterflies) are replaced by loops.  tests/test_osd_checker.py holds it to the serial checker osd_check.cpp.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../rtlsdr-wsprd_amd/csrc/host/wspr_message.cpp"
#include "../../rtlsdr-wsprd_amd/csrc/kernels/osd.h"

using namespace wspr::osd;

extern "C" int osd_packed(const unsigned char* symbols, int depth, unsigned char* data11, unsigned* dist, unsigned* nhard,
                          unsigned* order_out) {
    if (depth < 0 || depth > kMaxDepth) return -1;
    unsigned char symd[kN];
    memcpy(symd, symbols, kN);
    wspr::deinterleave162(symd);
    // decisions, reliabilities, bit-planes
    uint32_t plane[kPlanes][kCodeWords] = {}, hw[kCodeWords] = {};
    int rel[kN];
    for (int i = 0; i < kN; ++i) {
        rel[i] = reliab(symd[i]);
        if (hard(symd[i])) row_set(hw, i);
        for (int b = 0; b < kPlanes; ++b) if ((rel[i] >> b) & 1) row_set(plane[b], i);
    }
    // order: rank = number of positions that come first
    int ord[kN];
    for (int i = 0; i < kN; ++i) {
        int rank = 0;
        for (int j = 0; j < kN; ++j) rank += (rel[j] > rel[i] || (rel[j] == rel[i] && j < i)) ? 1 : 0;
        ord[rank] = i;
    }
    // most reliable basis: one row per lane, the lowest free lane with the bit set is the pivot
    uint32_t w[64][kRowWords] = {};
    bool used[64];
    int mypiv[64], pivpos[kK], npiv = 0;
    for (int l = 0; l < 64; ++l) { used[l] = l >= kK; mypiv[l] = -1; }
    for (int j = 0; j < kK; ++j) {
        unsigned char d[11] = {0}, code[176];
        d[j >> 3] = (unsigned char)(0x80u >> (j & 7));
        wspr::conv_encode(code, d, 11);
        pack_generator_row(code, j, w[j]);
    }
    for (int t = 0; t < kN && npiv < kK; ++t) {
        const int p = ord[t];
        int pl = -1;
        for (int l = 0; l < 64 && pl < 0; ++l) if (!used[l] && row_bit(w[l], p)) pl = l;
        if (pl < 0) continue;
        for (int l = 0; l < 64; ++l)
            if (l != pl && row_bit(w[l], p)) for (int k = 0; k < kRowWords; ++k) w[l][k] ^= w[pl][k];
        used[pl] = true; mypiv[pl] = npiv; pivpos[npiv] = p; ++npiv;
    }
    if (npiv != kK) return -2;
    uint32_t rows[kK * kRowWords];
    for (int l = 0; l < 64; ++l) if (mypiv[l] >= 0) memcpy(rows + mypiv[l] * kRowWords, w[l], sizeof w[l]);
    // c_0 and e_0 = c_0 XOR h
    uint32_t c0[kRowWords] = {}, e0[kCodeWords];
    for (int l = 0; l < 64; ++l)
        if (mypiv[l] >= 0 && symd[pivpos[mypiv[l]]] >= 128) for (int k = 0; k < kRowWords; ++k) c0[k] ^= w[l][k];
    for (int k = 0; k < kCodeWords; ++k) e0[k] = c0[k] ^ hw[k];
    // trials, lane by lane
    unsigned short pairs[kPairs];
    for (int lane = 0; lane < kK - 1; ++lane)
        for (int b = lane + 1, q = pair_base(lane); b < kK; ++b, ++q) pairs[q] = (unsigned short)((lane << 8) | b);
    uint64_t best_all = ~0ull;
    for (int lane = 0; lane < 64; ++lane) {
        uint64_t best = ~0ull;
        if (lane == 0) best = pack_key(cost(e0, plane), 0u, 0u, 0u, 0u);
        if (depth >= 1 && lane < kK) {
            uint32_t e[kCodeWords];
            for (int k = 0; k < kCodeWords; ++k) e[k] = e0[k] ^ rows[lane * kRowWords + k];
            best = std::min(best, pack_key(cost(e, plane), 1u, (unsigned)lane, 0u, 0u));
        }
        if (depth >= 2)
            for (int q = lane; q < kPairs; q += 64) {
                const unsigned ab = pairs[q], a = ab >> 8, b = ab & 255u;
                uint32_t e2[kCodeWords];
                for (int k = 0; k < kCodeWords; ++k) e2[k] = e0[k] ^ rows[a * kRowWords + k] ^ rows[b * kRowWords + k];
                best = std::min(best, pack_key(cost(e2, plane), 2u, a, b, 0u));
                if (depth >= 3)
                    for (unsigned c = b + 1; c < (unsigned)kK; ++c) {
                        uint32_t e3[kCodeWords];
                        for (int k = 0; k < kCodeWords; ++k) e3[k] = e2[k] ^ rows[c * kRowWords + k];
                        best = std::min(best, pack_key(cost(e3, plane), 3u, a, b, c));
                    }
            }
        best_all = std::min(best_all, best);
    }
    // the winner once more
    const unsigned ordw = key_order(best_all);
    uint32_t win[kRowWords], ew[kCodeWords];
    for (int k = 0; k < kRowWords; ++k) {
        win[k] = c0[k];
        for (unsigned e = 0; e < ordw; ++e) win[k] ^= rows[key_elem(best_all, (int)e) * kRowWords + k];
    }
    for (int k = 0; k < kCodeWords; ++k) ew[k] = win[k] ^ hw[k];
    for (int k = 0; k < 11; ++k) data11[k] = (unsigned char)message_byte(win, k);
    *dist = key_dist(best_all); *nhard = hamming(ew); *order_out = ordw;
    return 0;
}
