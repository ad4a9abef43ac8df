// CPU checker of the ordered-statistics decoder (rtlsdr-wsprd_amd/csrc/kernels/osd.h states the definition): the same
// decode written serially, one byte per bit, with none of the kernel's structure -- no packed rows, no bit-planes, no
// packed keys.  The kernel K9 (k9_osd.hip) must reproduce every output field of osd_check() exactly, and
// tests/test_osd_checker.py holds this file to an independent numpy statement of the definition.
// Also here: the "heard before" gate of the message layer (wspr::osd_accept) over the reference's flat tables, so that it
// is testable without a GPU.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../rtlsdr-wsprd_amd/csrc/host/wspr_message.cpp"
#include "../../rtlsdr-wsprd_amd/csrc/kernels/osd.h"

using namespace wspr;

namespace {
constexpr int N = osd::kN, K = osd::kK;

struct Code { unsigned char g[K][N]; };
const Code& code() {                                         // row j: the encoder's first 162 outputs for message bit j alone
    static const Code c = [] {
        Code t;
        for (int j = 0; j < K; ++j) {
            unsigned char data[11] = {0}, out[176];
            data[j >> 3] = (unsigned char)(0x80u >> (j & 7));
            conv_encode(out, data, 11);
            memcpy(t.g[j], out, N);
        }
        return t;
    }();
    return c;
}

struct Best { unsigned d; int order; int t[3]; bool set; };
// the winner's rule: smaller D, then smaller |T|, then the lexicographically smaller ascending tuple
bool better(unsigned d, int order, const int* t, const Best& b) {
    if (!b.set) return true;
    if (d != b.d) return d < b.d;
    if (order != b.order) return order < b.order;
    for (int i = 0; i < order; ++i) if (t[i] != b.t[i]) return t[i] < b.t[i];
    return false;
}
}  // namespace

// symbols: 162 soft symbols in transmission (interleaved) order, as wspr_osd_batch_device() takes them.
// Returns 0, or -1 for a depth outside 0..3.
extern "C" int osd_check(const unsigned char* symbols, int depth, unsigned char* data11, unsigned* dist, unsigned* nhard,
                         unsigned* order_out) {
    if (depth < 0 || depth > osd::kMaxDepth) return -1;
    unsigned char s[N];
    memcpy(s, symbols, N);
    deinterleave162(s);
    int h[N], r[N];
    for (int i = 0; i < N; ++i) { h[i] = osd::hard(s[i]); r[i] = osd::reliab(s[i]); }
    // order: r descending, ties to the lower index (insertion sort: stable by construction)
    int ord[N];
    for (int i = 0; i < N; ++i) {
        int k = i;
        while (k > 0 && r[ord[k - 1]] < r[i]) { ord[k] = ord[k - 1]; --k; }
        ord[k] = i;
    }
    // most reliable basis: Gauss-Jordan on a copy of G, message bits carried along (columns N .. N+K-1)
    std::vector<std::vector<unsigned char>> row(K, std::vector<unsigned char>(N + K, 0));
    for (int j = 0; j < K; ++j) { memcpy(row[j].data(), code().g[j], N); row[j][N + j] = 1; }
    int piv[K], npiv = 0;
    for (int t = 0; t < N && npiv < K; ++t) {
        const int p = ord[t];
        int f = -1;
        for (int j = npiv; j < K; ++j) if (row[j][p]) { f = j; break; }
        if (f < 0) continue;                                 // depends on the columns already kept
        std::swap(row[npiv], row[f]);
        for (int j = 0; j < K; ++j)
            if (j != npiv && row[j][p])
                for (int i = 0; i < N + K; ++i) row[j][i] ^= row[npiv][i];
        piv[npiv++] = p;                                     // row npiv of G~: 1 at p_npiv, 0 at every other kept position
    }
    if (npiv != K) return -2;                                // the code has rank 50: not reached
    // c_0
    std::vector<unsigned char> c0(N + K, 0);
    for (int k = 0; k < K; ++k)
        if (h[piv[k]]) for (int i = 0; i < N + K; ++i) c0[i] ^= row[k][i];
    auto cost_of = [&](const unsigned char* c) { unsigned d = 0; for (int i = 0; i < N; ++i) if (c[i] != h[i]) d += (unsigned)r[i]; return d; };
    Best best{0, 0, {0, 0, 0}, false};
    auto consider = [&](const unsigned char* c, int order, int a, int b, int cc) {
        const int t[3] = {a, b, cc};
        const unsigned d = cost_of(c);
        if (better(d, order, t, best)) best = Best{d, order, {a, b, cc}, true};
    };
    consider(c0.data(), 0, 0, 0, 0);
    std::vector<unsigned char> c1(N + K), c2(N + K), c3(N + K);
    if (depth >= 1)
        for (int a = 0; a < K; ++a) {
            for (int i = 0; i < N + K; ++i) c1[i] = c0[i] ^ row[a][i];
            consider(c1.data(), 1, a, 0, 0);
            if (depth >= 2)
                for (int b = a + 1; b < K; ++b) {
                    for (int i = 0; i < N + K; ++i) c2[i] = c1[i] ^ row[b][i];
                    consider(c2.data(), 2, a, b, 0);
                    if (depth >= 3)
                        for (int c = b + 1; c < K; ++c) {
                            for (int i = 0; i < N + K; ++i) c3[i] = c2[i] ^ row[c][i];
                            consider(c3.data(), 3, a, b, c);
                        }
                }
        }
    // the winner once more, for its message and its Hamming distance
    std::vector<unsigned char> w = c0;
    for (int e = 0; e < best.order; ++e) for (int i = 0; i < N + K; ++i) w[i] ^= row[best.t[e]][i];
    unsigned nh = 0;
    for (int i = 0; i < N; ++i) nh += w[i] != h[i];
    memset(data11, 0, 11);
    for (int m = 0; m < K; ++m) if (w[N + m]) data11[m >> 3] |= (unsigned char)(0x80u >> (m & 7));
    *dist = best.d; *nhard = nh; *order_out = (unsigned)best.order;
    return 0;
}

// The gate over the reference's flat tables (hashtab[32768][13], loctab[32768][5]): 1 accepted, 0 refused.
extern "C" int osd_gate(const unsigned char* decdata11, char* hashtab, char* loctab) {
    FlatHashTable tab(hashtab, loctab);
    return osd_accept(decdata11, tab) ? 1 : 0;
}
