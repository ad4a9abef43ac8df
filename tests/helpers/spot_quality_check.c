/* Serial statement of the decode-quality figures of a spot (rtlsdr-wsprd_amd/csrc/kernels/spot_quality.h), in plain C:
 * what the kernel K19 is held to, field for field (tests/test_gpu_spot_quality.py).  It shares no code with the library:
 * the encoder is the shift register written out bit by bit, the interleaver the bit-reversed counter.
 *
 *   gcc -O2 -std=c11 -shared -fPIC -o spot_quality_check.so spot_quality_check.c
 */
#include <stdint.h>
#include <string.h>

#define N 162

static unsigned parity(uint32_t v) {
    unsigned p = 0;
    while (v) { p ^= v & 1u; v >>= 1; }
    return p;
}

/* c[i], i = 0 .. 161 in transmission order: encode() + interleave() of the 50 message bits of decdata and 31 zero bits */
void spot_quality_codeword(const unsigned char *decdata, unsigned char *c) {
    unsigned char coded[N], sent[N];
    uint32_t state = 0;
    int j, i, p = 0;
    for (j = 0; j < 81; ++j) {
        const unsigned bit = j < 50 ? (decdata[j >> 3] >> (7 - (j & 7))) & 1u : 0u;
        state = (state << 1) | bit;
        coded[2 * j] = (unsigned char)parity(state & 0xf2d05351u);
        coded[2 * j + 1] = (unsigned char)parity(state & 0xe4613c47u);
    }
    for (i = 0; i < 256 && p < N; ++i) {
        unsigned rev = 0;
        int b;
        for (b = 0; b < 8; ++b) rev |= (((unsigned)i >> b) & 1u) << (7 - b);
        if (rev < N) sent[rev] = coded[p++];
    }
    memcpy(c, sent, N);
}

/* n jobs: symbols n x 162 (transmission order), decdata n x 11, mettab [2][256] -> out n x 5 (nhard, dist, rsum, v2,
 * metric).  Returns 0; -1 with nothing written for n < 0. */
int spot_quality_check(const unsigned char *symbols, const unsigned char *decdata, int n, const int *mettab, int32_t *out) {
    int k, i;
    if (n < 0) return -1;
    for (k = 0; k < n; ++k) {
        const unsigned char *s = symbols + (size_t)k * N;
        unsigned char c[N];
        int32_t nhard = 0, dist = 0, rsum = 0, v2 = 0, metric = 0;
        spot_quality_codeword(decdata + (size_t)k * 11, c);
        for (i = 0; i < N; ++i) {
            const int h = s[i] >= 128, v = 2 * (int)s[i] - 255, r = v < 0 ? -v : v;
            if (h != c[i]) { nhard += 1; dist += r; }
            rsum += r;
            v2 += v * v;
            metric += mettab[256 * c[i] + s[i]];
        }
        out[5 * k + 0] = nhard; out[5 * k + 1] = dist; out[5 * k + 2] = rsum; out[5 * k + 3] = v2; out[5 * k + 4] = metric;
    }
    return 0;
}
