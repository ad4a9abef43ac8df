/* List decoding against known messages, the serial statement of rtlsdr-wsprd_amd/csrc/kernels/listmatch.h in plain C:
 * what the kernel K14 (k14_list.hip) is held to, field for field.  Nothing is shared with the product: the definition is
 * written out once more, one multiplication at a time.
 *
 *   entry m    162 channel symbols 0..3 in transmission order;  c[i] = 2 * (symbol[i] >> 1) - 1
 *   vector     162 soft symbols s[i] in transmission order;     v[i] = 2 * s[i] - 255
 *   S(m)       sum of c_m[i] * v[i]
 *   winner     largest S, ties to the lower index;  second = largest S among all other entries, INT32_MIN if there is none
 *   V          sum of v[i]^2
 *   gate       S1 > 0 and 256 * S1^2 >= zmin16^2 * V, in 64-bit integers
 *
 * cc -O2 -shared -fPIC -o list_check.so list_check.c            (tests/list_lib.py)
 * cc -O1 -g -fsanitize=address,undefined -DLIST_CHECK_MAIN -o list_check list_check.c && ./list_check     (stand-alone) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#define LIST_N 162

/* out[4 * t + 0..3] = index, score, second, v2 of vector t; returns 0, or -1 for m < 1 or n < 0 */
int list_check(const unsigned char *entries, int m, const unsigned char *vectors, int n, int32_t *out) {
    if (m < 1 || n < 0) return -1;
    for (int t = 0; t < n; ++t) {
        const unsigned char *s = vectors + (size_t)t * LIST_N;
        int32_t best = 0, second = INT32_MIN, index = -1, v2 = 0;
        for (int i = 0; i < LIST_N; ++i) {
            const int32_t v = 2 * (int32_t)s[i] - 255;
            v2 += v * v;
        }
        for (int e = 0; e < m; ++e) {
            const unsigned char *sym = entries + (size_t)e * LIST_N;
            int32_t score = 0;
            for (int i = 0; i < LIST_N; ++i) {
                const int32_t c = 2 * (int32_t)(sym[i] >> 1) - 1;
                score += c * (2 * (int32_t)s[i] - 255);
            }
            if (index < 0) {
                index = e; best = score;
            } else if (score > best) {               /* strictly larger: an equal score leaves the lower index in place */
                second = best;
                index = e; best = score;
            } else if (score > second) {
                second = score;
            }
        }
        out[4 * t + 0] = index; out[4 * t + 1] = best; out[4 * t + 2] = second; out[4 * t + 3] = v2;
    }
    return 0;
}

int list_gate(int32_t s1, int32_t v2, int zmin16) {
    if (s1 <= 0) return 0;
    return 256 * (int64_t)s1 * (int64_t)s1 >= (int64_t)zmin16 * (int64_t)zmin16 * (int64_t)v2 ? 1 : 0;
}

#ifdef LIST_CHECK_MAIN
/* A run of the checker on pseudo-random entries and vectors, for a sanitizer build: prints a checksum. */
int main(void) {
    enum { M = 300, NV = 70 };
    unsigned char *entries = malloc((size_t)M * LIST_N), *vectors = malloc((size_t)NV * LIST_N);
    int32_t *out = malloc((size_t)NV * 4 * sizeof(int32_t));
    if (!entries || !vectors || !out) return 2;
    uint32_t x = 12345u;
    for (int i = 0; i < M * LIST_N; ++i) { x = x * 1664525u + 1013904223u; entries[i] = (unsigned char)((x >> 24) & 3u); }
    for (int i = 0; i < NV * LIST_N; ++i) { x = x * 1664525u + 1013904223u; vectors[i] = (unsigned char)(x >> 24); }
    for (int i = 0; i < LIST_N; ++i) {               /* the extremes: all 0, all 255, a clean code word and its complement */
        vectors[i] = 0; vectors[LIST_N + i] = 255;
        vectors[2 * LIST_N + i] = (entries[7 * LIST_N + i] >> 1) ? 255 : 0;
        vectors[3 * LIST_N + i] = (entries[7 * LIST_N + i] >> 1) ? 0 : 255;
    }
    if (list_check(entries, M, vectors, NV, out) != 0 || list_check(entries, 0, vectors, NV, out) != -1) return 1;
    if (out[4 * 2] != 7 || out[4 * 2 + 1] != 41310 || out[4 * 2 + 3] != 10534050 || !list_gate(out[4 * 2 + 1], out[4 * 2 + 3], 203)) return 1;
    if (list_check(entries, 1, vectors, NV, out + 0) != 0 || out[2] != INT32_MIN) return 1;
    uint32_t sum = 0;
    for (int i = 0; i < NV * 4; ++i) sum = sum * 31u + (uint32_t)out[i];
    printf("list_check ok %08x\n", sum);
    free(entries); free(vectors); free(out);
    return 0;
}
#endif
