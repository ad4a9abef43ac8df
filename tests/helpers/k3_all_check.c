/* TEST INFRASTRUCTURE ONLY: the coarse sync search (wsprd.c:646-678) of ONE candidate with every hypothesis kept.
 * The loops, expressions and their order are those of oracle/orc_dsp.c: orc_coarse_sync(); where that function compares
 * `sync > best`, this one stores `sync` -- including the value carried over from the previous hypothesis when no symbol
 * of a short record lies inside it (sync is assigned inside `if (kidx < blocks)` only).  The first strict maximum of
 * the table is therefore orc_coarse_sync()'s pick; tests/k2k3_lib.py takes it and tests/test_k2k3_cases_cpu.py holds it
 * to the oracle.  Built on demand by tests/k2k3_lib.py (gcc -O2 -ffp-contract=off against liboracle.so, for the sync
 * vector). */
#include <math.h>

#include "wspr_oracle.h"

static const double kHalfDf = 375.0 / 256.0 / 2.0;         /* (DF / 2.0) */

/* table[3][32][2 maxdrift + 1] in loop order (ifr, k0, idr); inside[...] (may be null): symbols with kidx < blocks.
 * Returns if0. */
int k3_all(const float *ps, int blocks, float freq, int maxdrift, float *table, int *inside) {
    const unsigned char *pr3 = orc_sync_vector;
    float sync = 0.0f;
    int n = 0;
    int if0 = freq / kHalfDf + ORC_SPS;
    for (int ifr = if0 - 1; ifr <= if0 + 1; ifr++) {
        for (int k0 = -10; k0 < 22; k0++) {
            for (int idr = -maxdrift; idr <= maxdrift; idr++) {
                float ss = 0.0f, pw = 0.0f;
                int in = 0;
                for (int k = 0; k < ORC_NSYM; k++) {
                    int ifd = ifr + ((float)k - (float)ORC_NBITS) / (float)ORC_NBITS
                                        * ((float)idr) / 375.0 / 256.0;
                    int kidx = k0 + 2 * k;
                    if (kidx < blocks) {
                        long o = (long)kidx;
                        float p0 = sqrtf(ps[(long)(ifd - 3) * blocks + o]);
                        float p1 = sqrtf(ps[(long)(ifd - 1) * blocks + o]);
                        float p2 = sqrtf(ps[(long)(ifd + 1) * blocks + o]);
                        float p3 = sqrtf(ps[(long)(ifd + 3) * blocks + o]);
                        ss = ss + (2 * pr3[k] - 1) * ((p1 + p3) - (p0 + p2));
                        pw = pw + p0 + p1 + p2 + p3;
                        sync = ss / pw;
                        in++;
                    }
                }
                table[n] = sync;
                if (inside) inside[n] = in;
                n++;
            }
        }
    }
    return if0;
}
