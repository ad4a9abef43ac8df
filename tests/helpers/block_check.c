/* ============================================================================
 * block_check.c -- CPU CHECKER OF THE NONCOHERENT BLOCK DETECTION (TEST INFRASTRUCTURE)
 *
 * The definition of rtlsdr-wsprd_amd/csrc/kernels/blockdemod.h, stated once more in serial C: for one hypothesis
 * (freq, shift, drift) the complex tone sums of sync_and_demodulate() mode 2 (wsprd.c:158-207), the phase advance of
 * every tone over every symbol, and from them the soft-symbol vectors of block sizes 1, 2 and 3 with their rms, and
 * the hypothesis' mode-2 sync.  The kernel (k10_blockdemod.hip) is held to this file byte for byte.
 *
 * Built twice, as tests/helpers/contract_dsp.c is: CONTRACT=0 separately rounded operations (the exact mode),
 * CONTRACT=1 the fusions clang's -ffp-contract=on makes in the statements as the definition writes them.  Every
 * site goes through one macro; the sites of the tone sums are contract_dsp.c's (its table), the combine adds
 *
 *   xi  = xi + is*cm + qs*sm          MAD(qs, sm, MAD(is, cm, xi))
 *   xq  = xq + qs*cm - is*sm          NMAD(is, sm, MAD(qs, cm, xq))
 *   cmp = cf*cm - sf*sm               MMS(cf, cm, sf, sm)
 *   smp = sf*cm + cf*sm               MMA(sf, cm, cf, sm)
 *   p   = sqrt(xi*xi + xq*xq)         MMA(xi, xi, xq, xq)
 *
 * At block size 1 the vector is mode 2's (tests/test_block_checker.py pins it to the oracle, to contract_dsp.c and,
 * where it is built, to the compiled reference).  Build with -ffp-contract=off.
 * ==========================================================================*/
#include "wspr_oracle.h"

#include <math.h>
#include <string.h>

#ifndef CONTRACT
#error "build with -DCONTRACT=0 or -DCONTRACT=1"
#endif

#if CONTRACT
#define MAD(a, b, c)     fmaf((a), (b), (c))                       /* a*b + c, one rounding */
#define NMAD(a, b, c)    fmaf(-(a), (b), (c))                      /* c - a*b */
#define MMA(a, b, c, d)  fmaf((a), (b), (c) * (d))                 /* a*b + c*d, left product fused */
#define MMS(a, b, c, d)  fmaf((a), (b), -((c) * (d)))              /* a*b - c*d */
#else
#define MAD(a, b, c)     ((a) * (b) + (c))
#define NMAD(a, b, c)    ((c) - (a) * (b))
#define MMA(a, b, c, d)  ((a) * (b) + (c) * (d))
#define MMS(a, b, c, d)  ((a) * (b) - (c) * (d))
#endif

static const double kTwoPiDt = 2.0 * M_PI * 1.0 / 375.0;    /* TWOPIDT */
static const double kDf05    = 375.0 / 256.0 * 0.5;         /* DF05    */
static const double kDf15    = 375.0 / 256.0 * 1.5;         /* DF15    */

static unsigned char soft_to_u8(float v) {
    if (v != v) return 0;              /* NaN -> 0, as the mode-2 quantiser */
    return (unsigned char)(int)v;
}

/* fsymb[162] -> bytes and rms, wsprd.c:243-256 and the ladder's rms (:752-757) */
static void quantise(const float *fsymb, unsigned char *symbols, float *rms) {
    const int symfac = 50;
    float fsum = 0.0f, f2sum = 0.0f;
    for (int i = 0; i < ORC_NSYM; i++) {
        fsum  += fsymb[i] / ORC_NSYM;
        f2sum += fsymb[i] * fsymb[i] / ORC_NSYM;
    }
    float var = NMAD(fsum, fsum, f2sum);
    float fac = sqrtf(var);
    float sq = 0.0f;
    for (int i = 0; i < ORC_NSYM; i++) {
        float v = symfac * fsymb[i] / fac;
        if (v > 127) v = 127.0f;
        if (v < -128) v = -128.0f;
        symbols[i] = soft_to_u8(v + 128);
        float y = (float)symbols[i] - 128.0;
        sq += y * y;
    }
    *rms = sqrtf(sq / (float)ORC_NSYM);
}

/* sums (may be NULL): [162][4][4] = (is, qs, cf, sf) per symbol and tone; symbols [3][162]; rms [3]; *sync */
int blk_demod(const float *id, const float *qd, long np, float freq, int shift, float drift,
              float *sums, unsigned char *symbols, float *rms, float *sync) {
    const unsigned char *pr3 = orc_sync_vector;
    float is[ORC_NSYM][4], qs[ORC_NSYM][4], cf[ORC_NSYM][4], sf[ORC_NSYM][4];
    float ct[4][ORC_SPS], st[4][ORC_SPS];
    float fsymb[ORC_NSYM];
    float ss = 0.0f, totp = 0.0f;
    const float f0 = freq;

    /* ---- tone sums and advances: wsprd.c:158-207 ------------------------------------------------------------------ */
    for (int i = 0; i < ORC_NSYM; i++) {
        float fp = f0 + (drift / 2.0) * ((float)i - (float)ORC_NBITS) / (float)ORC_NBITS;
        float dphi[4];
        dphi[0] = kTwoPiDt * (fp - kDf15);
        dphi[1] = kTwoPiDt * (fp - kDf05);
        dphi[2] = kTwoPiDt * (fp + kDf05);
        dphi[3] = kTwoPiDt * (fp + kDf15);
        for (int t = 0; t < 4; t++) {
            float cd = cosf(dphi[t]), sd = sinf(dphi[t]);
            ct[t][0] = 1.0f; st[t][0] = 0.0f;
            for (int j = 1; j < ORC_SPS; j++) {
                ct[t][j] = MMS(ct[t][j - 1], cd, st[t][j - 1], sd);
                st[t][j] = MMA(ct[t][j - 1], sd, st[t][j - 1], cd);
            }
            /* the recurrence one step past the table's last entry: the phase the tone gains over the symbol */
            cf[i][t] = MMS(ct[t][ORC_SPS - 1], cd, st[t][ORC_SPS - 1], sd);
            sf[i][t] = MMA(ct[t][ORC_SPS - 1], sd, st[t][ORC_SPS - 1], cd);
        }
        float ai[4] = {0, 0, 0, 0}, aq[4] = {0, 0, 0, 0};
        for (int j = 0; j < ORC_SPS; j++) {
            long k = (long)shift + i * ORC_SPS + j;
            if (k > 0 && k < np) {
                float x = id[k], y = qd[k];
                for (int t = 0; t < 4; t++) {
                    ai[t] = MAD(y, st[t][j], MAD(x, ct[t][j], ai[t]));
                    aq[t] = MAD(y, ct[t][j], NMAD(x, st[t][j], aq[t]));
                }
            }
        }
        float p[4];
        for (int t = 0; t < 4; t++) {
            is[i][t] = ai[t]; qs[i][t] = aq[t];
            p[t] = sqrtf(MMA(ai[t], ai[t], aq[t], aq[t]));
        }
        totp = totp + p[0] + p[1] + p[2] + p[3];
        float cmet = (p[1] + p[3]) - (p[0] + p[2]);
        ss = (pr3[i] == 1) ? ss + cmet : ss - cmet;
    }
    ss = ss / totp;
    *sync = (ss > -1e30f) ? ss : -1e30f;                       /* syncmax starts at -1e30 (wsprd.c:143, :228) */
    if (sums)
        for (int i = 0; i < ORC_NSYM; i++)
            for (int t = 0; t < 4; t++) {
                float *o = sums + ((size_t)i * 4 + t) * 4;
                o[0] = is[i][t]; o[1] = qs[i][t]; o[2] = cf[i][t]; o[3] = sf[i][t];
            }

    /* ---- combine, block sizes 1, 2, 3 ----------------------------------------------------------------------------- */
    for (int B = 1; B <= 3; B++) {
        const int nseq = 1 << B;
        for (int i0 = 0; i0 < ORC_NSYM; i0 += B) {
            float p[8];
            for (int j = 0; j < nseq; j++) {
                float xi = 0.0f, xq = 0.0f, cm = 1.0f, sm = 0.0f;
                for (int ib = 0; ib < B; ib++) {
                    const int i = i0 + ib, b = (j >> (B - 1 - ib)) & 1, t = pr3[i] + 2 * b;
                    xi = MAD(qs[i][t], sm, MAD(is[i][t], cm, xi));
                    xq = NMAD(is[i][t], sm, MAD(qs[i][t], cm, xq));
                    float cmp = MMS(cf[i][t], cm, sf[i][t], sm);
                    float smp = MMA(sf[i][t], cm, cf[i][t], sm);
                    cm = cmp; sm = smp;
                }
                p[j] = sqrtf(MMA(xi, xi, xq, xq));
            }
            for (int ib = 0; ib < B; ib++) {
                float xm1 = 0.0f, xm0 = 0.0f;
                for (int j = 0; j < nseq; j++) {
                    if ((j >> (B - 1 - ib)) & 1) { if (p[j] > xm1) xm1 = p[j]; }
                    else                         { if (p[j] > xm0) xm0 = p[j]; }
                }
                fsymb[i0 + ib] = xm1 - xm0;
            }
        }
        quantise(fsymb, symbols + (size_t)(B - 1) * ORC_NSYM, &rms[B - 1]);
    }
    return 0;
}
