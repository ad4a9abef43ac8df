/* ============================================================================
 * contract_dsp.c -- CPU CHECKER OF THE CONTRACTED ARITHMETIC (TEST INFRASTRUCTURE)
 *
 * wspr_set_arithmetic(WSPR_ARITH_CONTRACTED) evaluates the fusions that clang's
 * front end makes in the reference's wsprd/wsprd.c under its default
 * -ffp-contract=on, and no others.  clang fuses within one expression, the left
 * product first.  This file restates the oracle's (oracle/orc_dsp.c) functions
 * that hold such a site, and writes every site through one macro:
 *
 *   wsprd.c line   statement                                   macro form
 *   151            f0 = *freq + ifreq*fstep                     MAD(ifreq, fstep, *freq)
 *   180-187        c[j] = c*cd - s*sd ; s[j] = c*sd + s*cd      MMS(c, cd, s, sd) ; MMA(c, sd, s, cd)
 *   200-207        i = i + id*c + qd*s ; q = q - id*s + qd*c    MAD(qd, s, MAD(id, c, i)) ; MAD(qd, c, NMAD(id, s, q))
 *   211-214        sqrt(i*i + q*q)                              MMA(i, i, q, q)
 *   249            sqrt(f2sum - fsum*fsum)                      NMAD(fsum, fsum, f2sum)
 *   378-379        id*refi + qd*refq ; qd*refi - id*refq        MMA(...) ; MMS(...)
 *   388-389        cfi = cfi + w*ci                             MAD(w, ci, cfi)
 *   408-409        cfi*refi - cfq*refq ; cfi*refq + cfq*refi    MMS(...) ; MMA(...)  (then / norm)
 *   551            re*re + im*im                                MMA(re, re, im, im)
 * (516, 571, 616, 663 and 754 fuse integer-valued products: exact either way, not restated.)
 *
 * CONTRACT=1: each macro is one fmaf() (a single rounding).  CONTRACT=0: the same
 * expression as two separately rounded operations, which is the oracle's
 * arithmetic; tests/test_contract_checker.py pins the CONTRACT=0 build to
 * orc_wspr_decode byte for byte, so only the sites differ between the two builds.
 * Everything without a site (the FFT butterflies, peak picking, coarse sync,
 * Fano, the message layer) is oracle/liboracle.so's, linked, not restated.
 *
 * PIN.  The table above is pinned to the reference's own wsprd.c as clang compiles it with
 * -ffp-contract=on -mfma (oracle/Makefile: _ref/libwsprd_dsp_ref_fma.so, the oracle's FFT behind an
 * <fftw3.h> stand-in): the CONTRACT=1 build gives that library's spots and residual IQ bit for bit
 * (tests/test_reference_pin.py), so the table is right and complete for wspr_decode,
 * sync_and_demodulate and subtract_signal2.  Two limits: site 249 feeds only the truncation of the
 * soft symbols to bytes, where one rounding is all but invisible; and subtract_signal()
 * (wsprd.c:263-312, never called by the decoder) has no site here although clang fuses inside it.
 *
 * Build with -ffp-contract=off so that the host compiler adds no fusion of its own.
 * ==========================================================================*/
#include "wspr_oracle.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
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

static int cmp_spot_snr_desc(const void *a, const void *b) {   /* wsprd.c:53-57 */
    float x = ((const orc_spot *)a)->snr, y = ((const orc_spot *)b)->snr;
    return (x < y) - (x > y);
}

/* wsprd.c:509-553 (site 551) */
void ctr_fft_bank(const float *idat, const float *qdat, int samples, float *ps) {
    const int blocks = orc_blocks_for(samples);
    float win[ORC_FFT];
    for (int j = 0; j < ORC_FFT; j++) win[j] = sinf(0.006147931 * j);
    float xr[ORC_FFT], xi[ORC_FFT];
    for (int t = 0; t < blocks; t++) {
        for (int j = 0; j < ORC_FFT; j++) {
            int k = t * 128 + j;
            xr[j] = idat[k] * win[j];
            xi[j] = qdat[k] * win[j];
        }
        orc_fft512(xr, xi);
        for (int j = 0; j < ORC_FFT; j++) {
            int k = (j + ORC_FFT / 2) & (ORC_FFT - 1);
            ps[(size_t)j * blocks + t] = MMA(xr[k], xr[k], xi[k], xi[k]);
        }
    }
}

static inline unsigned char soft_to_u8(float v) {
    if (v != v) return 0;              /* NaN: x86 cvttss2si -> 0x80000000 -> low byte 0 */
    return (unsigned char)(int)v;
}

/* wsprd.c:101-259 (sites 151, 180-187, 200-207, 211-214, 249) */
void ctr_sync_demod(const float *id, const float *qd, long np, unsigned char *symbols,
                    float *freq, int ifmin, int ifmax, float fstep,
                    int *shift, int lagmin, int lagmax, int lagstep,
                    const float *drift, int symfac, float *sync, int mode) {
    const unsigned char *pr3 = orc_sync_vector;
    float ct[4][ORC_SPS], st[4][ORC_SPS];
    float fsymb[ORC_NSYM];
    float syncmax = -1e30f, fbest = 0.0f;
    int   best_shift = 0;

    if (mode == 0) { ifmin = 0; ifmax = 0; fstep = 0.0f; }
    else if (mode == 1) { lagmin = *shift; lagmax = *shift; }
    else if (mode == 2) { lagmin = *shift; lagmax = *shift; ifmin = 0; ifmax = 0; }

    for (int ifreq = ifmin; ifreq <= ifmax; ifreq++) {
        float f0 = MAD((float)ifreq, fstep, *freq);
        for (int lag = lagmin; lag <= lagmax; lag += lagstep) {
            float ss = 0.0f, totp = 0.0f;
            float fplast = 0.0f;
            for (int i = 0; i < ORC_NSYM; i++) {
                float fp = f0 + (*drift / 2.0) * ((float)i - (float)ORC_NBITS) / (float)ORC_NBITS;
                if (i == 0 || fp != fplast) {
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
                    }
                    fplast = fp;
                }
                float ai[4] = {0, 0, 0, 0}, aq[4] = {0, 0, 0, 0};
                for (int j = 0; j < ORC_SPS; j++) {
                    int k = lag + i * ORC_SPS + j;
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
                    float e = MMA(ai[t], ai[t], aq[t], aq[t]);
                    p[t] = sqrt(e);
                }
                totp = totp + p[0] + p[1] + p[2] + p[3];
                float cmet = (p[1] + p[3]) - (p[0] + p[2]);
                ss = (pr3[i] == 1) ? ss + cmet : ss - cmet;
                if (mode == 2) fsymb[i] = (pr3[i] == 1) ? p[3] - p[1] : p[2] - p[0];
            }
            ss = ss / totp;
            if (ss > syncmax) { syncmax = ss; best_shift = lag; fbest = f0; }
        }
    }

    if (mode <= 1) {
        *sync = syncmax; *shift = best_shift; *freq = fbest;
        return;
    }
    *sync = syncmax;
    float fsum = 0.0f, f2sum = 0.0f;
    for (int i = 0; i < ORC_NSYM; i++) {
        fsum  += fsymb[i] / ORC_NSYM;
        f2sum += fsymb[i] * fsymb[i] / ORC_NSYM;
    }
    float var = NMAD(fsum, fsum, f2sum);
    float fac = sqrt(var);
    for (int i = 0; i < ORC_NSYM; i++) {
        float v = symfac * fsymb[i] / fac;
        if (v > 127) v = 127.0f;
        if (v < -128) v = -128.0f;
        symbols[i] = soft_to_u8(v + 128);
    }
}

/* wsprd.c:316-413 (sites 378-379, 388-389, 408-409) */
void ctr_subtract(float *id, float *qd, long np, float f0, int shift, float drift,
                  const unsigned char *cs) {
    enum { NF = 360, NS = ORC_MAXSAMPLES, NSIG = ORC_NSYM * ORC_SPS };
    float *buf = (float *)calloc((size_t)6 * NS, sizeof(float));
    if (!buf) return;
    float *refi = buf, *refq = buf + NS, *ci = buf + 2 * NS, *cq = buf + 3 * NS,
          *cfi = buf + 4 * NS, *cfq = buf + 5 * NS;

    float phi = 0.0f;
    for (int i = 0; i < ORC_NSYM; i++) {
        float s = (float)cs[i];
        float dphi = kTwoPiDt * (f0 + (drift / 2.0) * ((float)i - (float)ORC_NSYM / 2.0)
                                      / ((float)ORC_NSYM / 2.0) + (s - 1.5) * 375.0 / 256.0);
        for (int j = 0; j < ORC_SPS; j++) {
            int n = ORC_SPS * i + j;
            refi[n] = cosf(phi);
            refq[n] = sinf(phi);
            phi = phi + dphi;
        }
    }

    float w[NF], part[NF], norm = 0.0f;
    for (int i = 0; i < NF; i++) {
        w[i] = sinf(M_PI * (float)i / (float)(NF - 1));
        norm = norm + w[i];
    }
    for (int i = 0; i < NF; i++) w[i] = w[i] / norm;
    part[0] = 0.0f;
    for (int i = 1; i < NF; i++) part[i] = part[i - 1] + w[i];

    for (int i = 0; i < NSIG; i++) {
        int k = shift + i;
        if (k > 0 && k < np) {
            ci[i + NF] = MMA(id[k], refi[i], qd[k], refq[i]);
            cq[i + NF] = MMS(qd[k], refi[i], id[k], refq[i]);
        }
    }
    for (int i = NF / 2; i < NS - NF / 2; i++) {
        float si = 0.0f, sq = 0.0f;
        for (int j = 0; j < NF; j++) {
            si = MAD(w[j], ci[i - NF / 2 + j], si);
            sq = MAD(w[j], cq[i - NF / 2 + j], sq);
        }
        cfi[i] = si;
        cfq[i] = sq;
    }
    for (int i = 0; i < NSIG; i++) {
        if (i < NF / 2)                  norm = part[NF / 2 + i];
        else if (i > NSIG - 1 - NF / 2)  norm = part[NF / 2 + NSIG - 1 - i];
        else                             norm = 1.0f;
        int k = shift + i, j = i + NF;
        if (k > 0 && k < np) {
            float ri = MMS(cfi[j], refi[i], cfq[j], refq[i]);
            float rq = MMA(cfi[j], refq[i], cfq[j], refi[i]);
            id[k] = id[k] - ri / norm;
            qd[k] = qd[k] - rq / norm;
        }
    }
    free(buf);
}

/* ----------------------------------------------------------- orchestration -- */
/* wsprd.c:416-855, as oracle/orc_dsp.c states it, with the stages above */
int ctr_wspr_decode(float *idat, float *qdat, int samples, orc_options opt,
                    orc_spot *spots, int *n_results, orc_trace *tr);
int ctr_wspr_decode_stops(float *idat, float *qdat, int samples, orc_options opt,
                          orc_spot *spots, int *n_results, orc_trace *tr, orc_stops *st);
int ctr_wspr_decode(float *idat, float *qdat, int samples, orc_options opt,
                    orc_spot *spots, int *n_results, orc_trace *tr) {
    return ctr_wspr_decode_stops(idat, qdat, samples, opt, spots, n_results, tr, NULL);
}

int ctr_wspr_decode_stops(float *idat, float *qdat, int samples, orc_options opt,
                          orc_spot *spots, int *n_results, orc_trace *tr, orc_stops *st) {
    const float minsync1 = 0.10f;
    float minsync2 = 0.12f;
    const int iifac = 3, symfac = 50;
    int   maxdrift = 4;
    const float minrms = 52.0 * (symfac / 64.0);
    const int delta = 60;
    const unsigned maxcycles = 10000;

    int mettab[2][256];
    orc_build_mettab(mettab);

    char *hashtab = (char *)calloc((size_t)ORC_HASH_N * ORC_HASH_W, 1);
    char *loctab  = (char *)calloc((size_t)ORC_HASH_N * ORC_LOC_W, 1);
    if (opt.usehashtable) {                                   /* wsprd.c:481-494 */
        FILE *fh = fopen("hashtable.txt", "r+");
        if (fh) {
            char line[80], hcall[13], hgrid[5];
            int nh;
            while (fgets(line, sizeof line, fh) != NULL) {
                hgrid[0] = '\0';
                hcall[0] = '\0';
                if (sscanf(line, "%d %12s %4s", &nh, hcall, hgrid) < 2) continue;
                if (nh >= 0 && nh < ORC_HASH_N) {
                    snprintf(hashtab + nh * ORC_HASH_W, ORC_HASH_W, "%s", hcall);
                    if (strlen(hgrid) > 0) snprintf(loctab + nh * ORC_LOC_W, ORC_LOC_W, "%s", hgrid);
                }
            }
            fclose(fh);
        }
    }
    const int blocks = orc_blocks_for(samples);
    float *ps = (float *)calloc((size_t)ORC_FFT * (blocks > 0 ? blocks : 1), sizeof(float));
    orc_cand cand[ORC_MAXCAND];
    float allfreqs[ORC_MAXUNIQ];
    char  allcalls[ORC_MAXUNIQ][ORC_HASH_W];
    memset(allfreqs, 0, sizeof allfreqs);
    memset(allcalls, 0, sizeof allcalls);
    int uniques = 0;
    unsigned metric = 0, cycles = 0, maxnp = 0;
    unsigned char symbols[ORC_NSYM], decdata[11];
    signed char message[12];
    memset(symbols, 0, sizeof symbols);
    memset(decdata, 0, sizeof decdata);
    memset(message, 0, sizeof message);
    if (tr) { memset(tr, 0, sizeof *tr); tr->blocks = blocks; }
    if (st) memset(st, 0, sizeof *st);

    for (int ipass = 0; ipass < opt.npasses; ipass++) {
        if (ipass == 1 && uniques == 0) break;
        if (ipass < 2) { maxdrift = 4; minsync2 = 0.12f; }
        if (ipass == 2) { maxdrift = 0; minsync2 = 0.10f; }

        ctr_fft_bank(idat, qdat, samples, ps);
        float noise;
        int npk = orc_pick_peaks(ps, blocks, cand, &noise,
                                 (tr && ipass < ORC_TRACE_PASSES) ? tr->smspec_raw[ipass] : NULL, NULL);
        if (tr && ipass < ORC_TRACE_PASSES) {
            tr->passes_run = ipass + 1;
            tr->noise_level[ipass] = noise;
            tr->npk[ipass] = npk;
            memcpy(tr->cand_peaks[ipass], cand, sizeof cand);
        }
        orc_coarse_sync(ps, blocks, cand, npk, maxdrift);
        if (tr && ipass < ORC_TRACE_PASSES) memcpy(tr->cand_coarse[ipass], cand, sizeof cand);

        int stop = 0;
        for (int j = 0; j < npk && !stop; j++) {
            char callsign[ORC_HASH_W], call_loc_pow[23], call[ORC_HASH_W], loc[7], pwr[3];
            memset(callsign, 0, sizeof callsign);
            memset(call_loc_pow, 0, sizeof call_loc_pow);
            memset(call, 0, sizeof call);
            memset(loc, 0, sizeof loc);
            memset(pwr, 0, sizeof pwr);

            float freq = cand[j].freq, drift = cand[j].drift, sync = cand[j].sync;
            int   shift = cand[j].shift;
            int   lagmin = shift - 128, lagmax = shift + 128;
            int   lagstep = opt.quickmode ? 16 : 8;

            ctr_sync_demod(idat, qdat, samples, symbols, &freq, 0, 0, 0.0f, &shift,
                           lagmin, lagmax, lagstep, &drift, symfac, &sync, 0);
            if (tr && ipass < ORC_TRACE_PASSES) {
                tr->n_visited[ipass] = j + 1;
                tr->mode0_shift[ipass][j] = shift;
                tr->mode0_sync[ipass][j] = sync;
            }
            float fstep = 0.1;
            ctr_sync_demod(idat, qdat, samples, symbols, &freq, -2, 2, fstep, &shift,
                           lagmin, lagmax, lagstep, &drift, symfac, &sync, 1);
            cand[j].freq = freq; cand[j].shift = shift; cand[j].drift = drift; cand[j].sync = sync;
            if (tr && ipass < ORC_TRACE_PASSES) tr->cand_fine[ipass][j] = cand[j];

            int worth = (sync > minsync1);
            int idt = 0, ii = 0, not_decoded = 1;
            while (worth && not_decoded && idt <= (128 / iifac)) {
                ii = (idt + 1) / 2;
                if (idt % 2 == 1) ii = -ii;
                ii = iifac * ii;
                int jig = shift + ii;
                ctr_sync_demod(idat, qdat, samples, symbols, &freq, -2, 2, fstep, &jig,
                               lagmin, lagmax, lagstep, &drift, symfac, &sync, 2);
                float sq = 0.0f;
                for (int i = 0; i < ORC_NSYM; i++) {
                    float y = (float)symbols[i] - 128.0;
                    sq += y * y;
                }
                float rms = sqrtf(sq / (float)ORC_NSYM);
                if (tr && ipass < ORC_TRACE_PASSES) {
                    if (idt == 0) {
                        tr->first_rms[ipass][j] = rms;
                        tr->first_sync2[ipass][j] = sync;
                        memcpy(tr->first_symbols[ipass][j], symbols, ORC_NSYM);
                    }
                    tr->attempts[ipass][j]++;
                }
                if (sync > minsync2 && rms > minrms) {
                    orc_deinterleave(symbols);
                    not_decoded = orc_fano(&metric, &cycles, &maxnp, decdata, symbols, ORC_NBITS,
                                           (const int (*)[256])mettab, delta, maxcycles);
                    if (tr) {
                        tr->fano_cycles_total += cycles;
                        if (ipass < ORC_TRACE_PASSES) tr->fano_calls[ipass][j]++;
                    }
                }
                idt++;
                if (opt.quickmode) break;
            }

            if (worth && !not_decoded) {
                for (int i = 0; i < 11; i++)
                    message[i] = (decdata[i] > 127) ? (signed char)(decdata[i] - 256) : (signed char)decdata[i];
                if (tr && ipass < ORC_TRACE_PASSES) {
                    tr->decoded[ipass][j] = 1;
                    tr->fano_metric[ipass][j] = metric;
                    tr->fano_cycles[ipass][j] = cycles;
                    tr->fano_maxnp[ipass][j] = maxnp;
                    memcpy(tr->decdata[ipass][j], decdata, 11);
                }
                int noprint = orc_unpk(message, hashtab, loctab, call_loc_pow, call, loc, pwr, callsign);
                if (opt.subtraction && ipass == 0 && !noprint) {
                    unsigned char chan[ORC_NSYM];
                    if (orc_channel_symbols(call_loc_pow, hashtab, loctab, chan)) {
                        ctr_subtract(idat, qdat, samples, freq, shift, drift, chan);
                        if (tr) tr->subtracted[ipass][j] = 1;
                    } else {
                        stop = 1;         /* wsprd.c:787 leaves the candidate loop */
                        if (st && ipass < ORC_TRACE_PASSES) { st->reason[ipass] = 1; st->cand[ipass] = j; }
                        continue;
                    }
                }
                if (!strcmp(loc, "A000AA")) {                         /* wsprd.c:792 */
                    stop = 1;
                    if (st && ipass < ORC_TRACE_PASSES) { st->reason[ipass] = 2; st->cand[ipass] = j; }
                    continue;
                }

                int dupe = 0;
                for (int i = 0; i < uniques; i++)
                    if (!strcmp(callsign, allcalls[i]) && fabs(freq - allfreqs[i]) < 3.0) dupe = 1;
                if (!dupe && uniques < ORC_MAXUNIQ) {
                    snprintf(allcalls[uniques], sizeof allcalls[0], "%s", callsign);
                    allfreqs[uniques] = freq;
                    uniques++;
                    double dial = (double)opt.freq / 1e6;
                    orc_spot *o = &spots[uniques - 1];
                    o->sync   = cand[j].sync;
                    o->snr    = cand[j].snr;
                    o->dt     = shift * 1.0 / 375.0 - 2.0;
                    o->freq   = dial + (1500.0 + freq) / 1e6;
                    o->drift  = drift;
                    o->cycles = (int)cycles;
                    o->jitter = ii;
                    snprintf(o->message, sizeof o->message, "%s", call_loc_pow);
                    snprintf(o->call, sizeof o->call, "%s", call);
                    snprintf(o->loc, sizeof o->loc, "%s", loc);
                    snprintf(o->pwr, sizeof o->pwr, "%s", pwr);
                }
            }
        }
    }
    qsort(spots, uniques, sizeof(orc_spot), cmp_spot_snr_desc);
    *n_results = uniques;
    if (opt.usehashtable) {                                   /* wsprd.c:842-852 */
        FILE *fh = fopen("hashtable.txt", "w");
        if (fh) {
            for (int i = 0; i < ORC_HASH_N; i++)
                if (hashtab[i * ORC_HASH_W] != '\0')
                    fprintf(fh, "%5d %s %s\n", i, hashtab + i * ORC_HASH_W, loctab + i * ORC_LOC_W);
            fclose(fh);
        }
    }
    free(ps); free(hashtab); free(loctab);
    return 0;
}
