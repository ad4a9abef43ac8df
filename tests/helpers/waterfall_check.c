// TEST INFRASTRUCTURE ONLY: the waterfall of a segment (K20, rtlsdr-wsprd_amd/csrc/kernels/waterfall.h over noise.h) in plain
// serial code -- the contract of wspr_waterfall_batch_device() and wspr_waterfall(), statement by statement: frame by
// frame, image row by image row, pixel by pixel.  Nothing clever.  The floor of floor mode is the fft_p30 of the noise
// figures' own serial checker (noise_check.c, included here as it stands).  It calls the functions of the two headers (C++:
// tests/waterfall_lib.py compiles this file with g++ -x c++ -O2 -ffp-contract=off) and nothing of the product library.
// With -DWATERFALL_CHECK_MAIN it is a stand-alone program that runs the checker over random rows and images that are
// exactly as large as the contract allows (lengths around the frame, the hop, the averaging group and the full row; both
// hops; narrow and wide column ranges), for a run under -fsanitize=address,undefined.
#include <stdlib.h>
#include <string.h>

#include "noise_check.c"
#include "waterfall.h"

using namespace wspr::waterfall;

extern "C" {

void waterfall_check_default_params(void* p32) {
    const Params d = default_params();
    memcpy(p32, &d, sizeof d);
}

// T[0 .. 255] of the definition (T[0] = 0.0 is never compared)
void waterfall_check_levels(float db_min, float db_step, double* T256) { level_table(db_min, db_step, T256); }

// the level of a ratio r, and of a pixel power m over a reference
int waterfall_check_level_of_ratio(double r, float db_min, float db_step) {
    double T[kLevels];
    level_table(db_min, db_step, T);
    return level_of(r, T);
}
int waterfall_check_level(float m, float ref, float db_min, float db_step) {
    return waterfall_check_level_of_ratio(level_ratio(m, ref), db_min, db_step);
}

// the parameters the call uses (null: the default) and what the library answers to them: 0, -1 or -2
static int settle(int nseg, int samples, const void* p32, Params* p) {
    *p = default_params();
    if (p32) memcpy(p, p32, sizeof *p);
    if (nseg < 0 || samples < 0) return -1;
    if (samples > wspr::waterfall::kMaxSamples) return -2;
    return params_ok(*p) ? 0 : -1;
}

int waterfall_check_shape(int samples, const void* p32, int* nrows, int* ncols) {
    Params p;
    if (const int bad = settle(0, samples, p32, &p)) return bad;
    if (nrows) *nrows = rows_of(samples, p.hop, p.tavg);
    if (ncols) *ncols = cols_of(p.j0, p.j1);
    return 0;
}

// One row of np samples (0 .. 45 000, p valid: the caller has checked) into nrows * ncols bytes at img and one record.
// detail_m (may be null): m of every pixel, nrows * ncols floats (0 where there is no reference); detail_P (may be null):
// P_f[j] of every frame, nframes * 512 floats, j = -256 .. 255 in that order.
static void waterfall_row(const float* I, const float* Q, int np, const Params& p, uint8_t* img, Info* info, float* detail_m,
                          float* detail_P) {
    static float table[kTableFloats];
    static double w2 = 0.0;
    if (w2 == 0.0) w2 = noise_tables(table);
    const float* tw = table;
    const float* w = table + 2 * kTwiddles;
    double T[kLevels];
    level_table(p.db_min, p.db_step, T);

    const int nframes = wspr::waterfall::frames_of(np, p.hop), nrows = nframes / p.tavg, ncols = cols_of(p.j0, p.j1);
    Info out;
    out.ref = p.ref;
    out.nframes = nframes;
    out.nrows = nrows;
    out.flags = nrows > 0 ? kWritten : 0;
    bool has_ref = true;
    if (p.ref_mode == kRefFloor) {
        Result k16;
        const Windows win = {kPreB0, kPreB1, kPostB0, kPostB1};
        check_row(I, Q, np, win, &k16, NULL, NULL, NULL);
        has_ref = floor_ref(k16.fft_p30, k16.flags, &out.ref);
        if (!has_ref) out.flags |= kNoRef | ((k16.flags & wspr::noise::kNonFinite) ? wspr::waterfall::kNonFinite : 0);
    }
    if (detail_P)
        for (int f = 0; f < nframes; ++f) {
            float re[kFft], im[kFft];
            for (int n = 0; n < kFft; ++n) {
                re[n] = I[p.hop * f + n] * w[n];
                im[n] = Q[p.hop * f + n] * w[n];
            }
            for (int st = 0; st < kStages; ++st)
                for (int t = 0; t < kTwiddles; ++t) noise_butterfly(re, im, tw, st, t);
            for (int s = 0; s < kFft; ++s) detail_P[(size_t)f * kFft + (bin_of_slot(s) + kFft / 2)] = slot_power(re[s], im[s]);
        }
    for (int r = 0; r < nrows; ++r) {
        uint8_t* line = img + (size_t)r * ncols;
        float* line_m = detail_m ? detail_m + (size_t)r * ncols : NULL;
        if (!has_ref) {
            memset(line, 0, (size_t)ncols);
            if (line_m) memset(line_m, 0, (size_t)ncols * sizeof(float));
            continue;
        }
        const int first = p.hop * (r * p.tavg), last = p.hop * (r * p.tavg + p.tavg - 1) + kFft - 1;
        int bad = 0;
        for (int k = first; k <= last; ++k) bad |= (non_finite(I[k]) || non_finite(Q[k])) ? 1 : 0;
        double M[kFft];
        for (int s = 0; s < kFft; ++s) M[s] = 0.0;
        for (int f = r * p.tavg; f < r * p.tavg + p.tavg; ++f) {
            float re[kFft], im[kFft];
            for (int n = 0; n < kFft; ++n) {
                re[n] = I[p.hop * f + n] * w[n];
                im[n] = Q[p.hop * f + n] * w[n];
            }
            for (int st = 0; st < kStages; ++st)
                for (int t = 0; t < kTwiddles; ++t) noise_butterfly(re, im, tw, st, t);
            for (int s = 0; s < kFft; ++s) M[s] += (double)slot_power(re[s], im[s]);
        }
        for (int s = 0; s < kFft; ++s) {
            const int c = bin_of_slot(s) - p.j0;
            if (c < 0 || c >= ncols) continue;
            const float m = pixel_power(M[s], p.tavg, w2);
            line[c] = (uint8_t)(bad ? 255 : level_of(level_ratio(m, out.ref), T));
            if (line_m) line_m[c] = m;
        }
        if (bad) out.flags |= wspr::waterfall::kNonFinite;
    }
    *info = out;
}

// nseg rows (row s at I + s * stride) into nseg images (image s at img + s * img_stride, nrows * ncols bytes written) and nseg
// records of 16 bytes.  p32: the 32 bytes of the parameters, or null for the default.  Returns 0; -1 (nothing written) for
// negative counts, parameters out of range, stride < samples, img_stride < nrows * ncols or no records; -2 for samples >
// 45 000.
int waterfall_check_rows(const float* I, const float* Q, int nseg, int samples, size_t stride, const void* p32, uint8_t* img,
                         size_t img_stride, void* info) {
    Params p;
    if (const int bad = settle(nseg, samples, p32, &p)) return bad;
    if (!info) return -1;
    if (nseg > 0 && (stride < (size_t)samples || img_stride < (size_t)rows_of(samples, p.hop, p.tavg) * (size_t)cols_of(p.j0, p.j1)))
        return -1;
    for (int s = 0; s < nseg; ++s)
        waterfall_row(I + (size_t)s * stride, Q + (size_t)s * stride, samples, p, img + (size_t)s * img_stride, (Info*)info + s, NULL,
                      NULL);
    return 0;
}

// the details of one row (see waterfall_row); returns as waterfall_check_rows()
int waterfall_check_detail(const float* I, const float* Q, int samples, const void* p32, uint8_t* img, void* info, float* m,
                           float* P) {
    Params p;
    if (const int bad = settle(1, samples, p32, &p)) return bad;
    if (!info) return -1;
    waterfall_row(I, Q, samples, p, img, (Info*)info, m, P);
    return 0;
}

}  // extern "C"

#ifdef WATERFALL_CHECK_MAIN
#include <stdio.h>
int main(void) {
    static const int extra[] = {0, 511, 512, 44999, 45000};
    static const int hops[] = {128, 256}, tavgs[] = {1, 2, 3, 16};
    static const int cols[][2] = {{-150, 150}, {-256, 255}, {0, 0}, {255, 255}};
    unsigned long long state = 0x9E3779B97F4A7C15ull;
    long pixels = 0, rows = 0;
    int combo = 0;
    for (size_t hi = 0; hi < 2; ++hi)
        for (size_t ti = 0; ti < 4; ++ti) {
            const int hop = hops[hi], tavg = tavgs[ti];
            int lengths[9];
            memcpy(lengths, extra, sizeof extra);
            lengths[5] = 512 + hop - 1; lengths[6] = 512 + hop; lengths[7] = 512 + hop * tavg - 1; lengths[8] = 512 + hop * tavg;
            for (size_t li = 0; li < 9; ++li, ++combo) {
                const int np = lengths[li], nseg = 2;
                /* the full rows cost the most: one column range and one mode each, in turn */
                const int big = np > 40000;
                for (size_t ci = 0; ci < 4; ++ci)
                    for (int mode = 0; mode < 2; ++mode) {
                        if (big && ((int)ci != combo % 4 || mode != (combo / 4) % 2)) continue;
                        Params p = default_params();
                        p.hop = hop; p.tavg = tavg; p.j0 = cols[ci][0]; p.j1 = cols[ci][1]; p.ref_mode = mode; p.ref = 0.5f;
                        const size_t stride = (size_t)np + 3;
                        /* exactly as large as the contract allows: one element more read or written is out of bounds */
                        const size_t count = ((size_t)nseg - 1) * stride + (size_t)np;
                        const size_t image = (size_t)rows_of(np, hop, tavg) * (size_t)cols_of(p.j0, p.j1), img_stride = image + 5;
                        float* I = (float*)malloc(count * sizeof *I + 1);
                        float* Q = (float*)malloc(count * sizeof *Q + 1);
                        uint8_t* img = (uint8_t*)malloc(((size_t)nseg - 1) * img_stride + image + 1);
                        Info info[2];
                        if (!I || !Q || !img) return 2;
                        for (size_t i = 0; i < count; ++i) {
                            state = state * 6364136223846793005ull + 1442695040888963407ull;
                            I[i] = (float)((int)(state >> 40 & 0xffff) - 32768) / 4096.0f;
                            Q[i] = (float)((int)(state >> 20 & 0xffff) - 32768) / 4096.0f;
                        }
                        int nr = -1, nc = -1;
                        if (waterfall_check_shape(np, &p, &nr, &nc) != 0 || (size_t)nr * (size_t)nc != image) return 3;
                        if (waterfall_check_rows(I, Q, nseg, np, stride, &p, img, img_stride, info) != 0) return 4;
                        for (int s = 0; s < nseg; ++s) {
                            if (info[s].nframes != wspr::waterfall::frames_of(np, hop) || info[s].nrows != nr) return 5;
                            if ((info[s].flags & wspr::waterfall::kNonFinite) || ((info[s].flags & kWritten) != 0) != (nr > 0)) return 6;
                            if (mode == kRefFloor && np >= 512 && !(info[s].ref > 0.0f)) return 7;
                            for (size_t i = 0; i < image; ++i) pixels += img[(size_t)s * img_stride + i];
                            rows += nr;
                        }
                        if (nr > 0) {                       /* the guard: the last sample that a complete row uses */
                            union { uint32_t u; float f; } inf;
                            inf.u = 0x7f800000u;
                            Q[stride + (size_t)hop * ((size_t)nr * tavg - 1) + 511] = inf.f;
                            p.ref_mode = kRefAbsolute;
                            if (waterfall_check_rows(I, Q, nseg, np, stride, &p, img, img_stride, info) != 0) return 8;
                            if ((info[0].flags & wspr::waterfall::kNonFinite) || !(info[1].flags & wspr::waterfall::kNonFinite)) return 9;
                            if (img[img_stride + image - 1] != 255 || (nr > 1 && img[img_stride] == 255)) return 10;
                        }
                        free(I);
                        free(Q);
                        free(img);
                    }
            }
        }
    printf("waterfall_check: ok, %ld image rows, pixel sum %ld\n", rows, pixels);
    return 0;
}
#endif
