// TEST INFRASTRUCTURE ONLY: the band noise figures of a segment (K16, rtlsdr-wsprd_amd/csrc/kernels/noise.h) in plain serial
// code -- the contract of wspr_noise_batch_device() and wspr_noise(), statement by statement: block by block, frame by frame,
// a sort by counting.  Nothing clever.  It calls the functions of noise.h (a C++ header: tests/noise_lib.py compiles this
// file with g++ -x c++ -O2 -ffp-contract=off) and nothing of the product library.
// With -DNOISE_CHECK_MAIN it is a stand-alone program that runs the checker over random rows that are exactly as long as
// the contract allows (lengths around the block, the frame and the full row; default, empty, clipped and whole-row
// windows), for a run under -fsanitize=address,undefined: the clipping of windows and frames is where an off-by-one would
// live.
#include <stdlib.h>
#include <string.h>

#include "noise.h"

using namespace wspr;
using namespace wspr::noise;

extern "C" {

void noise_check_default_windows(int32_t* w4) {
    w4[0] = kPreB0; w4[1] = kPreB1; w4[2] = kPostB0; w4[3] = kPostB1;
}

double noise_check_w2(void) {
    static float table[kTableFloats];
    return noise_tables(table);
}

// One row of np samples (0 .. 45 000, windows valid: the caller has checked).  detail_p (may be null): p[b] of every whole
// block, 2 812 floats (0 behind np / 16).  detail_a (may be null): a[j] for j = -256 .. 255 in that order (0 if there is no
// frame).  detail_rank (may be null): the ranks of the 443 band bins, j = -221 .. 221.  The details are those of the row as
// it is, non-finite samples included (the guard only replaces the record).
static void check_row(const float* I, const float* Q, int np, const Windows& win, Result* out, float* detail_p, float* detail_a,
                      int32_t* detail_rank) {
    static float table[kTableFloats];
    static double w2 = 0.0;
    if (w2 == 0.0) w2 = noise_tables(table);
    const float* tw = table;
    const float* w = table + 2 * kTwiddles;

    int bad = 0;
    for (int k = 0; k < np; ++k) bad |= (non_finite(I[k]) || non_finite(Q[k])) ? 1 : 0;

    // 1. the gap figure
    static float p[kBlocks];
    const int nblk = whole_blocks(np);
    for (int b = 0; b < kBlocks; ++b) p[b] = b < nblk ? block_power(I + kBlockLen * b, Q + kBlockLen * b) : 0.0f;
    if (detail_p) memcpy(detail_p, p, sizeof p);
    Result r;
    memset(&r, 0, sizeof r);
    const int pre1 = win.pre_b1 < nblk ? win.pre_b1 : nblk, post1 = win.post_b1 < nblk ? win.post_b1 : nblk;
    if (window_figures(p, win.pre_b0, pre1, &r.pre_mean, &r.pre_trough)) r.flags |= kPreUsed;
    if (window_figures(p, win.post_b0, post1, &r.post_mean, &r.post_trough)) r.flags |= kPostUsed;

    // 2. the spectrum figure
    const int nframes = frames_of(np);
    r.nframes = nframes;
    static double part[kClasses][kFft];
    memset(part, 0, sizeof part);                          // (all bits zero: 0.0)
    for (int f = 0; f < nframes; ++f) {
        float re[kFft], im[kFft];
        for (int n = 0; n < kFft; ++n) {
            re[n] = I[kFrameHop * f + n] * w[n];
            im[n] = Q[kFrameHop * f + n] * w[n];
        }
        for (int st = 0; st < kStages; ++st)
            for (int t = 0; t < kTwiddles; ++t) noise_butterfly(re, im, tw, st, t);
        for (int s = 0; s < kFft; ++s) part[f % kClasses][s] += (double)slot_power(re[s], im[s]);
    }
    uint32_t band[kBand], ranked[kBand];
    memset(band, 0, sizeof band);
    if (detail_a) memset(detail_a, 0, kFft * sizeof(float));
    for (int s = 0; s < kFft; ++s) {
        const int j = bin_of_slot(s);
        const float a = nframes > 0 ? bin_level(join_classes(part[0][s], part[1][s], part[2][s], part[3][s]), nframes, w2) : 0.0f;
        if (detail_a) detail_a[j + kFft / 2] = a;
        if (j >= -kBandHalf && j <= kBandHalf) band[j + kBandHalf] = f32_bits(a);
    }
    for (int i = 0; i < kBand; ++i) {
        const int rank = band_rank(band, i);
        if (detail_rank) detail_rank[i] = rank;
        ranked[rank] = band[i];
    }
    if (nframes > 0) {
        r.fft_floor = band_floor(ranked);
        memcpy(&r.fft_p30, &ranked[kLowest], 4);
        r.flags |= kSpectrumUsed;
    }
    if (bad) {
        memset(&r, 0, sizeof r);
        r.nframes = nframes;
        r.flags = kNonFinite;
    }
    *out = r;
}

// nseg rows (row s at I + s * stride) into nseg records of 32 bytes.  win4: pre_b0, pre_b1, post_b0, post_b1, or null for
// the default.  Returns 0; -1 (nothing written) for negative counts, stride < samples or a window outside
// 0 <= b0 <= b1 <= 2812; -2 for samples > 45 000.
int noise_check_rows(const float* I, const float* Q, int nseg, int samples, size_t stride, const int32_t* win4, void* out) {
    int32_t d[4];
    noise_check_default_windows(d);
    if (win4) memcpy(d, win4, sizeof d);
    const Windows win = {d[0], d[1], d[2], d[3]};
    if (nseg < 0 || samples < 0) return -1;
    if (samples > kMaxSamples) return -2;
    if (!windows_ok(win.pre_b0, win.pre_b1) || !windows_ok(win.post_b0, win.post_b1)) return -1;
    if (nseg > 0 && stride < (size_t)samples) return -1;
    for (int s = 0; s < nseg; ++s)
        check_row(I + (size_t)s * stride, Q + (size_t)s * stride, samples, win, (Result*)out + s, NULL, NULL, NULL);
    return 0;
}

// the details of one row under the given windows (see check_row); returns as noise_check_rows()
int noise_check_detail(const float* I, const float* Q, int samples, const int32_t* win4, void* out, float* p2812, float* a512,
                       int32_t* rank443) {
    int32_t d[4];
    noise_check_default_windows(d);
    if (win4) memcpy(d, win4, sizeof d);
    const Windows win = {d[0], d[1], d[2], d[3]};
    if (samples < 0) return -1;
    if (samples > kMaxSamples) return -2;
    if (!windows_ok(win.pre_b0, win.pre_b1) || !windows_ok(win.post_b0, win.post_b1)) return -1;
    check_row(I, Q, samples, win, (Result*)out, p2812, a512, rank443);
    return 0;
}

}  // extern "C"

#ifdef NOISE_CHECK_MAIN
#include <stdio.h>
int main(void) {
    static const int lengths[] = {0, 15, 16, 17, 511, 512, 767, 768, 1000, 44999, 45000};
    static const int32_t windows[][4] = {{6, 42, 2672, 2790}, {0, 0, 2812, 2812}, {0, 2812, 0, 2812}, {100, 200, 150, 2812}, {2811, 2812, 0, 1}};
    unsigned long long state = 0x9E3779B97F4A7C15ull;
    long used = 0, frames = 0;
    for (size_t li = 0; li < sizeof lengths / sizeof lengths[0]; ++li)
        for (size_t wi = 0; wi < sizeof windows / sizeof windows[0]; ++wi) {
            const int np = lengths[li], nseg = 2;
            const size_t stride = (size_t)np + 3;
            /* exactly as large as the contract allows the rows to be: one float more read is out of bounds */
            const size_t count = ((size_t)nseg - 1) * stride + (size_t)np;
            float* I = (float*)malloc(count * sizeof *I + 1);
            float* Q = (float*)malloc(count * sizeof *Q + 1);
            Result out[2];
            if (!I || !Q) return 2;
            for (size_t i = 0; i < count; ++i) {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                I[i] = (float)((int)(state >> 40 & 0xffff) - 32768) / 4096.0f;
                Q[i] = (float)((int)(state >> 20 & 0xffff) - 32768) / 4096.0f;
            }
            if (noise_check_rows(I, Q, nseg, np, stride, wi ? windows[wi] : NULL, out) != 0) return 3;
            for (int s = 0; s < nseg; ++s) {
                if (out[s].nframes != frames_of(np) || (out[s].flags & kNonFinite)) return 4;
                if (!(out[s].fft_floor >= 0.0f) || !(out[s].pre_trough <= out[s].pre_mean)) return 5;
                used += out[s].flags;
                frames += out[s].nframes;
            }
            if (np > 0) {                                   /* the guard: the last sample that counts */
                union { uint32_t u; float f; } inf;
                inf.u = 0x7f800000u;
                Q[stride + (size_t)np - 1] = inf.f;
                if (noise_check_rows(I, Q, nseg, np, stride, windows[wi], out) != 0) return 6;
                if ((out[0].flags & kNonFinite) || out[1].flags != kNonFinite || out[1].fft_floor != 0.0f) return 7;
            }
            free(I);
            free(Q);
        }
    printf("noise_check: ok, flags sum %ld, %ld frames\n", used, frames);
    return 0;
}
#endif
