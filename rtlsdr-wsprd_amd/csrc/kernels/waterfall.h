// The waterfall of one segment (K20, wspr_waterfall_batch_device(), wspr_waterfall()): THE DEFINITION, written once for the
// kernel (k20_waterfall.hip) and for a CPU; tests/helpers/waterfall_check.c is its serial form over the functions of this
// header and of noise.h, and include/wspr_mi355x.h repeats it.  There is no reference behaviour to match (the reference
// shows a picture of a waterfall and computes none): the definition is this project's own.  It is built on noise.h -- the
// window, the twiddles (noise_tables()), butterfly_values() / noise_butterfly(), bin_of_slot(), slot_power(), non_finite()
// and W2 are K16's and are not restated here.
//
// Parameters (Params below; an argument of the calls, not state): hop 128 or 256, tavg 1 .. 16, the signed bins
// -256 <= j0 <= j1 <= 255 (ncols = j1 - j0 + 1), ref_mode (kRefAbsolute: `ref`, finite and > 0; kRefFloor: the row's own K16
// fft_p30), db_min -60 .. 60, db_step 0.05 .. 4.
//
// For one row of np samples (0 .. 45 000) of I and Q at 375 samples per second:
//   Frames.      nframes = np >= 512 ? (np - 512)/hop + 1 : 0; frame f holds the samples hop*f .. hop*f + 511.
//                nrows = nframes / tavg; image row r is formed from the frames r*tavg .. r*tavg + tavg - 1, a trailing
//                incomplete group is dropped.  Row 0 is the earliest; column c is bin j0 + c, so +f is to the right.
//   Frame power. P_f[j] exactly K16's: float products with the Hann window, the nine stages of noise_butterfly(),
//                slot_power(), no fused multiply-add.
//   Pixel power. M = the double sum of (double)P_f[j] over the row's frames in rising f from 0.0;
//                m = (float)(M / (double)tavg / W2): noise::bin_level() with tavg for nframes, the units of K16's a[j].
//   Reference.   Absolute mode: `ref` as given.  Floor mode: the fft_p30 of K16's record for the same row and `samples`
//                (K16's own hop of 256 whatever `hop` is here; the windows play no part).  There is NO usable floor when
//                that record lacks the spectrum-used bit, carries the non-finite bit or has fft_p30 == 0: then info.ref
//                = 0, flags gets kNoRef (and kNonFinite if K16 reported it) and every pixel of the image is 0.
//   Row guard    (when a reference exists).  If any sample of hop*(r*tavg) .. hop*(r*tavg + tavg - 1) + 511, on either rail,
//                has exponent bits 0xff (noise::non_finite()), every pixel of row r is 255 and kNonFinite is set: a white
//                stripe where the capture is garbage.  Samples that no complete row uses are not looked at.
//   Level.       r = (double)m / (double)ref;  T[i] = pow(10.0, ((double)db_min + (double)i*(double)db_step)/10.0) for
//                i = 1 .. 255, built in double on the host (level_table()) and handed to the kernel as a table.  The
//                pixel is the number of i with r >= T[i]: a NaN r gives 0, +Inf gives 255.  T is strictly increasing,
//                so the eight steps of level_of() with the same >= are the same function; no logarithm on the device.
//   Info.        ref as used, nframes, nrows, flags; kWritten iff nrows > 0.
// wspr_set_arithmetic() does not touch any of this.
#pragma once
#include <stdint.h>

#include "noise.h"

namespace wspr {
namespace waterfall {

constexpr int kMaxSamples = noise::kMaxSamples;
constexpr int kMaxAvg = 16;
constexpr int kLevels = 256;                               // pixel values 0 .. 255; T[1 .. 255], T[0] unused (0.0)
constexpr int kRefAbsolute = 0, kRefFloor = 1;
constexpr int kWritten = 1, kNoRef = 2, kNonFinite = 8;

struct Params {
    int32_t hop, tavg, j0, j1, ref_mode;
    float ref, db_min, db_step;
};
struct Info {
    float ref;
    int32_t nframes, nrows, flags;
};

WSPR_HD Params default_params() { return Params{128, 1, -150, 150, kRefFloor, 1.0f, -10.0f, 0.25f}; }

// (the comparisons are written so that a NaN fails them)
WSPR_HD bool hop_ok(int hop) { return hop == 128 || hop == 256; }
WSPR_HD bool tavg_ok(int tavg) { return tavg >= 1 && tavg <= kMaxAvg; }
WSPR_HD bool bins_ok(int j0, int j1) { return -noise::kFft / 2 <= j0 && j0 <= j1 && j1 <= noise::kFft / 2 - 1; }
WSPR_HD bool ref_mode_ok(int mode) { return mode == kRefAbsolute || mode == kRefFloor; }
WSPR_HD bool ref_ok(float ref) { return !noise::non_finite(ref) && ref > 0.0f; }
WSPR_HD bool levels_ok(float db_min, float db_step) {
    return !noise::non_finite(db_min) && !noise::non_finite(db_step) && db_min >= -60.0f && db_min <= 60.0f && db_step >= 0.05f &&
           db_step <= 4.0f;
}
WSPR_HD bool params_ok(const Params& p) {
    return hop_ok(p.hop) && tavg_ok(p.tavg) && bins_ok(p.j0, p.j1) && ref_mode_ok(p.ref_mode) &&
           (p.ref_mode != kRefAbsolute || ref_ok(p.ref)) && levels_ok(p.db_min, p.db_step);
}

WSPR_HD int frames_of(int np, int hop) { return np >= noise::kFft ? (np - noise::kFft) / hop + 1 : 0; }
WSPR_HD int rows_of(int np, int hop, int tavg) { return frames_of(np, hop) / tavg; }
WSPR_HD int cols_of(int j0, int j1) { return j1 - j0 + 1; }

// T[0] = 0.0 (never compared), T[i] for i = 1 .. 255.  From the host libm, in double.
#if defined(__HIPCC__)
__host__
#endif
static inline void level_table(float db_min, float db_step, double* T) {
    T[0] = 0.0;
    for (int i = 1; i < kLevels; ++i) T[i] = pow(10.0, ((double)db_min + (double)i * (double)db_step) / 10.0);
}

// m of one pixel from the double sum M of its tavg frame powers
// (M / 1.0 is M, bit for bit, for every M: with tavg 1 the first of bin_level()'s two divisions is left out)
WSPR_HD float pixel_power(double M, int tavg, double w2) { return tavg == 1 ? (float)(M / w2) : noise::bin_level(M, tavg, w2); }
WSPR_HD double level_ratio(float m, float ref) { return (double)m / (double)ref; }
// the number of i in 1 .. 255 with r >= T[i], T strictly increasing: eight steps
WSPR_HD int level_of(double r, const double* T) {
    int lo = 0;
    for (int step = kLevels / 2; step > 0; step >>= 1)
        if (r >= T[lo + step]) lo += step;
    return lo;
}

// the reference of floor mode from K16's record; false: no usable floor
WSPR_HD bool floor_ref(float fft_p30, int noise_flags, float* ref) {
    const bool usable = (noise_flags & noise::kSpectrumUsed) && !(noise_flags & noise::kNonFinite) && fft_p30 != 0.0f;
    *ref = usable ? fft_p30 : 0.0f;
    return usable;
}

}  // namespace waterfall
}  // namespace wspr
