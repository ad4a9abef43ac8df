/* K21, the tunable multi-band front end: THE DEFINITION (repeated in include/wspr_mi355x.h; tests/helpers/tune_check.c is
 * the same in serial C, k21_tune.hip the gfx950 kernel).  Plain C: included by the kernel, the host code and the checker.
 *
 * One row of 2.4 Msps unsigned-8-bit IQ bytes (I, Q, I, Q, ...; the row starts 16-byte aligned and its length in bytes is a
 * multiple of 16) and one oscillator step per band give one 375.000 Hz float row per band.
 *
 *   samples     s_n = (I_n - 128) + j (Q_n - 128), n = 0 .. nsamples - 1.  Vector v is samples 8v .. 8v + 7.
 *   oscillator  unsigned 32-bit phase, 0 at the start of every row.  step = tune_step(offset_hz) =
 *               floor(-offset_hz * 2^32 / 2.4e6 + 0.5) mod 2^32 brings a signal at +offset_hz to 0 Hz; the realised
 *               offset is -(int32)step * 2.4e6 / 2^32 (resolution 0.00056 Hz).
 *   rs14(x)     = (x + 8192) >> 14 with an arithmetic shift: floor(x / 16384 + 1/2), halves towards +infinity; of a
 *               complex number, of its two parts separately.
 *   rot(P)      = rs14(C[P >> 24] * F[(P >> 16) & 255]), the complex product exact in int32;
 *               C[k] = round(16384 e^{2 pi i k / 256}), F[k] = round(16384 e^{2 pi i k / 65536}) (tune_tables.h).
 *               F HAS NO HALF-STEP OFFSET (the issue's draft had e^{2 pi i (k + 1/2) / 65536}): with it rot(0) would be
 *               (16384, 1) and no rotor exact.  Without it F[0] = 16384 and rot(m 2^30) = (1, j, -1, -j)[m] * 16384, so
 *               that the bands at 0, +-fs/4 and fs/2 are mixed exactly; the truncated 16 phase bits then lag by half a
 *               step on average, a constant rotation of the row by pi/65536, and the phase noise is the same sawtooth.
 *   mixer       per band H_k = rot(k step), k = 0 .. 7, built on the host;
 *               z_v = sum_k s_{8v+k} H_k                        exact in int32 (|part| <= 8 * 2 * 128 * 16385 < 2^26)
 *               y_v = rs14(z_v * rot(8 v step mod 2^32))        64-bit products; |part| < 2^27
 *   decimation  y_v runs at 300 kHz.  Two cascaded running sums (i1 += y_v; i2 += i1) are sampled behind every 800th
 *               vector, c_b = i2 behind vector 800 b + 799, and differenced twice over TWO outputs, as the reference's
 *               front end does: d_b = c_b - 2 c_{b-2} + c_{b-4} (c = 0 before the start).  All int64, no wrap
 *               (|d_b| < 4 * 800^2 * 2^27 < 2^49).  With S_b = sum of block b's y, W_b = sum (800 - r) y_{800 b + r}:
 *                   d_b = 800 (S_{b-1} + 2 S_{b-2} + S_{b-3}) + W_b + W_{b-1} - W_{b-2} - W_{b-3}       (K0's, R = 800)
 *               One output covers 6400 samples: 375 Hz exactly.
 *   float tail  x_b = (float)(double)d_b * TUNE_SCALE: the conversion to double is exact, the one to float rounds to
 *               nearest even, the product is one float multiplication.  out_m = K0's 33 taps (wspr_front_end_constants())
 *               over x_{m-32} .. x_m in K0's order from a zero history (x_b = 0.0f for b < 0):
 *                   acc = 0.0f; for j = 0 .. 32: acc = acc + x_{m-32+j} * taps[j]     (each product and sum rounded: no fma)
 *               wspr_set_arithmetic() does not reach this stage.
 *   lengths     n_out = min(floor(nsamples / 6400), 45000); a trailing partial block is dropped; columns n_out .. of the
 *               row are 0.0f.  No carried state.
 *   normalise   != 0: afterwards the receiver's scaling of the row to a peak of 0.5, the kernel K0's rows take.
 */
#pragma once
#include <stdint.h>

#include "tune_tables.h"

#define TUNE_MAX_BANDS 16
#define TUNE_VEC 8                      /* samples per vector */
#define TUNE_R 800                      /* vectors per output */
#define TUNE_SAMPLES_PER_OUTPUT 6400
#define TUNE_MAX_OUT 45000
#define TUNE_FS 2400000.0

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TUNE_HD __host__ __device__ static inline
#else
#define TUNE_HD static inline
#endif

typedef struct { int32_t re, im; } tune_c32;

TUNE_HD int32_t tune_rs14(int64_t x) { return (int32_t)((x + 8192) >> 14); }

/* the product of a C entry (cr, ci) and an F entry (fr, fi), rounded */
TUNE_HD tune_c32 tune_rot_of(int32_t cr, int32_t ci, int32_t fr, int32_t fi) {
    tune_c32 r;
    r.re = (cr * fr - ci * fi + 8192) >> 14;
    r.im = (cr * fi + ci * fr + 8192) >> 14;
    return r;
}
TUNE_HD uint32_t tune_hi(uint32_t P) { return P >> 24; }
TUNE_HD uint32_t tune_lo(uint32_t P) { return (P >> 16) & 255u; }

/* y = rs14(z * r) */
TUNE_HD tune_c32 tune_mix(tune_c32 z, tune_c32 r) {
    tune_c32 y;
    y.re = tune_rs14((int64_t)z.re * r.re - (int64_t)z.im * r.im);
    y.im = tune_rs14((int64_t)z.re * r.im + (int64_t)z.im * r.re);
    return y;
}

TUNE_HD float tune_scale(void) {
    union { uint32_t u; float f; } v;
    v.u = TUNE_SCALE_BITS;
    return v.f;
}
/* x_b of d_b */
TUNE_HD float tune_to_float(int64_t d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return (float)(double)d * tune_scale();
}

TUNE_HD int tune_n_out(uint64_t nsamples) {
    const uint64_t n = nsamples / TUNE_SAMPLES_PER_OUTPUT;
    return n < TUNE_MAX_OUT ? (int)n : TUNE_MAX_OUT;
}

/* ---- host only: the tables as they are committed, the step of an offset, what the kernel takes per band ------------- */
static inline tune_c32 tune_rot(uint32_t P) {
    const uint32_t h = tune_hi(P), l = tune_lo(P);
    return tune_rot_of(kTuneC256[2 * h], kTuneC256[2 * h + 1], kTuneF256[2 * l], kTuneF256[2 * l + 1]);
}

/* floor(-offset_hz 2^32 / 2.4e6 + 0.5) mod 2^32 without libm; 0 (and a realised offset of 0) for an offset that is not
 * finite.  The reduction modulo fs comes first and is exact enough: |offset| < 2^52 Hz loses nothing a step can hold. */
static inline uint32_t tune_step(double offset_hz, double* realised_hz) {
    uint32_t step = 0;
    if (offset_hz == offset_hz && offset_hz - offset_hz == 0.0) {
        double t = -offset_hz / TUNE_FS;                    /* turns per sample */
        if (t > 4503599627370496.0 || t < -4503599627370496.0) t = 0.0;   /* beyond 2^52 every double is a whole turn */
        t -= (double)(int64_t)t;                            /* (-1, 1) */
        double x = t * 4294967296.0 + 0.5;                  /* exact scaling; floor next */
        int64_t k = (int64_t)x;
        if ((double)k > x) --k;
        step = (uint32_t)((uint64_t)k & 0xffffffffu);
    }
    if (realised_hz) *realised_hz = -(double)(int32_t)step * TUNE_FS / 4294967296.0;
    return step;
}

/* One band as the kernel takes it: the phase step, H_k packed for the 16-bit dot products over a sample's UNSIGNED bytes
 * (u_I, u_Q):  re = u_I hr - u_Q hi,  im = u_I hi + u_Q hr,  and what the -128 of both rails adds to a whole vector:
 *   bias_re = -128 sum_k (hr_k - hi_k),  bias_im = -128 sum_k (hi_k + hr_k). */
typedef struct {
    uint32_t step;
    int32_t bias_re, bias_im;
    uint32_t h_re[TUNE_VEC];            /* (hr_k, -hi_k) as two int16, the first in the low half */
    uint32_t h_im[TUNE_VEC];            /* (hi_k,  hr_k) */
} tune_band;

static inline void tune_band_setup(uint32_t step, tune_band* b) {
    b->step = step;
    b->bias_re = b->bias_im = 0;
    for (uint32_t k = 0; k < TUNE_VEC; ++k) {
        const tune_c32 h = tune_rot(k * step);
        b->h_re[k] = ((uint32_t)h.re & 0xffffu) | ((uint32_t)(-h.im) << 16);
        b->h_im[k] = ((uint32_t)h.im & 0xffffu) | ((uint32_t)h.re << 16);
        b->bias_re -= 128 * (h.re - h.im);
        b->bias_im -= 128 * (h.im + h.re);
    }
}
