// What can be wrong with a stage call (K8/K13, K12, K15, K16, K17, K18, K19, K20, K21), each condition stated once.  Plain C++ without
// HIP: pointers are looked at as addresses and never dereferenced -- the transmissions, their channels and the noise
// windows are host memory and are read.  tests/helpers/stage_args_check.cpp runs a table of calls through this header on
// a CPU.
//
// Every function returns 0, or the code its entry point returns (-1, or -2 for a record or row that is too long) after
// one line on stderr; nothing has been written then.  The checks of an entry point (the second half of this file) test
// their conditions in a fixed order: with several things wrong, that order picks the line and decides between -2 and -1.
// No flag names in the texts: the product binary carries no new macro-style string (tests/test_abi.py).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../../include/wspr_mi355x.h"
#include "../kernels/audio_blank.h"
#include "../kernels/audio_front.h"
#include "../kernels/audio_synth.h"
#include "../kernels/fade.h"
#include "../kernels/iq_audio.h"
#include "../kernels/noise.h"
#include "../kernels/tune.h"
#include "../kernels/waterfall.h"

namespace wspr {
namespace args {

inline int refuse(const char* where, const char* why, int code = -1) {
    fprintf(stderr, "libwspr_mi355x: %s: %s\n", where, why);
    return code;
}
inline bool aligned16(const void* p) { return p && !(reinterpret_cast<uintptr_t>(p) & 15); }

// ---- device rows and records --------------------------------------------------------------------------------------------
// rows are read and written with aligned 16-byte vector accesses
inline int rows_bad(const char* where, const void* d_i, const void* d_q, int nseg) {
    if (nseg > 0 && !(aligned16(d_i) && aligned16(d_q))) return refuse(where, "d_idat and d_qdat must be 16-byte aligned device rows");
    return 0;
}
inline int row_stride_bad(const char* where, size_t seg_stride, int samples, int nseg) {
    if (nseg > 0 && ((seg_stride & 3) || seg_stride < (size_t)samples))
        return refuse(where, "seg_stride must be a multiple of 4 floats and at least samples");
    return 0;
}
// records of 16-bit samples; `need` samples of each are touched.  The names are the entry point's own arguments.
inline int pcm_bad(const char* where, const void* d_pcm, size_t pcm_stride, size_t need, int nseg, const char* need_text = "nsamp",
                   const char* pointer = "d_pcm", const char* stride = "pcm_stride") {
    if (nseg <= 0) return 0;
    if (!aligned16(d_pcm)) {
        fprintf(stderr, "libwspr_mi355x: %s: %s must be 16-byte aligned device memory\n", where, pointer);
        return -1;
    }
    if ((pcm_stride & 7) || pcm_stride < need) {
        fprintf(stderr, "libwspr_mi355x: %s: %s must be a multiple of 8 and at least %s\n", where, stride, need_text);
        return -1;
    }
    return 0;
}
// a record of audio or a row of IQ that is longer than 120 s is refused with a code of its own, not cut
inline int too_long(const char* where, long long n, long long most, const char* text) {
    return n > most ? refuse(where, text, -2) : 0;
}
constexpr const char* kRecordTooLong = "a record holds at most 1440000 samples (120 s); longer ones are refused, not cut";
constexpr const char* kRowTooLong = "a row holds at most 45000 samples (120 s); longer ones are refused, not cut";

// ---- transmission lists (K8/K13 and K17) --------------------------------------------------------------------------------
struct TxLimits {
    int flag_mask;                  // the flag bits the call knows
    double max_hz;                  // |f0| + |drift|/2 beyond this is refused ...
    const char* hz_text;            // ... with this line
    double max_level;               // |amp| and noise_sigma beyond this are refused (infinity: no limit)
    bool sigma_may_be_negative;     // K8 takes sigma <= 0 as "no noise"
};
inline const TxLimits& iq_tx_limits() {      // K8 and K13
    static const TxLimits l{kSynthFlagAccumulate | kSynthFlagNormalise, kSynthMaxHz, "|f0| + |drift|/2 above 1000 Hz", INFINITY, true};
    return l;
}
inline const TxLimits& audio_tx_limits() {   // K17
    static const TxLimits l{kSynthFlagAccumulate, kAudioSynthMaxHz, "|f0| + |drift|/2 above 800 Hz", kAudioSynthMaxLevel, false};
    return l;
}
inline int tx_list_bad(const char* where, const wspr_synth_tx* tx, int ntx, int nseg, float sigma, int flags, const TxLimits& lim) {
    if (ntx < 0 || nseg < 0) return refuse(where, "negative count");
    if (ntx > 0 && !tx) return refuse(where, "no transmission list");
    if (!std::isfinite(sigma)) return refuse(where, "noise_sigma is not finite");
    if (!lim.sigma_may_be_negative && sigma < 0.0f) return refuse(where, "noise_sigma is negative");
    if ((double)sigma > lim.max_level) return refuse(where, "noise_sigma above 1e6");
    if (flags & ~lim.flag_mask) return refuse(where, "unknown flag bit");
    for (int t = 0; t < ntx; ++t) {
        const wspr_synth_tx& x = tx[t];
        const char* why = nullptr;
        if (x.seg < 0 || x.seg >= nseg) why = "seg outside the batch";
        else if (t > 0 && x.seg < tx[t - 1].seg) why = "list not sorted by seg";
        else if (!std::isfinite(x.f0) || !std::isfinite(x.t0) || !std::isfinite(x.amp) || !std::isfinite(x.drift))
            why = "f0, t0, amp or drift is not finite";
        else if (std::fabs((double)x.amp) > lim.max_level) why = "|amp| above 1e6";
        else if (std::fabs((double)x.f0) + std::fabs((double)x.drift) / 2.0 > lim.max_hz) why = lim.hz_text;
        else
            for (int i = 0; i < 162; ++i) if (x.symbols[i] > 3) { why = "channel symbol above 3"; break; }
        if (why) { fprintf(stderr, "libwspr_mi355x: %s: transmission %d: %s\n", where, t, why); return -1; }
    }
    return 0;
}
// The channels of a faded call (null: none, and `out` stays empty); fills `out` with the constants the kernel takes (fade.h)
inline int fade_args_bad(const char* where, const wspr_synth_channel* ch, int ntx, std::vector<FadeChannel>& out) {
    if (!ch) return 0;
    out.resize((size_t)(ntx > 0 ? ntx : 0));
    for (int t = 0; t < ntx; ++t)
        for (int p = 0; p < 2; ++p) {
            const wspr_synth_path& a = ch[t].path[p];
            const char* why = nullptr;
            if (!std::isfinite(a.gain) || !std::isfinite(a.shift) || !std::isfinite(a.sigma)) why = "gain, shift or sigma is not finite";
            else if (a.sigma != 0.0f && !(a.sigma >= kFadeMinSigma && a.sigma <= kFadeMaxSigma)) why = "sigma neither 0 nor within 0.001 .. 10 Hz";
            else if (std::fabs(a.shift) > kFadeMaxShift) why = "|shift| above 100 Hz";
            if (why) { fprintf(stderr, "libwspr_mi355x: %s: transmission %d, path %d: %s\n", where, t, p, why); return -1; }
            out[(size_t)t].path[p] = fade_path_setup(a.gain, a.shift, a.sigma);
        }
    return 0;
}

// ---- settings of a stage ------------------------------------------------------------------------------------------------
inline int blank_settings_bad(const char* where, int thr16, int guard) {
    return audio_blank_settings_ok(thr16, guard) ? 0 : refuse(where, "thr16 must be 16 .. 4096 and guard 0 .. 64");
}
// K12's counts; K15's calls take the same
inline int audio_counts_bad(const char* where, long long nsamp, int nseg) {
    if (nseg < 0 || nsamp < 0) return refuse(where, "negative count");
    return too_long(where, nsamp, AUDIO_FRONT_MAX_SAMPLES, kRecordTooLong);
}
inline noise::Windows default_noise_windows() { return noise::Windows{noise::kPreB0, noise::kPreB1, noise::kPostB0, noise::kPostB1}; }
// K16's counts and windows, the same for both calls; *win = the windows the call uses
inline int noise_args_bad(const char* where, int nseg, int samples, const wspr_noise_windows* w, const void* out, noise::Windows* win) {
    *win = default_noise_windows();
    if (w) std::memcpy(win, w, sizeof *win);
    if (nseg < 0 || samples < 0) return refuse(where, "negative count");
    if (const int bad = too_long(where, samples, noise::kMaxSamples, kRowTooLong)) return bad;
    if (!noise::windows_ok(win->pre_b0, win->pre_b1) || !noise::windows_ok(win->post_b0, win->post_b1))
        return refuse(where, "a window must satisfy 0 <= b0 <= b1 <= 2812");
    if (nseg > 0 && !out) return refuse(where, "no output records");
    return 0;
}
// K18's counts and gain, the same for both calls
inline int iq_audio_args_bad(const char* where, int nseg, int samples, float gain) {
    if (nseg < 0 || samples < 0) return refuse(where, "negative count");
    if (const int bad = too_long(where, samples, IQ_AUDIO_MAX_SAMPLES, kRowTooLong)) return bad;
    if (!std::isfinite(gain)) return refuse(where, "gain is not finite");
    return 0;
}
// K20's counts, parameters and records, the same for both calls; *use = the parameters the call uses
inline int waterfall_args_bad(const char* where, int nseg, int samples, const wspr_waterfall_params* p, const void* info,
                              waterfall::Params* use) {
    *use = waterfall::default_params();
    if (p) std::memcpy(use, p, sizeof *use);
    if (nseg < 0 || samples < 0) return refuse(where, "negative count");
    if (const int bad = too_long(where, samples, waterfall::kMaxSamples, kRowTooLong)) return bad;
    if (!waterfall::hop_ok(use->hop)) return refuse(where, "hop must be 128 or 256");
    if (!waterfall::tavg_ok(use->tavg)) return refuse(where, "tavg must be 1 .. 16");
    if (!waterfall::bins_ok(use->j0, use->j1)) return refuse(where, "the bins must satisfy -256 <= j0 <= j1 <= 255");
    if (!waterfall::ref_mode_ok(use->ref_mode)) return refuse(where, "unknown ref_mode");
    if (use->ref_mode == waterfall::kRefAbsolute && !waterfall::ref_ok(use->ref)) return refuse(where, "ref must be finite and above 0");
    if (!waterfall::levels_ok(use->db_min, use->db_step)) return refuse(where, "db_min must be -60 .. 60 and db_step 0.05 .. 4");
    if (!info) return refuse(where, "no info records");
    return 0;
}
// K21's counts and steps, the same for both calls
inline int tune_args_bad(const char* where, int nseg, const void* steps, int nbands) {
    if (nseg < 0) return refuse(where, "negative count");
    if (nbands < 1 || nbands > TUNE_MAX_BANDS) return refuse(where, "nbands must be 1 .. 16");
    if (!steps) return refuse(where, "no steps");
    return 0;
}
// K17's counts, length and list, the same for both calls
inline int synth_audio_args_bad(const char* where, const wspr_synth_tx* tx, int ntx, int nseg, long long nsamp, float sigma, int flags) {
    if (ntx < 0 || nseg < 0 || nsamp < 0) return refuse(where, "negative count");
    if (const int bad = too_long(where, nsamp, kAudioSynthMaxSamples, "a record holds at most 1440000 samples (120 s)")) return bad;
    return tx_list_bad(where, tx, ntx, nseg, sigma, flags, audio_tx_limits());
}

// ---- the entry points: everything each of them checks, in its order -----------------------------------------------------
// wspr_synth_batch_device() (ch null) and wspr_synth_faded_batch_device()
inline int synth_batch(const char* where, const wspr_synth_tx* tx, const wspr_synth_channel* ch, int ntx, int nseg, float sigma,
                       int flags, const void* d_i, const void* d_q, std::vector<FadeChannel>& fade) {
    if (const int bad = tx_list_bad(where, tx, ntx, nseg, sigma, flags, iq_tx_limits())) return bad;
    if (const int bad = fade_args_bad(where, ch, ntx, fade)) return bad;
    return rows_bad(where, d_i, d_q, nseg);
}
// wspr_synth() (ch null) and wspr_synth_faded()
inline int synth_host(const char* where, const wspr_synth_tx* tx, const wspr_synth_channel* ch, int ntx, float sigma, int flags,
                      const void* I, const void* Q, std::vector<FadeChannel>& fade) {
    if (const int bad = tx_list_bad(where, tx, ntx, 1, sigma, flags, iq_tx_limits())) return bad;
    if (const int bad = fade_args_bad(where, ch, ntx, fade)) return bad;
    return (!I || !Q) ? refuse(where, "no output rows") : 0;
}
inline int synth_audio_batch(const char* where, const wspr_synth_tx* tx, int ntx, int nseg, int nsamp, float sigma, int flags,
                             const void* d_pcm, size_t pcm_stride) {
    if (const int bad = synth_audio_args_bad(where, tx, ntx, nseg, nsamp, sigma, flags)) return bad;
    return pcm_bad(where, d_pcm, pcm_stride, (size_t)nsamp, nseg);
}
inline int synth_audio_host(const char* where, const wspr_synth_tx* tx, int ntx, int nsamp, float sigma, int flags, const void* pcm) {
    if (const int bad = synth_audio_args_bad(where, tx, ntx, 1, nsamp, sigma, flags)) return bad;
    return (!pcm && nsamp) ? refuse(where, "no output record") : 0;
}
// wspr_audio_batch_device(); wspr_audio_blanked_batch_device() after its settings
inline int audio_batch(const char* where, const void* d_pcm, size_t pcm_stride, long long nsamp, int nseg, const void* d_i, const void* d_q) {
    if (const int bad = audio_counts_bad(where, nsamp, nseg)) return bad;
    if (const int bad = pcm_bad(where, d_pcm, pcm_stride, (size_t)nsamp, nseg)) return bad;
    return rows_bad(where, d_i, d_q, nseg);
}
inline int audio_blanked_batch(const char* where, const void* d_pcm, size_t pcm_stride, long long nsamp, int nseg, int thr16, int guard,
                               const void* d_i, const void* d_q) {
    if (const int bad = blank_settings_bad(where, thr16, guard)) return bad;
    return audio_batch(where, d_pcm, pcm_stride, nsamp, nseg, d_i, d_q);
}
inline int audio_blank_batch(const char* where, const void* d_pcm, size_t pcm_stride, long long nsamp, int nseg, int thr16, int guard,
                             const void* d_out, size_t out_stride) {
    if (const int bad = blank_settings_bad(where, thr16, guard)) return bad;
    if (const int bad = audio_counts_bad(where, nsamp, nseg)) return bad;
    if (const int bad = pcm_bad(where, d_pcm, pcm_stride, (size_t)nsamp, nseg)) return bad;
    if (const int bad = pcm_bad(where, d_out, out_stride, (size_t)nsamp, nseg, "nsamp", "d_out", "out_stride")) return bad;
    if (nseg == 0 || nsamp == 0) return 0;
    // in place is a race: a neighbouring block's halo would read samples that are already blanked
    const size_t padded = ((size_t)nsamp + 7) & ~(size_t)7;
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(d_pcm), out0 = reinterpret_cast<uintptr_t>(d_out);
    const uintptr_t in1 = in0 + (((size_t)nseg - 1) * pcm_stride + padded) * sizeof(int16_t);
    const uintptr_t out1 = out0 + (((size_t)nseg - 1) * out_stride + padded) * sizeof(int16_t);
    return (in0 < out1 && out0 < in1) ? refuse(where, "the output rows overlap the input rows") : 0;
}
// wspr_audio_to_iq() (blank null) and wspr_audio_to_iq_blanked() (blank = thr16, guard)
inline int audio_host(const char* where, const void* pcm, size_t nsamp, const int* blank, const void* I, const void* Q) {
    if (blank) if (const int bad = blank_settings_bad(where, blank[0], blank[1])) return bad;
    if (nsamp > (size_t)AUDIO_FRONT_MAX_SAMPLES) return refuse(where, kRecordTooLong, -2);
    return ((!pcm && nsamp) || !I || !Q) ? refuse(where, "no record, or no output rows") : 0;
}
inline int noise_batch(const char* where, const void* d_i, const void* d_q, int nseg, int samples, size_t seg_stride,
                       const wspr_noise_windows* w, const void* out, noise::Windows* win) {
    if (const int bad = noise_args_bad(where, nseg, samples, w, out, win)) return bad;
    if (const int bad = rows_bad(where, d_i, d_q, nseg)) return bad;
    return row_stride_bad(where, seg_stride, samples, nseg);
}
inline int noise_host(const char* where, const void* I, const void* Q, int samples, const wspr_noise_windows* w, const void* out,
                      noise::Windows* win) {
    if (const int bad = noise_args_bad(where, 1, samples, w, out, win)) return bad;
    return ((!I || !Q) && samples) ? refuse(where, "no row") : 0;
}
inline int iq_audio_batch(const char* where, const void* d_i, const void* d_q, int nseg, int samples, size_t seg_stride, float gain,
                          const void* d_pcm, size_t pcm_stride) {
    if (const int bad = iq_audio_args_bad(where, nseg, samples, gain)) return bad;
    if (const int bad = rows_bad(where, d_i, d_q, nseg)) return bad;
    if (const int bad = row_stride_bad(where, seg_stride, samples, nseg)) return bad;
    return pcm_bad(where, d_pcm, pcm_stride, (size_t)IQ_AUDIO_INTERP * (size_t)samples, nseg, "32 * samples");
}
inline int iq_audio_host(const char* where, const void* I, const void* Q, int samples, float gain, const void* pcm) {
    if (const int bad = iq_audio_args_bad(where, 1, samples, gain)) return bad;
    return ((!I || !Q || !pcm) && samples) ? refuse(where, "no row or no output record") : 0;
}
// wspr_waterfall_batch_device(): the image rows are written with aligned 16-byte vector stores
inline int waterfall_batch(const char* where, const void* d_i, const void* d_q, int nseg, int samples, size_t seg_stride,
                           const wspr_waterfall_params* p, const void* d_img, size_t img_stride, const void* info,
                           waterfall::Params* use) {
    if (const int bad = waterfall_args_bad(where, nseg, samples, p, info, use)) return bad;
    if (const int bad = rows_bad(where, d_i, d_q, nseg)) return bad;
    if (const int bad = row_stride_bad(where, seg_stride, samples, nseg)) return bad;
    if (nseg > 0 && !aligned16(d_img)) return refuse(where, "d_img must be 16-byte aligned device memory");
    const size_t need = (size_t)waterfall::rows_of(samples, use->hop, use->tavg) * (size_t)waterfall::cols_of(use->j0, use->j1);
    if (nseg > 0 && ((img_stride & 15) || img_stride < need))
        return refuse(where, "img_stride must be a multiple of 16 and at least nrows * ncols");
    return 0;
}
inline int waterfall_host(const char* where, const void* I, const void* Q, int samples, const wspr_waterfall_params* p,
                          const void* img, const void* info, waterfall::Params* use) {
    if (const int bad = waterfall_args_bad(where, 1, samples, p, info, use)) return bad;
    if ((!I || !Q) && samples) return refuse(where, "no row");
    return (!img && waterfall::rows_of(samples, use->hop, use->tavg) > 0) ? refuse(where, "no image") : 0;
}
// wspr_tune_u8_batch_device(): the raw rows are read with aligned 16-byte vector loads
inline int tune_batch(const char* where, const void* d_raw, size_t bytes_per_seg, int nseg, const void* steps, int nbands,
                      const void* d_i, const void* d_q) {
    if (const int bad = tune_args_bad(where, nseg, steps, nbands)) return bad;
    if (bytes_per_seg & 15) return refuse(where, "bytes_per_seg must be a multiple of 16");
    if (nseg > 0 && !aligned16(d_raw)) return refuse(where, "d_raw must be 16-byte aligned device memory");
    return rows_bad(where, d_i, d_q, nseg);
}
inline int tune_host(const char* where, const void* iq, size_t nbytes, const void* steps, int nbands, const void* I, const void* Q) {
    if (const int bad = tune_args_bad(where, 1, steps, nbands)) return bad;
    return ((!iq && nbytes) || !I || !Q) ? refuse(where, "no capture, or no output rows") : 0;
}
// wspr_spot_quality_batch_device() (K19): n host vectors of 162 bytes, n x 11 bytes of decdata, n records out
inline int spot_quality_batch(const char* where, const void* symbols, const void* decdata, int n, const void* out) {
    if (n < 0) return refuse(where, "negative count");
    if (n > 0 && (!symbols || !decdata)) return refuse(where, "no vectors or no decdata");
    if (n > 0 && !out) return refuse(where, "no output records");
    return 0;
}

}  // namespace args
}  // namespace wspr
