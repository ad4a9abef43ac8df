// The stage calls' argument checks (rtlsdr-wsprd_amd/csrc/host/wspr_stage_args.h) on a fixed table of calls: one line per
// case, "<entry point>/<case> <code> |<what the check wrote to stderr>".  A stand-alone program: no library is loaded and
// no device touched; the "device" pointers are addresses that are never dereferenced.  tests/test_stage_args.py holds the
// lines to what the entry points answered before the checks were gathered in that header.  TEST INFRASTRUCTURE ONLY.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <unistd.h>
#include <vector>

#include "wspr_stage_args.h"

namespace a = wspr::args;

static FILE* g_err = nullptr;   // stderr lands here

static void run(const std::string& id, int rc) {
    fflush(stderr);
    char text[512];
    const ssize_t got = pread(2, text, sizeof text - 1, 0);     // fd 2 is the temporary file: what this case wrote
    text[got > 0 ? got : 0] = 0;
    for (char* p = text; *p; ++p) if (*p == '\n') *p = p[1] ? ' ' : 0;
    if (ftruncate(2, 0) || lseek(2, 0, SEEK_SET)) {}
    printf("%s %d |%s\n", id.c_str(), rc, text);
}

static void* const kOk = reinterpret_cast<void*>(0x10000);      // 16-byte aligned
static void* const kOk2 = reinterpret_cast<void*>(0x4000000);   // another one, far away
static void* const kOdd = reinterpret_cast<void*>(0x10004);     // not aligned

static wspr_synth_tx tx_of(int seg) {
    wspr_synth_tx x;
    memset(&x, 0, sizeof x);
    x.seg = seg; x.f0 = 10.0f; x.t0 = 2.0f; x.amp = 1.0f;
    return x;
}

// a transmission list and the scalars checked with it
struct List {
    const char* id;
    std::vector<wspr_synth_tx> tx;
    int ntx;
    bool null_list;
    float sigma;
    int flags;
    const wspr_synth_tx* p() const { return null_list ? nullptr : tx.data(); }
};
static std::vector<List> lists(int nseg) {
    std::vector<List> l;
    auto add = [&](const char* id, std::function<void(List&)> f) {
        List x{id, {tx_of(0)}, 1, false, 0.5f, 0};
        f(x);
        l.push_back(x);
    };
    add("fine", [](List&) {});
    add("empty_list_null", [](List& x) { x.ntx = 0; x.null_list = true; });
    add("ntx_negative_and_null_list", [](List& x) { x.ntx = -1; x.null_list = true; });
    add("no_list", [](List& x) { x.null_list = true; });
    add("sigma_nan", [](List& x) { x.sigma = NAN; });
    add("sigma_negative", [](List& x) { x.sigma = -1.0f; });
    add("sigma_negative_and_flag_bit_4", [](List& x) { x.sigma = -1.0f; x.flags = 4; });
    add("sigma_2e6", [](List& x) { x.sigma = 2.0e6f; });
    add("flag_bit_2", [](List& x) { x.flags = 2; });
    add("flag_bit_4", [](List& x) { x.flags = 4; });
    add("seg_negative", [](List& x) { x.tx[0].seg = -1; });
    add("seg_outside", [nseg](List& x) { x.tx[0].seg = nseg; });
    add("unsorted", [nseg](List& x) { x.tx[0].seg = nseg - 1; x.tx.push_back(tx_of(nseg - 2)); x.ntx = 2; });
    add("f0_nan", [](List& x) { x.tx[0].f0 = NAN; });
    add("drift_inf", [](List& x) { x.tx[0].drift = INFINITY; });
    add("amp_2e6", [](List& x) { x.tx[0].amp = 2.0e6f; });
    add("amp_2e6_and_900_hz", [](List& x) { x.tx[0].amp = -2.0e6f; x.tx[0].f0 = 900.0f; });
    add("900_hz", [](List& x) { x.tx[0].f0 = 900.0f; });
    add("700_hz_and_drift_300", [](List& x) { x.tx[0].f0 = -700.0f; x.tx[0].drift = 300.0f; });
    add("1100_hz", [](List& x) { x.tx[0].f0 = 1100.0f; });
    add("symbol_4_in_second", [](List& x) { x.tx.push_back(tx_of(0)); x.tx[1].symbols[161] = 4; x.ntx = 2; });
    return l;
}

// one wspr_synth_channel per transmission of the longest list
struct Fade {
    const char* id;
    bool null_ch;
    wspr_synth_channel ch[2];
};
static std::vector<Fade> fades() {
    std::vector<Fade> l;
    auto add = [&](const char* id, std::function<void(Fade&)> f) {
        Fade x{id, false, {}};
        for (auto& c : x.ch) { c.path[0] = {1.0f, 0.0f, 0.5f}; c.path[1] = {0.5f, 1.0f, 0.0f}; }
        f(x);
        l.push_back(x);
    };
    add("fine", [](Fade&) {});
    add("no_channels", [](Fade& x) { x.null_ch = true; });
    add("gain_nan", [](Fade& x) { x.ch[0].path[0].gain = NAN; });
    add("sigma_20", [](Fade& x) { x.ch[0].path[1].sigma = 20.0f; });
    add("sigma_1e-4", [](Fade& x) { x.ch[0].path[0].sigma = 1.0e-4f; });
    add("sigma_negative", [](Fade& x) { x.ch[0].path[0].sigma = -1.0f; });
    add("shift_200", [](Fade& x) { x.ch[0].path[1].shift = -200.0f; });
    add("sigma_20_and_shift_200", [](Fade& x) { x.ch[0].path[0].sigma = 20.0f; x.ch[0].path[0].shift = 200.0f; });
    return l;
}

int main() {
    g_err = tmpfile();
    if (!g_err || dup2(fileno(g_err), 2) < 0) return 2;
    std::vector<wspr::FadeChannel> fc;
    const List fine{"fine", {tx_of(0)}, 1, false, 0.5f, 0};

    // ---- K8 and K13 -----------------------------------------------------------------------------------------------------
    for (const char* where : {"wspr_synth_batch_device", "wspr_synth_faded_batch_device"}) {
        const std::string w = std::string(where) + "/";
        const bool faded = strstr(where, "faded") != nullptr;
        const Fade ok = fades()[0];
        const wspr_synth_channel* ch = faded ? ok.ch : nullptr;
        for (const List& l : lists(2)) run(w + l.id, a::synth_batch(where, l.p(), ch, l.ntx, 2, l.sigma, l.flags, kOk, kOk2, fc));
        run(w + "nseg_negative", a::synth_batch(where, nullptr, ch, 0, -1, 0.f, 0, kOk, kOk2, fc));
        run(w + "nseg_0_and_bad_rows", a::synth_batch(where, nullptr, ch, 0, 0, 0.f, 0, nullptr, kOdd, fc));
        run(w + "no_i", a::synth_batch(where, fine.p(), ch, 1, 2, 0.f, 0, nullptr, kOk2, fc));
        run(w + "no_q", a::synth_batch(where, fine.p(), ch, 1, 2, 0.f, 0, kOk, nullptr, fc));
        run(w + "q_misaligned", a::synth_batch(where, fine.p(), ch, 1, 2, 0.f, 0, kOk, kOdd, fc));
        run(w + "flag_bit_4_and_q_misaligned", a::synth_batch(where, fine.p(), ch, 1, 2, 0.f, 4, kOk, kOdd, fc));
        if (faded) {
            for (const Fade& f : fades())
                run(w + "channel_" + f.id, a::synth_batch(where, fine.p(), f.null_ch ? nullptr : f.ch, 1, 2, 0.f, 0, kOk, kOk2, fc));
            const Fade bad = fades()[3];                       // sigma_20
            run(w + "channel_sigma_20_and_q_misaligned", a::synth_batch(where, fine.p(), bad.ch, 1, 2, 0.f, 0, kOk, kOdd, fc));
            run(w + "1100_hz_and_channel_sigma_20", a::synth_batch(where, lists(2)[19].p() /* 1100_hz */, bad.ch, 1, 2, 0.f, 0, kOk, kOk2, fc));
        }
    }
    for (const char* where : {"wspr_synth", "wspr_synth_faded"}) {
        const std::string w = std::string(where) + "/";
        const bool faded = strstr(where, "faded") != nullptr;
        const Fade ok = fades()[0];
        const wspr_synth_channel* ch = faded ? ok.ch : nullptr;
        for (const List& l : lists(1)) run(w + l.id, a::synth_host(where, l.p(), ch, l.ntx, l.sigma, l.flags, kOdd, kOdd, fc));
        run(w + "no_i", a::synth_host(where, fine.p(), ch, 1, 0.f, 0, nullptr, kOk, fc));
        run(w + "no_q", a::synth_host(where, fine.p(), ch, 1, 0.f, 0, kOk, nullptr, fc));
        if (faded)
            for (const Fade& f : fades())
                run(w + "channel_" + f.id, a::synth_host(where, fine.p(), f.null_ch ? nullptr : f.ch, 1, 0.f, 0, kOdd, kOdd, fc));
    }

    // ---- K17 ------------------------------------------------------------------------------------------------------------
    {
        const char* where = "wspr_synth_audio_batch_device";
        const std::string w = std::string(where) + "/";
        for (const List& l : lists(2)) run(w + l.id, a::synth_audio_batch(where, l.p(), l.ntx, 2, 1000, l.sigma, l.flags, kOk, 1000));
        run(w + "nseg_negative", a::synth_audio_batch(where, nullptr, 0, -1, 1000, 0.f, 0, kOk, 1000));
        run(w + "nsamp_negative_and_no_pcm", a::synth_audio_batch(where, nullptr, 0, 2, -1, 0.f, 0, nullptr, 1000));
        run(w + "nsamp_1440000", a::synth_audio_batch(where, nullptr, 0, 2, 1440000, 0.f, 0, kOk, 1440000));
        run(w + "nsamp_1440001", a::synth_audio_batch(where, nullptr, 0, 2, 1440001, 0.f, 0, kOk, 1440008));
        run(w + "nsamp_1440001_and_pcm_misaligned", a::synth_audio_batch(where, nullptr, 0, 2, 1440001, 0.f, 0, kOdd, 1440008));
        run(w + "nsamp_1440001_and_sigma_nan", a::synth_audio_batch(where, nullptr, 0, 2, 1440001, NAN, 0, kOk, 1440008));
        run(w + "nseg_0_and_bad_pcm", a::synth_audio_batch(where, nullptr, 0, 0, 1000, 0.f, 0, kOdd, 3));
        run(w + "no_pcm", a::synth_audio_batch(where, fine.p(), 1, 2, 1000, 0.f, 0, nullptr, 1000));
        run(w + "pcm_misaligned", a::synth_audio_batch(where, fine.p(), 1, 2, 1000, 0.f, 0, kOdd, 1000));
        run(w + "pcm_misaligned_and_stride_odd", a::synth_audio_batch(where, fine.p(), 1, 2, 1000, 0.f, 0, kOdd, 1001));
        run(w + "stride_1004", a::synth_audio_batch(where, fine.p(), 1, 2, 1000, 0.f, 0, kOk, 1004));
        run(w + "stride_992", a::synth_audio_batch(where, fine.p(), 1, 2, 1000, 0.f, 0, kOk, 992));
        run(w + "flag_bit_2_and_stride_992", a::synth_audio_batch(where, fine.p(), 1, 2, 1000, 0.f, 2, kOk, 992));
    }
    {
        const char* where = "wspr_synth_audio";
        const std::string w = std::string(where) + "/";
        for (const List& l : lists(1)) run(w + l.id, a::synth_audio_host(where, l.p(), l.ntx, 1000, l.sigma, l.flags, kOdd));
        run(w + "nsamp_negative", a::synth_audio_host(where, nullptr, 0, -1, 0.f, 0, kOdd));
        run(w + "nsamp_1440001_and_no_record", a::synth_audio_host(where, nullptr, 0, 1440001, 0.f, 0, nullptr));
        run(w + "no_record", a::synth_audio_host(where, fine.p(), 1, 1000, 0.f, 0, nullptr));
        run(w + "nsamp_0_and_no_record", a::synth_audio_host(where, fine.p(), 1, 0, 0.f, 0, nullptr));
    }

    // ---- K12 and K15 ----------------------------------------------------------------------------------------------------
    // the same table for wspr_audio_batch_device() and, behind fine settings, wspr_audio_blanked_batch_device()
    for (const char* where : {"wspr_audio_batch_device", "wspr_audio_blanked_batch_device"}) {
        const std::string w = std::string(where) + "/";
        const bool blanked = strstr(where, "blanked") != nullptr;
        auto call = [&](const void* d_pcm, size_t stride, long long nsamp, int nseg, const void* d_i, const void* d_q) {
            return blanked ? a::audio_blanked_batch(where, d_pcm, stride, nsamp, nseg, 64, 2, d_i, d_q)
                           : a::audio_batch(where, d_pcm, stride, nsamp, nseg, d_i, d_q);
        };
        run(w + "fine", call(kOk, 1000, 1000, 2, kOk, kOk2));
        run(w + "nseg_negative_and_no_pcm", call(nullptr, 1000, 1000, -1, kOk, kOk2));
        run(w + "nsamp_negative", call(kOk, 1000, -1, 2, kOk, kOk2));
        run(w + "nsamp_1440000", call(kOk, 1440000, 1440000, 2, kOk, kOk2));
        run(w + "nsamp_1440001", call(kOk, 1440008, 1440001, 2, kOk, kOk2));
        run(w + "nsamp_1440001_and_pcm_misaligned", call(kOdd, 1440008, 1440001, 2, kOk, kOk2));
        run(w + "nsamp_1440001_and_nseg_0", call(kOk, 1440008, 1440001, 0, kOk, kOk2));
        run(w + "nseg_0_and_bad_pointers", call(kOdd, 3, 1000, 0, nullptr, kOdd));
        run(w + "no_pcm", call(nullptr, 1000, 1000, 2, kOk, kOk2));
        run(w + "pcm_misaligned", call(kOdd, 1000, 1000, 2, kOk, kOk2));
        run(w + "stride_1004", call(kOk, 1004, 1000, 2, kOk, kOk2));
        run(w + "stride_992", call(kOk, 992, 1000, 2, kOk, kOk2));
        run(w + "stride_992_and_no_rows", call(kOk, 992, 1000, 2, nullptr, nullptr));
        run(w + "no_i", call(kOk, 1000, 1000, 2, nullptr, kOk2));
        run(w + "no_q", call(kOk, 1000, 1000, 2, kOk, nullptr));
        run(w + "i_misaligned", call(kOk, 1000, 1000, 2, kOdd, kOk2));
        if (blanked) {
            run(w + "thr16_15", a::audio_blanked_batch(where, kOk, 1000, 1000, 2, 15, 2, kOk, kOk2));
            run(w + "guard_65_and_nsamp_1440001", a::audio_blanked_batch(where, kOk, 1440008, 1440001, 2, 64, 65, kOk, kOk2));
        }
    }
    {
        const char* where = "wspr_audio_blank_batch_device";
        const std::string w = std::string(where) + "/";
        auto call = [&](const void* d_pcm, size_t stride, long long nsamp, int nseg, const void* d_out, size_t out_stride, int thr16 = 64,
                        int guard = 2) { return a::audio_blank_batch(where, d_pcm, stride, nsamp, nseg, thr16, guard, d_out, out_stride); };
        run(w + "fine", call(kOk, 1000, 1000, 2, kOk2, 1000));
        run(w + "thr16_15", call(kOk, 1000, 1000, 2, kOk2, 1000, 15, 2));
        run(w + "thr16_4097", call(kOk, 1000, 1000, 2, kOk2, 1000, 4097, 2));
        run(w + "guard_negative", call(kOk, 1000, 1000, 2, kOk2, 1000, 64, -1));
        run(w + "guard_65_and_nsamp_1440001", call(kOk, 1440008, 1440001, 2, kOk2, 1440008, 64, 65));
        run(w + "nseg_negative_and_no_pcm", call(nullptr, 1000, 1000, -1, kOk2, 1000));
        run(w + "nsamp_negative", call(kOk, 1000, -1, 2, kOk2, 1000));
        run(w + "nsamp_1440001", call(kOk, 1440008, 1440001, 2, kOk2, 1440008));
        run(w + "nsamp_1440001_and_out_misaligned", call(kOk, 1440008, 1440001, 2, kOdd, 1440008));
        run(w + "nseg_0_and_bad_pointers", call(kOdd, 3, 1000, 0, nullptr, 5));
        run(w + "no_pcm", call(nullptr, 1000, 1000, 2, kOk2, 1000));
        run(w + "pcm_misaligned", call(kOdd, 1000, 1000, 2, kOk2, 1000));
        run(w + "stride_1004", call(kOk, 1004, 1000, 2, kOk2, 1000));
        run(w + "stride_992_and_no_out", call(kOk, 992, 1000, 2, nullptr, 1000));
        run(w + "no_out", call(kOk, 1000, 1000, 2, nullptr, 1000));
        run(w + "out_misaligned", call(kOk, 1000, 1000, 2, kOdd, 1000));
        run(w + "out_stride_1004", call(kOk, 1000, 1000, 2, kOk2, 1004));
        run(w + "out_stride_992", call(kOk, 1000, 1000, 2, kOk2, 992));
        run(w + "out_stride_992_in_place", call(kOk, 1000, 1000, 2, kOk, 992));
        run(w + "in_place", call(kOk, 1000, 1000, 2, kOk, 1000));
        run(w + "out_begins_in_the_last_input_row", call(kOk, 1000, 1000, 2, reinterpret_cast<char*>(kOk) + 2 * 1992, 1000));
        run(w + "out_begins_behind_the_last_input_row", call(kOk, 1000, 1000, 2, reinterpret_cast<char*>(kOk) + 2 * 2000, 1000));
        run(w + "in_place_and_nsamp_0", call(kOk, 1000, 0, 2, kOk, 1000));
    }
    for (const char* where : {"wspr_audio_to_iq", "wspr_audio_to_iq_blanked"}) {
        const std::string w = std::string(where) + "/";
        const int fine_settings[2] = {64, 2}, thr_15[2] = {15, 2}, guard_65[2] = {64, 65};
        const int* s = strstr(where, "blanked") ? fine_settings : nullptr;
        run(w + "fine", a::audio_host(where, kOdd, 1000, s, kOdd, kOdd));
        run(w + "nsamp_1440001_and_no_record", a::audio_host(where, nullptr, 1440001, s, kOdd, kOdd));
        run(w + "no_record", a::audio_host(where, nullptr, 1000, s, kOdd, kOdd));
        run(w + "nsamp_0_and_no_record", a::audio_host(where, nullptr, 0, s, kOdd, kOdd));
        run(w + "no_i", a::audio_host(where, kOdd, 1000, s, nullptr, kOdd));
        run(w + "nsamp_0_and_no_q", a::audio_host(where, kOdd, 0, s, kOdd, nullptr));
        if (s) {
            run(w + "thr16_15", a::audio_host(where, kOdd, 1000, thr_15, kOdd, kOdd));
            run(w + "guard_65_and_nsamp_1440001", a::audio_host(where, kOdd, 1440001, guard_65, kOdd, kOdd));
        }
    }

    // ---- K16 ------------------------------------------------------------------------------------------------------------
    {
        wspr::noise::Windows win;
        const wspr_noise_windows reversed{10, 9, 2672, 2790}, beyond{6, 42, 2672, 2813}, negative{-1, 42, 2672, 2790}, whole{0, 2812, 0, 2812};
        const char* where = "wspr_noise_batch_device";
        std::string w = std::string(where) + "/";
        auto call = [&](const void* d_i, const void* d_q, int nseg, int samples, size_t stride, const wspr_noise_windows* ww, const void* out) {
            return a::noise_batch(where, d_i, d_q, nseg, samples, stride, ww, out, &win);
        };
        run(w + "fine", call(kOk, kOk2, 2, 1000, 1000, nullptr, kOdd));
        run(w + "default_windows_are_6_42_2672_2790", !(win.pre_b0 == 6 && win.pre_b1 == 42 && win.post_b0 == 2672 && win.post_b1 == 2790));
        run(w + "whole_row_twice", call(kOk, kOk2, 2, 1000, 1000, &whole, kOdd));
        run(w + "the_windows_are_the_callers", !(win.pre_b0 == 0 && win.pre_b1 == 2812 && win.post_b0 == 0 && win.post_b1 == 2812));
        run(w + "nseg_negative_and_no_rows", call(nullptr, nullptr, -1, 1000, 1000, nullptr, kOdd));
        run(w + "samples_negative", call(kOk, kOk2, 2, -1, 1000, nullptr, kOdd));
        run(w + "samples_45000", call(kOk, kOk2, 2, 45000, 45000, nullptr, kOdd));
        run(w + "samples_45001", call(kOk, kOk2, 2, 45001, 45004, nullptr, kOdd));
        run(w + "samples_45001_and_q_misaligned", call(kOk, kOdd, 2, 45001, 45004, nullptr, kOdd));
        run(w + "samples_45001_and_window_reversed", call(kOk, kOk2, 2, 45001, 45004, &reversed, kOdd));
        run(w + "window_reversed", call(kOk, kOk2, 2, 1000, 1000, &reversed, kOdd));
        run(w + "window_beyond_the_row", call(kOk, kOk2, 2, 1000, 1000, &beyond, kOdd));
        run(w + "window_negative_and_no_out", call(kOk, kOk2, 2, 1000, 1000, &negative, nullptr));
        run(w + "no_out", call(kOk, kOk2, 2, 1000, 1000, nullptr, nullptr));
        run(w + "no_out_and_no_rows", call(nullptr, nullptr, 2, 1000, 1000, nullptr, nullptr));
        run(w + "nseg_0_and_bad_pointers", call(nullptr, kOdd, 0, 1000, 3, nullptr, nullptr));
        run(w + "no_i", call(nullptr, kOk2, 2, 1000, 1000, nullptr, kOdd));
        run(w + "q_misaligned", call(kOk, kOdd, 2, 1000, 1000, nullptr, kOdd));
        run(w + "q_misaligned_and_stride_odd", call(kOk, kOdd, 2, 1000, 1001, nullptr, kOdd));
        run(w + "stride_1002", call(kOk, kOk2, 2, 1000, 1002, nullptr, kOdd));
        run(w + "stride_996", call(kOk, kOk2, 2, 1000, 996, nullptr, kOdd));
        where = "wspr_noise";
        w = std::string(where) + "/";
        auto host = [&](const void* I, const void* Q, int samples, const wspr_noise_windows* ww, const void* out) {
            return a::noise_host(where, I, Q, samples, ww, out, &win);
        };
        run(w + "fine", host(kOdd, kOdd, 1000, nullptr, kOdd));
        run(w + "samples_negative", host(kOdd, kOdd, -1, nullptr, kOdd));
        run(w + "samples_45001_and_no_row", host(nullptr, nullptr, 45001, nullptr, kOdd));
        run(w + "window_reversed", host(kOdd, kOdd, 1000, &reversed, kOdd));
        run(w + "no_out_and_no_row", host(nullptr, nullptr, 1000, nullptr, nullptr));
        run(w + "no_i", host(nullptr, kOdd, 1000, nullptr, kOdd));
        run(w + "no_q", host(kOdd, nullptr, 1000, nullptr, kOdd));
        run(w + "samples_0_and_no_row", host(nullptr, nullptr, 0, nullptr, kOdd));
    }

    // ---- K18 ------------------------------------------------------------------------------------------------------------
    {
        const char* where = "wspr_iq_to_audio_batch_device";
        std::string w = std::string(where) + "/";
        auto call = [&](const void* d_i, const void* d_q, int nseg, int samples, size_t stride, float gain, const void* d_pcm, size_t pcm_stride) {
            return a::iq_audio_batch(where, d_i, d_q, nseg, samples, stride, gain, d_pcm, pcm_stride);
        };
        run(w + "fine", call(kOk, kOk2, 2, 1000, 1000, 32768.f, kOk, 32000));
        run(w + "nseg_negative_and_no_rows", call(nullptr, nullptr, -1, 1000, 1000, 1.f, kOk, 32000));
        run(w + "samples_negative", call(kOk, kOk2, 2, -1, 1000, 1.f, kOk, 32000));
        run(w + "samples_45000", call(kOk, kOk2, 2, 45000, 45000, 1.f, kOk, 1440000));
        run(w + "samples_45001", call(kOk, kOk2, 2, 45001, 45004, 1.f, kOk, 1440032));
        run(w + "samples_45001_and_i_misaligned", call(kOdd, kOk2, 2, 45001, 45004, 1.f, kOk, 1440032));
        run(w + "samples_45001_and_gain_nan", call(kOk, kOk2, 2, 45001, 45004, NAN, kOk, 1440032));
        run(w + "gain_nan", call(kOk, kOk2, 2, 1000, 1000, NAN, kOk, 32000));
        run(w + "gain_inf_and_no_rows", call(nullptr, nullptr, 2, 1000, 1000, INFINITY, kOk, 32000));
        run(w + "nseg_0_and_bad_pointers", call(nullptr, kOdd, 0, 1000, 3, 1.f, kOdd, 5));
        run(w + "no_q", call(kOk, nullptr, 2, 1000, 1000, 1.f, kOk, 32000));
        run(w + "i_misaligned_and_stride_odd", call(kOdd, kOk2, 2, 1000, 1001, 1.f, kOk, 32000));
        run(w + "stride_1002", call(kOk, kOk2, 2, 1000, 1002, 1.f, kOk, 32000));
        run(w + "stride_996_and_no_pcm", call(kOk, kOk2, 2, 1000, 996, 1.f, nullptr, 32000));
        run(w + "no_pcm", call(kOk, kOk2, 2, 1000, 1000, 1.f, nullptr, 32000));
        run(w + "pcm_misaligned_and_pcm_stride_odd", call(kOk, kOk2, 2, 1000, 1000, 1.f, kOdd, 32001));
        run(w + "pcm_stride_32004", call(kOk, kOk2, 2, 1000, 1000, 1.f, kOk, 32004));
        run(w + "pcm_stride_31992", call(kOk, kOk2, 2, 1000, 1000, 1.f, kOk, 31992));
        where = "wspr_iq_to_audio";
        w = std::string(where) + "/";
        run(w + "fine", a::iq_audio_host(where, kOdd, kOdd, 1000, 1.f, kOdd));
        run(w + "samples_negative", a::iq_audio_host(where, kOdd, kOdd, -1, 1.f, kOdd));
        run(w + "samples_45001_and_no_row", a::iq_audio_host(where, nullptr, nullptr, 45001, 1.f, kOdd));
        run(w + "gain_nan_and_no_row", a::iq_audio_host(where, nullptr, nullptr, 1000, NAN, kOdd));
        run(w + "no_i", a::iq_audio_host(where, nullptr, kOdd, 1000, 1.f, kOdd));
        run(w + "no_q", a::iq_audio_host(where, kOdd, nullptr, 1000, 1.f, kOdd));
        run(w + "no_record", a::iq_audio_host(where, kOdd, kOdd, 1000, 1.f, nullptr));
        run(w + "samples_0_and_nothing", a::iq_audio_host(where, nullptr, nullptr, 0, 1.f, nullptr));
    }
    return 0;
}
