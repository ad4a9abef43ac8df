// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): the signal synthesiser -- wspr_synth_batch_device(),
// wspr_synth() and wspr_selftest(), the reference's decoderSelfTest() (rtlsdr_wsprd.c:729-789) on the device -- and the
// same two calls with an HF fading channel per transmission, wspr_synth_faded_batch_device() and wspr_synth_faded().
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "wspr_capi_impl.h"
#include "wspr_context_impl.h"
#include "../kernels/fade.h"

using wspr::Context;
using namespace wspr::capi;

static_assert(sizeof(wspr_synth_channel) == 24 && sizeof(wspr_synth_path) == 12, "public channel layout");
static_assert(sizeof(wspr_synth_tx) == 184 && sizeof(wspr_synth_tx) == sizeof(wspr::SynthTx),
              "public and device transmission layouts differ");

namespace wspr {

int Context::synth_device(const wspr_synth_tx* tx, int ntx, int nseg, long long seg_index0, float sigma, uint64_t seed,
                          int flags, float* dI, float* dQ, const FadeChannel* fade) {
    Impl& c = *d;
    if (nseg <= 0) return 0;
    const hipStream_t st = c.stream;
    std::vector<int> off((size_t)nseg + 1, 0);                 // the list is sorted by seg: offsets per segment
    for (int t = 0; t < ntx; ++t) ++off[(size_t)tx[t].seg + 1];
    for (int s = 0; s < nseg; ++s) off[(size_t)s + 1] += off[s];
    int* d_off = static_cast<int*>(c.synthoff.need(off.size() * sizeof(int)));
    upload(d_off, off.data(), off.size() * sizeof(int), st);
    SynthTx* d_tx = nullptr;
    double* d_ckpt = nullptr;
    int* d_first = nullptr;
    if (ntx > 0) {
        d_tx = static_cast<SynthTx*>(c.synthtx.need((size_t)ntx * sizeof(SynthTx)));
        d_first = static_cast<int*>(c.synthfirst.need((size_t)ntx * sizeof(int)));
        d_ckpt = static_cast<double*>(c.synthckpt.need(synth_checkpoint_doubles(ntx) * sizeof(double)));
        upload(d_tx, tx, (size_t)ntx * sizeof(SynthTx), st);
    }
    if (fade) {
        FadeChannel* d_fade = nullptr;
        if (ntx > 0) {
            d_fade = static_cast<FadeChannel*>(c.synthfade.need((size_t)ntx * sizeof(FadeChannel)));
            upload(d_fade, fade, (size_t)ntx * sizeof(FadeChannel), st);
        }
        launch_synth_faded(d_tx, d_fade, ntx, d_off, nseg, seg_index0, sigma, (unsigned long long)seed,
                           (flags & kSynthFlagAccumulate) != 0, d_ckpt, d_first, dI, dQ, st);
    } else {
        launch_synth(d_tx, ntx, d_off, nseg, seg_index0, sigma, (unsigned long long)seed, (flags & kSynthFlagAccumulate) != 0,
                     d_ckpt, d_first, dI, dQ, st);
    }
    if (flags & kSynthFlagNormalise) launch_normalise(dI, dQ, nullptr, nseg, kMaxSamples, st);   // rtlsdr_wsprd.c:290-305
    HIP_OK(hipGetLastError());
    if (c.blocking) {                                          // off / tx are host memory of this call: wait either way
        HIP_OK(hipEventRecord(c.ev_sync, st));
        host_wait(c.ev_sync);
    } else {
        HIP_OK(hipStreamSynchronize(st));
    }
    return 0;
}

float* Context::synth_rows() { return static_cast<float*>(d->synthrows.need((size_t)2 * kIqStride * sizeof(float))); }

}  // namespace wspr

namespace {
// Everything that can be wrong with a call, checked before anything is written.  No flag names in the texts: the
// product binary carries no new macro-style string (tests/test_abi.py).
bool synth_args_ok(const char* where, const wspr_synth_tx* tx, int ntx, int nseg, float sigma, int flags) {
    const char* why = nullptr;
    if (ntx < 0 || nseg < 0) why = "negative count";
    else if (ntx > 0 && !tx) why = "no transmission list";
    else if (!std::isfinite(sigma)) why = "noise_sigma is not finite";
    else if (flags & ~(wspr::kSynthFlagAccumulate | wspr::kSynthFlagNormalise)) why = "unknown flag bit";
    for (int t = 0; t < ntx && !why; ++t) {
        const wspr_synth_tx& x = tx[t];
        if (x.seg < 0 || x.seg >= nseg) why = "seg outside the batch";
        else if (t > 0 && x.seg < tx[t - 1].seg) why = "list not sorted by seg";
        else if (!std::isfinite(x.f0) || !std::isfinite(x.t0) || !std::isfinite(x.amp) || !std::isfinite(x.drift))
            why = "f0, t0, amp or drift is not finite";
        else if (std::fabs((double)x.f0) + std::fabs((double)x.drift) / 2.0 > wspr::kSynthMaxHz)
            why = "|f0| + |drift|/2 above 1000 Hz";
        else
            for (int i = 0; i < 162; ++i) if (x.symbols[i] > 3) { why = "channel symbol above 3"; break; }
        if (why) { fprintf(stderr, "libwspr_mi355x: %s: transmission %d: %s\n", where, t, why); return false; }
    }
    if (why) { fprintf(stderr, "libwspr_mi355x: %s: %s\n", where, why); return false; }
    return true;
}
// The channels of a faded call, likewise; fills `out` with the constants the kernel takes (fade.h).
bool fade_args_ok(const char* where, const wspr_synth_channel* ch, int ntx, std::vector<wspr::FadeChannel>& out) {
    out.resize((size_t)ntx);
    for (int t = 0; t < ntx; ++t)
        for (int p = 0; p < 2; ++p) {
            const wspr_synth_path& a = ch[t].path[p];
            const char* why = nullptr;
            if (!std::isfinite(a.gain) || !std::isfinite(a.shift) || !std::isfinite(a.sigma)) why = "gain, shift or sigma is not finite";
            else if (a.sigma != 0.0f && !(a.sigma >= wspr::kFadeMinSigma && a.sigma <= wspr::kFadeMaxSigma))
                why = "sigma neither 0 nor within 0.001 .. 10 Hz";
            else if (std::fabs(a.shift) > wspr::kFadeMaxShift) why = "|shift| above 100 Hz";
            if (why) { fprintf(stderr, "libwspr_mi355x: %s: transmission %d, path %d: %s\n", where, t, p, why); return false; }
            out[(size_t)t].path[p] = wspr::fade_path_setup(a.gain, a.shift, a.sigma);
        }
    return true;
}
}  // namespace

extern "C" {

int wspr_synth_batch_device(const wspr_synth_tx* tx, int ntx, int nseg, int seg_index0, float noise_sigma, uint64_t seed,
                            int flags, void* d_idat, void* d_qdat) {
    LaneTurn lane_turn;
    try {
        if (!synth_args_ok("wspr_synth_batch_device", tx, ntx, nseg, noise_sigma, flags)) return -1;
        if (nseg > 0 && (!d_idat || !d_qdat || ((reinterpret_cast<uintptr_t>(d_idat) | reinterpret_cast<uintptr_t>(d_qdat)) & 15))) {
            fprintf(stderr, "libwspr_mi355x: wspr_synth_batch_device: d_idat and d_qdat must be 16-byte aligned device rows\n");
            return -1;
        }
        return Context::get().synth_device(tx, ntx, nseg, seg_index0, noise_sigma, seed, flags, (float*)d_idat, (float*)d_qdat);
    } catch (const std::exception& e) { return fail("wspr_synth_batch_device", e); }
}

int wspr_synth_faded_batch_device(const wspr_synth_tx* tx, const wspr_synth_channel* ch, int ntx, int nseg, int seg_index0,
                                  float noise_sigma, uint64_t seed, int flags, void* d_idat, void* d_qdat) {
    LaneTurn lane_turn;
    try {
        std::vector<wspr::FadeChannel> fade;
        if (!synth_args_ok("wspr_synth_faded_batch_device", tx, ntx, nseg, noise_sigma, flags)) return -1;
        if (ch && !fade_args_ok("wspr_synth_faded_batch_device", ch, ntx, fade)) return -1;
        if (nseg > 0 && (!d_idat || !d_qdat || ((reinterpret_cast<uintptr_t>(d_idat) | reinterpret_cast<uintptr_t>(d_qdat)) & 15))) {
            fprintf(stderr, "libwspr_mi355x: wspr_synth_faded_batch_device: d_idat and d_qdat must be 16-byte aligned device rows\n");
            return -1;
        }
        return Context::get().synth_device(tx, ntx, nseg, seg_index0, noise_sigma, seed, flags, (float*)d_idat, (float*)d_qdat,
                                           ch ? fade.data() : nullptr);
    } catch (const std::exception& e) { return fail("wspr_synth_faded_batch_device", e); }
}

// wspr_synth() and wspr_synth_faded(): one segment through the context's working rows
static int synth_host(const char* where, const wspr_synth_tx* tx, const wspr_synth_channel* ch, int ntx, float noise_sigma,
                      uint64_t seed, int flags, float* I, float* Q) {
    try {
        std::vector<wspr::FadeChannel> fade;
        if (!synth_args_ok(where, tx, ntx, 1, noise_sigma, flags)) return -1;
        if (ch && !fade_args_ok(where, ch, ntx, fade)) return -1;
        if (!I || !Q) { fprintf(stderr, "libwspr_mi355x: %s: no output rows\n", where); return -1; }
        Context& c = Context::get();
        float* wi = c.work_i(1);
        float* wq = c.work_q(1);
        const size_t bytes = (size_t)wspr::kMaxSamples * sizeof(float);
        if (flags & wspr::kSynthFlagAccumulate) {
            HIP_TRY(hipMemcpy(wi, I, bytes, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(wq, Q, bytes, hipMemcpyHostToDevice));
        }
        const int rc = c.synth_device(tx, ntx, 1, 0, noise_sigma, seed, flags, wi, wq, ch ? fade.data() : nullptr);
        if (rc) return rc;
        std::vector<float> oi(wspr::kMaxSamples), oq(wspr::kMaxSamples);    // both rails arrive before either is handed over
        HIP_TRY(hipMemcpy(oi.data(), wi, bytes, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(oq.data(), wq, bytes, hipMemcpyDeviceToHost));
        std::memcpy(I, oi.data(), bytes);
        std::memcpy(Q, oq.data(), bytes);
        return 0;
    } catch (const std::exception& e) { return fail(where, e); }
}

int wspr_synth(const wspr_synth_tx* tx, int ntx, float noise_sigma, uint64_t seed, int flags, float* I, float* Q) {
    LaneTurn lane_turn;
    return synth_host("wspr_synth", tx, nullptr, ntx, noise_sigma, seed, flags, I, Q);
}

int wspr_synth_faded(const wspr_synth_tx* tx, const wspr_synth_channel* ch, int ntx, float noise_sigma, uint64_t seed, int flags,
                     float* I, float* Q) {
    LaneTurn lane_turn;
    return synth_host("wspr_synth_faded", tx, ch, ntx, noise_sigma, seed, flags, I, Q);
}

// decoderSelfTest(), rtlsdr_wsprd.c:729-789: "K1JT FN20QI 20" at 50 Hz, 2.0 s, amplitude 1 over noise of 0.02,
// generated and decoded without the samples leaving the device; 1 / 0 by the rule of :782-788.
int wspr_selftest(struct decoder_options options, struct decoder_results* first) {
    LaneTurn lane_turn;
    try {
        wspr_synth_tx tx;
        std::memset(&tx, 0, sizeof tx);
        tx.f0 = 50.0f; tx.t0 = 2.0f; tx.amp = 1.0f;
        char message[] = "K1JT FN20QI 20";
        std::vector<char> hashtab((size_t)HASHTAB_SIZE * HASHTAB_ENTRY_LEN, 0), loctab((size_t)HASHTAB_SIZE * LOCTAB_ENTRY_LEN, 0);
        get_wspr_channel_symbols(message, hashtab.data(), loctab.data(), tx.symbols);
        Context& c = Context::get();
        float* rows = c.synth_rows();
        const int rc = c.synth_device(&tx, 1, 1, 0, 0.02f, 1, 0, rows, rows + wspr::kIqStride);
        if (rc) return rc < 0 ? rc : -1;
        std::vector<decoder_results> spots(50);                // dec_results of the reference's caller holds 50
        std::memset(spots.data(), 0, spots.size() * sizeof(decoder_results));
        int n = 0;
        const int drc = wspr_decode_batch_device(rows, rows + wspr::kIqStride, 1, wspr::kMaxSamples, wspr::kIqStride, options,
                                                 spots.data(), (int)spots.size(), &n);
        if (drc < 0) return drc;
        if (first) *first = spots[0];
        return (strcmp(spots[0].call, "K1JT") || strcmp(spots[0].loc, "FN20") || strcmp(spots[0].pwr, "20")) ? 0 : 1;
    } catch (const std::exception& e) { const int rc = fail("wspr_selftest", e); return rc; }
}

}  // extern "C"
