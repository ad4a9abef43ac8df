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
#include "wspr_stage_args.h"

using wspr::Context;
using namespace wspr::capi;
namespace args = wspr::args;

static_assert(sizeof(wspr_synth_channel) == 24 && sizeof(wspr_synth_path) == 12, "public channel layout");
static_assert(sizeof(wspr_synth_tx) == 184 && sizeof(wspr_synth_tx) == sizeof(wspr::SynthTx),
              "public and device transmission layouts differ");

// wspr_synth_batch_device() and, with channels, wspr_synth_faded_batch_device()
static int synth_batch(const char* where, const wspr_synth_tx* tx, const wspr_synth_channel* ch, int ntx, int nseg, int seg_index0,
                       float noise_sigma, uint64_t seed, int flags, void* d_idat, void* d_qdat) {
    try {
        std::vector<wspr::FadeChannel> fade;                   // the constants the kernel takes, one per transmission (fade.h)
        if (const int bad = args::synth_batch(where, tx, ch, ntx, nseg, noise_sigma, flags, d_idat, d_qdat, fade)) return bad;
        return Context::get().synth_device(tx, ntx, nseg, seg_index0, noise_sigma, seed, flags, (float*)d_idat, (float*)d_qdat,
                                           ch ? fade.data() : nullptr);
    } catch (const std::exception& e) { return fail(where, e); }
}

// wspr_synth() and wspr_synth_faded(): one segment through the context's working rows
static int synth_host(const char* where, const wspr_synth_tx* tx, const wspr_synth_channel* ch, int ntx, float noise_sigma,
                      uint64_t seed, int flags, float* I, float* Q) {
    try {
        std::vector<wspr::FadeChannel> fade;
        if (const int bad = args::synth_host(where, tx, ch, ntx, noise_sigma, flags, I, Q, fade)) return bad;
        Context& c = Context::get();
        float* wi = c.work_i(1);
        float* wq = c.work_q(1);
        if (flags & wspr::kSynthFlagAccumulate) rows_up(wi, wq, I, Q, wspr::kMaxSamples);
        const int rc = c.synth_device(tx, ntx, 1, 0, noise_sigma, seed, flags, wi, wq, ch ? fade.data() : nullptr);
        if (rc) return rc;
        rows_down(I, Q, wi, wq);
        return 0;
    } catch (const std::exception& e) { return fail(where, e); }
}

extern "C" {

int wspr_synth_batch_device(const wspr_synth_tx* tx, int ntx, int nseg, int seg_index0, float noise_sigma, uint64_t seed,
                            int flags, void* d_idat, void* d_qdat) {
    LaneTurn lane_turn;
    return synth_batch("wspr_synth_batch_device", tx, nullptr, ntx, nseg, seg_index0, noise_sigma, seed, flags, d_idat, d_qdat);
}

int wspr_synth_faded_batch_device(const wspr_synth_tx* tx, const wspr_synth_channel* ch, int ntx, int nseg, int seg_index0,
                                  float noise_sigma, uint64_t seed, int flags, void* d_idat, void* d_qdat) {
    LaneTurn lane_turn;
    return synth_batch("wspr_synth_faded_batch_device", tx, ch, ntx, nseg, seg_index0, noise_sigma, seed, flags, d_idat, d_qdat);
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
