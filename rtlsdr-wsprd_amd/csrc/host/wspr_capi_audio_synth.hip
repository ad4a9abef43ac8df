// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): the 12 kHz audio scene synthesiser (K17) --
// wspr_synth_audio_batch_device() and wspr_synth_audio(), the definition in kernels/audio_synth.h.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "wspr_capi_impl.h"
#include "wspr_context_impl.h"
#include "../kernels/audio_synth.h"

using wspr::Context;
using namespace wspr::capi;

static_assert(wspr::kAudioSynthMaxSamples == WSPR_AUDIO_MAX_SAMPLES, "public and internal record lengths differ");
static_assert(wspr::kSynthFlagAccumulate == WSPR_SYNTH_ACCUMULATE, "public and internal flag bits differ");

namespace wspr {

int Context::synth_audio_device(const wspr_synth_tx* tx, int ntx, int nseg, long long seg_index0, int nsamp, float sigma,
                                uint64_t seed, int flags, int16_t* d_pcm, size_t pcm_stride, int* h_clipped) {
    Impl& c = *d;
    if (nseg <= 0) return 0;
    const hipStream_t st = c.stream;
    std::vector<int> off((size_t)nseg + 1, 0);                 // the list is sorted by seg: offsets per segment
    for (int t = 0; t < ntx; ++t) ++off[(size_t)tx[t].seg + 1];
    for (int s = 0; s < nseg; ++s) off[(size_t)s + 1] += off[s];
    int* d_off = static_cast<int*>(c.synthoff.need(off.size() * sizeof(int)));
    upload(d_off, off.data(), off.size() * sizeof(int), st);
    SynthTx* d_tx = nullptr;
    double* d_phase = nullptr;
    int* d_first = nullptr;
    if (ntx > 0) {
        d_tx = static_cast<SynthTx*>(c.synthtx.need((size_t)ntx * sizeof(SynthTx)));
        d_first = static_cast<int*>(c.synthfirst.need((size_t)ntx * sizeof(int)));
        d_phase = static_cast<double*>(c.asynthphase.need(audio_synth_phase_doubles(ntx) * sizeof(double)));
        upload(d_tx, tx, (size_t)ntx * sizeof(SynthTx), st);
    }
    int* d_count = static_cast<int*>(c.asynthcount.need((size_t)nseg * sizeof(int)));
    HIP_OK(hipMemsetAsync(d_count, 0, (size_t)nseg * sizeof(int), st));
    launch_audio_synth(d_tx, ntx, d_off, nseg, seg_index0, nsamp, sigma, (unsigned long long)seed,
                       (flags & kSynthFlagAccumulate) != 0, d_phase, d_first, d_pcm, pcm_stride, d_count, st);
    HIP_OK(hipGetLastError());
    if (h_clipped) HIP_OK(hipMemcpyAsync(h_clipped, d_count, (size_t)nseg * sizeof(int), hipMemcpyDeviceToHost, st));
    if (c.blocking) {                                          // off / tx are host memory of this call: wait either way
        HIP_OK(hipEventRecord(c.ev_sync, st));
        host_wait(c.ev_sync);
    } else {
        HIP_OK(hipStreamSynchronize(st));
    }
    return 0;
}

}  // namespace wspr

namespace {
// Everything that can be wrong with a call, checked before anything is written: 0, -1 or -2.  No flag names in the texts:
// the product binary carries no new macro-style string (tests/test_abi.py).
int synth_audio_args_bad(const char* where, const wspr_synth_tx* tx, int ntx, int nseg, long long nsamp, float sigma, int flags) {
    const char* why = nullptr;
    if (ntx < 0 || nseg < 0 || nsamp < 0) why = "negative count";
    else if (nsamp > wspr::kAudioSynthMaxSamples) {
        fprintf(stderr, "libwspr_mi355x: %s: a record holds at most 1440000 samples (120 s)\n", where);
        return -2;
    }
    else if (ntx > 0 && !tx) why = "no transmission list";
    else if (!std::isfinite(sigma)) why = "noise_sigma is not finite";
    else if (sigma < 0.0f) why = "noise_sigma is negative";
    else if ((double)sigma > wspr::kAudioSynthMaxLevel) why = "noise_sigma above 1e6";
    else if (flags & ~wspr::kSynthFlagAccumulate) why = "unknown flag bit";
    for (int t = 0; t < ntx && !why; ++t) {
        const wspr_synth_tx& x = tx[t];
        if (x.seg < 0 || x.seg >= nseg) why = "seg outside the batch";
        else if (t > 0 && x.seg < tx[t - 1].seg) why = "list not sorted by seg";
        else if (!std::isfinite(x.f0) || !std::isfinite(x.t0) || !std::isfinite(x.amp) || !std::isfinite(x.drift))
            why = "f0, t0, amp or drift is not finite";
        else if (std::fabs((double)x.amp) > wspr::kAudioSynthMaxLevel) why = "|amp| above 1e6";
        else if (std::fabs((double)x.f0) + std::fabs((double)x.drift) / 2.0 > wspr::kAudioSynthMaxHz)
            why = "|f0| + |drift|/2 above 800 Hz";
        else
            for (int i = 0; i < 162; ++i) if (x.symbols[i] > 3) { why = "channel symbol above 3"; break; }
        if (why) { fprintf(stderr, "libwspr_mi355x: %s: transmission %d: %s\n", where, t, why); return -1; }
    }
    if (why) { fprintf(stderr, "libwspr_mi355x: %s: %s\n", where, why); return -1; }
    return 0;
}
}  // namespace

extern "C" {

int wspr_synth_audio_batch_device(const wspr_synth_tx* tx, int ntx, int nseg, int seg_index0, int nsamp, float noise_sigma,
                                  uint64_t seed, int flags, void* d_pcm, size_t pcm_stride, int* n_clipped) {
    static const char* where = "wspr_synth_audio_batch_device";
    LaneTurn lane_turn;
    try {
        if (const int bad = synth_audio_args_bad(where, tx, ntx, nseg, nsamp, noise_sigma, flags)) return bad;
        const char* why = nullptr;
        if (nseg > 0 && (!d_pcm || (reinterpret_cast<uintptr_t>(d_pcm) & 15))) why = "d_pcm must be 16-byte aligned device memory";
        else if (nseg > 0 && ((pcm_stride & 7) || pcm_stride < (size_t)nsamp)) why = "pcm_stride must be a multiple of 8 and at least nsamp";
        if (why) { fprintf(stderr, "libwspr_mi355x: %s: %s\n", where, why); return -1; }
        return Context::get().synth_audio_device(tx, ntx, nseg, seg_index0, nsamp, noise_sigma, seed, flags,
                                                 static_cast<int16_t*>(d_pcm), pcm_stride, n_clipped);
    } catch (const std::exception& e) { return fail(where, e); }
}

// one record through the context's own scratch row
int wspr_synth_audio(const wspr_synth_tx* tx, int ntx, int nsamp, float noise_sigma, uint64_t seed, int flags, int16_t* pcm,
                     int* n_clipped) {
    static const char* where = "wspr_synth_audio";
    LaneTurn lane_turn;
    try {
        if (const int bad = synth_audio_args_bad(where, tx, ntx, 1, nsamp, noise_sigma, flags)) return bad;
        if (!pcm && nsamp) { fprintf(stderr, "libwspr_mi355x: %s: no output record\n", where); return -1; }
        Context& c = Context::get();
        int16_t* d_pcm = c.audio_pcm((size_t)nsamp);
        const size_t bytes = (size_t)nsamp * sizeof(int16_t);
        if ((flags & wspr::kSynthFlagAccumulate) && nsamp) HIP_TRY(hipMemcpy(d_pcm, pcm, bytes, hipMemcpyHostToDevice));
        int clipped = 0;
        const int rc = c.synth_audio_device(tx, ntx, 1, 0, nsamp, noise_sigma, seed, flags, d_pcm, ((size_t)nsamp + 7) & ~(size_t)7,
                                            &clipped);
        if (rc) return rc;
        std::vector<int16_t> out((size_t)nsamp);                // the whole record arrives before any of it is handed over
        if (nsamp) HIP_TRY(hipMemcpy(out.data(), d_pcm, bytes, hipMemcpyDeviceToHost));
        if (nsamp) std::memcpy(pcm, out.data(), bytes);
        if (n_clipped) *n_clipped = clipped;
        return 0;
    } catch (const std::exception& e) { return fail(where, e); }
}

}  // extern "C"
