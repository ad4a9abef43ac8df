// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): the 12 kHz audio scene synthesiser (K17) --
// wspr_synth_audio_batch_device() and wspr_synth_audio(), the definition in kernels/audio_synth.h.
#include <cstdint>
#include <cstdio>
#include <exception>

#include "wspr_capi_impl.h"
#include "wspr_stage_args.h"

using wspr::Context;
using namespace wspr::capi;
namespace args = wspr::args;

static_assert(wspr::kAudioSynthMaxSamples == WSPR_AUDIO_MAX_SAMPLES, "public and internal record lengths differ");
static_assert(wspr::kSynthFlagAccumulate == WSPR_SYNTH_ACCUMULATE, "public and internal flag bits differ");

extern "C" {

int wspr_synth_audio_batch_device(const wspr_synth_tx* tx, int ntx, int nseg, int seg_index0, int nsamp, float noise_sigma,
                                  uint64_t seed, int flags, void* d_pcm, size_t pcm_stride, int* n_clipped) {
    static const char* where = "wspr_synth_audio_batch_device";
    LaneTurn lane_turn;
    try {
        if (const int bad = args::synth_audio_batch(where, tx, ntx, nseg, nsamp, noise_sigma, flags, d_pcm, pcm_stride)) return bad;
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
        if (const int bad = args::synth_audio_host(where, tx, ntx, nsamp, noise_sigma, flags, pcm)) return bad;
        Context& c = Context::get();
        int16_t* d_pcm = c.audio_pcm((size_t)nsamp);
        if ((flags & wspr::kSynthFlagAccumulate) && nsamp) HIP_TRY(hipMemcpy(d_pcm, pcm, (size_t)nsamp * sizeof(int16_t), hipMemcpyHostToDevice));
        int clipped = 0;
        const int rc = c.synth_audio_device(tx, ntx, 1, 0, nsamp, noise_sigma, seed, flags, d_pcm, ((size_t)nsamp + 7) & ~(size_t)7,
                                            &clipped);
        if (rc) return rc;
        record_down(pcm, d_pcm, (size_t)nsamp);
        if (n_clipped) *n_clipped = clipped;
        return 0;
    } catch (const std::exception& e) { return fail(where, e); }
}

}  // extern "C"
