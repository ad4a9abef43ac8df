// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): IQ to audio (K18) -- wspr_iq_to_audio_batch_device() and
// wspr_iq_to_audio(), the definition in kernels/iq_audio.h.  (wspr_write_c2_file() is host code: wspr_capi_files.hip.)
#include <cstdint>
#include <cstdio>
#include <exception>

#include "wspr_capi_impl.h"
#include "wspr_stage_args.h"

using wspr::Context;
using namespace wspr::capi;
namespace args = wspr::args;

static_assert(IQ_AUDIO_INTERP * IQ_AUDIO_MAX_SAMPLES == WSPR_AUDIO_MAX_SAMPLES, "a full row is a full record");

extern "C" {

int wspr_iq_to_audio_batch_device(const void* d_idat, const void* d_qdat, int nseg, int samples, size_t seg_stride, float gain,
                                  void* d_pcm, size_t pcm_stride, int* n_clipped) {
    static const char* where = "wspr_iq_to_audio_batch_device";
    LaneTurn lane_turn;
    try {
        // rows are read with aligned 16-byte vector loads and records written with aligned 16-byte vector stores
        if (const int bad = args::iq_audio_batch(where, d_idat, d_qdat, nseg, samples, seg_stride, gain, d_pcm, pcm_stride)) return bad;
        if (nseg == 0) return 0;
        return Context::get().iq_audio_device(static_cast<const float*>(d_idat), static_cast<const float*>(d_qdat), nseg, samples,
                                              seg_stride, gain, static_cast<int16_t*>(d_pcm), pcm_stride, n_clipped);
    } catch (const std::exception& e) { return fail(where, e); }
}

// one row through the context's own working rows and scratch record
int wspr_iq_to_audio(const float* I, const float* Q, int samples, float gain, int16_t* pcm, int* n_clipped) {
    static const char* where = "wspr_iq_to_audio";
    LaneTurn lane_turn;
    try {
        if (const int bad = args::iq_audio_host(where, I, Q, samples, gain, pcm)) return bad;
        Context& c = Context::get();
        const size_t nsamp = (size_t)IQ_AUDIO_INTERP * (size_t)samples;
        float* wi = c.work_i(1);
        float* wq = c.work_q(1);
        int16_t* d_pcm = c.audio_pcm(nsamp);
        rows_up(wi, wq, I, Q, (size_t)samples);
        int clipped = 0;
        const int rc = c.iq_audio_device(wi, wq, 1, samples, (size_t)wspr::kIqStride, gain, d_pcm, nsamp, &clipped);
        if (rc) return rc;
        record_down(pcm, d_pcm, nsamp);
        if (n_clipped) *n_clipped = clipped;
        return 0;
    } catch (const std::exception& e) { return fail(where, e); }
}

}  // extern "C"
