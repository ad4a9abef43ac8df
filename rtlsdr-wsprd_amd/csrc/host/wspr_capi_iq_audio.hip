// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): IQ to audio (K18) -- wspr_iq_to_audio_batch_device() and
// wspr_iq_to_audio(), the definition in kernels/iq_audio.h.  (wspr_write_c2_file() is host code: wspr_capi_files.hip.)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "wspr_capi_impl.h"
#include "wspr_context_impl.h"
#include "../kernels/iq_audio.h"

using wspr::Context;
using namespace wspr::capi;

static_assert(IQ_AUDIO_INTERP * IQ_AUDIO_MAX_SAMPLES == WSPR_AUDIO_MAX_SAMPLES, "a full row is a full record");

namespace wspr {

int Context::iq_audio_device(const float* dI, const float* dQ, int nseg, int samples, size_t stride, float gain, int16_t* d_pcm,
                             size_t pcm_stride, int* h_clipped) {
    Impl& c = *d;
    if (nseg <= 0) return 0;
    std::vector<int> count((size_t)nseg, 0);
    if (samples > 0) {
        const hipStream_t st = c.stream;
        const size_t bytes = (size_t)nseg * sizeof(int);
        int* d_count = static_cast<int*>(c.iqaudiocount.need(bytes));
        HIP_OK(hipMemsetAsync(d_count, 0, bytes, st));
        launch_iq_audio(dI, dQ, stride, samples, nseg, gain, d_pcm, pcm_stride, d_count, st);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(count.data(), d_count, bytes, hipMemcpyDeviceToHost, st));
        if (c.blocking) {                                      // count is host memory of this call: wait either way
            HIP_OK(hipEventRecord(c.ev_sync, st));
            host_wait(c.ev_sync);
        } else {
            HIP_OK(hipStreamSynchronize(st));
        }
    }
    if (h_clipped) std::memcpy(h_clipped, count.data(), count.size() * sizeof(int));   // every count has arrived first
    return 0;
}

}  // namespace wspr

namespace {
// The counts and the gain, the same for both calls: 0, or the code to return (nothing has been written)
int iq_audio_args_bad(const char* where, int nseg, int samples, float gain) {
    const char* why = nullptr;
    if (nseg < 0 || samples < 0) why = "negative count";
    else if (samples > IQ_AUDIO_MAX_SAMPLES) {
        fprintf(stderr, "libwspr_mi355x: %s: a row holds at most 45000 samples (120 s); longer ones are refused, not cut\n", where);
        return -2;
    }
    else if (!std::isfinite(gain)) why = "gain is not finite";
    if (why) { fprintf(stderr, "libwspr_mi355x: %s: %s\n", where, why); return -1; }
    return 0;
}
}  // namespace

extern "C" {

int wspr_iq_to_audio_batch_device(const void* d_idat, const void* d_qdat, int nseg, int samples, size_t seg_stride, float gain,
                                  void* d_pcm, size_t pcm_stride, int* n_clipped) {
    static const char* where = "wspr_iq_to_audio_batch_device";
    LaneTurn lane_turn;
    try {
        if (const int bad = iq_audio_args_bad(where, nseg, samples, gain)) return bad;
        const char* why = nullptr;
        // rows are read with aligned 16-byte vector loads and records written with aligned 16-byte vector stores
        if (nseg > 0 && (!d_idat || !d_qdat || ((reinterpret_cast<uintptr_t>(d_idat) | reinterpret_cast<uintptr_t>(d_qdat)) & 15)))
            why = "d_idat and d_qdat must be 16-byte aligned device rows";
        else if (nseg > 0 && ((seg_stride & 3) || seg_stride < (size_t)samples)) why = "seg_stride must be a multiple of 4 floats and at least samples";
        else if (nseg > 0 && (!d_pcm || (reinterpret_cast<uintptr_t>(d_pcm) & 15))) why = "d_pcm must be 16-byte aligned device memory";
        else if (nseg > 0 && ((pcm_stride & 7) || pcm_stride < (size_t)IQ_AUDIO_INTERP * (size_t)samples))
            why = "pcm_stride must be a multiple of 8 and at least 32 * samples";
        if (why) { fprintf(stderr, "libwspr_mi355x: %s: %s\n", where, why); return -1; }
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
        if (const int bad = iq_audio_args_bad(where, 1, samples, gain)) return bad;
        if ((!I || !Q || !pcm) && samples) { fprintf(stderr, "libwspr_mi355x: %s: no row or no output record\n", where); return -1; }
        Context& c = Context::get();
        const size_t nsamp = (size_t)IQ_AUDIO_INTERP * (size_t)samples;
        float* wi = c.work_i(1);
        float* wq = c.work_q(1);
        int16_t* d_pcm = c.audio_pcm(nsamp);
        if (samples) {
            HIP_TRY(hipMemcpy(wi, I, (size_t)samples * sizeof(float), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(wq, Q, (size_t)samples * sizeof(float), hipMemcpyHostToDevice));
        }
        int clipped = 0;
        const int rc = c.iq_audio_device(wi, wq, 1, samples, (size_t)wspr::kIqStride, gain, d_pcm, nsamp, &clipped);
        if (rc) return rc;
        std::vector<int16_t> out(nsamp);                        // the whole record arrives before any of it is handed over
        if (nsamp) HIP_TRY(hipMemcpy(out.data(), d_pcm, nsamp * sizeof(int16_t), hipMemcpyDeviceToHost));
        if (nsamp) std::memcpy(pcm, out.data(), nsamp * sizeof(int16_t));
        if (n_clipped) *n_clipped = clipped;
        return 0;
    } catch (const std::exception& e) { return fail(where, e); }
}

}  // extern "C"
