// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): the tunable multi-band front end (K21) -- wspr_tune_step(),
// wspr_tune_u8_batch_device(), wspr_tune_u8() and wspr_tune_constants(), the definition in kernels/tune.h.
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

static_assert(WSPR_TUNE_MAX_BANDS == TUNE_MAX_BANDS, "the public limit is the definition's");
static_assert(TUNE_MAX_OUT == wspr::kMaxSamples, "a full capture is a full row");

extern "C" {

uint32_t wspr_tune_step(double offset_hz, double* realised_hz) { return tune_step(offset_hz, realised_hz); }

void wspr_tune_constants(int16_t c256[512], int16_t f256[512], int* samples_per_output) {
    if (c256) std::memcpy(c256, kTuneC256, sizeof kTuneC256);
    if (f256) std::memcpy(f256, kTuneF256, sizeof kTuneF256);
    if (samples_per_output) *samples_per_output = TUNE_SAMPLES_PER_OUTPUT;
}

int wspr_tune_u8_batch_device(const void* d_raw, size_t bytes_per_seg, int nseg, const uint32_t* steps, int nbands, void* d_idat,
                              void* d_qdat, int normalise) {
    static const char* where = "wspr_tune_u8_batch_device";
    LaneTurn lane_turn;
    try {
        if (const int bad = args::tune_batch(where, d_raw, bytes_per_seg, nseg, steps, nbands, d_idat, d_qdat)) return bad;
        if (nseg == 0) return 0;
        return Context::get().tune_device(d_raw, bytes_per_seg, nseg, steps, nbands, static_cast<float*>(d_idat),
                                          static_cast<float*>(d_qdat), normalise, nullptr);
    } catch (const std::exception& e) { return fail(where, e); }
}

// one capture through the context's own scratch: the bytes up, nbands rows down
int wspr_tune_u8(const uint8_t* iq, size_t nbytes, const uint32_t* steps, int nbands, float* I, float* Q, uint32_t* n_out,
                 int normalise) {
    static const char* where = "wspr_tune_u8";
    LaneTurn lane_turn;
    try {
        if (const int bad = args::tune_host(where, iq, nbytes, steps, nbands, I, Q)) return bad;
        Context& c = Context::get();
        // whole vectors only (a block ends on one), and nothing behind the last block that counts
        const size_t most = (size_t)TUNE_MAX_OUT * TUNE_SAMPLES_PER_OUTPUT * 2;
        const size_t bytes = std::min(nbytes & ~(size_t)15, most);
        uint8_t* d_raw = c.tune_raw(bytes);
        if (bytes) HIP_TRY(hipMemcpy(d_raw, iq, bytes, hipMemcpyHostToDevice));
        float* wi = c.work_i(nbands);
        float* wq = c.work_q(nbands);
        std::vector<int> nout((size_t)nbands, 0);
        const int rc = c.tune_device(d_raw, bytes, 1, steps, nbands, wi, wq, normalise, nout.data());
        if (rc) return rc;
        const size_t row = (size_t)wspr::kMaxSamples;
        std::vector<float> oi(row * nbands), oq(row * nbands);
        HIP_TRY(hipMemcpy2D(oi.data(), row * sizeof(float), wi, (size_t)wspr::kIqStride * sizeof(float), row * sizeof(float),
                            (size_t)nbands, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy2D(oq.data(), row * sizeof(float), wq, (size_t)wspr::kIqStride * sizeof(float), row * sizeof(float),
                            (size_t)nbands, hipMemcpyDeviceToHost));
        std::memcpy(I, oi.data(), oi.size() * sizeof(float));
        std::memcpy(Q, oq.data(), oq.size() * sizeof(float));
        if (n_out) *n_out = (uint32_t)nout[0];
        return 0;
    } catch (const std::exception& e) { return fail(where, e); }
}

}  // extern "C"
