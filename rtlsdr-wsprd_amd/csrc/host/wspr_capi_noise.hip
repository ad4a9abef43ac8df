// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): the band noise figures of a segment (K16; the
// definition in kernels/noise.h).  The windows are arguments, not state: no decode call, setting or timing slot is touched.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>

#include "wspr_capi_impl.h"
#include "wspr_stage_args.h"

using wspr::Context;
using namespace wspr::capi;
namespace args = wspr::args;
namespace noise = wspr::noise;

static_assert(sizeof(struct wspr_noise) == sizeof(noise::Result) && sizeof(wspr_noise_windows) == sizeof(noise::Windows),
              "the public records are the kernel's");

extern "C" {

void wspr_noise_default_windows(wspr_noise_windows* w) {
    if (!w) return;
    const noise::Windows d = args::default_noise_windows();
    std::memcpy(w, &d, sizeof d);
}

int wspr_noise_batch_device(const void* d_idat, const void* d_qdat, int nseg, int samples, size_t seg_stride,
                            const wspr_noise_windows* w, struct wspr_noise* out) {
    static const char* where = "wspr_noise_batch_device";
    LaneTurn lane_turn;
    try {
        noise::Windows win;
        // rows are read with aligned 16-byte vector loads
        if (const int bad = args::noise_batch(where, d_idat, d_qdat, nseg, samples, seg_stride, w, out, &win)) return bad;
        if (nseg == 0) return 0;
        return Context::get().noise_device(static_cast<const float*>(d_idat), static_cast<const float*>(d_qdat), nseg, samples,
                                           seg_stride, win, reinterpret_cast<noise::Result*>(out));
    } catch (const std::exception& e) { return fail(where, e); }
}

int wspr_noise(const float* I, const float* Q, int samples, const wspr_noise_windows* w, struct wspr_noise* out) {
    static const char* where = "wspr_noise";
    LaneTurn lane_turn;
    try {
        noise::Windows win;
        if (const int bad = args::noise_host(where, I, Q, samples, w, out, &win)) return bad;
        Context& c = Context::get();
        float* wi = c.work_i(1);
        float* wq = c.work_q(1);
        rows_up(wi, wq, I, Q, (size_t)samples);
        return c.noise_device(wi, wq, 1, samples, (size_t)wspr::kIqStride, win, reinterpret_cast<noise::Result*>(out));
    } catch (const std::exception& e) { return fail(where, e); }
}

}  // extern "C"
