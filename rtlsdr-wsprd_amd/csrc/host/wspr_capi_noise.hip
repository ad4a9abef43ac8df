// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): the band noise figures of a segment (K16; the
// definition in kernels/noise.h).  The windows are arguments, not state: no decode call, setting or timing slot is touched.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "wspr_capi_impl.h"
#include "../kernels/noise.h"

using wspr::Context;
using namespace wspr::capi;
namespace noise = wspr::noise;

static_assert(sizeof(struct wspr_noise) == sizeof(noise::Result) && sizeof(wspr_noise_windows) == sizeof(noise::Windows),
              "the public records are the kernel's");

namespace {
noise::Windows default_windows() { return noise::Windows{noise::kPreB0, noise::kPreB1, noise::kPostB0, noise::kPostB1}; }

// the counts and the windows, the same for both calls: 0, or the code to return (nothing has been written)
int noise_args_bad(const char* where, int nseg, int samples, const wspr_noise_windows* w, const void* out, noise::Windows* win) {
    const char* why = nullptr;
    *win = default_windows();
    if (w) std::memcpy(win, w, sizeof *win);
    if (nseg < 0 || samples < 0) why = "negative count";
    else if (samples > noise::kMaxSamples) {
        fprintf(stderr, "libwspr_mi355x: %s: a row holds at most 45000 samples (120 s); longer ones are refused, not cut\n", where);
        return -2;
    }
    else if (!noise::windows_ok(win->pre_b0, win->pre_b1) || !noise::windows_ok(win->post_b0, win->post_b1))
        why = "a window must satisfy 0 <= b0 <= b1 <= 2812";
    else if (nseg > 0 && !out) why = "no output records";
    if (why) { fprintf(stderr, "libwspr_mi355x: %s: %s\n", where, why); return -1; }
    return 0;
}
}  // namespace

extern "C" {

void wspr_noise_default_windows(wspr_noise_windows* w) {
    if (!w) return;
    const noise::Windows d = default_windows();
    std::memcpy(w, &d, sizeof d);
}

int wspr_noise_batch_device(const void* d_idat, const void* d_qdat, int nseg, int samples, size_t seg_stride,
                            const wspr_noise_windows* w, struct wspr_noise* out) {
    static const char* where = "wspr_noise_batch_device";
    LaneTurn lane_turn;
    try {
        noise::Windows win;
        if (const int bad = noise_args_bad(where, nseg, samples, w, out, &win)) return bad;
        const char* why = nullptr;
        // rows are read with aligned 16-byte vector loads
        if (nseg > 0 && (!d_idat || !d_qdat || ((reinterpret_cast<uintptr_t>(d_idat) | reinterpret_cast<uintptr_t>(d_qdat)) & 15)))
            why = "d_idat and d_qdat must be 16-byte aligned device rows";
        else if (nseg > 0 && ((seg_stride & 3) || seg_stride < (size_t)samples)) why = "seg_stride must be a multiple of 4 floats and at least samples";
        if (why) { fprintf(stderr, "libwspr_mi355x: %s: %s\n", where, why); return -1; }
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
        if (const int bad = noise_args_bad(where, 1, samples, w, out, &win)) return bad;
        if ((!I || !Q) && samples) { fprintf(stderr, "libwspr_mi355x: %s: no row\n", where); return -1; }
        Context& c = Context::get();
        float* wi = c.work_i(1);
        float* wq = c.work_q(1);
        if (samples) {
            HIP_TRY(hipMemcpy(wi, I, (size_t)samples * sizeof(float), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(wq, Q, (size_t)samples * sizeof(float), hipMemcpyHostToDevice));
        }
        return c.noise_device(wi, wq, 1, samples, (size_t)wspr::kIqStride, win, reinterpret_cast<noise::Result*>(out));
    } catch (const std::exception& e) { return fail(where, e); }
}

}  // extern "C"
