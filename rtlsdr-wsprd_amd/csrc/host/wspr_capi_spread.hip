// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): the Doppler-spread figure -- wspr_spread_batch() (K11
// over host rows), the switch of the decoder's stage and the records of the calling thread's last decode call.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>

#include "wspr_capi_impl.h"
#include "../kernels/synth_math.h"

using wspr::Context;
using namespace wspr::capi;

static_assert(sizeof(wspr_spread_item) == 180 && sizeof(wspr_spread_item) == sizeof(wspr::SubJob) && sizeof(wspr_spread) == 32,
              "public and device job layouts differ");

extern "C" {

int wspr_spread_batch(const float* idat, const float* qdat, int nseg, int samples, size_t seg_stride,
                      const wspr_spread_item* items, int n, wspr_spread* out) {
    if (n < 0 || nseg < 0 || samples < 0 || samples > wspr::kMaxSamples) return -1;
    if (n > 0 && (!items || !out)) return -1;
    for (int i = 0; i < n; ++i) {
        const wspr_spread_item& x = items[i];
        if (x.seg < 0 || x.seg >= nseg || !std::isfinite(x.f0) || !std::isfinite(x.drift)) return -1;
        if (std::fabs((double)x.f0) + std::fabs((double)x.drift) / 2.0 > wspr::kSynthMaxHz) return -1;
        for (int k = 0; k < 162; ++k) if (x.symbols[k] > 3) return -1;
    }
    if (n == 0) return 0;
    if (samples > 0 && (!idat || !qdat)) return -1;
    LaneTurn lane_turn;
    try {
        return Context::get().spread_batch(idat, qdat, nseg, samples, seg_stride, items, n, out);
    } catch (const std::exception& e) { return fail("wspr_spread_batch", e); }
}

int wspr_set_spread_estimate(int on) {
    if (on != 0 && on != 1) return -2;
    return wspr::spread_setting().exchange(on);
}

int wspr_last_spreads(wspr_spread* spreads, int capacity) {
    const wspr::LastSpreads& last = wspr::last_spreads_of_thread();
    const size_t count = (size_t)last.nseg * (size_t)last.max_results;
    if (!last.on || count != last.rec.size() || capacity < 0 || (size_t)capacity < count || (count && !spreads)) return -1;
    if (count) memcpy(spreads, last.rec.data(), count * sizeof(wspr_spread));
    return (int)count;
}

}  // extern "C"
