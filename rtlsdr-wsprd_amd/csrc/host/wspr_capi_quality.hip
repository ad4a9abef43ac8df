// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): the decode-quality figures of a spot --
// wspr_spot_quality_batch_device() (K19 over host vectors; the definition in kernels/spot_quality.h), the switch of the
// decoder's stage and the records of the calling thread's last decode call.
#include <cstring>
#include <exception>

#include "wspr_capi_impl.h"
#include "wspr_stage_args.h"

using wspr::Context;
using namespace wspr::capi;
namespace args = wspr::args;

static_assert(sizeof(wspr_spot_quality) == 20 && sizeof(wspr_spot_detail) == 32 && sizeof(wspr_spot_quality) == sizeof(wspr::SpotQuality),
              "public and device record layouts differ");

extern "C" {

int wspr_spot_quality_batch_device(const unsigned char* symbols, const unsigned char* decdata, int n, wspr_spot_quality* out) {
    static const char* where = "wspr_spot_quality_batch_device";
    if (const int bad = args::spot_quality_batch(where, symbols, decdata, n, out)) return bad;
    if (n == 0) return 0;
    LaneTurn lane_turn;
    try {
        return Context::get().spot_quality_batch(symbols, decdata, n, out);
    } catch (const std::exception& e) { return fail(where, e); }
}

int wspr_set_spot_details(int on) {
    if (on != 0 && on != 1) return -2;
    return wspr::details_setting().exchange(on);
}

int wspr_last_spot_details(wspr_spot_detail* details, int capacity) {
    const wspr::LastDetails& last = wspr::last_details_of_thread();
    const size_t count = (size_t)last.nseg * (size_t)last.max_results;
    if (!last.on || count != last.rec.size() || capacity < 0 || (size_t)capacity < count || (count && !details)) return -1;
    if (count) memcpy(details, last.rec.data(), count * sizeof(wspr_spot_detail));
    return (int)count;
}

}  // extern "C"
