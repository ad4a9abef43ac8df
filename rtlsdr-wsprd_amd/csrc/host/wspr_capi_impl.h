// What more than one entry-point family of the C ABI (wspr_capi_*.hip) uses: error reporting, the turn a call takes
// on its (device, lane), device scratch, the bounce of one row pair or record between the caller and the context's
// scratch.  Internal: not part of any interface.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <exception>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "wspr_pipeline.h"

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) throw std::runtime_error(std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

// External linkage on purpose (the export map keeps the names out of the dynamic table): lane_turn_of()'s table of
// mutexes must be ONE object per library, not one per translation unit that includes this header.
namespace wspr {
namespace capi {
// The reference reports nothing but "zero spots" on failure (wsprd.c:854 returns 0
// always).  A missing GPU is a deployment error, not a weak-signal condition: say so
// loudly on stderr and return a negative code; there is no CPU fallback.
inline int fail(const char* where, const std::exception& e) {
    fprintf(stderr, "libwspr_mi355x: %s failed: %s\n", where, e.what());
    (void)hipGetLastError();          // the runtime's sticky error belongs to THIS call: the next one starts clean
    return -1;
}
// One call at a time per (device, lane).  The library is not re-entrant within a lane (neither is the reference:
// global FFTW plan, static state and fixed file names, wsprd.c:81, :133); threads that never bound a lane all sit on
// lane 0, and until round 5 two of them calling at once shared a context -- streams, working buffers, pools -- silently.
// Now their calls take turns: slow instead of wrong.  Recursive, because entry points call each other on one thread
// (wspr_decode -> wspr_decode_batch -> wspr_decode_batch_hashed); the node-level calls do NOT take it (their worker
// threads bind the caller's lane on each device and call the batch entry points).
inline std::recursive_mutex& lane_turn_of(int dev, int lane) {
    static std::recursive_mutex turns[Context::kMaxDevices][Context::kMaxLanes];
    return turns[std::max(0, std::min(dev, Context::kMaxDevices - 1))][std::max(0, std::min(lane, Context::kMaxLanes - 1))];
}
inline int current_device_or_0() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    return dev;
}
struct LaneTurn {                                  // the calling thread's lane of the current device
    wspr::CallScope settings;                      // the outermost entry point reads the call's settings here, once
    std::unique_lock<std::recursive_mutex> hold;
    LaneTurn() : hold(lane_turn_of(current_device_or_0(), Context::lane())) {}
};
struct AllLanesTurn {                              // every lane of the current device, in index order (wspr_release_buffers)
    std::vector<std::unique_lock<std::recursive_mutex>> hold;
    AllLanesTurn() {
        const int dev = current_device_or_0();
        for (int lane = 0; lane < Context::kMaxLanes; ++lane) hold.emplace_back(lane_turn_of(dev, lane));
    }
};
// device scratch of one call, released on every exit path
struct TempDev {
    void* p = nullptr;
    explicit TempDev(size_t bytes) { HIP_TRY(hipMalloc(&p, bytes)); }
    ~TempDev() { if (p) (void)hipFree(p); }
    TempDev(const TempDev&) = delete;
    TempDev& operator=(const TempDev&) = delete;
    template <class T> T* as() { return static_cast<T*>(p); }
};
// One row pair or one record between the caller's host memory and the context's scratch (the single-segment forms of the
// stage calls).  Down, the whole result arrives in memory of the call's own before any of it is handed over: a call
// that fails has written nothing.
inline void rows_up(float* wi, float* wq, const float* I, const float* Q, size_t n) {
    if (!n) return;
    HIP_TRY(hipMemcpy(wi, I, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(wq, Q, n * sizeof(float), hipMemcpyHostToDevice));
}
inline void rows_down(float* I, float* Q, const float* wi, const float* wq) {
    const size_t bytes = (size_t)kMaxSamples * sizeof(float);
    std::vector<float> oi(kMaxSamples), oq(kMaxSamples);
    HIP_TRY(hipMemcpy(oi.data(), wi, bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(oq.data(), wq, bytes, hipMemcpyDeviceToHost));
    std::memcpy(I, oi.data(), bytes);
    std::memcpy(Q, oq.data(), bytes);
}
inline void record_down(int16_t* pcm, const int16_t* d_pcm, size_t nsamp) {
    if (!nsamp) return;
    std::vector<int16_t> out(nsamp);
    HIP_TRY(hipMemcpy(out.data(), d_pcm, nsamp * sizeof(int16_t), hipMemcpyDeviceToHost));
    std::memcpy(pcm, out.data(), nsamp * sizeof(int16_t));
}
}  // namespace capi
}  // namespace wspr
