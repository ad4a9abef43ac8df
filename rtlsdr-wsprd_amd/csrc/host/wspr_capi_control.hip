// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): version, device / lane / slot selection, settings
// and the statistics of the last call.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>

#include "wspr_capi_impl.h"
#include "../kernels/listmatch.h"
#include "../kernels/osd.h"

using wspr::Context;
using namespace wspr::capi;

extern "C" {

const char* wspr_mi355x_version(void) { return "wspr-mi355x 0.3 (gfx950, HIP)"; }

int wspr_device_ready(void) {
    try { Context::get(); return 1; } catch (const std::exception& e) { fail("wspr_device_ready", e); return 0; }
}

size_t wspr_iq_stride(void) { return (size_t)wspr::kIqStride; }

int wspr_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int wspr_set_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n || device >= Context::kMaxDevices) {
        fprintf(stderr, "libwspr_mi355x: wspr_set_device(%d): no such HIP device (%d visible)\n", device, n);
        return -1;
    }
    return hipSetDevice(device) == hipSuccess ? 0 : -1;
}

int wspr_bind_thread_lane(int lane) {
    // the last lane is the receiver sessions' (wspr_session_feed runs beside a decode): callers get 0 .. kUserLanes - 1
    Context::bind_lane(lane < 0 ? 0 : (lane >= Context::kUserLanes ? Context::kUserLanes - 1 : lane));
    return Context::lane();
}

int wspr_set_thread_slots(int n) {
    Context::cap_slots(n <= 0 ? 8 : n);
    return Context::slot_cap();
}

size_t wspr_release_buffers(void) {
    try {
        AllLanesTurn every_lane;                   // calls in flight on this device finish first; new ones wait
        return Context::release_buffers();
    } catch (const std::exception& e) {
        fprintf(stderr, "libwspr_mi355x: wspr_release_buffers failed: %s\n", e.what());
        return 0;
    }
}

unsigned wspr_set_fano_fast_budget(unsigned cycles_per_bit) {
    return wspr::fano_fast_budget().exchange(cycles_per_bit);
}

int wspr_set_arithmetic(int mode) {
    if (mode != 0 && mode != 1) return -1;
    return wspr::arith_setting().exchange(mode);
}

int wspr_set_fano_device_mode(int mode) {
    return wspr::fano_device_setting().exchange(mode < 0 ? -1 : (mode ? 1 : 0));
}

int wspr_fano_batch_device_wave(const unsigned char* symbols, int n, unsigned maxcycles, int* ret, unsigned* cycles,
                                unsigned* metric, unsigned* maxnp, unsigned char* data, unsigned* steps) {
    LaneTurn lane_turn;
    try {
        return Context::get().fano_batch(symbols, n, maxcycles, ret, cycles, metric, maxnp, data, steps);
    } catch (const std::exception& e) { return fail("wspr_fano_batch_device_wave", e); }
}

int wspr_set_osd_depth(int depth) {
    if (depth < -1 || depth > wspr::osd::kMaxDepth) return -2;
    return wspr::osd_depth_setting().exchange(depth);
}

int wspr_osd_batch_device(const unsigned char* symbols, int n, int depth, unsigned char* data, unsigned* dist,
                          unsigned* nhard, unsigned* order) {
    if (depth < 0 || depth > wspr::osd::kMaxDepth || n < 0) return -1;
    if (n == 0) return 0;
    LaneTurn lane_turn;
    try {
        return Context::get().osd_batch(symbols, n, depth, data, dist, nhard, order);
    } catch (const std::exception& e) { return fail("wspr_osd_batch_device", e); }
}

int wspr_set_block_detection(int maxblock) {
    if (maxblock < 1 || maxblock > 3) return -2;
    return wspr::block_setting().exchange(maxblock);
}

int wspr_set_message_list(const char* const* messages, int n, int zmin16) {
    if (!messages || n == 0) {                             // the stage off
        wspr::set_message_list_setting(nullptr);
        return 0;
    }
    int bad = -1;
    std::shared_ptr<const wspr::MessageList> list = wspr::build_message_list(messages, n, zmin16, &bad);
    if (!list) {
        if (bad >= 0)
            fprintf(stderr, "libwspr_mi355x: wspr_set_message_list: entry %d is not a message this stage can hold "
                            "(a type-1 or type-2 text that encodes and decodes to itself without a hash look-up)\n", bad);
        else
            fprintf(stderr, "libwspr_mi355x: wspr_set_message_list: %d entries (0 .. %d) and zmin16 = %d (%d .. %d) refused\n", n,
                    wspr::listmatch::kMaxEntries, zmin16, wspr::listmatch::kZminLo, wspr::listmatch::kZminHi);
        return -1;                                         // the list in force stays in force
    }
    const int kept = list->n;
    wspr::set_message_list_setting(std::move(list));
    return kept;
}

int wspr_message_list_entry(int index, char text[23], unsigned char decdata[11], unsigned char symbols[162]) {
    const std::shared_ptr<const wspr::MessageList> list = wspr::message_list_setting();
    if (!list || index < 0 || index >= list->n) return -1;
    if (text) memcpy(text, list->text.data() + (size_t)index * 23, 23);
    if (decdata) memcpy(decdata, list->decdata.data() + (size_t)index * 11, 11);
    if (symbols) memcpy(symbols, list->symbols.data() + (size_t)index * 162, 162);
    return 0;
}

int wspr_list_match_batch_device(const unsigned char* symbols, int n, wspr_list_match* out) {
    if (n < 0) return -1;
    LaneTurn lane_turn;                                    // takes the snapshot of the list, like a decode call
    const std::shared_ptr<const wspr::MessageList> list = wspr::call_list();
    if (!list) return -1;
    if (n == 0) return 0;
    try {
        return Context::get().list_batch(symbols, n, *list, out);
    } catch (const std::exception& e) { return fail("wspr_list_match_batch_device", e); }
}

int wspr_host_pool_workers(void) { return wspr::pool_workers_alive().load(); }

int wspr_last_timings(double* ms, int capacity) {
    // times: the slowest slot (slots run concurrently); from kTimingFirstSummed on: summed over the slots -- of the
    // slots the calling thread's LAST batch call ran on (a capped or small call uses fewer than Context::slots();
    // contexts are never created here)
    try {
        double acc[wspr::kTimingSlots] = {0};
        int n = wspr::kTimingSlots;
        const int used = std::max(1, Context::last_slots_used());
        for (int g = 0; g < used; ++g) {
            Context* c = Context::slot_if_exists(g);
            if (!c) continue;
            double t[wspr::kTimingSlots] = {0};
            n = c->last_timings(t, wspr::kTimingSlots);
            for (int i = 0; i < n; ++i) acc[i] = (i < wspr::kTimingFirstSummed) ? (t[i] > acc[i] ? t[i] : acc[i]) : acc[i] + t[i];
        }
        n = n < capacity ? n : capacity;
        for (int i = 0; i < n; ++i) ms[i] = acc[i];
        return n;
    } catch (const std::exception& e) { return fail("wspr_last_timings", e); }
}

}  // extern "C"
