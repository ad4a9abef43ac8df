// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): the batch decode, its hashed / ordered form, and
// the reference's own decoder entry points.  The decode templates live here, in the one file that instantiates them.
#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <cmath>

#include "wspr_capi_impl.h"

using wspr::Context;
using namespace wspr::capi;

namespace {
// The callsign hash memory makes a segment's result depend on what was decoded before it (wsprd.c:481-494, 842-852:
// hashtable.txt read before, written after every decode).  The product decodes a usehashtable batch in parallel all the
// same (decode_hashed() below); the per-candidate TRACE of the lab library keeps the plain form of rounds 2-4: one
// segment after the other, each as the reference's own call would be (load the file, decode, save the file).
// (a template: instantiated by the lab library's trace entry point only)
template <class One>
int decode_in_order(int nseg, int* n_results, One one) {
    int rc = 0;
    for (int s = 0; s < nseg; ++s) {
        const int r = one(s);
        if (r < 0) { rc = r; for (int k = s; k < nseg; ++k) n_results[k] = 0; break; }
    }
    return rc;
}

// Splits a batch over the pipelines (slots).  Segments are independent, so every slot decodes a
// contiguous share on its own stream while the others are in their host phases.
// hb (usehashtable on a batch): the shared, ordered hash memory; after the first round the segments whose look-ups no
// longer hold are decoded again, round by round, until none is left (see HashBatch in wspr_pipeline.h).
template <class Load, class Reload>
int decode_split(int nseg, int samples, const decoder_options& options, decoder_results* decodes, int max_results,
                 int* n_results, Load load, Reload reload, bool writeback, float* idat, float* qdat, size_t seg_stride,
                 wspr_trace* trace = nullptr, wspr::HashBatch* hb = nullptr, const std::vector<int>* revisit = nullptr,
                 const std::function<void()>& before_validation = nullptr) {
    const int nslots = (nseg >= 128) ? Context::slot_cap() : 1;
    Context::note_slots_used(nslots);
    Context& c0 = Context::get();
    const int dev = c0.device(), lane = Context::lane();
    const wspr::CallSettings settings = wspr::call_settings();
    const int spread_on = settings.spread;
    // wspr_last_spreads(): the calling thread's record takes the layout of `decodes`; a revisit of the same layout keeps
    // the entries of the segments it does not decode again.  The traced form does not record.
    wspr::LastSpreads& last = wspr::last_spreads_of_thread();
    wspr_spread* spread_rec = nullptr;
    if (spread_on > 0 && !trace && max_results > 0) {
        const bool keep = revisit && last.on && last.nseg == nseg && last.max_results == max_results;
        if (!keep) last.rec.assign((size_t)nseg * (size_t)max_results, wspr_spread{});
        last.nseg = nseg; last.max_results = max_results;
        spread_rec = last.rec.data();
    }
    last.on = false;                                       // until this call has run to its end
    // wspr_last_spot_details(): the same, for the records of wspr_set_spot_details()
    wspr::LastDetails& last_det = wspr::last_details_of_thread();
    wspr_spot_detail* detail_rec = nullptr;
    if (settings.details > 0 && !trace && max_results > 0) {
        const bool keep = revisit && last_det.on && last_det.nseg == nseg && last_det.max_results == max_results;
        if (!keep) last_det.rec.assign((size_t)nseg * (size_t)max_results, wspr_spot_detail{});
        last_det.nseg = nseg; last_det.max_results = max_results;
        detail_rec = last_det.rec.data();
    }
    last_det.on = false;
    struct Share { int lo, hi; };
    std::vector<Share> share(nslots);
    for (int g = 0; g < nslots; ++g) share[g] = {(int)((long)nseg * g / nslots), (int)((long)nseg * (g + 1) / nslots)};
    // runs fn(g, context of slot g) for every slot, slot 0 on the calling thread when it is the only one
    auto on_slots = [&](const std::function<void(int, Context&)>& fn) {
        if (nslots == 1) { fn(0, c0); return; }
        std::vector<std::thread> th;
        std::vector<std::string> errs(nslots);
        std::vector<char> bad(nslots, 0);
        for (int g = 0; g < nslots; ++g)
            th.emplace_back([&, g] {
                try {
                    wspr::CallScope call_scope(settings);
                    if (hipSetDevice(dev) != hipSuccess) throw std::runtime_error("hipSetDevice failed");
                    Context::bind_lane(lane);
                    fn(g, Context::slot(g));
                } catch (const std::exception& e) { bad[g] = 1; errs[g] = e.what(); }
            });
        for (auto& t : th) t.join();
        for (int g = 0; g < nslots; ++g)
            if (bad[g]) throw std::runtime_error(errs[g].empty() ? "slot failed" : errs[g]);
    };
    auto again = [&](const std::vector<int>& todo) {         // global (call-relative) indices, ascending
        on_slots([&](int g, Context& c) {
            const int lo = share[g].lo, hi = share[g].hi;
            std::vector<int> mine;
            for (int t : todo) if (t >= lo && t < hi) mine.push_back(t - lo);
            if (mine.empty()) return;
            reload(c, lo, mine);
            c.set_spread_out(spread_rec ? spread_rec + (size_t)lo * max_results : nullptr);
            c.set_detail_out(detail_rec ? detail_rec + (size_t)lo * max_results : nullptr);
            c.decode_again(hi - lo, samples, options, decodes + (size_t)lo * max_results, max_results, n_results + lo, mine, hb, lo);
        });
    };
    if (!revisit) {
        on_slots([&](int g, Context& c) {
            const int lo = share[g].lo, hi = share[g].hi;
            load(c, lo, hi - lo);
            c.set_spread_out(spread_rec ? spread_rec + (size_t)lo * max_results : nullptr);
            c.set_detail_out(detail_rec ? detail_rec + (size_t)lo * max_results : nullptr);
            const int rc = c.decode_resident(hi - lo, samples, options, decodes + (size_t)lo * max_results, max_results, n_results + lo,
                                             [&c, &reload, lo](const std::vector<int>& segs) { reload(c, lo, segs); },
                                             trace ? trace + lo : nullptr, hb, lo);
            if (rc < 0) throw std::runtime_error("decode failed");
        });
    } else if (!revisit->empty()) {
        // the batch of the previous call once more (its rows are still in the slots' working buffers, decoded): only
        // the listed segments are restored and decoded again
        ++hb->rounds; hb->redecoded += (int)revisit->size();
        again(*revisit);
    }
    if (hb && before_validation) before_validation();      // e.g. wait for the calls before this one, take their file as the base
    if (hb)
        for (;;) {
            hb->rebuild();
            const std::vector<int> todo = hb->invalid();
            if (todo.empty()) break;
            ++hb->rounds; hb->redecoded += (int)todo.size();
            again(todo);
        }
    if (writeback)
        on_slots([&](int g, Context& c) {
            const int lo = share[g].lo, hi = share[g].hi;
            c.store_host(idat + (size_t)lo * seg_stride, qdat + (size_t)lo * seg_stride, hi - lo, samples, seg_stride);
        });
    last.on = spread_rec != nullptr;
    last_det.on = detail_rec != nullptr;
    return 0;
}

// usehashtable: calls are ordered by definition -- each reads the file the previous one wrote.  The order is the order
// in which they ENTER (a ticket), and a call's turn comes when every earlier ticket has left.  A batch call decodes its
// first round BEFORE its turn (against the file as it is then: speculation, beside the calls ahead of it on other
// lanes), waits, takes the file its predecessors have written as its base, decodes again what that changes, writes the
// file and leaves; single calls and the sharded form simply wait for their turn first.
struct HashChain {
    std::mutex m;
    std::condition_variable cv;
    unsigned long next = 0, serving = 0;
    static HashChain& get() { static HashChain c; return c; }
    struct Ticket {
        HashChain& c;
        unsigned long t;
        bool left = false;
        explicit Ticket(HashChain& c_) : c(c_) { std::lock_guard<std::mutex> g(c.m); t = c.next++; }
        void wait_turn() { std::unique_lock<std::mutex> g(c.m); c.cv.wait(g, [&] { return c.serving == t; }); }
        void leave() {
            if (left) return;
            wait_turn();
            { std::lock_guard<std::mutex> g(c.m); ++c.serving; }
            left = true;
            c.cv.notify_all();
        }
        ~Ticket() { leave(); }                               // whatever happened: the calls behind must not wait for ever
        Ticket(const Ticket&) = delete;
        Ticket& operator=(const Ticket&) = delete;
    };
};

// usehashtable on a batch: parallel decode against the shared, ordered hash memory (HashBatch), to the fixed point.
// The memory of the calling thread's last such call is kept: WSPR_HASH_REVISIT decodes only what a new `prior` changes.
thread_local std::unique_ptr<wspr::HashBatch> t_hash;
static_assert(sizeof(wspr_hash_op) == sizeof(wspr::HashOp), "public and internal hash-op layouts differ");

template <class Load, class Reload>
int decode_hashed(int nseg, int samples, const decoder_options& options, decoder_results* decodes, int max_results,
                  int* n_results, Load load, Reload reload, bool writeback, float* idat, float* qdat, size_t seg_stride,
                  int seg_index0, const wspr_hash_op* prior, int n_prior, int flags, wspr_hash_op* stores_out, int cap,
                  int* n_stores, int* n_redecoded) {
    HashChain::Ticket ticket(HashChain::get());
    const bool revisit = (flags & WSPR_HASH_REVISIT) != 0;
    // a plain batch call (all of its job in one call, the file its own to write) may run its first round ahead of its
    // turn; a shard of a larger job is driven round by round from outside and waits first -- and keeps its turn for the
    // whole call, so shards driven from several threads of ONE process (several devices or lanes) decode one after the
    // other (include/wspr_mi355x.h says so; shards in different processes -- rtlsdr-wsprd_amd/dist.py -- do not meet here)
    const bool ahead = !revisit && !(flags & WSPR_HASH_KEEP_FILE) && n_prior <= 0;
    if (!ahead) ticket.wait_turn();
    // a revisit works on the state the previous call of this thread left: its log, and the decoded rows in the slots'
    // working buffers.  It is refused unless that call COMPLETED (a call that threw leaves a half-updated log) over the
    // same segments, samples and slot layout (wspr_set_thread_slots / a node-level share in between change the shares)
    const int nslots_now = (nseg >= 128) ? Context::slot_cap() : 1;
    if (revisit && !(t_hash && t_hash->valid && (int)t_hash->log.size() == nseg && t_hash->seg0 == seg_index0 &&
                     t_hash->samples == samples && t_hash->nslots == nslots_now && t_hash->arith == wspr::call_arith() &&
                     t_hash->osd_depth == wspr::call_osd_depth() && t_hash->maxblock == wspr::call_maxblock() &&
                     t_hash->list_gen == wspr::call_list_generation() &&
                     t_hash->list_zmin16 == (wspr::call_list() ? wspr::call_list()->zmin16 : 0)))
        throw std::runtime_error("WSPR_HASH_REVISIT without a matching, completed previous call on this thread");
    if (!revisit) {
        t_hash.reset(new wspr::HashBatch);
        t_hash->load_file();
        t_hash->seg0 = seg_index0;
        t_hash->arith = wspr::call_arith();
        t_hash->osd_depth = wspr::call_osd_depth();
        t_hash->maxblock = wspr::call_maxblock();
        t_hash->list_gen = wspr::call_list_generation();
        t_hash->list_zmin16 = wspr::call_list() ? wspr::call_list()->zmin16 : 0;
        t_hash->resize(nseg);
    }
    wspr::HashBatch& hb = *t_hash;
    hb.valid = false;                                      // until this call has run to its end
    hb.nslots = nslots_now; hb.samples = samples;
    hb.rounds = hb.redecoded = 0;
    hb.prior.assign(reinterpret_cast<const wspr::HashOp*>(prior), reinterpret_cast<const wspr::HashOp*>(prior) + std::max(0, n_prior));
    std::stable_sort(hb.prior.begin(), hb.prior.end(), [](const wspr::HashOp& a, const wspr::HashOp& b) { return a.seg < b.seg; });
    std::vector<int> todo;
    if (revisit) { hb.rebuild(); todo = hb.invalid(); }
    decode_split(nseg, samples, options, decodes, max_results, n_results, load, reload, writeback, idat, qdat, seg_stride,
                 nullptr, &hb, revisit ? &todo : nullptr,
                 ahead ? std::function<void()>([&] { ticket.wait_turn(); hb.load_file(); }) : std::function<void()>());
    hb.valid = true;
    const std::vector<wspr::HashOp> st = hb.stores();
    if (n_stores) *n_stores = (int)st.size();
    if (n_redecoded) *n_redecoded = hb.redecoded;
    // a store buffer that is too small fails the call BEFORE anything is committed: hashtable.txt is untouched, the
    // result arrays hold the decode, *n_stores the capacity needed, and the same call with WSPR_HASH_REVISIT (same
    // prior, a larger buffer) completes it without decoding anything again
    if (stores_out && (int)st.size() > cap) return -3;
    if (!(flags & WSPR_HASH_KEEP_FILE)) hb.commit_file();
    if (stores_out && !st.empty()) memcpy(stores_out, st.data(), st.size() * sizeof(wspr::HashOp));
    return 0;
}
}  // namespace

extern "C" {

int wspr_decode_batch(float* idat, float* qdat, int nseg, int samples, size_t seg_stride,
                      struct decoder_options options, struct decoder_results* decodes, int max_results,
                      int* n_results, int writeback) {
    LaneTurn lane_turn;
    if (options.usehashtable && nseg > 1)                 // the hash memory orders the segments: parallel all the same
        return wspr_decode_batch_hashed(idat, qdat, nseg, samples, seg_stride, options, decodes, max_results, n_results,
                                        writeback, 0, nullptr, 0, 0, nullptr, 0, nullptr, nullptr);
    try {
        // a single call with the option reads and writes hashtable.txt itself (wsprd.c:481-494, 842-852): in its turn
        std::unique_ptr<HashChain::Ticket> turn;
        if (options.usehashtable) { turn.reset(new HashChain::Ticket(HashChain::get())); turn->wait_turn(); }
        if (samples > wspr::kMaxSamples) {
            // the reference derives its block count from `samples` (wsprd.c:516) and would read past the 45 000 samples
            // its callers hold; this library's working rows are 45 000 samples, so a longer record is refused, not cut
            fprintf(stderr, "libwspr_mi355x: samples = %d exceeds the %d this library decodes\n", samples, wspr::kMaxSamples);
            for (int s = 0; s < nseg; ++s) n_results[s] = 0;
            return -2;
        }
        return decode_split(nseg, samples, options, decodes, max_results, n_results,
                            [&](Context& c, int lo, int n) {
                                c.load_host(idat + (size_t)lo * seg_stride, qdat + (size_t)lo * seg_stride, n, samples, seg_stride);
                            },
                            [&](Context& c, int lo, const std::vector<int>& segs) {
                                c.reload_rows(idat + (size_t)lo * seg_stride, qdat + (size_t)lo * seg_stride, false, seg_stride, samples, segs);
                            },
                            writeback != 0, idat, qdat, seg_stride);
    } catch (const std::exception& e) {
        for (int s = 0; s < nseg; ++s) n_results[s] = 0;
        return fail("wspr_decode_batch", e);
    }
}

int wspr_decode_batch_hashed(float* idat, float* qdat, int nseg, int samples, size_t seg_stride,
                             struct decoder_options options, struct decoder_results* decodes, int max_results,
                             int* n_results, int writeback, int seg_index0, const wspr_hash_op* prior, int n_prior,
                             int flags, wspr_hash_op* stores_out, int cap, int* n_stores, int* n_redecoded) {
    LaneTurn lane_turn;
    try {
        if (samples > wspr::kMaxSamples) {
            fprintf(stderr, "libwspr_mi355x: samples = %d exceeds the %d this library decodes\n", samples, wspr::kMaxSamples);
            for (int s = 0; s < nseg; ++s) n_results[s] = 0;
            return -2;
        }
        options.usehashtable = 1;
        return decode_hashed(nseg, samples, options, decodes, max_results, n_results,
                             [&](Context& c, int lo, int n) {
                                 c.load_host(idat + (size_t)lo * seg_stride, qdat + (size_t)lo * seg_stride, n, samples, seg_stride);
                             },
                             [&](Context& c, int lo, const std::vector<int>& segs) {
                                 c.reload_rows(idat + (size_t)lo * seg_stride, qdat + (size_t)lo * seg_stride, false, seg_stride, samples, segs);
                             },
                             writeback != 0, idat, qdat, seg_stride, seg_index0, prior, n_prior, flags, stores_out, cap,
                             n_stores, n_redecoded);
    } catch (const std::exception& e) {
        if (!(flags & WSPR_HASH_REVISIT)) for (int s = 0; s < nseg; ++s) n_results[s] = 0;
        return fail("wspr_decode_batch_hashed", e);
    }
}

int wspr_hash_commit(const wspr_hash_op* stores, int n) {
    try {
        HashChain::Ticket ticket(HashChain::get());
        ticket.wait_turn();
        wspr::HashBatch hb;
        hb.load_file();
        wspr::HashBatch::commit_file(hb.base_call, hb.base_grid, reinterpret_cast<const wspr::HashOp*>(stores), (size_t)std::max(0, n));
        return 0;
    } catch (const std::exception& e) { return fail("wspr_hash_commit", e); }
}

#ifdef WSPR_LAB   /* include/wspr_mi355x_bench.h: lab build only */
int wspr_decode_batch_trace(float* idat, float* qdat, int nseg, int samples, size_t seg_stride,
                            struct decoder_options options, struct decoder_results* decodes, int max_results,
                            int* n_results, wspr_trace* trace) {
    LaneTurn lane_turn;
    if (!trace) return -1;
    if (options.usehashtable && nseg > 1)
        return decode_in_order(nseg, n_results, [&](int s) {
            return wspr_decode_batch_trace(idat + (size_t)s * seg_stride, qdat + (size_t)s * seg_stride, 1, samples, seg_stride,
                                           options, decodes + (size_t)s * max_results, max_results, n_results + s, trace + s);
        });
    try {
        // a single traced call with the option reads and writes hashtable.txt itself: in its turn, like wspr_decode_batch()
        std::unique_ptr<HashChain::Ticket> turn;
        if (options.usehashtable) { turn.reset(new HashChain::Ticket(HashChain::get())); turn->wait_turn(); }
        if (samples > wspr::kMaxSamples) {
            // the reference derives its block count from `samples` (wsprd.c:516) and would read past the 45 000 samples
            // its callers hold; this library's working rows are 45 000 samples, so a longer record is refused, not cut
            fprintf(stderr, "libwspr_mi355x: samples = %d exceeds the %d this library decodes\n", samples, wspr::kMaxSamples);
            for (int s = 0; s < nseg; ++s) n_results[s] = 0;
            return -2;
        }
        return decode_split(nseg, samples, options, decodes, max_results, n_results,
                            [&](Context& c, int lo, int n) {
                                c.load_host(idat + (size_t)lo * seg_stride, qdat + (size_t)lo * seg_stride, n, samples, seg_stride);
                            },
                            [&](Context& c, int lo, const std::vector<int>& segs) {
                                c.reload_rows(idat + (size_t)lo * seg_stride, qdat + (size_t)lo * seg_stride, false, seg_stride, samples, segs);
                            },
                            false, idat, qdat, seg_stride, trace);
    } catch (const std::exception& e) {
        for (int s = 0; s < nseg; ++s) n_results[s] = 0;
        return fail("wspr_decode_batch_trace", e);
    }
}
#endif  // WSPR_LAB

int wspr_decode_batch_device(const void* d_idat, const void* d_qdat, int nseg, int samples, size_t seg_stride,
                             struct decoder_options options, struct decoder_results* decodes, int max_results,
                             int* n_results) {
    LaneTurn lane_turn;
    try {
        if (samples > wspr::kMaxSamples) {
            // the reference derives its block count from `samples` (wsprd.c:516) and would read past the 45 000 samples
            // its callers hold; this library's working rows are 45 000 samples, so a longer record is refused, not cut
            fprintf(stderr, "libwspr_mi355x: samples = %d exceeds the %d this library decodes\n", samples, wspr::kMaxSamples);
            for (int s = 0; s < nseg; ++s) n_results[s] = 0;
            return -2;
        }
        const float* di = static_cast<const float*>(d_idat);
        const float* dq = static_cast<const float*>(d_qdat);
        auto load = [&](Context& c, int lo, int n) {
            c.load_device(di + (size_t)lo * seg_stride, dq + (size_t)lo * seg_stride, n, samples, seg_stride);
        };
        auto reload = [&](Context& c, int lo, const std::vector<int>& segs) {
            c.reload_rows(di + (size_t)lo * seg_stride, dq + (size_t)lo * seg_stride, true, seg_stride, samples, segs);
        };
        if (options.usehashtable && nseg > 1)             // the hash memory orders the segments: parallel all the same
            return decode_hashed(nseg, samples, options, decodes, max_results, n_results, load, reload, false, nullptr, nullptr,
                                 seg_stride, 0, nullptr, 0, 0, nullptr, 0, nullptr, nullptr);
        std::unique_ptr<HashChain::Ticket> turn;
        if (options.usehashtable) { turn.reset(new HashChain::Ticket(HashChain::get())); turn->wait_turn(); }
        return decode_split(nseg, samples, options, decodes, max_results, n_results, load, reload, false, nullptr, nullptr, seg_stride);
    } catch (const std::exception& e) {
        for (int s = 0; s < nseg; ++s) n_results[s] = 0;
        return fail("wspr_decode_batch_device", e);
    }
}

// Pins caller memory for the host-buffer entry points (hipHostRegister without the caller needing HIP headers): the
// reference's callers keep their I/Q buffers for the life of the process (rtlsdr_wsprd.c:78-90, 331-336), so they
// pin them once and every wspr_decode*() call on them is a plain DMA.
int wspr_pin_host_buffer(void* p, size_t bytes) {
    if (!p || !bytes) return -1;
    try { Context::get(); } catch (const std::exception& e) { return fail("wspr_pin_host_buffer", e); }
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (e == hipSuccess || e == hipErrorHostMemoryAlreadyRegistered) { (void)hipGetLastError(); return 0; }
    fprintf(stderr, "libwspr_mi355x: wspr_pin_host_buffer: %s\n", hipGetErrorString(e));
    (void)hipGetLastError();
    return -1;
}
int wspr_unpin_host_buffer(void* p) {
    if (!p) return -1;
    const hipError_t e = hipHostUnregister(p);
    (void)hipGetLastError();
    return e == hipSuccess ? 0 : -1;
}

int wspr_decode(float* idat, float* qdat, int samples, struct decoder_options options,
                struct decoder_results* decodes, int* n_results) {
    // the reference caller owns decodes[] with room for its own count (50 in rtlsdr_wsprd.c:117)
    std::vector<decoder_results> tmp(MAX_UNIQUES);
    int n = 0;
    const int rc = wspr_decode_batch(idat, qdat, 1, samples, (size_t)samples, options, tmp.data(), MAX_UNIQUES, &n, 1);
    for (int i = 0; i < n; ++i) decodes[i] = tmp[i];
    *n_results = n;
    // wspr_last_spreads() follows the caller's array: entry i, n of them
    wspr::LastSpreads& last = wspr::last_spreads_of_thread();
    if (last.on && last.nseg == 1) { last.max_results = n < 0 ? 0 : n; last.rec.resize((size_t)last.max_results); }
    wspr::LastDetails& last_det = wspr::last_details_of_thread();
    if (last_det.on && last_det.nseg == 1) { last_det.max_results = n < 0 ? 0 : n; last_det.rec.resize((size_t)last_det.max_results); }
    return rc < 0 ? rc : 0;
}

void sync_and_demodulate(float* id, float* qd, long np, unsigned char* symbols, float* freq, int ifmin, int ifmax,
                         float fstep, int* shift, int lagmin, int lagmax, int lagstep, float* drift, int symfac,
                         float* sync, int mode) {
    LaneTurn lane_turn;
    try {            // symfac scales the soft symbols of mode 2 (wsprd.c:250); the decoder itself always passes 50 (:427)
        Context::get().demod_single(id, qd, np, symbols, freq, ifmin, ifmax, fstep, shift, lagmin, lagmax, lagstep,
                                    drift, sync, mode, symfac);
    } catch (const std::exception& e) { fail("sync_and_demodulate", e); }
}

int wspr_block_demod_batch(const float* idat, const float* qdat, int nseg, int samples, size_t seg_stride,
                           const wspr_block_item* items, int n, unsigned char* symbols) {
    static_assert(sizeof(wspr_block_item) == sizeof(wspr::BlockHyp), "wspr_block_item is the kernel's hypothesis");
    if (n < 0 || nseg < 0 || samples < 0 || samples > wspr::kMaxSamples) return -1;
    for (int i = 0; i < n; ++i)
        if (items[i].seg < 0 || items[i].seg >= nseg || !std::isfinite(items[i].freq) || !std::isfinite(items[i].drift)) return -1;
    if (n == 0) return 0;
    LaneTurn lane_turn;
    try {
        return Context::get().block_demod_batch(idat, qdat, nseg, samples, seg_stride, reinterpret_cast<const wspr::BlockHyp*>(items), n,
                                   symbols);
    } catch (const std::exception& e) { return fail("wspr_block_demod_batch", e); }
}

void subtract_signal2(float* id, float* qd, long np, float f0, int shift, float drift,
                      const unsigned char* channel_symbols) {
    LaneTurn lane_turn;
    try { Context::get().subtract_single(id, qd, np, f0, shift, drift, channel_symbols); }
    catch (const std::exception& e) { fail("subtract_signal2", e); }
}

void subtract_signal(float* id, float* qd, long np, float f0, int shift, float drift,
                     const unsigned char* channel_symbols) {
    LaneTurn lane_turn;
    try { Context::get().subtract_symbolwise_single(id, qd, np, f0, shift, drift, channel_symbols); }
    catch (const std::exception& e) { fail("subtract_signal", e); }
}

}  // extern "C"
