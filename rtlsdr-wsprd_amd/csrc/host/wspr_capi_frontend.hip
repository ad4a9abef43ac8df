// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): the front end -- the decimator entry points and the
// receiver sessions.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <mutex>
#include <new>
#include <vector>

#include "wspr_capi_impl.h"
#include "wspr_stage_args.h"

using wspr::Context;
using namespace wspr::capi;
namespace args = wspr::args;

// ---- receiver session: the reference's double buffer and decoder thread body ----------------
// rx_state of rtlsdr_wsprd.c:78-90 (two I/Q buffers, their fill counters, the active index) plus the
// decimator's static state (:135-160), as one object the application drives from its own threads:
//   RX thread       wspr_session_feed()      = rtlsdr_callback()                       (:126-244)
//   main loop       wspr_session_rollover()  = switch buffers on the even minute       (:1179-1182)
//   decoder thread  wspr_session_decode()    = decoder(): too-short check, zero the tail, normalise, decode (:263-328)
struct wspr_session {
    decoder_options opt;
    wspr::DecimState dec;                      // all zero = the receiver at start-up
    std::vector<float> I[2], Q[2];
    std::atomic<uint32_t> fill[2];
    std::atomic<uint32_t> active;
    // feed() holds it from reading `active` to committing the new fill, rollover() takes it: a roll-over waits for
    // the callback in flight (the reference tests bufferIndex per output sample, rtlsdr_wsprd.c:236-242, so its
    // window is one sample; a GPU round trip must not straddle the switch), and no feed can write into a buffer
    // after rollover() has handed it to the decoder thread.
    std::mutex feed_mu;
};

namespace {
constexpr uint32_t kSessionSamples = 120 * 375;              // SIGNAL_LENGHT * SIGNAL_SAMPLE_RATE
constexpr uint32_t kSessionMinSamples = (120 - 3) * 375;     // rtlsdr_wsprd.c:277
constexpr int kFrontEndLane = Context::kMaxLanes - 1;        // feed() runs beside decode(): its own lane

// decoder()'s preparation of a completed buffer, rtlsdr_wsprd.c:277-305: false if it is too short to decode, else
// the tail zeroed and both rails scaled to a peak of 0.5
bool session_prepare(wspr_session* s, int buffer) {
    const uint32_t n = s->fill[buffer].load();
    if (n < kSessionMinSamples) return false;              // "Signal too short, skipping!" (:277-280)
    float* I = s->I[buffer].data();
    float* Q = s->Q[buffer].data();
    for (uint32_t i = n; i < kSessionSamples; ++i) { I[i] = 0.0f; Q[i] = 0.0f; }     // :284-288
    float peak = 1e-24f;                                    // :290-305
    for (uint32_t i = 0; i < kSessionSamples; ++i) {
        const float a = fabsf(I[i]), b = fabsf(Q[i]);
        if (a > peak) peak = a;
        if (b > peak) peak = b;
    }
    const float scale = (float)(0.5 / (double)peak);
    for (uint32_t i = 0; i < kSessionSamples; ++i) { I[i] *= scale; Q[i] *= scale; }
    return true;
}
}  // namespace

extern "C" {

int wspr_decimate_u8_batch_device(const void* d_raw, size_t bytes_per_seg, int nseg, void* d_idat, void* d_qdat,
                                  int normalise) {
    LaneTurn lane_turn;
    try {
        // rows are read with aligned 16-byte vector loads (a misaligned row stride would also let the last vector of
        // the last row run past the caller's allocation)
        if ((bytes_per_seg & 15) || (reinterpret_cast<uintptr_t>(d_raw) & 15)) {
            fprintf(stderr, "libwspr_mi355x: wspr_decimate_u8_batch_device: d_raw and bytes_per_seg must be multiples of 16\n");
            return -1;
        }
        return Context::get().decimate_device(d_raw, bytes_per_seg, nseg, (float*)d_idat, (float*)d_qdat, normalise, nullptr);
    } catch (const std::exception& e) { return fail("wspr_decimate_u8_batch_device", e); }
}

int wspr_decimate_u8_batch_device_stateful(const void* d_raw, size_t bytes_per_seg, int nseg, void* d_states,
                                           void* d_idat, void* d_qdat, int* n_out) {
    LaneTurn lane_turn;
    try {
        if (!d_states || (bytes_per_seg & 15)) return -1;
        return Context::get().decimate_device(d_raw, bytes_per_seg, nseg, (float*)d_idat, (float*)d_qdat, 0, n_out,
                                              static_cast<wspr::DecimState*>(d_states));
    } catch (const std::exception& e) { return fail("wspr_decimate_u8_batch_device_stateful", e); }
}

void wspr_front_end_constants(float* taps33, int* samples_per_output) { wspr::front_end_constants(taps33, samples_per_output); }

void wspr_decim_stream_reset(wspr_decim_state* st) {
    if (st) std::memset(st, 0, sizeof *st);
}

int wspr_decimate_u8_stream(wspr_decim_state* st, const uint8_t* iq, size_t nbytes, float* I, float* Q, uint32_t fill,
                            uint32_t capacity, uint32_t* new_fill) {
    LaneTurn lane_turn;
    static_assert(sizeof(wspr_decim_state) == sizeof(wspr::DecimState), "public and device state layouts differ");
    try {
        if (!st || (nbytes & 15)) return -1;
        return Context::get().decimate_stream(reinterpret_cast<wspr::DecimState*>(st), iq, nbytes, I, Q, fill, capacity,
                                              new_fill);
    } catch (const std::exception& e) { return fail("wspr_decimate_u8_stream", e); }
}

int wspr_decimate_u8(const uint8_t* iq, size_t nbytes, float* I, float* Q, uint32_t* n_out, int normalise) {
    LaneTurn lane_turn;
    try {
        Context& c = Context::get();
        nbytes &= ~(size_t)7;
        TempDev raw(nbytes + 16);
        HIP_TRY(hipMemcpy(raw.p, iq, nbytes, hipMemcpyHostToDevice));
        float* wi = c.work_i(1);
        float* wq = c.work_q(1);
        int nout = 0;
        const int rc = c.decimate_device(raw.p, nbytes, 1, wi, wq, normalise, &nout);
        if (rc) return rc;
        rows_down(I, Q, wi, wq);
        if (n_out) *n_out = (uint32_t)nout;
        return 0;
    } catch (const std::exception& e) { return fail("wspr_decimate_u8", e); }
}

// ---- K12, the 12 kHz audio front end (kernels/audio_front.h), and K15, the impulse-noise blanker in front of it
// (kernels/audio_blank.h) ---------------------------------------------------------------------------------------------
int wspr_audio_batch_device(const void* d_pcm, size_t pcm_stride, int nsamp, int nseg, void* d_idat, void* d_qdat,
                            int normalise) {
    static const char* where = "wspr_audio_batch_device";
    LaneTurn lane_turn;
    try {
        if (const int bad = args::audio_batch(where, d_pcm, pcm_stride, nsamp, nseg, d_idat, d_qdat)) return bad;
        return Context::get().audio_device(d_pcm, pcm_stride, nsamp, nseg, (float*)d_idat, (float*)d_qdat, normalise);
    } catch (const std::exception& e) { return fail(where, e); }
}

int wspr_audio_blank_batch_device(const void* d_pcm, size_t pcm_stride, int nsamp, int nseg, int thr16, int guard, void* d_out,
                                  size_t out_stride, int* n_blanked) {
    static const char* where = "wspr_audio_blank_batch_device";
    LaneTurn lane_turn;
    try {
        if (const int bad = args::audio_blank_batch(where, d_pcm, pcm_stride, nsamp, nseg, thr16, guard, d_out, out_stride)) return bad;
        if (nseg == 0) return 0;
        return Context::get().audio_blank_device(d_pcm, pcm_stride, nsamp, nseg, thr16, guard, d_out, out_stride, n_blanked);
    } catch (const std::exception& e) { return fail(where, e); }
}

int wspr_audio_blanked_batch_device(const void* d_pcm, size_t pcm_stride, int nsamp, int nseg, int thr16, int guard,
                                    void* d_idat, void* d_qdat, int normalise, int* n_blanked) {
    static const char* where = "wspr_audio_blanked_batch_device";
    LaneTurn lane_turn;
    try {
        if (const int bad = args::audio_blanked_batch(where, d_pcm, pcm_stride, nsamp, nseg, thr16, guard, d_idat, d_qdat)) return bad;
        return Context::get().audio_blanked_device(d_pcm, pcm_stride, nsamp, nseg, thr16, guard, (float*)d_idat, (float*)d_qdat,
                                                   normalise, n_blanked);
    } catch (const std::exception& e) { return fail(where, e); }
}

// wspr_audio_to_iq() and, with blank = (thr16, guard), wspr_audio_to_iq_blanked(): one record through the context's scratch
static int audio_to_iq(const char* where, const int16_t* pcm, size_t nsamp, const int* blank, float* I, float* Q, uint32_t* n_out,
                       int normalise, int* n_blanked) {
    try {
        if (const int bad = args::audio_host(where, pcm, nsamp, blank, I, Q)) return bad;
        Context& c = Context::get();
        int16_t* d_pcm = c.audio_pcm(nsamp);
        if (nsamp) HIP_TRY(hipMemcpy(d_pcm, pcm, nsamp * sizeof(int16_t), hipMemcpyHostToDevice));
        float* wi = c.work_i(1);
        float* wq = c.work_q(1);
        const size_t stride = (nsamp + 7) & ~(size_t)7;
        int blanked = 0;
        const int rc = blank ? c.audio_blanked_device(d_pcm, stride, (int)nsamp, 1, blank[0], blank[1], wi, wq, normalise, &blanked)
                             : c.audio_device(d_pcm, stride, (int)nsamp, 1, wi, wq, normalise);
        if (rc) return rc;
        rows_down(I, Q, wi, wq);
        if (n_out) *n_out = (uint32_t)audio_front_n_out((int)nsamp);
        if (n_blanked) *n_blanked = blanked;
        return 0;
    } catch (const std::exception& e) { return fail(where, e); }
}

int wspr_audio_to_iq(const int16_t* pcm, size_t nsamp, float* I, float* Q, uint32_t* n_out, int normalise) {
    LaneTurn lane_turn;
    return audio_to_iq("wspr_audio_to_iq", pcm, nsamp, nullptr, I, Q, n_out, normalise, nullptr);
}

int wspr_audio_to_iq_blanked(const int16_t* pcm, size_t nsamp, int thr16, int guard, float* I, float* Q, uint32_t* n_out,
                             int normalise, int* n_blanked) {
    LaneTurn lane_turn;
    const int blank[2] = {thr16, guard};
    return audio_to_iq("wspr_audio_to_iq_blanked", pcm, nsamp, blank, I, Q, n_out, normalise, n_blanked);
}

void wspr_audio_constants(float* taps_i511, float* taps_q511, int* samples_per_output) {
    float gi[AUDIO_FRONT_NTAPS], gq[AUDIO_FRONT_NTAPS];
    wspr::audio_front_taps(gi, gq);
    if (taps_i511) std::memcpy(taps_i511, gi, sizeof gi);
    if (taps_q511) std::memcpy(taps_q511, gq, sizeof gq);
    if (samples_per_output) *samples_per_output = AUDIO_FRONT_DECIM;
}

wspr_session* wspr_session_create(struct decoder_options options) {
    wspr_session* s = new (std::nothrow) wspr_session;
    if (!s) return nullptr;
    s->opt = options;
    std::memset(&s->dec, 0, sizeof s->dec);
    for (int b = 0; b < 2; ++b) {
        s->I[b].assign(kSessionSamples, 0.0f);
        s->Q[b].assign(kSessionSamples, 0.0f);
        s->fill[b].store(0);
    }
    s->active.store(0);                                     // initSampleStorage(), rtlsdr_wsprd.c:331-336
    return s;
}

void wspr_session_destroy(wspr_session* s) { delete s; }

int wspr_session_feed(wspr_session* s, const uint8_t* buf, uint32_t len) {
    if (!s || !buf || (len & 15u)) return -1;
    const int caller_lane = Context::lane();
    std::lock_guard<std::mutex> hold(s->feed_mu);
    try {
        Context::bind_lane(kFrontEndLane);
        // every session's front end runs on the ONE lane reserved for it: the RX threads of several receivers take
        // turns at its context (stream, staging buffers) -- a callback is ~0.1 ms of it against the 13.65 ms it covers
        LaneTurn lane_turn;
        const uint32_t idx = s->active.load();
        uint32_t nf = s->fill[idx].load();
        const int rc = Context::get().decimate_stream(&s->dec, buf, len, s->I[idx].data(), s->Q[idx].data(), nf,
                                                      kSessionSamples, &nf);           // :236-242: full buffer drops the rest
        Context::bind_lane(caller_lane);
        if (rc) return rc;
        s->fill[idx].store(nf);
        return (int)nf;
    } catch (const std::exception& e) {
        Context::bind_lane(caller_lane);
        return fail("wspr_session_feed", e);
    }
}

int wspr_session_feed_many(wspr_session* const* sessions, const uint8_t* const* bufs, uint32_t len, int n, int* fills) {
    if (!sessions || !bufs || n < 0 || (len & 15u)) return -1;
    if (n == 0) return 0;
    std::vector<wspr_session*> order(sessions, sessions + n);
    for (int k = 0; k < n; ++k) if (!sessions[k] || !bufs[k]) return -1;
    std::sort(order.begin(), order.end());                      // one locking order for every caller; duplicates refused
    if (std::adjacent_find(order.begin(), order.end()) != order.end()) return -1;
    std::vector<std::unique_lock<std::mutex>> held;
    for (wspr_session* s : order) held.emplace_back(s->feed_mu);
    const int caller_lane = Context::lane();
    try {
        Context::bind_lane(kFrontEndLane);
        LaneTurn lane_turn;
        std::vector<wspr::DecimState*> st(n);
        std::vector<float*> I(n), Q(n);
        std::vector<uint32_t> fill(n), nf(n);
        std::vector<uint32_t> idx(n);
        for (int k = 0; k < n; ++k) {
            idx[k] = sessions[k]->active.load();
            st[k] = &sessions[k]->dec;
            I[k] = sessions[k]->I[idx[k]].data();
            Q[k] = sessions[k]->Q[idx[k]].data();
            fill[k] = sessions[k]->fill[idx[k]].load();
        }
        const int rc = Context::get().decimate_stream_many(st.data(), bufs, len, n, I.data(), Q.data(), fill.data(),
                                                           kSessionSamples, nf.data());
        Context::bind_lane(caller_lane);
        if (rc) return rc;
        for (int k = 0; k < n; ++k) {
            sessions[k]->fill[idx[k]].store(nf[k]);
            if (fills) fills[k] = (int)nf[k];
        }
        return 0;
    } catch (const std::exception& e) {
        Context::bind_lane(caller_lane);
        return fail("wspr_session_feed_many", e);
    }
}

int wspr_session_rollover(wspr_session* s) {
    if (!s) return -1;
    std::lock_guard<std::mutex> hold(s->feed_mu);            // not while a callback's outputs are still on their way
    const uint32_t prev = s->active.load(), next = prev ^ 1u;
    s->fill[next].store(0);                                 // rx_state.iqIndex[rx_state.bufferIndex] = 0
    s->active.store(next);
    return (int)prev;
}

uint32_t wspr_session_fill(const wspr_session* s, int buffer) { return (s && (buffer & ~1) == 0) ? s->fill[buffer].load() : 0u; }

const float* wspr_session_samples(const wspr_session* s, int buffer, int rail) {
    if (!s || (buffer & ~1) != 0) return nullptr;
    return rail ? s->Q[buffer].data() : s->I[buffer].data();
}

int wspr_session_decode(wspr_session* s, int buffer, struct decoder_results* decodes, int* n_results) {
    wspr::NoSpreadRecord no_record;
    if (!s || (buffer & ~1) != 0 || !n_results) return -1;
    *n_results = 0;
    if (!session_prepare(s, buffer)) return 0;
    const int rc = wspr_decode(s->I[buffer].data(), s->Q[buffer].data(), (int)kSessionSamples, s->opt, decodes, n_results);   // :312-317
    return rc < 0 ? rc : 1;
}

// Many receivers, one slot: the completed buffers of n sessions decoded TOGETHER -- the decoder thread's body
// (rtlsdr_wsprd.c:263-328) for every receiver of a service in one batch call per distinct set of decoder options
// (receivers of one band share theirs; `freq` enters the reported frequency in double precision, so receivers with
// different options are not folded into one call).  Results, and what the buffers hold afterwards, are those of
// wspr_session_decode() on each session in index order -- with usehashtable that order is the order of the hash memory,
// and only runs of consecutive sessions with equal options share a call (see `ordered` below).
int wspr_session_decode_many(wspr_session* const* sessions, const int* buffers, int n, struct decoder_results* decodes,
                             int max_results, int* n_results, int* decoded) {
    wspr::NoSpreadRecord no_record;
    if (!sessions || !buffers || n < 0 || !decodes || max_results < 1 || !n_results) return -1;
    wspr::CallScope call_scope;            // one set of settings for every group of options this call decodes
    for (int k = 0; k < n; ++k) {
        n_results[k] = 0;
        if (decoded) decoded[k] = 0;
        if (!sessions[k] || (buffers[k] & ~1) != 0) return -1;
    }
    std::vector<int> ready;
    for (int k = 0; k < n; ++k)
        if (session_prepare(sessions[k], buffers[k])) { ready.push_back(k); if (decoded) decoded[k] = 1; }
    std::vector<char> taken(ready.size(), 0);
    std::vector<float> I, Q;
    std::vector<decoder_results> out;
    std::vector<int> nout, group;
    // the hash memory (hashtable.txt) is shared by every session with the option and ordered by the calls: as soon as one
    // ready session uses it, only RUNS of consecutive sessions with equal options are folded, so that the memory sees
    // the sessions in index order whatever their options (opt A, opt B, opt A stays 0, 1, 2 -- not 0, 2, 1)
    bool ordered = false;
    for (int k : ready) ordered = ordered || sessions[k]->opt.usehashtable != 0;
    for (size_t a = 0; a < ready.size(); ++a) {
        if (taken[a]) continue;
        const decoder_options& opt = sessions[ready[a]]->opt;
        group.clear();
        for (size_t b = a; b < ready.size(); ++b) {
            const bool same = !taken[b] && std::memcmp(&sessions[ready[b]]->opt, &opt, sizeof opt) == 0;
            if (same) { taken[b] = 1; group.push_back(ready[b]); }
            else if (ordered) break;
        }
        const int m = (int)group.size();
        int rc;
        if (m == 1) {
            wspr_session* s = sessions[group[0]];
            const int b = buffers[group[0]];
            rc = wspr_decode_batch(s->I[b].data(), s->Q[b].data(), 1, (int)kSessionSamples, kSessionSamples, opt,
                                   decodes + (size_t)group[0] * max_results, max_results, n_results + group[0], 1);
        } else {
            I.resize((size_t)m * kSessionSamples); Q.resize((size_t)m * kSessionSamples);
            out.assign((size_t)m * max_results, decoder_results{});
            nout.assign((size_t)m, 0);
            for (int g = 0; g < m; ++g) {
                std::memcpy(I.data() + (size_t)g * kSessionSamples, sessions[group[g]]->I[buffers[group[g]]].data(), kSessionSamples * sizeof(float));
                std::memcpy(Q.data() + (size_t)g * kSessionSamples, sessions[group[g]]->Q[buffers[group[g]]].data(), kSessionSamples * sizeof(float));
            }
            rc = wspr_decode_batch(I.data(), Q.data(), m, (int)kSessionSamples, kSessionSamples, opt, out.data(), max_results, nout.data(), 1);
            if (rc >= 0)
                for (int g = 0; g < m; ++g) {               // spots, and the residual the single call leaves in the buffer
                    std::memcpy(decodes + (size_t)group[g] * max_results, out.data() + (size_t)g * max_results, (size_t)nout[g] * sizeof(decoder_results));
                    n_results[group[g]] = nout[g];
                    std::memcpy(sessions[group[g]]->I[buffers[group[g]]].data(), I.data() + (size_t)g * kSessionSamples, kSessionSamples * sizeof(float));
                    std::memcpy(sessions[group[g]]->Q[buffers[group[g]]].data(), Q.data() + (size_t)g * kSessionSamples, kSessionSamples * sizeof(float));
                }
        }
        if (rc < 0) { for (int k = 0; k < n; ++k) n_results[k] = 0; return rc; }
    }
    return (int)ready.size();
}

uint32_t wspr_usec_to_next_slot(long tv_sec, long tv_usec) {                              // :1170-1175
    const uint32_t sec = (uint32_t)(tv_sec % 120);
    const uint32_t usec = sec * 1000000u + (uint32_t)tv_usec;
    return 120000000u - usec;
}

}  // extern "C"
