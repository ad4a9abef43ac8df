// Context of the MI355X WSPR decoder (one per process, created lazily on the first
// call): HIP stream, constant tables, grow-only device/pinned buffers, host pool.
#pragma once
#include <chrono>
#include <atomic>
#include <functional>
#include <string>
#include <unordered_map>
#include <memory>
#include <vector>

#include "../../../include/wspr_mi355x.h"
#include "../../../include/wspr_mi355x_bench.h"   // declarations only: the definitions exist in the lab build (-DWSPR_LAB)
#include "../kernels/wspr_device.h"
#include "wspr_hashmem.h"
#include "wspr_msglist.h"

namespace wspr {

// Fano attempts the host pool left unfinished (see Context::decode_resident)
// cycles/bit the host Fano pool spends before leaving an attempt to the device tail (K6)
std::atomic<unsigned>& fano_fast_budget();
// -1 automatic, 0 host pool only, 1 device search for every attempt of a batch (see wspr_pipeline.hip)
std::atomic<int>& fano_device_setting();
// worker threads of all host pools alive in this process
std::atomic<int>& pool_workers_alive();
// shards of a node-level call sharing this host's CPUs (see wspr_decode_batch_node)
std::atomic<int>& node_share();
// CUs the front end (K0) may occupy, 0 = all (wspr_set_front_end_cus / WSPR_K0_CUS)
std::atomic<int>& front_end_cus();
#ifdef WSPR_LAB
// vectors K6w returned as -2 and Context::fano_resident() handed to the serial host decoder since the process began:
// [0] on the pool (the caller had a host copy), [1] one by one after a fetch (wspr_fano_host_handovers)
std::atomic<unsigned long long>& fano_handovers(int branch);
#endif

// The six process-wide settings a decode call honours: wspr_set_arithmetic() (0 exact, 1 contracted),
// wspr_set_osd_depth() (-1 off, 0..3), wspr_set_block_detection() (1 off, 2, 3), wspr_set_spread_estimate() (0 off, 1 on),
// wspr_set_spot_details() (0 off, 1 on) and the list of wspr_set_message_list() (null: off; message_list_setting() in
// wspr_msglist.h).
std::atomic<int>& arith_setting();
std::atomic<int>& osd_depth_setting();
std::atomic<int>& block_setting();
std::atomic<int>& spread_setting();
std::atomic<int>& details_setting();
// A call reads them ONCE, on entry: the outermost entry point of the calling thread holds a CallScope, which takes the
// snapshot, and everything the call does reads it through the call_*() accessors (outside a call they read the
// process-wide value).  A thread the call starts for itself (slots, node workers) installs the caller's snapshot with
// CallScope(settings).
struct CallSettings {
    int arith = 0, osd_depth = -1, maxblock = 1, spread = 0, details = 0;
    std::shared_ptr<const MessageList> list;
    static CallSettings snapshot();
};
const CallSettings*& call_settings_slot();                // thread-local: the current call's snapshot, null outside a call
inline CallSettings call_settings() { const CallSettings* s = call_settings_slot(); return s ? *s : CallSettings::snapshot(); }
inline int call_arith() { const CallSettings* s = call_settings_slot(); return s ? s->arith : arith_setting().load(); }
inline int call_osd_depth() { const CallSettings* s = call_settings_slot(); return s ? s->osd_depth : osd_depth_setting().load(); }
inline int call_maxblock() { const CallSettings* s = call_settings_slot(); return s ? s->maxblock : block_setting().load(); }
inline int call_spread() { const CallSettings* s = call_settings_slot(); return s ? s->spread : spread_setting().load(); }
inline int call_details() { const CallSettings* s = call_settings_slot(); return s ? s->details : details_setting().load(); }
inline std::shared_ptr<const MessageList> call_list() {
    const CallSettings* s = call_settings_slot();
    return s ? s->list : message_list_setting();
}
inline uint64_t call_list_generation() { const auto l = call_list(); return l ? l->generation : 0; }
struct CallScope {
    const bool owner;
    CallSettings mine;
    CallScope() : owner(!call_settings_slot()) { if (owner) { mine = CallSettings::snapshot(); call_settings_slot() = &mine; } }
    explicit CallScope(const CallSettings& s) : owner(!call_settings_slot()) { if (owner) { mine = s; call_settings_slot() = &mine; } }
    ~CallScope() { if (owner) call_settings_slot() = nullptr; }
    CallScope(const CallScope&) = delete;
    CallScope& operator=(const CallScope&) = delete;
};
// The records wspr_last_spreads() hands back: the calling thread's most recent decode call's, in the layout of that
// call's `decodes` array.  on = the call ran with the stage on and is of a family that records them.
struct LastSpreads {
    bool on = false;
    int nseg = 0, max_results = 0;
    std::vector<wspr_spread> rec;
};
LastSpreads& last_spreads_of_thread();
// The same for wspr_last_spot_details(): the records of wspr_set_spot_details(), kept and handed out alike.
struct LastDetails {
    bool on = false;
    int nseg = 0, max_results = 0;
    std::vector<wspr_spot_detail> rec;
};
LastDetails& last_details_of_thread();
// An entry point of a family that does not record them (node-level calls, receiver sessions): whatever batch calls it
// made on the calling thread, wspr_last_spreads() and wspr_last_spot_details() answer -1 after it.
struct NoSpreadRecord {
    ~NoSpreadRecord() { last_spreads_of_thread().on = false; last_details_of_thread().on = false; }
};

// The values of wspr_last_timings(), in the order include/wspr_mi355x.h documents (that order is ABI; the Python
// wrapper's TIMING_NAMES repeats it).  A new value goes at the end, here and in both of those.
enum TimingSlot : int {
    kTmFftSyncMs = 0, kTmHostBookkeepingMs, kTmDeviceFanoTailMs, kTmDemodMs, kTmSubtractMs, kTmHostFanoMs, kTmTotalMs,
    kTmFanoCalls, kTmFanoTimeouts, kTmFanoCycles, kTmCandidatesRefined, kTmGpuWaves, kTmFanoLeftToDevice,
    kTmSegmentsRedecoded, kTmCandidatesConsumed, kTmSubtractions,
    kTmCpuMsCall, kTmCpuMsPassStart, kTmCpuMsBuildWave, kTmCpuMsRefine, kTmCpuMsLadder, kTmCpuMsBooks, kTmCpuMsSubtract,
    kTmCpuMsFinish,
    kTmMessageCacheLookups, kTmMessageCacheHits,
    kTmOsdMs, kTmOsdVectors, kTmOsdSpots,
    kTmLagPruned, kTmLagExactEvals, kTmLagFallbacks,
    kTmBlockMs, kTmBlockVectors, kTmBlock2Decodes, kTmBlock3Decodes,
    kTmSpreadMs, kTmSpreadJobs,
    kTmListMs, kTmListVectors, kTmListSpots,
    kTmLagDriftPruned, kTmLagDriftExactEvals, kTmLagDriftFallbacks,
    kTmDetailMs, kTmDetailJobs,
    kTimingSlots
};
// A batch runs on several pipelines at once and each keeps its own values; wspr_last_timings() folds them.  The stage
// times and the wall time before this index overlap between pipelines: the call's figure is the MAXIMUM.  Everything
// from it on is SUMMED -- the counts, and the CPU times kTmCpuMs* as well (CPU time spent on different threads adds
// up; the public header says "summed over the slots").
constexpr int kTimingFirstSummed = kTmFanoCalls;
static_assert(kTimingSlots == 46 && kTimingFirstSummed == 7, "the layout of wspr_last_timings() is ABI");

struct PendingFano {
    std::vector<int> seg;                 // owning segment of each attempt
    std::vector<unsigned char> sym;       // 162 soft symbols each, transmission order
    void add(int s, const unsigned char* v) { seg.push_back(s); sym.insert(sym.end(), v, v + 162); }
};

// Exact full-budget results of Fano attempts that were already run, keyed by the soft-symbol vector
// (the search is a pure function of it): the re-decode of a segment replays the same vectors up to
// the point where the late success changes the IQ, and takes their results from here.
struct FanoMemo {
    struct Entry { int ret; unsigned cycles; unsigned char data[11]; };
    std::unordered_map<std::string, Entry> map;
    void add(const unsigned char* sym, int ret, unsigned cycles, const unsigned char* data10) {
        Entry e{ret, cycles, {0}};
        for (int k = 0; k < 10; ++k) e.data[k] = data10[k];
        map.emplace(std::string(reinterpret_cast<const char*>(sym), 162), e);
    }
    const Entry* find(const unsigned char* sym) const {
        const auto it = map.find(std::string(reinterpret_cast<const char*>(sym), 162));
        return it == map.end() ? nullptr : &it->second;
    }
};

class Context {
public:
    static Context& get();          // slot 0; throws std::runtime_error when no HIP device is usable
    static Context& slot(int i);    // i in [0, slots())
    static int slots();             // concurrent pipelines per process (env WSPR_SLOTS, default 3)
    static constexpr int kMaxLanes = 17;         // lanes 0..15 for callers, the last one for receiver sessions (feed)
    static constexpr int kUserLanes = kMaxLanes - 1;
    static constexpr int kMaxDevices = 16;
    static int lane();              // lane of the calling thread
    static void bind_lane(int lane);
    static void cap_slots(int n);   // calling thread: use at most n slots per batch (a shard's share of the host)
    static size_t release_buffers();   // current device, every lane and slot: bytes of device memory returned
    static int slot_cap();          // min(slots(), the thread's cap, the CPUs of its share)
    static Context* slot_if_exists(int i);   // slot i of the calling thread's (device, lane) if it was ever created
    static void note_slots_used(int n);      // slots the calling thread's current batch call runs on ...
    static int last_slots_used();            // ... as wspr_last_timings() reads it back
    int device();
    ~Context();

    hipStream_t stream();
    hipStream_t front_end_stream();   // the CU-masked stream of K0 when a share is set, else stream()
    const DeviceTables& tables();
    int host_threads();

    // working IQ buffers (planar, rows of kIqStride floats)
    float* work_i(int nseg);
    float* work_q(int nseg);
    void load_host(const float* I, const float* Q, int nseg, int samples, size_t stride);
    void load_device(const void* dI, const void* dQ, int nseg, int samples, size_t stride);
    void store_host(float* I, float* Q, int nseg, int samples, size_t stride);
    void reload_rows(const float* I, const float* Q, bool device, size_t stride, int samples,
                     const std::vector<int>& segs);
    void sync();

    float* ps_buffer(int nseg);
    void run_fft_sync(int nseg, int samples, int maxdrift, bool coarse, const int* d_seglist, int nactive,
                      float* noise_out, float* smspec_out);
    void fetch_candidates(int nseg, std::vector<int>& npk, std::vector<DevCand>& cand);
    void fetch_candidates_async(int nseg);                 // copies queued on the stream ...
    void finish_fetch_candidates(int nseg, std::vector<int>& npk, std::vector<DevCand>& cand);   // ... consumed after a wait

    // the decoder proper, on the working buffers
    // reload(segs): restore the original IQ of the listed segments in the working buffers (needed
    // for the exact re-decode after a late Fano success); empty function = no fast/tail split
    // hb / hb_off: the batch's shared hash memory and the index of this context's segment 0 within the call
    int decode_resident(int nseg, int samples, const decoder_options& opt, decoder_results* out,
                        int max_results, int* n_results,
                        const std::function<void(const std::vector<int>&)>& reload = nullptr,
                        wspr_trace* trace = nullptr, HashBatch* hb = nullptr, int hb_off = 0);
    int decode_core(int nseg, int samples, const decoder_options& opt, decoder_results* out, int max_results,
                    int* n_results, const std::vector<int>& active0, unsigned fast, PendingFano& pend,
                    const FanoMemo* memo = nullptr, wspr_trace* trace = nullptr, HashBatch* hb = nullptr, int hb_off = 0);
    // a later round of a usehashtable batch: the listed segments (rows already restored) once more, everything else
    // of the working buffers and of out / n_results left alone
    int decode_again(int nseg, int samples, const decoder_options& opt, decoder_results* out, int max_results,
                     int* n_results, const std::vector<int>& segs, HashBatch* hb, int hb_off);
    int last_timings(double* ms, int cap);
    int bench_fft_sync(int nseg, int samples, int iters, double* ms);
    int bench_valu(int nseg, int samples, int iters, double* ms);
    int bench_lag_drift(int nseg, int samples, double* ms);

    void demod_single(float* id, float* qd, long np, unsigned char* symbols, float* freq, int ifmin, int ifmax,
                      float fstep, int* shift, int lagmin, int lagmax, int lagstep, float* drift, float* sync,
                      int mode, int symfac = 50);
    void subtract_single(float* id, float* qd, long np, float f0, int shift, float drift, const unsigned char* sym);
    void subtract_symbolwise_single(float* id, float* qd, long np, float f0, int shift, float drift,
                                    const unsigned char* sym);
    // the wave-parallel search (k6_fano_wave.hip) over host vectors; steps (may be null): expansion steps per vector
    int fano_batch(const unsigned char* symbols, int n, unsigned maxcycles, int* ret, unsigned* cycles,
                   unsigned* metric, unsigned* maxnp, unsigned char* data, unsigned* steps = nullptr);
    // ... and over vectors already in HBM (vector i at d_symbols + h_offsets[i] * 162; h_symbols: their host copy, if any)
    int fano_resident(const unsigned char* d_symbols, const int* h_offsets, int n, unsigned maxcycles, int* ret,
                      unsigned* cycles, unsigned char* data, unsigned* metric = nullptr, unsigned* maxnp = nullptr,
                      unsigned* steps = nullptr, const unsigned char* h_symbols = nullptr);
    // K9 (k9_osd.hip; the definition in kernels/osd.h) over host vectors, and over vectors already in HBM (vector i at
    // d_symbols + h_offsets[i] * 162); results on the host: data n*11, dist, nhard, order
    int osd_batch(const unsigned char* symbols, int n, int depth, unsigned char* data, unsigned* dist, unsigned* nhard,
                  unsigned* order);
    int osd_resident(const unsigned char* d_symbols, const int* h_offsets, int n, int depth, unsigned char* data,
                     unsigned* dist, unsigned* nhard, unsigned* order);
    // K14 (k14_list.hip; the definition in kernels/listmatch.h) over host vectors, and over vectors already in HBM (vector i
    // at d_symbols + h_offsets[i] * 162) against `list`, whose table this context uploads on first use; results on the host
    int list_batch(const unsigned char* symbols, int n, const MessageList& list, wspr_list_match* out);
    int list_resident(const unsigned char* d_symbols, const int* h_offsets, int n, const MessageList& list, wspr_list_match* out);
    // K10 (k10_blockdemod.hip; the definition in kernels/blockdemod.h): the vectors of block sizes 1, 2, 3 of n hypotheses,
    // on the working rows (results on the host; rms n*3, sync n and d_symbols may be null) and over host rows
    int block_resident(const BlockHyp* hyps, int n, int samples, unsigned char* symbols, float* rms_out, float* sync_out,
                       const unsigned char** d_symbols = nullptr);
    int block_demod_batch(const float* I, const float* Q, int nseg, int samples, size_t stride, const BlockHyp* hyps, int n,
                          unsigned char* symbols);
    // K11 (k11_spread.hip; the definition in kernels/spread.h): the figure of n jobs over host rows; on the working rows,
    // queued without a wait (n x 4 words in pinned memory once the stream has passed); where a decode call's records go
    int spread_batch(const float* I, const float* Q, int nseg, int samples, size_t stride, const wspr_spread_item* items, int n,
                     wspr_spread* out);
    const uint32_t* spread_enqueue(const SubJob* jobs, int n, int samples);
    const float* spread_twiddle_table();
    void set_spread_out(wspr_spread* out);
    // K19 (k19_spot_quality.hip; the definition in kernels/spot_quality.h): the figures of n host vectors and their decdata;
    // over vectors already in HBM, queued without a wait (n x 5 words in pinned memory once the stream has passed): jobs
    // [first, first + count) of a group are the vectors at d_symbols + h_offsets[job] * 162 of that group's buffer -- a
    // wave's decodes lie in up to three (rung 0, the ladder's block, vectors a stage handed on); decdata n x 11 on the
    // host; where a decode call's records go
    struct SpotQualityGroup { const unsigned char* d_symbols; int first, count; };
    int spot_quality_batch(const unsigned char* symbols, const unsigned char* decdata, int n, wspr_spot_quality* out);
    const int32_t* spot_quality_enqueue(const SpotQualityGroup* groups, int ngroups, const int* h_offsets,
                                        const unsigned char* decdata, int n);
    const unsigned char* spot_quality_where_table();
    unsigned char* spot_quality_keep(size_t vectors);   // device room for vectors a stage hands on to the bookkeeping
    void set_detail_out(wspr_spot_detail* out);
    int bench_decimate(const void* d_raw, size_t bytes_per_seg, int nseg, float* dI, float* dQ, int iters, double* ms);
    int decimate_device(const void* d_raw, size_t bytes_per_seg, int nseg, float* dI, float* dQ, int normalise,
                        int* h_nout, DecimState* d_states = nullptr);
    int decimate_stream(DecimState* h_state, const uint8_t* iq, size_t nbytes, float* I, float* Q, uint32_t fill,
                        uint32_t cap, uint32_t* new_fill);
    // one chunk of EACH of n receivers' streams (all of nbytes): one transfer and one launch set for all of them
    int decimate_stream_many(DecimState* const* h_states, const uint8_t* const* iq, size_t nbytes, int n, float* const* I,
                             float* const* Q, const uint32_t* fill, uint32_t cap, uint32_t* new_fill);
    // K12 (k12_audio.hip): nseg validated records of 16-bit audio resident on the device into IQ rows; complete on return
    int audio_device(const void* d_pcm, size_t pcm_stride, int nsamp, int nseg, float* dI, float* dQ, int normalise);
    int16_t* audio_pcm(size_t nsamp);   // device scratch for one record (wspr_audio_to_iq)
    // K15 (k15_blank.hip): nseg validated records into blanked records; h_blanked (nseg, may be null) = samples blanked of
    // each; complete on return
    int audio_blank_device(const void* d_pcm, size_t pcm_stride, int nsamp, int nseg, int thr16, int guard, void* d_out,
                           size_t out_stride, int* h_blanked);
    // K15 then K12 through the context's own scratch rows, kBlankChunk records at a time; complete on return
    static constexpr int kBlankChunk = 128;
    int audio_blanked_device(const void* d_pcm, size_t pcm_stride, int nsamp, int nseg, int thr16, int guard, float* dI,
                             float* dQ, int normalise, int* h_blanked);

    // K16 (k16_noise.hip; the definition in kernels/noise.h): the noise figures of nseg validated device rows into out (host,
    // nseg records); complete on return.  The table of twiddles and window is built on first use, as spread_twiddle_table().
    int noise_device(const float* dI, const float* dQ, int nseg, int samples, size_t stride, const noise::Windows& win,
                     noise::Result* out);
    // K20 (k20_waterfall.hip; the definition in kernels/waterfall.h): the images of nseg validated device rows into nseg
    // validated device images and info (host, nseg records); floor mode runs K16 into scratch of its own first, on the same
    // stream and with no host wait in between; complete on return
    int waterfall_device(const float* dI, const float* dQ, int nseg, int samples, size_t stride, const waterfall::Params& p,
                         uint8_t* d_img, size_t img_stride, waterfall::Info* info);
    uint8_t* waterfall_image(size_t bytes);   // device scratch for one image (wspr_waterfall)

    // The stage calls below are wspr_context_stages.hip; their arguments have been validated (wspr_stage_args.h).
    // K8 (k8_synth.hip): a validated, sorted transmission list into nseg device rows; complete on return
    // fade: one FadeChannel (kernels/fade.h) per transmission in host memory for the fading channel (K13), or null (K8)
    int synth_device(const wspr_synth_tx* tx, int ntx, int nseg, long long seg_index0, float sigma, uint64_t seed,
                     int flags, float* dI, float* dQ, const FadeChannel* fade = nullptr);
    float* synth_rows();            // two rows of kIqStride floats of the context's own (wspr_selftest)
    // K17 (k17_audio_synth.hip; the definition in kernels/audio_synth.h): a validated, sorted transmission list into
    // nseg validated device records of nsamp 16-bit samples; h_clipped (nseg, may be null) = samples clipped of each;
    // complete on return
    int synth_audio_device(const wspr_synth_tx* tx, int ntx, int nseg, long long seg_index0, int nsamp, float sigma,
                           uint64_t seed, int flags, int16_t* d_pcm, size_t pcm_stride, int* h_clipped);
    // K18 (k18_iq_audio.hip; the definition in kernels/iq_audio.h): nseg validated device rows of `samples` samples into
    // nseg validated device records of 32 * samples 16-bit samples; h_clipped (nseg, may be null) = samples clipped of each;
    // complete on return
    int iq_audio_device(const float* dI, const float* dQ, int nseg, int samples, size_t stride, float gain, int16_t* d_pcm,
                        size_t pcm_stride, int* h_clipped);

    // K21 (k21_tune.hip; the definition in kernels/tune.h): nseg validated device rows of raw bytes and nbands validated host
    // steps into nseg * nbands device rows; h_nout (nseg * nbands, may be null) = outputs of each; complete on return
    int tune_device(const void* d_raw, size_t bytes_per_seg, int nseg, const uint32_t* steps, int nbands, float* dI, float* dQ,
                    int normalise, int* h_nout);
    uint8_t* tune_raw(size_t bytes);   // device scratch for one capture (wspr_tune_u8)

    struct Impl;
    struct DecodeRun;               // state of one decode_core() call (wspr_pipeline.hip)
    std::unique_ptr<Impl> d;

private:
    explicit Context(int nslots);
};

}  // namespace wspr
