// The stage calls of a context: device rows or records in, device rows or records out, outside a decode -- K0 (the
// RTL-SDR front end and its streams), K12 (audio front end), K15 (blanker), K16 (noise figures), K8/K13 (signal
// synthesiser), K17 (audio scene synthesiser), K18 (IQ to audio), K20 (waterfall), K21 (tunable front end).  Each is complete on return: it ends with
// Impl::wait() on its stream and does NOT resolve the decode's deferred timings (that is sync()).  What they share is
// stated once, below: the staging of a transmission list and the per-record counters.  Arguments have been checked by
// the callers (wspr_stage_args.h); contexts, buffers and loads are wspr_context.hip.
#include "wspr_context_impl.h"
#include "../kernels/fade.h"
#include "../kernels/noise.h"
#include "../kernels/waterfall.h"

namespace wspr {

namespace {
// Per-record counters of a call (K15 samples blanked, K17 / K18 samples clipped): zeroed on the stream before the
// kernels add to them, fetched into memory of the call's own behind them, and handed to the caller only once the wait
// has succeeded -- a call whose device work fails has written nothing.
struct Counters {
    std::vector<int> host;
    int* dev;
    Counters(DevBuf& buf, int nseg, hipStream_t st) : host((size_t)nseg, 0), dev(static_cast<int*>(buf.need((size_t)nseg * sizeof(int)))) {
        HIP_OK(hipMemsetAsync(dev, 0, host.size() * sizeof(int), st));
    }
    void fetch(hipStream_t st) { HIP_OK(hipMemcpyAsync(host.data(), dev, host.size() * sizeof(int), hipMemcpyDeviceToHost, st)); }
    void hand_over(int* out) const { if (out) memcpy(out, host.data(), host.size() * sizeof(int)); }
};

// A sorted transmission list on the device (K8, K13, K17): the transmissions, the offsets per segment and room for the
// first index of each.  `off` is host memory of the call and must outlive the upload: the caller waits before it returns.
struct TxList {
    std::vector<int> off;
    SynthTx* d_tx = nullptr;
    int* d_off = nullptr;
    int* d_first = nullptr;
};
void stage_tx_list(Context::Impl& c, const wspr_synth_tx* tx, int ntx, int nseg, hipStream_t st, TxList& l) {
    l.off.assign((size_t)nseg + 1, 0);                         // the list is sorted by seg: offsets per segment
    for (int t = 0; t < ntx; ++t) ++l.off[(size_t)tx[t].seg + 1];
    for (int s = 0; s < nseg; ++s) l.off[(size_t)s + 1] += l.off[s];
    l.d_off = static_cast<int*>(c.synthoff.need(l.off.size() * sizeof(int)));
    upload(l.d_off, l.off.data(), l.off.size() * sizeof(int), st);
    if (ntx > 0) {
        l.d_tx = static_cast<SynthTx*>(c.synthtx.need((size_t)ntx * sizeof(SynthTx)));
        l.d_first = static_cast<int*>(c.synthfirst.need((size_t)ntx * sizeof(int)));
        upload(l.d_tx, tx, (size_t)ntx * sizeof(SynthTx), st);
    }
}
}  // namespace

// ------------------------------------------------------------------------------------------------------- K0 --
// CUs the front end may occupy (0 = all).  K0 is HBM-bound and launches hundreds of thousands of short workgroups:
// on an unmasked stream they take every CU as it frees up and the decoder's fp32-bound kernels of the other lanes
// wait.  Confined to a share of the CUs (a stream created with hipExtStreamCreateWithCUMask; consecutive mask bits
// fall on different XCDs, so the share is spread over all eight and keeps every HBM stack busy), K0 still finds
// the memory bandwidth it needs while the rest of the chip keeps computing.
std::atomic<int>& front_end_cus() {
    static std::atomic<int> v{[] { const char* e = lab_env("WSPR_K0_CUS"); return e ? atoi(e) : 0; }()};
    return v;
}

hipStream_t Context::front_end_stream() {
    Impl& c = *d;
    const int want = front_end_cus().load();
    if (want != c.fe_cus) {
        if (c.fe_stream) { (void)hipStreamSynchronize(c.fe_stream); (void)hipStreamDestroy(c.fe_stream); c.fe_stream = nullptr; }
        c.fe_cus = want;
        if (want > 0) {
            hipDeviceProp_t prop;
            HIP_OK(hipGetDeviceProperties(&prop, c.device));
            const int ncu = prop.multiProcessorCount;
            const int n = std::max(8, std::min(want, ncu));
            std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
            for (int i = 0; i < n; ++i) mask[i >> 5] |= 1u << (i & 31);
            HIP_OK(hipExtStreamCreateWithCUMask(&c.fe_stream, (uint32_t)mask.size(), mask.data()));
        }
    }
    return c.fe_stream ? c.fe_stream : c.stream;
}

int Context::decimate_device(const void* d_raw, size_t bytes_per_seg, int nseg, float* dI, float* dQ, int normalise,
                             int* h_nout, DecimState* d_states) {
    Impl& c = *d;
    const hipStream_t st = d_states ? c.stream : front_end_stream();     // whole segments only: streaming chunks are small
    const size_t nblocks = (size_t)decimate_blocks(bytes_per_seg / 2, d_states != nullptr);
    if (nblocks == 0) return -1;
    int32_t* scratch = static_cast<int32_t*>(c.decscratch.need((size_t)nseg * nblocks * 24));
    int* d_nv = static_cast<int*>(c.nvalid.need((size_t)nseg * 4));
    if (!d_states) {                                          // whole segments: the unfilled tail must read as zero
        HIP_OK(hipMemsetAsync(dI, 0, (size_t)nseg * kIqStride * 4, st));
        HIP_OK(hipMemsetAsync(dQ, 0, (size_t)nseg * kIqStride * 4, st));
    }
    launch_decimate(static_cast<const uint8_t*>(d_raw), bytes_per_seg, nseg, dI, dQ, d_nv, scratch, st, d_states);
    if (normalise) launch_normalise(dI, dQ, d_nv, nseg, kMaxSamples, st);
    if (h_nout) HIP_OK(hipMemcpyAsync(h_nout, d_nv, (size_t)nseg * 4, hipMemcpyDeviceToHost, st));
    c.wait(st);
    return 0;
}

// one chunk of one receiver's stream: state in, appended outputs and state out (host buffers)
int Context::decimate_stream(DecimState* h_state, const uint8_t* iq, size_t nbytes, float* I, float* Q, uint32_t fill,
                             uint32_t cap, uint32_t* new_fill) {
    Impl& c = *d;
    if (nbytes == 0) { if (new_fill) *new_fill = fill; return 0; }
    uint8_t* d_raw = static_cast<uint8_t*>(c.streamraw.need(nbytes + 16));
    DecimState* d_st = static_cast<DecimState*>(c.streamstate.need(sizeof(DecimState)));
    upload(d_raw, iq, nbytes, c.stream);
    upload(d_st, h_state, sizeof(DecimState), c.stream);
    float* wi = work_i(1);
    float* wq = work_q(1);
    int nout = 0;
    const int rc = decimate_device(d_raw, nbytes, 1, wi, wq, 0, &nout, d_st);
    if (rc) return rc;
    HIP_OK(hipMemcpy(h_state, d_st, sizeof(DecimState), hipMemcpyDeviceToHost));
    const uint32_t room = fill < cap ? cap - fill : 0u;
    const uint32_t take = std::min<uint32_t>((uint32_t)nout, room);       // outputs beyond the capacity are dropped
    if (take) {                                                            // (rtlsdr_wsprd.c:236-242)
        HIP_OK(hipMemcpy(I + fill, wi, (size_t)take * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(Q + fill, wq, (size_t)take * 4, hipMemcpyDeviceToHost));
    }
    if (new_fill) *new_fill = fill + take;
    return 0;
}

// One chunk of each of n receivers' streams: what n calls of decimate_stream() do, as ONE host-to-device transfer, one
// launch set over n rows with n carried states, and three transfers back (states, the rows' first outputs per rail).
// A callback of 65 536 bytes yields five or six samples: its cost is the round trips, not the arithmetic.
int Context::decimate_stream_many(DecimState* const* h_states, const uint8_t* const* iq, size_t nbytes, int n, float* const* I,
                                  float* const* Q, const uint32_t* fill, uint32_t cap, uint32_t* new_fill) {
    Impl& c = *d;
    if (n <= 0 || nbytes == 0) { for (int k = 0; k < n; ++k) new_fill[k] = fill[k]; return 0; }
    const int maxout = (int)(nbytes / 2 / 6401) + 2;                       // outputs a chunk of this size can yield
    const size_t ocols = (size_t)((maxout + 3) & ~3);
    uint8_t* h_raw = static_cast<uint8_t*>(c.h_streamraw.need((size_t)n * nbytes));
    DecimState* h_st = static_cast<DecimState*>(c.h_streamstate.need((size_t)n * sizeof(DecimState) + (size_t)n * 4));
    int* h_nout = reinterpret_cast<int*>(h_st + n);
    float* h_out = static_cast<float*>(c.h_streamout.need(2 * (size_t)n * ocols * 4));
    for (int k = 0; k < n; ++k) {
        memcpy(h_raw + (size_t)k * nbytes, iq[k], nbytes);
        h_st[k] = *h_states[k];
    }
    uint8_t* d_raw = static_cast<uint8_t*>(c.streamraw.need((size_t)n * nbytes + 16));
    DecimState* d_st = static_cast<DecimState*>(c.streamstate.need((size_t)n * sizeof(DecimState)));
    HIP_OK(hipMemcpyAsync(d_raw, h_raw, (size_t)n * nbytes, hipMemcpyHostToDevice, c.stream));
    HIP_OK(hipMemcpyAsync(d_st, h_st, (size_t)n * sizeof(DecimState), hipMemcpyHostToDevice, c.stream));
    float* wi = work_i(n);
    float* wq = work_q(n);
    const size_t nblocks = (size_t)decimate_blocks(nbytes / 2, true);
    if (nblocks == 0) return -1;
    int32_t* scratch = static_cast<int32_t*>(c.decscratch.need((size_t)n * nblocks * 24));
    int* d_nv = static_cast<int*>(c.nvalid.need((size_t)n * 4));
    launch_decimate(d_raw, nbytes, n, wi, wq, d_nv, scratch, c.stream, d_st);
    HIP_OK(hipMemcpyAsync(h_nout, d_nv, (size_t)n * 4, hipMemcpyDeviceToHost, c.stream));
    HIP_OK(hipMemcpyAsync(h_st, d_st, (size_t)n * sizeof(DecimState), hipMemcpyDeviceToHost, c.stream));
    HIP_OK(hipMemcpy2DAsync(h_out, ocols * 4, wi, (size_t)kIqStride * 4, ocols * 4, n, hipMemcpyDeviceToHost, c.stream));
    HIP_OK(hipMemcpy2DAsync(h_out + (size_t)n * ocols, ocols * 4, wq, (size_t)kIqStride * 4, ocols * 4, n, hipMemcpyDeviceToHost, c.stream));
    sync();
    for (int k = 0; k < n; ++k) {
        *h_states[k] = h_st[k];
        const uint32_t room = fill[k] < cap ? cap - fill[k] : 0u;
        const uint32_t take = std::min<uint32_t>((uint32_t)std::max(0, std::min(h_nout[k], maxout)), room);   // beyond the capacity: dropped
        if (take) {                                                                          // (rtlsdr_wsprd.c:236-242)
            memcpy(I[k] + fill[k], h_out + (size_t)k * ocols, (size_t)take * 4);
            memcpy(Q[k] + fill[k], h_out + (size_t)n * ocols + (size_t)k * ocols, (size_t)take * 4);
        }
        new_fill[k] = fill[k] + take;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- K12 and K15 --
// K12: the audio front end on the lane's stream, then (normalise) the receiver's scaling as for the RTL-SDR front end
int Context::audio_device(const void* d_pcm, size_t pcm_stride, int nsamp, int nseg, float* dI, float* dQ, int normalise) {
    Impl& c = *d;
    if (nseg <= 0) return 0;
    launch_audio_front(static_cast<const int16_t*>(d_pcm), pcm_stride, nsamp, nseg, dI, dQ, c.stream);
    if (normalise) launch_normalise(dI, dQ, nullptr, nseg, kMaxSamples, c.stream);
    HIP_OK(hipGetLastError());
    c.wait(c.stream);
    return 0;
}

int16_t* Context::audio_pcm(size_t nsamp) { return static_cast<int16_t*>(d->audiopcm.need(((nsamp + 7) & ~(size_t)7) * 2 + 16)); }

// K15: the blanker on the lane's stream; the records' counters come back with it
int Context::audio_blank_device(const void* d_pcm, size_t pcm_stride, int nsamp, int nseg, int thr16, int guard, void* d_out,
                                size_t out_stride, int* h_blanked) {
    Impl& c = *d;
    if (nseg <= 0) return 0;
    Counters blanked(c.blankcount, nseg, c.stream);
    launch_audio_blank(static_cast<const int16_t*>(d_pcm), pcm_stride, nsamp, nseg, thr16, guard, static_cast<int16_t*>(d_out),
                       out_stride, blanked.dev, c.stream);
    HIP_OK(hipGetLastError());
    blanked.fetch(c.stream);
    c.wait(c.stream);
    blanked.hand_over(h_blanked);
    return 0;
}

// K15 then K12, kBlankChunk records at a time through the context's scratch rows (both kernels on the lane's stream, so a
// chunk's K15 waits for the K12 that still reads the rows): the scratch never exceeds kBlankChunk rows, whatever nseg is
int Context::audio_blanked_device(const void* d_pcm, size_t pcm_stride, int nsamp, int nseg, int thr16, int guard, float* dI,
                                  float* dQ, int normalise, int* h_blanked) {
    Impl& c = *d;
    if (nseg <= 0) return 0;
    const size_t row = ((size_t)nsamp + 7) & ~(size_t)7;
    const size_t bytes = (size_t)std::min(nseg, kBlankChunk) * row * sizeof(int16_t) + 16;
    if (bytes > c.blankrows.cap) {                            // exactly what is needed: need() would add a quarter to 369 MB
        c.blankrows.release();
        HIP_OK(hipMalloc(&c.blankrows.p, bytes));
        c.blankrows.cap = bytes;
    }
    int16_t* rows = c.blankrows.as<int16_t>();
    Counters blanked(c.blankcount, nseg, c.stream);
    const int16_t* in = static_cast<const int16_t*>(d_pcm);
    for (int s0 = 0; s0 < nseg; s0 += kBlankChunk) {
        const int n = std::min(kBlankChunk, nseg - s0);
        launch_audio_blank(in + (size_t)s0 * pcm_stride, pcm_stride, nsamp, n, thr16, guard, rows, row, blanked.dev + s0, c.stream);
        launch_audio_front(rows, row, nsamp, n, dI + (size_t)s0 * kIqStride, dQ + (size_t)s0 * kIqStride, c.stream);
    }
    if (normalise) launch_normalise(dI, dQ, nullptr, nseg, kMaxSamples, c.stream);
    HIP_OK(hipGetLastError());
    blanked.fetch(c.stream);
    c.wait(c.stream);
    blanked.hand_over(h_blanked);
    return 0;
}

// ------------------------------------------------------------------------------------------------------ K16 --
// The table of K16 and K20 (twiddles and window) is built on first use: a process that never asks for the figures or the
// pictures allocates nothing for them.
namespace {
void noise_table(Context::Impl& c) {
    if (c.noise_tab.p) return;
    std::vector<float> host(noise::kTableFloats);
    const double w2 = noise::noise_tables(host.data());
    float* p = static_cast<float*>(c.noise_tab.need(host.size() * sizeof(float)));
    HIP_OK(hipMemcpy(p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    c.noise_w2 = w2;
}
}  // namespace

// K16 on the lane's stream; the records come back with it.
int Context::noise_device(const float* dI, const float* dQ, int nseg, int samples, size_t stride, const noise::Windows& win,
                          noise::Result* out) {
    Impl& c = *d;
    if (nseg <= 0) return 0;
    noise_table(c);
    const size_t bytes = (size_t)nseg * sizeof(noise::Result);
    void* d_out = c.noise_out.need(bytes);
    noise::Result* h_out = static_cast<noise::Result*>(c.h_noise.need(bytes));
    launch_noise(dI, dQ, samples, stride, nseg, c.noise_tab.as<float>(), c.noise_w2, win, d_out, c.stream);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h_out, d_out, bytes, hipMemcpyDeviceToHost, c.stream));
    c.wait(c.stream);
    memcpy(out, h_out, bytes);                               // every record has arrived before the first is handed over
    return 0;
}

// ------------------------------------------------------------------------------------------------------ K20 --
// K20 on the lane's stream: the thresholds go up, floor mode runs K16 into scratch of its own (its default windows: they
// play no part in fft_p30), K20 reads that, the 16-byte records come down -- three steps and one wait
int Context::waterfall_device(const float* dI, const float* dQ, int nseg, int samples, size_t stride, const waterfall::Params& p,
                              uint8_t* d_img, size_t img_stride, waterfall::Info* info) {
    Impl& c = *d;
    if (nseg <= 0) return 0;
    const hipStream_t st = c.stream;
    noise_table(c);
    double* h_levels = static_cast<double*>(c.h_wf_levels.need(waterfall::kLevels * sizeof(double)));
    waterfall::level_table(p.db_min, p.db_step, h_levels);
    double* d_levels = static_cast<double*>(c.wf_levels.need(waterfall::kLevels * sizeof(double)));
    upload(d_levels, h_levels, waterfall::kLevels * sizeof(double), st);
    const size_t bytes = (size_t)nseg * sizeof(waterfall::Info);
    waterfall::Info* d_info = static_cast<waterfall::Info*>(c.wf_info.need(bytes));
    waterfall::Info* h_info = static_cast<waterfall::Info*>(c.h_wf_info.need(bytes));
    HIP_OK(hipMemsetAsync(d_info, 0, bytes, st));
    noise::Result* d_floor = nullptr;
    if (p.ref_mode == waterfall::kRefFloor) {
        d_floor = static_cast<noise::Result*>(c.wf_floor.need((size_t)nseg * sizeof(noise::Result)));
        launch_noise(dI, dQ, samples, stride, nseg, c.noise_tab.as<float>(), c.noise_w2,
                     noise::Windows{noise::kPreB0, noise::kPreB1, noise::kPostB0, noise::kPostB1}, d_floor, st);
    }
    launch_waterfall(dI, dQ, samples, stride, nseg, c.noise_tab.as<float>(), c.noise_w2, p, d_levels, d_floor, d_img, img_stride,
                     d_info, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h_info, d_info, bytes, hipMemcpyDeviceToHost, st));
    c.wait(st);
    memcpy(info, h_info, bytes);                             // every record has arrived before the first is handed over
    return 0;
}

uint8_t* Context::waterfall_image(size_t bytes) { return static_cast<uint8_t*>(d->wf_img.need(bytes + 16)); }

// ---------------------------------------------------------------------------------------- K8, K13 and K17 --
// K8, or K13 with one FadeChannel per transmission
int Context::synth_device(const wspr_synth_tx* tx, int ntx, int nseg, long long seg_index0, float sigma, uint64_t seed,
                          int flags, float* dI, float* dQ, const FadeChannel* fade) {
    Impl& c = *d;
    if (nseg <= 0) return 0;
    const hipStream_t st = c.stream;
    TxList l;
    stage_tx_list(c, tx, ntx, nseg, st, l);
    double* d_ckpt = ntx > 0 ? static_cast<double*>(c.synthckpt.need(synth_checkpoint_doubles(ntx) * sizeof(double))) : nullptr;
    if (fade) {
        FadeChannel* d_fade = nullptr;
        if (ntx > 0) {
            d_fade = static_cast<FadeChannel*>(c.synthfade.need((size_t)ntx * sizeof(FadeChannel)));
            upload(d_fade, fade, (size_t)ntx * sizeof(FadeChannel), st);
        }
        launch_synth_faded(l.d_tx, d_fade, ntx, l.d_off, nseg, seg_index0, sigma, (unsigned long long)seed,
                           (flags & kSynthFlagAccumulate) != 0, d_ckpt, l.d_first, dI, dQ, st);
    } else {
        launch_synth(l.d_tx, ntx, l.d_off, nseg, seg_index0, sigma, (unsigned long long)seed, (flags & kSynthFlagAccumulate) != 0,
                     d_ckpt, l.d_first, dI, dQ, st);
    }
    if (flags & kSynthFlagNormalise) launch_normalise(dI, dQ, nullptr, nseg, kMaxSamples, st);   // rtlsdr_wsprd.c:290-305
    HIP_OK(hipGetLastError());
    c.wait(st);                                                // the list's offsets and tx are host memory of this call
    return 0;
}

float* Context::synth_rows() { return static_cast<float*>(d->synthrows.need((size_t)2 * kIqStride * sizeof(float))); }

// K17: the list as for K8, P_i and dphi_i of each transmission instead of the checkpoints
int Context::synth_audio_device(const wspr_synth_tx* tx, int ntx, int nseg, long long seg_index0, int nsamp, float sigma,
                                uint64_t seed, int flags, int16_t* d_pcm, size_t pcm_stride, int* h_clipped) {
    Impl& c = *d;
    if (nseg <= 0) return 0;
    const hipStream_t st = c.stream;
    TxList l;
    stage_tx_list(c, tx, ntx, nseg, st, l);
    double* d_phase = ntx > 0 ? static_cast<double*>(c.asynthphase.need(audio_synth_phase_doubles(ntx) * sizeof(double))) : nullptr;
    Counters clipped(c.asynthcount, nseg, st);
    launch_audio_synth(l.d_tx, ntx, l.d_off, nseg, seg_index0, nsamp, sigma, (unsigned long long)seed,
                       (flags & kSynthFlagAccumulate) != 0, d_phase, l.d_first, d_pcm, pcm_stride, clipped.dev, st);
    HIP_OK(hipGetLastError());
    clipped.fetch(st);
    c.wait(st);                                                // the list's offsets and tx are host memory of this call
    clipped.hand_over(h_clipped);
    return 0;
}

// ------------------------------------------------------------------------------------------------------ K21 --
int Context::tune_device(const void* d_raw, size_t bytes_per_seg, int nseg, const uint32_t* steps, int nbands, float* dI, float* dQ,
                         int normalise, int* h_nout) {
    Impl& c = *d;
    if (nseg <= 0) return 0;
    const int nrows = nseg * nbands;
    long long* scratch = static_cast<long long*>(c.tunescratch.need(tune_scratch_bytes(bytes_per_seg, nseg, nbands) + 16));
    int* d_nv = static_cast<int*>(c.nvalid.need((size_t)nrows * 4));
    launch_tune(static_cast<const uint8_t*>(d_raw), bytes_per_seg, nseg, steps, nbands, dI, dQ, d_nv, scratch, c.stream);
    HIP_OK(hipGetLastError());
    if (normalise) launch_normalise(dI, dQ, d_nv, nrows, kMaxSamples, c.stream);
    std::vector<int> nout((size_t)nrows, 0);
    if (h_nout) HIP_OK(hipMemcpyAsync(nout.data(), d_nv, (size_t)nrows * 4, hipMemcpyDeviceToHost, c.stream));
    c.wait(c.stream);
    if (h_nout) memcpy(h_nout, nout.data(), (size_t)nrows * 4);
    return 0;
}

uint8_t* Context::tune_raw(size_t bytes) { return static_cast<uint8_t*>(d->tuneraw.need(bytes + 16)); }

// ------------------------------------------------------------------------------------------------------ K18 --
int Context::iq_audio_device(const float* dI, const float* dQ, int nseg, int samples, size_t stride, float gain, int16_t* d_pcm,
                             size_t pcm_stride, int* h_clipped) {
    Impl& c = *d;
    if (nseg <= 0) return 0;
    if (samples <= 0) {                                        // empty rows: empty records, nothing clipped, no device work
        if (h_clipped) std::fill(h_clipped, h_clipped + nseg, 0);
        return 0;
    }
    Counters clipped(c.iqaudiocount, nseg, c.stream);
    launch_iq_audio(dI, dQ, stride, samples, nseg, gain, d_pcm, pcm_stride, clipped.dev, c.stream);
    HIP_OK(hipGetLastError());
    clipped.fetch(c.stream);
    c.wait(c.stream);
    clipped.hand_over(h_clipped);
    return 0;
}

}  // namespace wspr
