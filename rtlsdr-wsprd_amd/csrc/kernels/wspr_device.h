// Device-side data layout and kernel launchers of the MI355X WSPR decoder.
//
// HBM layout (all float32 unless noted), sized for thousands of resident
// 2-minute segments (one segment = 45 000 complex samples at 375 sps):
//   iq      I[nseg][kIqStride], Q[nseg][kIqStride]   planar, rows 256-B aligned
//   ps      [nseg][417 bins][kPsTPitch]               |X|^2, bin-major like the reference's
//                                                     ps[512][blocks]: row b = fft-shifted bin 48+b,
//                                                     its time blocks contiguous (pitch 352 floats)
//   cand    DevCand[nseg][200] + npk[nseg]            peak list, strongest first
// Everything a kernel needs besides these is a small constant table uploaded once
// (window, twiddles, sync vector, subtraction low-pass taps).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

namespace wspr {

// Kernel-selection and measurement switches exist in the LAB build only (libwspr_mi355x_lab.so, -DWSPR_LAB: what the
// parity suite and bench.py's kernel-level timings load); in the product library every one of them reads as unset, so
// the product carries no way to pick a different kernel, repeat a stage or fold virtual devices.
#ifdef WSPR_LAB
inline const char* lab_env(const char* name) { return getenv(name); }
#else
inline const char* lab_env(const char*) { return nullptr; }
#endif

constexpr int kMaxSamples = 45000;
constexpr int kIqStride   = 45056;      // 176 * 256
constexpr int kFftSize    = 512;
constexpr int kHop        = 128;
constexpr int kMaxBlocks  = 347;        // 4*floor(45000/512) - 1
constexpr int kPsBin0     = 48;         // first fft-shifted bin kept
constexpr int kPsBins     = 417;        // bins 48..464 (all that any consumer reads)
constexpr int kPsStride   = 432;        // floats per segment of the time-averaged spectrum (psavg)
constexpr int kPsTPitch   = 352;        // floats per (segment, bin) row of the spectrogram: 347 time blocks + padding
                                        // (1408 bytes = 11 x 128: every row starts on a 128-byte line)
constexpr int kSmooth     = 411;        // smoothed-spectrum length
constexpr int kMaxCand    = 200;
constexpr int kNSymD      = 162;
constexpr int kNBitsD     = 81;
constexpr int kSps        = 256;
constexpr int kSigLen     = kNSymD * kSps;   // 41 472 samples of signal
constexpr int kLpfTaps    = 360;
constexpr int kMaxLags    = 43;

struct DevCand {
    float freq;     // Hz relative to 1500 Hz
    float snr;      // dB in 2500 Hz (device log10f)
    float peak;     // normalised smoothed-spectrum value the snr derives from
    int   shift;    // samples
    float drift;    // Hz over the frame
    float sync;
    int   bin;      // index of the peak in the smoothed spectrum (the reference's list order before its sort)
};

// One candidate being refined/demodulated (fine sync, soft symbols)
struct FineState {
    int   seg;
    float freq;         // in: coarse freq  -> after mode 1: refined freq
    float drift;
    int   shift;        // in: coarse shift -> after mode 0: refined shift
    float sync;         // sync after the latest mode-0/1 search
    int   shift_coarse; // kept so that the lag window can be rebuilt
    float freq_coarse;
    int   pad;
};

// One coherent subtraction job
struct SubJob {
    int   seg;
    float f0;
    int   shift;
    float drift;
    unsigned char sym[kNSymD];
    unsigned char pad[2];
};

struct DeviceTables {
    const float*  window;      // [512]  sinf(0.006147931*j)
    const float2* twiddle;     // [256]  exp(-2*pi*i*k/512), float
    const unsigned char* sync; // [162]
    const float*  lpf;         // [360]  normalised sine taps
    const float*  lpf_part;    // [360]  running sums for the edge correction
    float min_snr;             // powf(10, -0.8)
    float floor_snr;           // 0.1 * min_snr
};

// ---- launchers (all asynchronous on `st`) ----------------------------------
// `arith` (wspr_set_arithmetic, read once per call): 0 = WSPR_ARITH_EXACT, the reference's separately rounded
// multiplies and adds; 1 = WSPR_ARITH_CONTRACTED, the fusions clang's -ffp-contract=on makes in wsprd.c.  Launchers of
// kernels without such a site take no `arith`.
void launch_fft_bank(const float* dI, const float* dQ, const int* seg_list, int nseg_active,
                     int samples, float* ps, const DeviceTables& t, hipStream_t st, int arith);
// K1 fused with the time average (one workgroup per segment): ps as above, psavg[seg][kPsStride]
void launch_fft_bank_avg(const float* dI, const float* dQ, const int* seg_list, int nseg_active,
                         int samples, float* ps, float* psavg, const DeviceTables& t, hipStream_t st, int arith);
void launch_calib_copy(const float* src, float* dst, size_t n, hipStream_t st);
void launch_calib_copy16(const float* src, float* dst, size_t n, hipStream_t st, int variant = 0);

// Opt a kernel in to `bytes` of dynamic LDS on the CURRENT device, once per device (a process that drives
// several devices through wspr_set_device reaches every launch site from each of them).
inline void lds_opt_in(const void* kernel, size_t bytes, std::atomic<unsigned>& done) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 31) dev = 0;
    if (done.load(std::memory_order_relaxed) & (1u << dev)) return;
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    done.fetch_or(1u << dev, std::memory_order_relaxed);
}
double launch_calib_valu(float* out, int iters, hipStream_t st);
void launch_calib_read(const uint8_t* raw, size_t bytes_per_seg, int nseg, unsigned* out, hipStream_t st);
// psavg: scratch, nseg * kPsStride floats (time-averaged spectrum per segment)
// K2a alone: psavg[seg][kPsStride] = sum over time blocks of ps, in block order (wsprd.c:556-561)
void launch_time_average(const float* ps, const int* seg_list, int nseg_active, int blocks, float* psavg,
                         hipStream_t st);
// have_avg: psavg was already filled by launch_time_average
void launch_pick_peaks(const float* ps, const int* seg_list, int nseg_active, int blocks, float* psavg,
                       DevCand* cand, int* npk, float* noise_out, float* smspec_out,
                       const DeviceTables& t, hipStream_t st, bool have_avg = false);
// kernel: 0 = the launcher's own choice (by batch size; WSPR_K3_KERNEL in the lab build), 1 = one wave per frequency bin,
// 2 = one lane per (candidate, lag) where the record is full length (a stage hook of the lab build passes 1 or 2)
void launch_coarse_sync(const float* ps, const int* seg_list, int nseg_active, int blocks,
                        DevCand* cand, const int* npk, int maxdrift,
                        const DeviceTables& t, hipStream_t st, int kernel = 0);
// nhyp hypotheses per item, results in sync_out[item][nhyp]:
// mode 0: lags shift_coarse-128 + lagstep*h at freq_coarse
// mode 1: frequencies state.freq + (ifmin+h)*fstep at state.shift
// mode 2: lags state.shift + jitter[h] at state.freq; also soft symbols and their rms;
//         skipped (nothing written) for items whose state.sync <= minsync1
void launch_demod(const float* dI, const float* dQ, int samples, const FineState* items, int nitems,
                  int mode, int nhyp, int lagstep, int ifmin, float fstep, const int* jitter,
                  float minsync1, float* sync_out, unsigned char* sym_out, float* rms_out,
                  const DeviceTables& t, hipStream_t st, int symfac, int arith);
// Tiled fast path for the wide searches.  FineState.pad must hold the index of the item's
// first phasor table in `tabs` (1 table if drift == 0, else 162); list_shared/list_own are the
// item indices without / with drift.  mode 0: nlag lags shift_coarse-128 + lagstep*m;
// mode 2: 43 lags shift-63+3*m (lagstep must be 3).  pw: nitems*nlag*162 float4 of scratch.
void launch_phasor_tables(const FineState* items, int nitems, int mode, float* tabs, hipStream_t st, int arith);
// Lag pruning of the full mode-0 scan (33 lags, step 8; k4_lag_prune.h, launched from k4_demod.hip): a cheap bounded pass names the lags that can still
// win, exact sums are formed for those only.  The caller provides `scratch` (lag_prune_scratch_bytes(nitems) bytes) and
// `counts`, three ints of device memory it has zeroed: [0] exact single-lag evaluations, [1] candidates that fell back
// to the whole scan, [2] candidates pruned; launch_demod_tiled() sets `mask` (per item, bit m = lag m was summed; null
// when it did not prune) for launch_pick_lag().  `audit` (null everywhere but in tools/lagprune_check.hip): nitems x 33 x 7
// floats of device memory that receive the coarse pass' own numbers per (item, lag) -- sync~, eps, totp~, ss~, T~, delta_tab,
// flagged bad (1.0f / 0.0f) -- for the drift-free candidates; see k4_lag_prune.h.
// `drift` (opt-in; the decode pipeline sets it): the drifting candidates are pruned as well: a coarse pass of their own
// (lag_coarse_drift_kernel + lag_coarse_drift_fold_kernel), then the same contender stage (lp_decide) and the same exact
// kernel (lag_exact_kernel<., true>).  `counts` is then EIGHT zeroed ints: [4] exact single-lag evaluations, [5] fallbacks and
// [6] candidates pruned among the drifting ones; their lists follow the drift-free ones in `scratch`, and `audit` receives
// their rows too.  A drifting candidate that falls back takes demod_drift_kernel's whole scan (<., true>: over the fallback
// list).  Off: drifting candidates take the whole scan, mask all ones, counts[4..] and the rest of scratch untouched.
struct LagPrune {
    void* scratch;
    int* counts;
    const unsigned long long* mask;
    float* audit = nullptr;
    bool drift = false;
};
size_t lag_prune_scratch_bytes(int nitems);
void launch_demod_tiled(const float* dI, const float* dQ, int samples, const FineState* items, int nitems,
                        const int* list_shared, int n_shared, const int* list_own, int n_own, int mode,
                        int nlag, int lagstep, float minsync1, const float* tabs, float* pw,
                        float* sync_out, unsigned char* sym_out, float* rms_out,
                        const DeviceTables& t, hipStream_t st, int arith, LagPrune* prune = nullptr);
// mode 1 (5 frequencies) + first ladder rung; see k4_demod.hip.  tabs: n_shared*5 tables,
// pw: n_shared*5*162 float4, scratch_sync: nitems*5 floats.
void launch_freq_scan_and_first_rung(const float* dI, const float* dQ, int samples, FineState* items,
                                     const int* list_shared, int n_shared, const int* list_own, int n_own,
                                     int lagstep, float minsync1, const int* jitter0, float* tabs, float* pw,
                                     float* scratch_sync, float* sync_out, unsigned char* sym_out,
                                     float* rms_out, const DeviceTables& t, hipStream_t st,
                                     const float* pw_lag, int nlag_lag, int arith);
void launch_pick_lag(FineState* items, int nitems, const float* sync_in, int nlag, int lagstep, hipStream_t st,
                     const unsigned long long* mask = nullptr);
void launch_pick_freq(FineState* items, int nitems, const float* sync_in, int nfreq, int ifmin,
                      float fstep, hipStream_t st, int arith);
// The subtraction's low-pass taps and their running sums as DeviceTables holds them (lpf[kLpfTaps], lpf_part[kLpfTaps]),
// computed with the host libm exactly as the reference does, wsprd.c:353-368.  The context uploads these; so does
// tools/subtract_check.hip.
inline void subtract_lpf_tables(float* lpf, float* part) {
    float norm = 0.0f;
    for (int i = 0; i < kLpfTaps; ++i) { lpf[i] = sinf(M_PI * (float)i / (float)(kLpfTaps - 1)); norm = norm + lpf[i]; }
    for (int i = 0; i < kLpfTaps; ++i) lpf[i] = lpf[i] / norm;
    part[0] = 0.0f;
    for (int i = 1; i < kLpfTaps; ++i) part[i] = part[i - 1] + lpf[i];
}
size_t subtract_scratch_floats(int njobs);
void launch_subtract(float* dI, float* dQ, int samples, const SubJob* jobs, int njobs,
                     float* scratch /* subtract_scratch_floats(njobs) */, const DeviceTables& t, hipStream_t st,
                     int arith);
// subtract_signal() of the reference (wsprd.c:263-312): one segment row, symbols in device memory
void launch_subtract_symbolwise(float* dI, float* dQ, int samples, float f0, int shift, float drift,
                                const unsigned char* d_sym, hipStream_t st);
// Device Fano search (K6) for n soft-symbol vectors symbols[offsets[i]*162 ...] (interleaved order, as the
// demodulator writes them); metric0 = the 256-entry "sent 0" branch-metric row.
// One wavefront per vector, 64 tree visits per step (k6_fano_wave.hip): exact return
// code, cycle count and decoded bytes; metric/maxnp only for decoded frames.  ret -2 = the wave's
// pending-visit store overflowed (the caller decodes that vector some other way).  steps may be null.
// scratch: fano_wave_scratch_words(n) words of device memory (the waves' stack slices; their tops live in LDS).
size_t fano_wave_scratch_words(int n);
void launch_fano_wave(const unsigned char* symbols, const int* offsets, int n, const short* metric0,
                      unsigned maxcycles, int* ret, unsigned* cycles, unsigned* metric, unsigned* maxnp,
                      unsigned char* data, unsigned* steps, uint32_t* scratch, hipStream_t st);
// K9, ordered-statistics decoding (k9_osd.hip; the definition in osd.h): one wavefront per vector, vector i = the 162 soft
// symbols at symbols + offsets[i] * 162 (transmission order).  depth 0..3; gen = the 50 generator rows of 7 words
// (osd::pack_generator_row).  Outputs per vector: data[11], dist, nhard, order.
void launch_osd(const unsigned char* symbols, const int* offsets, int n, int depth, const uint32_t* gen,
                unsigned char* data, unsigned* dist, unsigned* nhard, unsigned* order, hipStream_t st);
// K10, noncoherent block detection (k10_blockdemod.hip; the definition in blockdemod.h).  BlockHyp is wspr_block_item of the
// public header: one hypothesis, `shift` with the rung's jitter already added.  Per hypothesis h: sym_out[h][3][162] (block
// sizes 1, 2, 3, transmission order), rms_out[h][3] and sync_out[h], the mode-2 sync of the hypothesis.
struct BlockHyp {
    int32_t seg;
    float freq;
    int32_t shift;
    float drift;
};
void launch_block_demod(const float* dI, const float* dQ, int samples, const BlockHyp* hyps, int nhyp,
                        unsigned char* sym_out, float* rms_out, float* sync_out, const DeviceTables& t, hipStream_t st,
                        int arith);
// K11, the Doppler-spread figure (k11_spread.hip; the definition in spread.h).  A job is a SubJob -- wspr_spread_item of the
// public header has its layout.  ckpt: spread_checkpoint_doubles(n) doubles of scratch, tw: the 2 x 1 024 floats of
// spread::spread_twiddles() in device memory, out: n x 4 words (w50, f50, ratio as floats, valid), 16-byte aligned.
size_t spread_checkpoint_doubles(int n);
void launch_spread(const float* dI, const float* dQ, int samples, const SubJob* jobs, int n, double* ckpt, const float* tw,
                   void* out, hipStream_t st);
// K8, the signal synthesiser (k8_synth.hip; arithmetic in synth_math.h).  SynthTx is wspr_synth_tx of the public header.
struct SynthTx {
    int32_t seg;
    float f0, t0, amp, drift;
    unsigned char symbols[kNSymD];
    unsigned char pad[2];
};
constexpr int kSynthCkptEvery = 64;                       // samples between phase checkpoints, layout [checkpoint][transmission]
size_t synth_checkpoint_doubles(int ntx);                 // phase checkpoints of ntx transmissions
// tx sorted by seg, seg_off[nseg + 1] its offsets per segment (both device memory); ckpt: synth_checkpoint_doubles(ntx)
// doubles, first: ntx ints of scratch.  Rows of kIqStride floats, 16-byte aligned; without `accumulate` the whole row is
// written (columns >= 45000 zero), with it those columns are left alone.
void launch_synth(const SynthTx* tx, int ntx, const int* seg_off, int nseg, long long seg_index0, float sigma,
                  unsigned long long seed, int accumulate, double* ckpt, int* first, float* dI, float* dQ, hipStream_t st);
void launch_synth_phase(const SynthTx* tx, int ntx, double* ckpt, int* first, hipStream_t st);   // launch_synth()'s first half
// K13, the fading channel (k13_fade.hip; the definition in fade.h): launch_synth() with one FadeChannel (fade.h, derived on
// the host by fade_path_setup()) per transmission in device memory.  Everything else as for launch_synth().
struct FadeChannel;
void launch_synth_faded(const SynthTx* tx, const FadeChannel* ch, int ntx, const int* seg_off, int nseg, long long seg_index0,
                        float sigma, unsigned long long seed, int accumulate, double* ckpt, int* first, float* dI, float* dQ,
                        hipStream_t st);
void launch_normalise(float* dI, float* dQ, const int* n_valid, int nseg, int n_total, hipStream_t st);
// resident input rows -> working rows (zero tail); false if the input is not 16-byte friendly
bool launch_load_rows(const float* sI, const float* sQ, size_t stride, int samples, int nseg, float* dI, float* dQ,
                      hipStream_t st);
// Front-end state of one receiver between chunks of its sample stream (all zero at start-up):
// samples into the open decimation block, both integrators per rail, and the integrator values at
// the last 36 decimation instants (what the two combs and the 33-tap FIR still need).
constexpr int kDecimHist = 36;
struct DecimState {
    uint32_t phase;
    uint32_t x1[2], x2[2];
    uint32_t hist[2][kDecimHist];
};
int decimate_blocks(size_t nsamp, bool stateful);
void front_end_constants(float* taps33, int* samples_per_output);   // the FIR taps and R as the kernels use them
// states: null = zero state, whole blocks only; else one DecimState per segment row, read and updated
void launch_decimate(const uint8_t* raw, size_t bytes_per_seg, int nseg, float* dI, float* dQ,
                     int* n_out, int32_t* scratch, hipStream_t st, DecimState* states = nullptr);
// K21, the tunable multi-band front end (k21_tune.hip; the definition in tune.h): nseg rows of bytes_per_seg bytes (raw 16-byte
// aligned, bytes_per_seg a multiple of 16) and nbands (1 .. 16) host steps into nseg * nbands rows of kIqStride floats, row
// s * nbands + b = segment s tuned by steps[b]; the whole row written (zero from tune n_out on); n_out: one device int per
// output row.  scratch: tune_scratch_bytes() bytes.  tune_band_tile(): bands a pass over the raw rows serves.
int tune_band_tile();
size_t tune_scratch_bytes(size_t bytes_per_seg, int nseg, int nbands);
void launch_tune(const uint8_t* raw, size_t bytes_per_seg, int nseg, const uint32_t* steps, int nbands, float* dI, float* dQ,
                 int* n_out, long long* scratch, hipStream_t st);
// K12, the 12 kHz audio front end (k12_audio.hip; the definition in audio_front.h): nseg records of nsamp 16-bit samples
// (row s at pcm + s * pcm_stride; pcm 16-byte aligned, pcm_stride a multiple of 8 and >= nsamp, 0 <= nsamp <= 1 440 000)
// into rows of kIqStride floats, the whole row written (zero from min(ceil(nsamp / 32), 45000) on).
void launch_audio_front(const int16_t* pcm, size_t pcm_stride, int nsamp, int nseg, float* dI, float* dQ, hipStream_t st);
void audio_front_taps(float* gi511, float* gq511);                  // the two tap tables of audio_front.h as floats
// K15, the impulse-noise blanker in front of K12 (k15_blank.hip; the definition in audio_blank.h): nseg records of nsamp
// samples (rows as for K12) into rows of out_stride samples (out 16-byte aligned, out_stride a multiple of 8 and >= nsamp,
// no overlap with the input): columns 0 .. roundup8(nsamp) - 1 written, the rest left alone.  thr16 = 16 .. 4096,
// guard = 0 .. 64.  n_blanked: one device counter per record, ADDED to (the caller zeroes it).
void launch_audio_blank(const int16_t* pcm, size_t pcm_stride, int nsamp, int nseg, int thr16, int guard, int16_t* out,
                        size_t out_stride, int* n_blanked, hipStream_t st);
// K17, the 12 kHz audio scene synthesiser (k17_audio_synth.hip; the definition in audio_synth.h).  tx, seg_off, first as for
// launch_synth(); phase: audio_synth_phase_doubles(ntx) doubles of scratch.  nseg records of nsamp samples (rows as K15's
// output rows: pcm 16-byte aligned, pcm_stride a multiple of 8 and >= nsamp, 0 <= nsamp <= 1 440 000): columns
// 0 .. roundup8(nsamp) - 1 written (from nsamp on zero, or with `accumulate` what they held), the rest left alone.
// n_clipped: one device counter per record, ADDED to (the caller zeroes it).
constexpr int kAudioSynthTile = 2048;                     // samples of a record per workgroup
size_t audio_synth_phase_doubles(int ntx);
void launch_audio_synth(const SynthTx* tx, int ntx, const int* seg_off, int nseg, long long seg_index0, int nsamp, float sigma,
                        unsigned long long seed, int accumulate, double* phase, int* first, int16_t* pcm, size_t pcm_stride,
                        int* n_clipped, hipStream_t st);
// K18, IQ to audio (k18_iq_audio.hip; the definition in iq_audio.h): nseg rows of `samples` samples (0 .. kMaxSamples; rows as
// for K16: 16-byte aligned, stride a multiple of 4 floats and >= samples, nothing at or behind `samples` is read) into nseg
// records of 32 * samples 16-bit samples (rows as K17's: pcm 16-byte aligned, pcm_stride a multiple of 8 and >= 32 * samples):
// columns 0 .. 32 * samples - 1 written, the rest left alone.  gain: finite.  n_clipped: one device counter per record,
// ADDED to (the caller zeroes it).
void launch_iq_audio(const float* dI, const float* dQ, size_t stride, int samples, int nseg, float gain, int16_t* pcm,
                     size_t pcm_stride, int* n_clipped, hipStream_t st);
// K16, the band noise figures of a segment (k16_noise.hip; the definition in noise.h): nseg rows of `samples` samples
// (0 .. kMaxSamples; rows 16-byte aligned, stride a multiple of 4 floats and >= samples; nothing at or behind `samples` is
// read) into nseg records of 32 bytes (noise::Result) at out.  table: noise::kTableFloats floats of noise::noise_tables(),
// w2 its return value; win: validated windows.
namespace noise { struct Windows; struct Result; }
void launch_noise(const float* dI, const float* dQ, int samples, size_t stride, int nseg, const float* table, double w2,
                  const noise::Windows& win, void* out, hipStream_t st);
// K20, the waterfall of a segment (k20_waterfall.hip; the definition in waterfall.h): rows as K16's into nseg images of
// rows_of() x cols_of() bytes (image s at img + s * img_stride; img 16-byte aligned, img_stride a multiple of 16 and >= the
// image; bytes behind the image left alone) and nseg records of 16 bytes (waterfall::Info) at info, which the caller has
// ZEROED.  table, w2: K16's.  p: validated.  levels: the waterfall::kLevels doubles of waterfall::level_table() on the
// device.  floors: K16's records of the same rows on the device (floor mode; queued before on the same stream) or null.
namespace waterfall { struct Params; struct Info; }
void launch_waterfall(const float* dI, const float* dQ, int samples, size_t stride, int nseg, const float* table, double w2,
                      const waterfall::Params& p, const double* levels, const noise::Result* floors, uint8_t* img,
                      size_t img_stride, waterfall::Info* info, hipStream_t st);
// K14, list decoding against known messages (k14_list.hip; the definition in listmatch.h): vector i = the 162 soft symbols at
// symbols + offsets[i] * 162 (transmission order) against the m listed code words.  table: 48 x padded(m) words of four int8
// chips, word-major, zero beyond position 161 and beyond entry m - 1; bias: B of each entry.  ListMatch is wspr_list_match
// of the public header: one per vector.
struct ListMatch {
    int32_t index, score, second, v2;
};
void launch_list_match(const unsigned char* symbols, const int* offsets, int n, const int* table, const int* bias, int m,
                       ListMatch* out, hipStream_t st);
// K19, the decode-quality figures of a spot (k19_spot_quality.hip; the definition in spot_quality.h): job i = the 162 soft
// symbols at symbols + offsets[i] * 162 (transmission order) against the code word of decdata + i * 11.  metric0: row 0 of
// the Fano metric table as 256 shorts (K6w's table); where: 162 bytes, the coder output sent at each transmission position.
// SpotQuality is wspr_spot_quality of the public header: one per job.
struct SpotQuality {
    int32_t nhard, dist, rsum, v2, metric;
};
void launch_spot_quality(const unsigned char* symbols, const int* offsets, const unsigned char* decdata, int n,
                         const short* metric0, const unsigned char* where, SpotQuality* out, hipStream_t st);

}  // namespace wspr
