/* ============================================================================
 * wspr_mi355x.h -- C ABI of libwspr_mi355x.so, the MI355X-native WSPR decoder.
 *
 * Drop-in boundary for Guenael/rtlsdr-wsprd v0.5.6: the library exports the
 * reference decoder's own entry point and spot struct, so rtlsdr_wsprd.c can be
 * linked against it instead of wsprd/wsprd.c.  Plain C
 * types only; device pointers are passed as void*.
 *
 * This header is EVERYTHING libwspr_mi355x.so exports: the reference's symbols, their batched / resident / sharded
 * forms, the front end, the receiver session, device selection and a few observability calls.  Stage-level parity
 * hooks, the per-candidate trace, kernel timings and calibration kernels live in wspr_mi355x_bench.h and exist only
 * in the lab build (libwspr_mi355x_lab.so, the same sources with -DWSPR_LAB), which is what the test suite and
 * bench.py's kernel-level measurements load next to the product.
 *
 * Runtime knobs of the product (environment, read once): WSPR_HOST_THREADS (CPUs this process may count on: a
 * rank's share), WSPR_SLOTS (pipelines per call, default 3), WSPR_BLOCKING_SYNC (how host threads wait: 2 = poll and
 * sleep, default; 1 = runtime blocking events; 0 = spin), WSPR_FANO_DEVICE and WSPR_FANO_FAST (initial values of
 * wspr_set_fano_device_mode() / wspr_set_fano_fast_budget()).  There are no others.
 *
 * Every declaration cites the reference interface it replaces.
 * ==========================================================================*/
#ifndef WSPR_MI355X_H
#define WSPR_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants the caller uses (reference wsprd/wsprd.h:36-41) ------------ */
#define HASHTAB_SIZE       32768
#define HASHTAB_ENTRY_LEN  13
#define LOCTAB_ENTRY_LEN   5
#define FFT_SIZE           512
#define MAX_CANDIDATES     200
#define MAX_UNIQUES        100

/* ---- structs, identical layout (reference wsprd/wsprd.h:44-74) ------------ */
struct decoder_options {            /* 40 bytes, passed BY VALUE */
    int  freq;                      /* dial frequency, Hz */
    char rcall[13];
    char rloc[7];
    int  quickmode;
    int  usehashtable;
    int  npasses;
    int  subtraction;
};

struct cand {                       /* 20 bytes */
    float freq;
    float snr;
    int   shift;
    float drift;
    float sync;
};

struct decoder_results {            /* 80 bytes: the spot record */
    double freq;
    float  sync;
    float  snr;
    float  dt;
    float  drift;
    int    jitter;
    char   message[23];
    char   call[13];
    char   loc[7];
    char   pwr[3];
    int    cycles;
};

/* ---- THE BOUNDARY --------------------------------------------------------- */
/* Replaces wspr_decode(), reference wsprd/wsprd.h:106-111 / wsprd/wsprd.c:416.
 * Same contract: idat/qdat (length `samples`, <= 45000) are overwritten with the
 * residual after coherent subtraction, decodes[0..*n_results) is filled strongest
 * first, returns 0.
 *
 * DIFFERENCE FROM THE REFERENCE -- CHECK THE RETURN VALUE.  The reference's wspr_decode() cannot fail and always
 * returns 0 (wsprd.c:854).  This one returns a NEGATIVE value, with a message on stderr and *n_results = 0, when
 *   -1  no HIP device is usable or a HIP call failed (there is no CPU fallback), or
 *   -2  samples > 45000: the reference sizes its FFT bank from `samples` (wsprd.c:516) and would read beyond the
 *       45 000 samples its callers hold; this library's working rows are 45 000 samples and a longer record is
 *       refused rather than silently cut (rounds 1-3 cut it).
 * The same codes come back from every wspr_decode_batch*() entry point.
 *
 * One call = a batch of one segment on the GPU.  With options.usehashtable the
 * reference's hashtable.txt side effect is kept (read before, written after the decode, wsprd.c:481-494,
 * 842-852); fftw_wisdom.dat is not (there is no FFTW). */
int wspr_decode(float *idat, float *qdat, int samples, struct decoder_options options,
                struct decoder_results *decodes, int *n_results);

/* Batched form of the same call (build-defined): nseg independent
 * segments, planar host buffers idat/qdat[s*seg_stride + i]; results for segment s
 * go to decodes[s*max_results ...], n_results[s]: a segment's unique spots are ranked by SNR first and
 * the strongest max_results are returned (the reference allows 100, its caller holds 50).  Inputs are not
 * modified unless writeback != 0.  With options.usehashtable the hash memory orders the segments
 * (wsprd.c:481-494, 842-852): the result -- spots and hashtable.txt -- is that of nseg reference calls in index
 * order, obtained in parallel (see wspr_decode_batch_hashed() below; rounds 2-4 decoded such a batch one segment at a
 * time).  Calls with the option are ordered as they enter the library (each reads the file the previous one wrote);
 * a call decodes its first round ahead of its turn, so several may be in flight on different lanes. */
int wspr_decode_batch(float *idat, float *qdat, int nseg, int samples, size_t seg_stride,
                      struct decoder_options options, struct decoder_results *decodes,
                      int max_results, int *n_results, int writeback);

/* usehashtable on a batch, the general form.  The reference reads hashtable.txt before and writes it after
 * every decode (wsprd.c:481-494, 842-852), so what a type-3 "<call>" message resolves to (wsprd_utils.c:296-300)
 * depends on the ORDER of the segments.  wspr_decode_batch*() with options.usehashtable decodes the batch in parallel all
 * the same: each segment logs its hash stores and look-ups, the logs are checked in index order, and only the segments
 * whose look-ups would have seen something else are decoded again, to the fixed point -- same spots and same
 * hashtable.txt as nseg reference calls in index order.  This entry adds what a job sharded over several processes /
 * GPUs needs: the call's segments are global indices seg_index0 .. seg_index0 + nseg - 1, `prior` holds the stores of
 * the other shards (any order; those of earlier segments take part), and the call's own stores come back in
 * stores_out[0 .. *n_stores) (segment order).  cap too small: -3 with *n_stores = the capacity needed, nothing written to
 * hashtable.txt, the result arrays filled; the same call again with WSPR_HASH_REVISIT, the same prior and a buffer of
 * that size completes it (nothing is decoded twice).  *n_redecoded: segments decoded more than once.
 * Protocol for R shards (rtlsdr-wsprd_amd/dist.py decode_hashed_sharded): every shard calls with no prior and
 * WSPR_HASH_KEEP_FILE; the stores are exchanged; a shard whose predecessors' stores changed calls again with
 * WSPR_HASH_REVISIT (same buffers and result arrays: only the affected segments are decoded again); when no store list
 * changes any more, ONE process calls wspr_hash_commit() with all stores in segment order.
 * WSPR_HASH_REVISIT is refused (negative return, results untouched) unless the calling thread's previous hashed call
 * completed over the same segments, samples and slot layout and the library's working buffers have not been released
 * since.  Calls with WSPR_HASH_KEEP_FILE or a prior are ordered by a process-wide turn which they keep while they decode:
 * shards driven from several threads of one process run one after the other; give every shard its own process (dist.py). */
typedef struct wspr_hash_op {
    int32_t seg;                /* global segment index */
    int32_t slot;               /* 0 .. HASHTAB_SIZE - 1 */
    int32_t kind;               /* 1 = type-1 store (call + locator), 2 = type-2 store (call only) */
    char    call[13];
    char    grid[5];
    char    pad[2];
} wspr_hash_op;
#define WSPR_HASH_KEEP_FILE 1   /* do not write hashtable.txt (a shard of a larger job) */
#define WSPR_HASH_REVISIT   2   /* the calling thread's previous hashed call once more, under a new `prior` */
int wspr_decode_batch_hashed(float *idat, float *qdat, int nseg, int samples, size_t seg_stride,
                             struct decoder_options options, struct decoder_results *decodes, int max_results,
                             int *n_results, int writeback, int seg_index0, const wspr_hash_op *prior, int n_prior,
                             int flags, wspr_hash_op *stores_out, int cap, int *n_stores, int *n_redecoded);
/* hashtable.txt := hashtable.txt + stores, applied in the order given (the job's stores in segment order). */
int wspr_hash_commit(const wspr_hash_op *stores, int n);

/* Host buffers at speed.  wspr_decode() / wspr_decode_batch() take the caller's HOST memory as the reference does
 * (wsprd.h:106-111; call sites rtlsdr_wsprd.c:316, :689).  Pageable memory is gathered through pinned chunks of the
 * library (host memcpy + DMA, chunk k+1 gathered under the DMA of chunk k); PINNED memory goes to the device as a plain
 * DMA with no host work.  The reference's callers allocate their I/Q buffers once (rtlsdr_wsprd.c:78-90, 331-336):
 * pin them once with this (hipHostRegister; no HIP headers needed on the caller's side) and unpin before free().
 * Returns 0 on success (also when the range is pinned already), -1 otherwise. */
int wspr_pin_host_buffer(void *p, size_t bytes);
int wspr_unpin_host_buffer(void *p);

/* Same, with the IQ already resident in HBM (device pointers, same layout).
 * The input is copied to a working buffer and left untouched.  This is the
 * entry point bench.py times.
 * Stream contract (every entry point that takes device pointers): the library works on streams of its own
 * and does not know the caller's; the buffers must be COMPLETE when the call is made (synchronise the stream
 * or event that produces them first), and everything the call writes is complete when it returns. */
int wspr_decode_batch_device(const void *d_idat, const void *d_qdat, int nseg, int samples,
                             size_t seg_stride, struct decoder_options options,
                             struct decoder_results *decodes, int max_results, int *n_results);

/* Node-level form (SURVEY §8e "one host process, 8 devices"): the nseg host segments are split into contiguous
 * blocks by wspr_shard_range() over `ndevices` HIP devices (0 = every visible device; more than are visible is an
 * error), one host thread per device, each block decoded by wspr_decode_batch() on its device straight into the
 * caller's arrays.  The segments are independent (hashtab/loctab are locals of wspr_decode, wsprd.c:478-479), so no
 * collective is involved and the result equals wspr_decode_batch() on one device.  The host's CPUs are shared
 * between the devices (pools of contexts created from then on are sized for a 1/ndevices share).  With
 * options.usehashtable the segments are ordered and the call is wspr_decode_batch() on the current device. */
int wspr_decode_batch_node(float *idat, float *qdat, int nseg, int samples, size_t seg_stride,
                           struct decoder_options options, struct decoder_results *decodes,
                           int max_results, int *n_results, int ndevices);
/* The same for IQ already RESIDENT on device `src_device` (rows of seg_stride floats, e.g. what
 * wspr_decimate_u8_batch_device() left there): every other device pulls its wspr_shard_range() block over xGMI
 * with a peer copy (the scatter of 360 000 B per segment for real inputs, here inside one process),
 * decodes it on its own host thread and writes its spots into the caller's arrays.  The stream contract of
 * wspr_decode_batch_device() applies to d_idat / d_qdat.
 * Failure semantics of both node-level calls: ndevices larger than the visible devices, or a source device that does not
 * exist: -1 before anything runs.  Refused peer access is NOT a failure: the block then travels source device -> pinned
 * host memory -> target device (a line on stderr says so).  A shard that fails (its device cannot be selected, its copy
 * or its decode fails) fails the WHOLE call: the return value is negative and every n_results[] is 0 -- the other shards'
 * spots are not reported, so that a caller never mistakes a partial result for the slot's spots; the call can be
 * repeated (with fewer devices) as it stands, the inputs are untouched. */
int wspr_decode_batch_node_device(const void *d_idat, const void *d_qdat, int src_device, int nseg, int samples,
                                  size_t seg_stride, struct decoder_options options,
                                  struct decoder_results *decodes, int max_results, int *n_results, int ndevices);
/* The partitioning rule of the node-level call and of the multi-process driver (rtlsdr-wsprd_amd/dist.py
 * shard_range): shard k of n owns segments [*lo, *hi), the first nseg % n shards one segment more. */
void wspr_shard_range(int nseg, int shard, int nshards, int *lo, int *hi);

/* Front end, replaces the static rtlsdr_callback() + decoder() normalisation
 * (reference rtlsdr_wsprd.c:126-244, :284-305).  iq = interleaved unsigned 8-bit
 * I/Q at 2.4 Msps, nbytes a multiple of 8, decimator state zero at the start.
 * Writes min(floor(nbytes/2/6401), 45000) samples to I/Q (capacity 45000 each;
 * the rest is zero-filled when normalise != 0, which also scales to peak 0.5). */
int wspr_decimate_u8(const uint8_t *iq, size_t nbytes, float *I, float *Q, uint32_t *n_out,
                     int normalise);
/* nseg raw segments resident in HBM -> planar float IQ in HBM (rows of
 * wspr_iq_stride() floats), normalised, ready for wspr_decode_batch_device.  d_raw and bytes_per_seg must be
 * multiples of 16 (rows are read with aligned 16-byte loads); -1 otherwise. */
int wspr_decimate_u8_batch_device(const void *d_raw, size_t bytes_per_seg, int nseg,
                                  void *d_idat, void *d_qdat, int normalise);

/* Streaming form of the front end.  The reference keeps the decimator state in `static` variables
 * of rtlsdr_callback() (rtlsdr_wsprd.c:135-160: integrators, comb delay lines, FIR line, decimation
 * counter), so it runs on across callbacks and across 2-minute segments; this state object carries
 * exactly that between calls.  All-zero = the receiver at start-up.  Fields: samples into the open
 * decimation block, integrators I1/I2 per rail (I, Q), and the second integrator at the last 36
 * decimation instants (from which both combs and the FIR history follow). */
typedef struct wspr_decim_state {
    uint32_t phase;
    uint32_t x1[2], x2[2];
    uint32_t hist[2][36];
} wspr_decim_state;
void wspr_decim_stream_reset(wspr_decim_state *st);
/* One callback's worth of samples (rtlsdr_wsprd.c:126: `buf`, `len`; nbytes a multiple of 16, the
 * mixer phase restarts with every call as in the reference): appends the new outputs to I/Q at
 * index `fill`, never beyond `capacity` (rtlsdr_wsprd.c:236-242), and updates the state.  Any
 * chunking of a stream gives the same outputs as one call over the whole of it. */
int wspr_decimate_u8_stream(wspr_decim_state *st, const uint8_t *iq, size_t nbytes, float *I, float *Q,
                            uint32_t fill, uint32_t capacity, uint32_t *new_fill);
/* Many receivers at once, resident data: row s of d_raw is the next bytes_per_seg bytes of receiver
 * s, d_states[s] its state (device memory, read and updated), outputs start at column 0 of row s of
 * d_idat/d_qdat (row stride wspr_iq_stride()), n_out[s] (host) = outputs produced. */
int wspr_decimate_u8_batch_device_stateful(const void *d_raw, size_t bytes_per_seg, int nseg, void *d_states,
                                           void *d_idat, void *d_qdat, int *n_out);
size_t wspr_iq_stride(void);        /* floats per segment row of device IQ buffers */
/* The front end's constants as the kernels use them: the 33 compensation-FIR taps (zCoef, reference
 * rtlsdr_wsprd.c:142-152) and the input samples per output (DOWNSAMPLING + 1 = 6401, :41, :198-202). */
void wspr_front_end_constants(float *taps33, int *samples_per_output);

/* ---- 12 kHz audio front end (K12) ---------------------------------------------------------------------------
 * What a receiver farm records (KiwiSDR / wsprdaemon style): one two-minute slot per file, 12 000 Hz 16-bit mono audio
 * with the WSPR band centred on 1 500 Hz.  The reference has no audio input; the definition is this project's own
 * (rtlsdr-wsprd_amd/csrc/kernels/audio_front.h; tests/helpers/audio_check.c is the contract in serial C):
 *   x[n] = pcm[n] * 2^-15, zero outside [0, nsamp);  n_out = min(ceil(nsamp / 32), 45000);  for m < n_out
 *   I[m] = the chain acc = fmaf(gI[k], x[32 m + k], acc) over k = -255 .. 255 from +0.0f, Q[m] the same with gQ,
 * 511 Kaiser-windowed-sinc taps per rail with the 1 500 Hz mixer folded in; every other column of the row is 0.0f.
 * Audio at 1500 + f Hz arrives at +f; output m is centred on input sample 32 m, so the front end adds no delay.
 * wspr_set_arithmetic() does not touch it. */
#define WSPR_AUDIO_RATE        12000
#define WSPR_AUDIO_MAX_SAMPLES 1440000
/* nseg rows of PCM resident in HBM (row s at d_pcm + s*pcm_stride samples) -> planar IQ rows, ready for
 * wspr_decode_batch_device().  d_pcm 16-byte aligned, pcm_stride a multiple of 8 and >= nsamp.  Stream contract as above.
 * normalise != 0: afterwards the receiver's scaling to a peak of 0.5, as wspr_decimate_u8_batch_device() does.
 * Returns 0; -1 with a line on stderr and NOTHING WRITTEN for: no device, nseg < 0, nsamp < 0, misalignment, a stride too
 * small; -2 for nsamp > 1 440 000 (a longer record is refused, not cut).  nseg == 0 does nothing, nsamp == 0 writes zero
 * rows.  Takes a turn on the calling thread's lane. */
int wspr_audio_batch_device(const void *d_pcm, size_t pcm_stride, int nsamp, int nseg,
                            void *d_idat, void *d_qdat, int normalise);
/* one record from host memory into host rows of 45000 floats (through the device; no CPU fallback); its device scratch
 * belongs to the lane's context and is returned by wspr_release_buffers() */
int wspr_audio_to_iq(const int16_t *pcm, size_t nsamp, float *I, float *Q, uint32_t *n_out, int normalise);
/* The two tables of 511 taps (index k + 255) and the input samples per output (32) as the kernel uses them. */
void wspr_audio_constants(float *taps_i511, float *taps_q511, int *samples_per_output /* 32 */);

/* ---- impulse-noise blanker in front of the audio front end (K15), opt-in ----------------------------------------
 * Lightning static, electric fences and switching supplies put short, huge spikes into the 12 kHz audio; the 511 taps of
 * K12 smear each over 43 ms of the IQ.  The blanker acts on the wide-band samples, before that filter.  All integer
 * (rtlsdr-wsprd_amd/csrc/kernels/audio_blank.h; tests/helpers/blank_check.c is the contract in serial C):
 *   a[n] = |pcm[n]| (-32768 gives 32768).  Block b = samples 8192 b .. min(8192 (b + 1), nsamp) - 1 (one WSPR symbol).
 *   L_b  = the lower median of the block's a[]: rank (count - 1) / 2 of its own samples inside the record.
 *   out[n] = 0 if L_b > 0 and some n' in [max(0, n - guard), min(nsamp - 1, n + guard)] has 16 a[n'] > thr16 L_b (strict),
 *   else pcm[n]; b is the block of n, and a neighbour n' in the next or the previous block is judged by L_b as well.
 *   A block with L_b == 0 (digital silence) is copied.  thr16 = 16 .. 4096 (sixteenths of the level), guard = 0 .. 64.
 * n_blanked[s] = the samples of record s for which the condition held.  thr16 = 4096 blanks nothing unless a sample is
 * 256 times the level; (96, 4) is what the figures in the README were measured with.
 * The settings are arguments, not state: wspr_audio_batch_device(), wspr_audio_to_iq() and every decode call are
 * untouched by these calls.
 *
 * K15 alone: nseg PCM rows in HBM -> nseg blanked PCM rows in HBM (row s at d_out + s*out_stride samples).  d_pcm, pcm_stride
 * as for wspr_audio_batch_device(); d_out 16-byte aligned, out_stride a multiple of 8 and >= nsamp.  Columns
 * 0 .. roundup8(nsamp) - 1 of an output row are written (zero from nsamp on), the columns behind are left alone.
 * Returns 0; -1 with a line on stderr and NOTHING WRITTEN (n_blanked included) for: no device, nseg < 0, nsamp < 0,
 * misalignment, a stride that is no multiple of 8 or is too small, thr16 outside 16 .. 4096, guard outside 0 .. 64, output
 * rows that overlap the input rows (in place is a race: a neighbouring block would read blanked samples); -2 for
 * nsamp > 1 440 000.  nseg == 0 does nothing, nsamp == 0 writes no sample (n_blanked: zeros).  Stream contract and lane
 * turn as wspr_audio_batch_device(). */
int wspr_audio_blank_batch_device(const void *d_pcm, size_t pcm_stride, int nsamp, int nseg, int thr16, int guard,
                                  void *d_out, size_t out_stride, int *n_blanked /* host, nseg, may be NULL */);
/* K15 then K12: what wspr_audio_batch_device() does, on blanked samples; refusals as above (nsamp == 0 writes zero rows).
 * The blanked samples pass through scratch rows of the lane's context, at most 128 records (369 MB) at a time however large
 * nseg is; wspr_release_buffers() returns them. */
int wspr_audio_blanked_batch_device(const void *d_pcm, size_t pcm_stride, int nsamp, int nseg, int thr16, int guard,
                                    void *d_idat, void *d_qdat, int normalise, int *n_blanked /* host, nseg, may be NULL */);
/* one record from host memory, as wspr_audio_to_iq(); n_blanked: one int, may be NULL */
int wspr_audio_to_iq_blanked(const int16_t *pcm, size_t nsamp, int thr16, int guard, float *I, float *Q,
                             uint32_t *n_out, int normalise, int *n_blanked);

/* ---- band noise figures per segment (K16) --------------------------------------------------------------------------
 * What a receiver farm logs per two-minute slot and band besides the spots (wsprdaemon-style noise graphs): an "RMS" figure
 * taken in the gaps before and after the transmissions, and an "FFT" figure, the mean of the quietest 30 % of the averaged
 * spectrum.  The reference has no such output (its noise_level, wsprd.c:590-616, is internal, taken on a smoothed +-150 Hz
 * spectrum, and only enters the SNR), so the definition is this library's own (rtlsdr-wsprd_amd/csrc/kernels/noise.h;
 * tests/helpers/noise_check.c is its serial form, and the kernel equals it bit for bit).
 * For one row of np samples (0 .. 45 000) of I and Q at 375 samples per second:
 *   guard     if any I[k] or Q[k], k < np, has exponent bits 0xff (NaN, +Inf, -Inf; an integer test on the bit pattern), every
 *             float of the record is 0 and flags = WSPR_NOISE_NONFINITE alone (nframes is still reported).
 *   gaps      block b = samples 16b .. 16b+15 (42.7 ms, the stand-in for sox's 50 ms trough window);  p[b] = (float)(S / 16.0),
 *             S the double sum, in sample order from 0.0, of (double)I*(double)I + (double)Q*(double)Q, unfused.  A window is
 *             a block range [b0, b1), 0 <= b0 <= b1 <= 2812, clipped to the blocks wholly inside [0, np).  mean = (float)(the
 *             double sum of (double)p[b] in rising b / the block count);  trough = the minimum p[b] ("if (p < m) m = p" from
 *             the first block).  An empty window (after clipping as well) gives 0 for both and leaves its flag bit clear.
 *             The two windows are arguments, not state.  wspr_noise_default_windows(): blocks 6 .. 41 (0.26 - 1.79 s) and
 *             2672 .. 2789 (114.0 - 119.0 s) -- wsprdaemon's 0.25 - 0.75 s and 113 - 118 s moved by one second, because in
 *             this library's rows a transmission with dt = 0 starts at 2.0 s (wspr_selftest(): dt = t0 - 2.0), not at 1.0 s.
 *   spectrum  frames of 512 samples at hop 256: nframes = np >= 512 ? (np - 512)/256 + 1 : 0 (174 for a full row).  Window
 *             w[n] = (float)(0.5 - 0.5*cos(2 pi n/512)), twiddles (float)cos, (float)(-sin) of 2 pi m/512, from the host libm
 *             in double.  x = (I*w, Q*w) as float products; 512-point complex float32 radix-2 decimation-in-frequency
 *             transform, nine stages with the butterfly of the Doppler-spread figure above, no fused multiply-add.
 *             P_f[j] = re*re + im*im in float, separately rounded; signed bin j = -256 .. 255 lies at j * 375/512 Hz.
 *             A[j] = the double sum of (double)P_f[j] over the frames IN THIS ORDER: four partial sums S_c[j], c = 0 .. 3, over
 *             the frames f = c, c+4, c+8, ... in rising f from 0.0, then A[j] = ((S_0[j] + S_1[j]) + S_2[j]) + S_3[j].
 *             a[j] = (float)(A[j] / (double)nframes / W2), W2 = the double sum of (double)w[n]*(double)w[n] in rising n: white
 *             noise of per-rail variance s^2 gives E a[j] = 2 s^2, the scale of the gap figure.
 *             The 443 bins j = -221 .. 221 (+-161.9 Hz: 1338 .. 1662 Hz of the audio world) are ranked by their uint32 bit
 *             pattern (finite and >= +0: the numeric order), ties to the lower j.  fft_floor = (float)(the double sum of the
 *             132 lowest in rank order / 132.0), the quietest 30 %; fft_p30 = the value of rank 132.  nframes == 0 gives 0
 *             for both and leaves the flag bit clear.
 *   flags     bit 0 pre window used, bit 1 post window used, bit 2 spectrum used, bit 3 WSPR_NOISE_NONFINITE.
 * UNITS.  All powers are linear, per complex sample, relative to the row's own scale; dB is 10*log10() on the caller's side.
 * THE FIGURES ARE UNCALIBRATED, and meaningless in absolute terms on a row that was normalised to a peak of 0.5: noise
 * logging wants the normalise = 0 rows of wspr_audio_batch_device() / wspr_decimate_u8_batch_device().
 * wspr_set_arithmetic() does not touch this stage, and no decode call runs it.
 * What to expect: on white noise the gap means are unbiased (2 s^2); fft_floor, the mean of the lowest 30 % of 443 averaged
 * bins, reads 0.911 of 2 s^2 (-0.41 dB) with a row-to-row standard deviation of 0.0061, and fft_p30 0.957 +- 0.0062
 * (MEASURED on 2 048 rows of the synthesiser's noise on an MI355X, profiles/noise_figure.json; 0.912 +- 0.0059 on 64 rows of
 * numpy's noise through the serial checker): an order-statistics bias of the estimator, not of the band.  The troughs read
 * 0.55 +- 0.08 (36 blocks) and 0.48 +- 0.06 (118 blocks) of 2 s^2: the minimum of that many block powers.  Ten strong
 * signals in the band (+0 .. +9 dB) raise fft_floor by 0.47 dB; stations that start up to a second early fill the pre window
 * (pre_mean +10.8 dB in that scene) while its trough moves by 0.05 dB in the median.
 *
 * wspr_noise_batch_device(): nseg rows resident on the device (row s at d_idat + s*seg_stride floats; rows 16-byte aligned,
 * seg_stride a multiple of 4 and >= samples; nothing at or behind `samples` is read) -> out[0 .. nseg) in HOST memory.
 * w == NULL takes the default windows.  Returns 0; -1 with a line on stderr and NOTHING WRITTEN for: no device, nseg < 0 or
 * samples < 0, rows that are not 16-byte aligned or a stride that is no multiple of 4 floats, seg_stride < samples, a window
 * outside 0 <= b0 <= b1 <= 2812; -2 (nothing written) for samples > 45000.  nseg == 0 does nothing; samples == 0 writes
 * records of zeros with flags = 0.  Stream contract, lane turn and scratch ownership as wspr_audio_batch_device(); the
 * scratch (32 bytes per segment, one table of 4 KB) is returned by wspr_release_buffers().
 * wspr_noise(): one row from host memory (any alignment), otherwise the same.
 * (In C the record is `struct wspr_noise`: the tag shares its name with the one-row call.) */
#define WSPR_NOISE_PRE_USED   1
#define WSPR_NOISE_POST_USED  2
#define WSPR_NOISE_FFT_USED   4
#define WSPR_NOISE_NONFINITE  8
typedef struct { int32_t pre_b0, pre_b1, post_b0, post_b1; } wspr_noise_windows;
struct wspr_noise {                 /* 32 bytes */
    float   pre_mean, pre_trough, post_mean, post_trough, fft_floor, fft_p30;
    int32_t nframes, flags;
};
void wspr_noise_default_windows(wspr_noise_windows *w);
int wspr_noise_batch_device(const void *d_idat, const void *d_qdat, int nseg, int samples, size_t seg_stride,
                            const wspr_noise_windows *w /* NULL = default */, struct wspr_noise *out /* host, nseg */);
int wspr_noise(const float *I, const float *Q, int samples, const wspr_noise_windows *w, struct wspr_noise *out);

/* ---- signal synthesiser (K8) ------------------------------------------------------------------------------
 * The reference's self-test generator (decoderSelfTest() / whiteGaussianNoise(), rtlsdr_wsprd.c:706-760) for batches
 * of scenes resident in HBM: from "symbols, frequency, time, level" to the IQ rows wspr_decode_batch_device() takes,
 * reproducible sample for sample by a CPU (tests/helpers/synth_check.cpp is the contract in serial C).
 *
 * Per output sample x of a rail, in this order:
 *   1. x = 0, or the row's present value with WSPR_SYNTH_ACCUMULATE.
 *   2. If noise_sigma > 0: x = (float)((double)x + (double)n), n a float32 N(0, noise_sigma^2) draw that is a pure
 *      function of (seed, seg_index0 + seg, sample index, rail): Philox-4x32-10 keyed by the seed, counter = (sample,
 *      0, segment), Box-Muller with I = r cos(theta), Q = r sin(theta).  No state is carried between samples, so a
 *      segment's noise does not depend on how a job is split into calls, batches or ranks.
 *   3. For each transmission of that segment IN LIST ORDER: x = (float)((double)x + (double)amp * cos(phi)) (I rail;
 *      sin for Q) -- for one transmission over zero or over a float noise sample the reference's statement :756-757.
 * phi is the reference's serial recurrence: phi = 0.0, then for symbol i, sample j: use phi, then phi += dphi_i, with
 *   dphi_i = 2.0 * M_PI * dt * ((f0 + fd_i) + ((double)symbols[i] - 1.5) * df),  df = 375.0/256.0,  dt = 1/375.0,
 *   fd_i = (drift/2.0) * ((double)i - 81.0) / 81.0      -- all double, in that order; drift == 0 is :753 exactly.
 * The recurrence is run as written (41 472 dependent double adds per transmission), not replaced by a prefix sum.
 * Output index = floor(t0/dt) (double, once per transmission) + 256*i + j; samples outside [0, 45000) are dropped, so
 * a frame may hang off either end of the row (the reference's index, :755, has no such guard).
 * sin/cos of phi are a fixed sequence of IEEE double operations without fused multiply-add (fdlibm's reduction and
 * kernels, rtlsdr-wsprd_amd/csrc/kernels/synth_math.h), the same on the device and on a CPU: they are WITHIN ONE
 * DOUBLE ULP OF glibc's sin/cos, NOT glibc's -- about 3 % of the double values differ in the last bit; no float32
 * sample of the scenes of tests/test_synth_checker.py does.  wspr_set_arithmetic() does not touch the synthesiser. */
typedef struct wspr_synth_tx {      /* one transmission of a scene, 184 bytes */
    int32_t seg;                    /* output row, 0 .. nseg-1; the list is sorted by seg (non-decreasing) */
    float   f0;                     /* Hz from band centre, centre of the four tones (rtlsdr_wsprd.c:743) */
    float   t0;                     /* s, start of symbol 0 (:744) */
    float   amp;                    /* linear amplitude (:745) */
    float   drift;                  /* Hz over the transmission, the decoder's own model (wsprd.c:156, 343); 0 = the reference generator */
    unsigned char symbols[162];     /* channel symbols 0..3, e.g. from get_wspr_channel_symbols() */
    unsigned char pad[2];
} wspr_synth_tx;
#define WSPR_SYNTH_ACCUMULATE 1     /* add to what the rows hold instead of starting from zero */
#define WSPR_SYNTH_NORMALISE  2     /* afterwards the receiver's scaling to a peak of 0.5 (rtlsdr_wsprd.c:290-305) */
/* d_idat / d_qdat: nseg device rows of wspr_iq_stride() floats, 16-byte aligned, exactly what
 * wspr_decode_batch_device() takes (stream contract above: complete on return).  Without WSPR_SYNTH_ACCUMULATE the whole
 * row is written (columns from 45000 on are zero); with it those columns are left alone.  Returns 0; -1 with a line on
 * stderr and NOTHING WRITTEN for: no device, a symbol > 3, seg outside the batch, an unsorted list, negative counts, a
 * non-finite f0 / t0 / amp / drift / noise_sigma, an unknown flag bit, misaligned rows, or |f0| + |drift|/2 > 1000 Hz
 * (the range of the phase reduction; the band is +-187.5 Hz wide).  Takes a turn on the calling thread's lane; its
 * scratch (the list, 5 184 B of phase checkpoints per transmission) belongs to the lane's context and is returned by
 * wspr_release_buffers(). */
int wspr_synth_batch_device(const wspr_synth_tx *tx, int ntx, int nseg, int seg_index0,
                            float noise_sigma, uint64_t seed, int flags, void *d_idat, void *d_qdat);
/* One segment into host rows of 45000 floats (read first with WSPR_SYNTH_ACCUMULATE), seg_index0 = 0: row 0 of the
 * batch call. */
int wspr_synth(const wspr_synth_tx *tx, int ntx, float noise_sigma, uint64_t seed, int flags,
               float *I, float *Q);
/* The reference's `-t` as one call (decoderSelfTest(), rtlsdr_wsprd.c:729-789): "K1JT FN20QI 20" at 50 Hz, 2.0 s,
 * amplitude 1, noise 0.02 (seed 1), generated and decoded on the device.  Returns 1 / 0 by the rule of :782-788
 * (negative: no usable device) and hands back the first spot (first may be NULL). */
int wspr_selftest(struct decoder_options options, struct decoder_results *first);

/* ---- fading channel of the synthesiser (K13) ----------------------------------------------------------------
 * Opt-in: wspr_synth_batch_device() / wspr_synth() with an HF channel per transmission, under the same contract (a CPU
 * reproduces every sample; tests/helpers/fade_check.cpp is the serial form, rtlsdr-wsprd_amd/csrc/kernels/fade.h the
 * shared arithmetic).  A channel is up to two paths, each with a linear gain, a Doppler shift (Hz) and a Doppler spread
 * sigma (Hz).  NO PATH DELAY IS MODELLED: differential delays on HF are 0.5 - 2 ms, so the coherence bandwidth is
 * hundreds of Hz against a 6 Hz signal; a delay is then a constant phase, which the random gain absorbs.
 *
 * The draws of a transmission are identified by S = seg_index0 + seg (the global segment), q = its ordinal among that
 * segment's transmissions in list order (0-based), the path p and its own sample index n = 0 .. 41 471 -- so a
 * realisation does not depend on how a job is split into calls, batches or ranks.
 *
 * A path is one of three kinds:
 *   skipped   gain == 0: it adds nothing.
 *   specular  sigma == 0: G_p[n] = (gain, 0).
 *   diffuse   sigma > 0.  All in double, unfused, in this order:
 *               s    = 375.0 / ((2.0*1.4142135623730951*3.14159265358979323846) * (double)sigma)
 *                      -- the Gaussian pulse's standard deviation in samples;
 *               L    = (int)s -- the spacing of the white impulses (sigma <= 10 gives L >= 4 and 1 <= s/L < 1.25);
 *               beta = 1.0/(2.0*s*s);     c = (double)gain / sqrt(2.0*(s*1.7724538509055159)/(double)L);
 *               W[k] = a complex float32 draw of unit variance per rail: Philox-4x32-10 keyed by the seed, counter =
 *                      (k + 16, 1 + 2q + p, S low, S high) -- the noise uses counter word 1 = 0, so the two never
 *                      collide -- through exactly the Box-Muller of the noise at sigma 1;
 *               with kc = n / L:  sum = 0.0;  for k = kc-7 .. kc+8 in rising k, d = n - k*L (int):
 *                      sum += (double)W[k] * exp(-((double)d*(double)d)*beta), each rail separately;  G_p[n] = c * sum.
 *             Sixteen terms: the nearest dropped impulse is at least 5.6 s away (weight below 2e-7), and the spectral
 *             images of the impulse train lie below exp(-2 pi^2) = 3e-9 in amplitude.  exp is synth_exp() of
 *             synth_math.h: reduction by ln 2 in two pieces, the Taylor polynomial to degree 12, 2^k through the exponent
 *             bits; a fixed sequence of IEEE double operations on [-40, 0] (here the argument is >= -32), within 2^-40
 *             of exp (measured: profiles/fade_channel.json), no maths library.
 *   shift     either kind: if shift != 0, G_p[n] is rotated by the synthesiser's (ss, cc) = sincos(w*(double)n), w =
 *             2.0*3.14159265358979323846*(1/375.0)*(double)shift:  (re*cc - im*ss, re*ss + im*cc).
 * G[n] = (0.0, 0.0), then + G_0[n], then + G_1[n] (skipped paths left out).  With (sn, cs) the synthesiser's sine and cosine
 * of phi, step 3 of the synthesiser's contract above becomes
 *   x_I = (float)((double)x_I + amp*(cs*G.re - sn*G.im));     x_Q = (float)((double)x_Q + amp*(sn*G.re + cs*G.im)).
 * Steps 1 and 2, the list order, the phase recurrence and the index rule are unchanged.  The channel {(1,0,0),(0,0,0)}
 * gives the unfaded samples bit for bit.
 * A diffuse path's Doppler spectrum is Gaussian with standard deviation sigma (its 2 sigma is what Watterson-model
 * tables call the Doppler spread) and E|G_p|^2 = gain^2: one diffuse path is Rayleigh fading, a specular plus a diffuse
 * one Rician. */
typedef struct wspr_synth_path    { float gain, shift, sigma; } wspr_synth_path;      /* linear, Hz, Hz */
typedef struct wspr_synth_channel { wspr_synth_path path[2]; } wspr_synth_channel;    /* 24 bytes, one per transmission */
/* wspr_synth_batch_device() with ch[t] the channel of tx[t]; ch == NULL is the unfaded call.  Flags, rows, stream contract,
 * lane turn and scratch ownership (64 B more per transmission) are those of wspr_synth_batch_device().  Returns 0; -1
 * with a line on stderr and NOTHING WRITTEN for everything that call refuses and for a non-finite gain, shift or sigma,
 * a sigma that is neither 0 nor within 0.001 .. 10 Hz, or |shift| > 100 Hz. */
int wspr_synth_faded_batch_device(const wspr_synth_tx *tx, const wspr_synth_channel *ch, int ntx, int nseg,
                                  int seg_index0, float noise_sigma, uint64_t seed, int flags,
                                  void *d_idat, void *d_qdat);
/* One segment into host rows of 45000 floats, seg_index0 = 0: row 0 of the batch call (as wspr_synth()). */
int wspr_synth_faded(const wspr_synth_tx *tx, const wspr_synth_channel *ch, int ntx, float noise_sigma,
                     uint64_t seed, int flags, float *I, float *Q);

/* ---- 12 kHz audio scene synthesiser (K17) ---------------------------------------------------------------------
 * The synthesiser above for the AUDIO path: from "symbols, frequency, time, level, drift" to the 16-bit records
 * wspr_audio_batch_device() and wspr_audio_blank*_batch_device() take -- 12 000 samples per second, the band centred on
 * 1 500 Hz, 8 192 samples per symbol.  It is also the transmit side: get_wspr_channel_symbols(), wspr_synth_audio() and
 * wspr_write_wav_file() turn a message into the audio a transmitter plays.  Under the contract of K8 a CPU reproduces
 * every sample bit for bit (rtlsdr-wsprd_amd/csrc/kernels/audio_synth.h is the definition, tests/helpers/
 * audio_synth_check.cpp its serial form).  All arithmetic is double, unfused, in the order written; sine, cosine and the
 * Gaussian draw are those of K8 (synth_math.h).  A transmission is a wspr_synth_tx as above; here amp and noise_sigma are
 * in PCM units (LSB).
 *
 * For record s of nsamp samples (0 .. 1 440 000), global segment S = seg_index0 + s, output sample k, in this order:
 *   1. acc = 0.0, or (double)pcm[k] with WSPR_SYNTH_ACCUMULATE (the bit of wspr_synth_batch_device(): a known test signal
 *      onto a recorded slot that is already resident in HBM).
 *   2. If noise_sigma > 0: acc = acc + (double)n_k.  One float32 Gaussian pair (a, b) per PAIR of samples, m = k >> 1:
 *      Philox-4x32-10 keyed by the seed, counter = (m, 0x80000000, S low, S high), through exactly the Box-Muller of K8's
 *      noise; sample 2m takes a, sample 2m + 1 takes b.  Counter word 1 = 0x80000000 is a stream of its own (K8's noise
 *      uses 0, K13's impulses 1 + 2q + p).  A record's noise does not depend on how a job is split.
 *   3. For each transmission of the segment IN LIST ORDER: acc = acc + (double)amp * cos(phi), with
 *        df = 12000.0/8192.0,  fd_i = ((double)drift/2.0) * ((double)i - 81.0)/81.0,
 *        dphi_i = (2.0*3.14159265358979323846) * (1/12000.0) * (((1500.0 + (double)f0) + fd_i) + ((double)symbols[i] - 1.5) * df),
 *        P_0 = 0.0,  P_{i+1} = P_i + 8192.0 * dphi_i     (162 dependent adds, run as written),
 *        phi = P_i + (double)j * dphi_i                   for sample j = 0 .. 8191 of symbol i,
 *      at output index k = first + 8192 i + j, first = floor((double)t0 * 12000.0) clamped to +-4 000 000 (a far-away
 *      frame simply misses the record).  Indices outside [0, nsamp) are dropped: a frame may hang off either end.
 *   4. acc > 32767.0 gives 32767, acc < -32768.0 gives -32768, and either counts as clipped; otherwise the sample is
 *      (acc + 6755399441055744.0) - 6755399441055744.0 -- nearest, ties to even -- as an int16.  n_clipped[s] is the
 *      record's count.
 * RANGE: the sine and cosine are valid below 2^20 * pi/2 rad, which 1 327 104 samples reach at 2 370 Hz; 1500 + |f0| +
 * |drift|/2 + 2.2 Hz stays below that for |f0| + |drift|/2 <= 800 Hz, and a call beyond is refused.
 * LEVELS: real noise of standard deviation sigma at 12 kHz has power sigma^2 * 2500/6000 in 2 500 Hz, so a signal at
 * `snr` dB in the decoder's convention has amp = sigma * sqrt(5000/6000) * 10^(snr/20).
 *
 * wspr_synth_audio_batch_device(): row s is at d_pcm + s*pcm_stride samples; d_pcm 16-byte aligned device memory,
 * pcm_stride a multiple of 8 and >= nsamp.  Columns 0 .. roundup8(nsamp) - 1 are written: from nsamp on they are zero
 * without WSPR_SYNTH_ACCUMULATE and keep what they held with it; the columns behind are left alone.  Returns 0; -1 with a
 * line on stderr and NOTHING WRITTEN (n_clipped included) for: no device, a symbol > 3, seg outside the batch, an unsorted
 * list, negative counts, a non-finite f0 / t0 / amp / drift / noise_sigma, noise_sigma < 0, |amp| or noise_sigma > 1e6,
 * |f0| + |drift|/2 > 800 Hz, any flag bit other than WSPR_SYNTH_ACCUMULATE, misalignment, a stride that is no multiple of
 * 8 or is too small; -2 for nsamp > 1 440 000.  nseg == 0 does nothing, nsamp == 0 writes no sample (n_clipped: zeros).
 * Stream contract and lane turn as wspr_audio_batch_device(); the scratch (the list, 2 592 B of phases per transmission,
 * one counter per record) belongs to the lane's context and is returned by wspr_release_buffers(). */
int wspr_synth_audio_batch_device(const wspr_synth_tx *tx, int ntx, int nseg, int seg_index0, int nsamp,
                                  float noise_sigma, uint64_t seed, int flags,
                                  void *d_pcm, size_t pcm_stride, int *n_clipped /* host, nseg, may be NULL */);
/* One record into host memory (read first with WSPR_SYNTH_ACCUMULATE), seg_index0 = 0: row 0 of the batch call.
 * n_clipped: one int, may be NULL. */
int wspr_synth_audio(const wspr_synth_tx *tx, int ntx, int nsamp, float noise_sigma, uint64_t seed, int flags,
                     int16_t *pcm, int *n_clipped);

/* ---- IQ to audio (K18) ------------------------------------------------------------------------------------------
 * The way back from the decoder's rows to audio: a slot that exists only as 375 Hz IQ -- a receiver capture behind
 * wspr_decimate_u8*(), a .iq or .c2 file, a scene of wspr_synth*(), the residual a decode call writes back -- becomes the
 * 12 000 Hz, 16-bit, mono record with the band at 1 500 Hz that wspr_audio_batch_device(), wspr_write_wav_file(), WSJT-X's
 * wsprd and wsprdaemon archives take.  It is the transpose of the audio front end over that stage's own two tap tables
 * (wspr_audio_constants(): gI[k], gQ[k], k = -255 .. 255); no table of its own.  A CPU reproduces every sample bit for bit
 * (rtlsdr-wsprd_amd/csrc/kernels/iq_audio.h is the definition, tests/helpers/iq_audio_check.c its serial form).
 * wspr_set_arithmetic() does not touch this stage.
 *
 * For one row of np samples (0 .. 45 000) of I and Q the record has 32 np samples.  Output sample n, in this order:
 *   acc = +0.0f
 *   for every m with 0 <= m < np and |n - 32 m| <= 255, IN RISING m, with k = n - 32 m:
 *       acc = fmaf(gI[k], I[m], acc)        unless k = 2, 6 (mod 8)
 *       acc = fmaf(gQ[k], Q[m], acc)        unless k = 0, 4 (mod 8)        (k mod 8 non-negative)
 *   y = 16.0f * acc
 *   p = (double)y * (double)gain
 *   p is NaN: the sample is 0 and counts as clipped.  Otherwise step 4 of the audio scene synthesiser above: p > 32767.0
 *   gives 32767, p < -32768.0 gives -32768, either counts as clipped, else (p + 6755399441055744.0) - 6755399441055744.0
 *   (nearest, ties to even) as an int16.  n_clipped[s] is the record's count.
 * Nothing else is fused or reordered.  The taps named in the two "unless" are +0.0f, but the input is float and may be Inf
 * or NaN, so leaving those steps out IS the definition, not a shortcut: output n takes I alone for n = 0, 4 (mod 8), Q alone
 * for n = 2, 6 (mod 8), both for odd n; at most 16 inputs and 24 multiply-adds per output.
 * SCALE AND TIME: a phasor A e^{+j 2 pi f m / 375} leaves as A cos(2 pi (1500 + f) n / 12000) -- a tone at +f in the decoder's
 * convention is audio at 1500 + f Hz.  gain = 32768 is the inverse of the front end's 2^-15 and suits rows normalised to a
 * peak of 0.5.  Output n = 32 m is centred on input m: no delay is added in either direction, and this call followed by
 * wspr_audio_batch_device() is the identity inside the search band up to that filter's ripple, twice (1.4e-4 relative at
 * +-110 Hz), and the 16-bit rounding.
 *
 * wspr_iq_to_audio_batch_device(): input rows as for wspr_noise_batch_device() (d_idat, d_qdat 16-byte aligned device
 * memory, seg_stride floats apart, a multiple of 4 and >= samples; nothing at or behind `samples` is read); output rows as
 * for wspr_synth_audio_batch_device() (d_pcm 16-byte aligned device memory, pcm_stride a multiple of 8 and >= 32 * samples).
 * Columns 0 .. 32 * samples - 1 are written; the columns behind them and the input are left alone.  Returns 0; -1 with a
 * line on stderr and NOTHING WRITTEN (n_clipped included) for: no device, negative counts, misalignment, a stride that is
 * too small or no multiple of its unit, a non-finite gain; -2 for samples > 45 000.  nseg == 0 does nothing, samples == 0
 * writes no sample (n_clipped: zeros).  Stream contract and lane turn as wspr_audio_batch_device(); the scratch (one counter
 * per record) belongs to the lane's context and is returned by wspr_release_buffers(). */
int wspr_iq_to_audio_batch_device(const void *d_idat, const void *d_qdat, int nseg, int samples, size_t seg_stride,
                                  float gain, void *d_pcm, size_t pcm_stride, int *n_clipped /* host, nseg, may be NULL */);
/* One row of host memory into a record of 32 * samples int16 in host memory: row 0 of the batch call.  n_clipped: one
 * int, may be NULL. */
int wspr_iq_to_audio(const float *I, const float *Q, int samples, float gain, int16_t *pcm /* 32*samples */, int *n_clipped);

/* ---- waterfall: dB-quantised spectrogram images (K20) --------------------------------------------------------------
 * What was on the band during a slot, as a picture: one byte per (time, frequency) cell, made on the device from the
 * resident 375 Hz rows -- 105 KB to fetch by default (hop 128; 52 KB at hop 256) where the row is 360 KB -- and two file writers to look at it.  The reference
 * computes no such picture, so the definition is this library's own (rtlsdr-wsprd_amd/csrc/kernels/waterfall.h over
 * noise.h; tests/helpers/waterfall_check.c is its serial form, and the kernel equals it byte for byte).  It is K16's frame
 * transform with the frames kept instead of averaged: window, twiddles, butterfly, bin order and W2 are those of the band
 * noise figures above.  The parameters are an argument of the calls, not state:
 *   hop       128 or 256 samples between frames of 512 (128 is the reference's own frame step, two rows per symbol)
 *   tavg      1 .. 16 frames averaged into one image row
 *   j0, j1    signed bins, -256 <= j0 <= j1 <= 255; bin j lies at j*375/512 Hz; ncols = j1 - j0 + 1
 *   ref_mode  WSPR_WF_REF_ABSOLUTE: `ref`, finite and > 0, in K16's units (linear power per complex sample);
 *             WSPR_WF_REF_FLOOR: the row's own K16 fft_p30
 *   db_min    level 0 is "below db_min + db_step"; -60 .. 60        db_step  dB per level, 0.05 .. 4
 * wspr_waterfall_default_params(): hop 128, tavg 1, bins -150 .. 150 (+-109.9 Hz, the search band, 301 columns), floor
 * mode, db_min -10, db_step 0.25: the levels span -10 .. +53.75 dB over the floor.
 * For one row of np samples (0 .. 45 000):
 *   frames    nframes = np >= 512 ? (np - 512)/hop + 1 : 0; frame f holds the samples hop*f .. hop*f + 511.  nrows = nframes /
 *             tavg; image row r is formed from the frames r*tavg .. r*tavg + tavg - 1; a trailing incomplete group is dropped.
 *             Row 0 is the earliest; column c is bin j0 + c, so +f is to the right.  348 (hop 128) or 174 rows for a full row.
 *   power     P_f[j] exactly K16's (float products with the Hann window, nine stages, re*re + im*im separately rounded, no
 *             fused multiply-add).  M = the double sum of (double)P_f[j] over the row's frames in rising f from 0.0;
 *             m = (float)(M / (double)tavg / W2): the units of K16's a[j].
 *   reference absolute mode: `ref`.  Floor mode: the fft_p30 that wspr_noise_batch_device() returns for the same row and
 *             `samples`, bit for bit (K16's own hop of 256 whatever hop is here; the windows play no part).  There is no
 *             usable floor when K16's record lacks WSPR_NOISE_FFT_USED, carries WSPR_NOISE_NONFINITE or has fft_p30 == 0:
 *             then info.ref = 0, flags gets WSPR_WF_NO_REF (and WSPR_WF_NONFINITE if K16 reported it) and every pixel is 0.
 *   guard     (when a reference exists) if any sample of hop*(r*tavg) .. hop*(r*tavg + tavg - 1) + 511, the samples image row
 *             r is formed from, has exponent bits 0xff on either rail, every pixel of row r is 255 and WSPR_WF_NONFINITE is
 *             set: a white stripe where the capture is garbage.  Samples that no complete row uses are not looked at.
 *   level     r = (double)m / (double)ref;  T[i] = pow(10.0, ((double)db_min + (double)i*(double)db_step)/10.0), i = 1 .. 255,
 *             from the host libm in double.  The pixel is the number of i with r >= T[i]: a NaN r gives 0, +Inf gives 255.
 *             (No logarithm runs on the device: it searches the table.)
 *   info      the ref used, nframes, nrows, flags; WSPR_WF_WRITTEN iff nrows > 0.
 * wspr_set_arithmetic() does not touch this stage, and no decode call runs it.
 *
 * wspr_waterfall_shape(): nrows and ncols (either may be NULL) of a row of `samples` samples under p.  Returns 0; -1 for
 * samples < 0 or parameters out of range, -2 for samples > 45000.  Needs no device.
 * wspr_waterfall_batch_device(): input rows as for wspr_noise_batch_device().  Image s lies at (uint8_t*)d_img +
 * s*img_stride and pixel (r, c) at + r*ncols + c; d_img is 16-byte aligned device memory, img_stride a multiple of 16 and >=
 * nrows*ncols.  Bytes [0, nrows*ncols) of each image are written, everything behind them is left alone; info[0 .. nseg) is
 * HOST memory.  Returns 0; -1 with a line on stderr and NOTHING WRITTEN (info included) for: no device, negative counts,
 * misalignment, a stride too small or no multiple of its unit, hop other than 128 / 256, tavg outside 1 .. 16, bins outside
 * -256 <= j0 <= j1 <= 255, an unknown ref_mode, absolute mode with a ref that is not finite and > 0, db_min or db_step
 * non-finite or out of range, info == NULL; -2 for samples > 45000.  nseg == 0 does nothing; samples < 512 writes no pixel
 * and gives info records with nrows 0.  Stream contract and lane turn as wspr_audio_batch_device(); the scratch (16 bytes
 * per segment, 32 more in floor mode, two tables of 4 KB and 2 KB) belongs to the lane's context and is returned by
 * wspr_release_buffers().
 * wspr_waterfall(): one row from host memory (any alignment) into an image of nrows*ncols bytes in host memory: row 0 of the
 * batch call.
 *
 * wspr_waterfall_palette(): 256 RGB triples for the levels.  which = 0: grey, (v, v, v).  which = 1 (any other value is taken
 * as 1): a piecewise-linear integer ramp black - blue - cyan - yellow - red - white: with k = min(v / 51, 4) and t = v - 51*k
 * (integer division), (R, G, B) = k = 0: (0, 0, 5t);  k = 1: (0, 5t, 255);  k = 2: (5t, 255, 255 - 5t);  k = 3: (255, 255 - 5t, 0);
 * k = 4: (255, 5t, 5t).
 * wspr_write_pgm_file(): binary P5, "P5\n<width> <height>\n255\n" and the bytes.  wspr_write_png_file(): 8 bits per sample,
 * colour type 0 (grey), or colour type 3 with a PLTE of the 256 entries when rgb768 is given; one IDAT chunk holding one zlib
 * stream of stored deflate blocks, filter 0 on every scan line; no compression and no library.  Both take width, height >= 1
 * (width * height + height below 2^31), image row 0 on top, and return 0, or -1 if the arguments are unusable or the file
 * cannot be written.  Host code: they need no device. */
#define WSPR_WF_REF_ABSOLUTE 0
#define WSPR_WF_REF_FLOOR    1
#define WSPR_WF_WRITTEN   1   /* nrows > 0 and pixels were written */
#define WSPR_WF_NO_REF    2   /* floor mode and no usable floor: every pixel is 0 */
#define WSPR_WF_NONFINITE 8   /* some image row was guarded */
typedef struct wspr_waterfall_params {      /* 32 bytes */
    int32_t hop, tavg, j0, j1, ref_mode;
    float   ref, db_min, db_step;
} wspr_waterfall_params;
typedef struct wspr_waterfall_info { float ref; int32_t nframes, nrows, flags; } wspr_waterfall_info;   /* 16 bytes */
void wspr_waterfall_default_params(wspr_waterfall_params *p);
int wspr_waterfall_shape(int samples, const wspr_waterfall_params *p /* NULL = default */, int *nrows, int *ncols);
int wspr_waterfall_batch_device(const void *d_idat, const void *d_qdat, int nseg, int samples, size_t seg_stride,
                                const wspr_waterfall_params *p /* NULL = default */,
                                void *d_img, size_t img_stride, wspr_waterfall_info *info /* host, nseg */);
int wspr_waterfall(const float *I, const float *Q, int samples, const wspr_waterfall_params *p,
                   uint8_t *img /* host, nrows*ncols */, wspr_waterfall_info *info);
void wspr_waterfall_palette(int which /* 0 grey, 1 the colour ramp */, uint8_t rgb[768]);
int wspr_write_pgm_file(const char *filename, const uint8_t *img, int width, int height);
int wspr_write_png_file(const char *filename, const uint8_t *img, int width, int height, const uint8_t *rgb768 /* NULL = grey */);

/* ---- tunable multi-band front end: one 2.4 Msps capture, many bands (K21) --------------------------------------------
 * wspr_decimate_u8*() extracts the one band that lies fs/4 below the tuner at the reference's ratio of 6401 (374.94 Hz
 * rows).  A 2.4 MHz capture often holds several WSPR bands (2200 m, 630 m and 160 m of a direct-sampling receiver; 80 m and
 * both 60 m segments), and a dongle may be tuned off-centre.  This stage reads the raw rows ONCE and writes, for each of up
 * to WSPR_TUNE_MAX_BANDS offsets, a 375.000 Hz row that wspr_decode_batch_device() takes as it stands.  The reference tunes
 * one dongle to one band, so the definition is this library's own (rtlsdr-wsprd_amd/csrc/kernels/tune.h;
 * tests/helpers/tune_check.c is its serial form, and the kernel equals it bit for bit).  Integer up to the 375 Hz outputs:
 *   samples     s_n = (I_n - 128) + j (Q_n - 128); a vector v is samples 8v .. 8v + 7 (16 bytes).
 *   oscillator  unsigned 32-bit phase, 0 at the start of every row; step = wspr_tune_step(offset_hz) =
 *               floor(-offset_hz * 2^32 / 2.4e6 + 0.5) mod 2^32 brings a signal at +offset_hz to 0 Hz.  *realised_hz =
 *               -(int32)step * 2.4e6 / 2^32, the offset the step stands for (resolution 0.00056 Hz).
 *   rs14(x)     = (x + 8192) >> 14, arithmetic shift (halves towards +infinity), of each part of a complex number.
 *   rot(P)      = rs14(C[P >> 24] * F[(P >> 16) & 255]), C[k] = round(16384 e^{2 pi i k / 256}), F[k] = round(16384
 *               e^{2 pi i k / 65536}): the committed integer tables of wspr_tune_constants() (tools/gen_tune_tables.py).
 *               rot(m 2^30) = 16384 (1, j, -1, -j)[m]: the offsets 0, +-fs/4 and fs/2 are mixed exactly.
 *   mixer       H_k = rot(k step), k = 0 .. 7;  z_v = sum_k s_{8v+k} H_k (int32);  y_v = rs14(z_v * rot(8 v step)) (64-bit).
 *   decimation  y_v (300 kHz) through the reference front end's filter family at R = 800: i1 += y_v; i2 += i1; c_b = i2
 *               behind vector 800 b + 799; d_b = c_b - 2 c_{b-2} + c_{b-4} (c = 0 before the start); int64, no wrap.  One
 *               output covers 6400 samples: 375 Hz exactly.
 *   float tail  x_b = (float)(double)d_b * scale, scale = float32(6401^2 / (800^2 * 8 * 16384)): an in-band tone leaves
 *               with the amplitude wspr_decimate_u8*() gives it.  Then the 33 taps of wspr_front_end_constants() over
 *               x_{m-32} .. x_m from a zero history, acc = acc + x * tap in rising tap order, every product and sum rounded
 *               (no fused multiply-add).  wspr_set_arithmetic() does not touch any of this.
 *   lengths     n_out = min(floor(nsamples / 6400), 45000); a trailing partial block is dropped; every other column of the
 *               row is 0.0f.  No carried state: this is the batch form only.
 * wspr_tune_u8_batch_device(): d_raw and bytes_per_seg as for wspr_decimate_u8_batch_device(); steps: nbands host words.
 * Row s * nbands + b of d_idat / d_qdat (16-byte aligned, stride wspr_iq_stride()) = segment s tuned by steps[b], ready for
 * wspr_decode_batch_device(..., nseg * nbands, ...); normalise as in wspr_decimate_u8_batch_device().  The kernel serves 4
 * bands per pass over the raw rows.  Returns 0; -1 with a line on stderr and NOTHING WRITTEN without a usable device, for
 * nseg < 0, nbands outside 1 .. 16, steps == NULL, a misaligned pointer or bytes_per_seg % 16 != 0; nseg == 0 does nothing; a
 * row shorter than one block gives rows of zeros.
 * wspr_tune_u8(): one capture from host memory (any alignment) into nbands host rows of 45000 floats each, through the
 * device; *n_out (may be NULL) = the outputs of every row.
 * wspr_tune_constants(): the two tables (re, im of entry k at [2k], [2k + 1]) and 6400; any pointer may be NULL. */
#define WSPR_TUNE_MAX_BANDS 16
uint32_t wspr_tune_step(double offset_hz, double *realised_hz /* may be NULL */);
int wspr_tune_u8_batch_device(const void *d_raw, size_t bytes_per_seg, int nseg, const uint32_t *steps, int nbands,
                              void *d_idat, void *d_qdat, int normalise);
int wspr_tune_u8(const uint8_t *iq, size_t nbytes, const uint32_t *steps, int nbands, float *I, float *Q,
                 uint32_t *n_out, int normalise);
void wspr_tune_constants(int16_t c256[512], int16_t f256[512], int *samples_per_output /* 6400 */);

/* ---- receiver session --------------------------------------------------------------------
 * The reference's rx_state (two I/Q buffers of 45000 samples, their fill counters, the active index,
 * rtlsdr_wsprd.c:78-90), the decimator's static state (:135-160) and the body of its decoder thread (:263-328) as
 * one object.  The application keeps its three threads: the RX thread feeds librtlsdr callback buffers, the main
 * loop rolls the buffers over on the even minute, the decoder thread decodes the completed buffer.  feed() may
 * run beside decode(): feed() and rollover() exclude each other (a roll-over waits for the callback in flight, and
 * nothing is written into a buffer once rollover() has returned its index), and the front end runs on a lane of
 * the library that wspr_bind_thread_lane() never hands out. */
typedef struct wspr_session wspr_session;
wspr_session *wspr_session_create(struct decoder_options options);     /* initSampleStorage(), :331-336 */
void wspr_session_destroy(wspr_session *s);
/* rtlsdr_callback(buf, len), :126-244: mixer + CIC + FIR into the active buffer (outputs beyond 45000 are
 * dropped, :236-242).  len a multiple of 16 (librtlsdr delivers 65536).  Returns the buffer's fill, < 0 on error. */
int wspr_session_feed(wspr_session *s, const uint8_t *buf, uint32_t len);
/* One callback of EACH of n receivers at once (bufs[k]: len bytes for sessions[k]; the same len, a multiple of 16, for
 * all; the sessions distinct): what n wspr_session_feed() calls do, as one transfer and one launch set -- a callback's
 * cost is its round trips, not its arithmetic.  fills[k] (optional): sessions[k]'s fill afterwards.  0, < 0 on error. */
int wspr_session_feed_many(wspr_session *const *sessions, const uint8_t *const *bufs, uint32_t len, int n, int *fills);
/* Main loop on the 2-minute boundary, :1179-1182: switches to the other buffer (fill reset to 0) and returns the
 * index of the buffer that just completed. */
int wspr_session_rollover(wspr_session *s);
/* decoder(), :263-328, on a completed buffer: returns 0 without decoding if it holds fewer than 117 s of samples
 * (:277), else zeroes the tail (:284-288), normalises to a peak of 0.5 (:290-305), calls wspr_decode() (:312-317)
 * and returns 1 (negative: no usable device).  The buffer then holds what the reference's saveSample() would see. */
int wspr_session_decode(wspr_session *s, int buffer, struct decoder_results *decodes, int *n_results);
/* Many receivers, one slot: the completed buffers (buffers[k] of sessions[k]) of n sessions decoded TOGETHER -- one
 * batch call per distinct set of decoder options (the receivers of one band share theirs).  decodes: n rows of
 * max_results spots; n_results[k]; decoded[k] (optional) = 1 / 0 as wspr_session_decode() would have returned.  Spots
 * and what the buffers hold afterwards are those of wspr_session_decode() on each session in index order (with
 * usehashtable on any of them that is the order of the hash memory: then only RUNS of consecutive sessions with equal
 * options share a batch call, so sessions with options A, B, A are decoded 0, 1, 2).  Returns the number of buffers
 * decoded, negative on error. */
int wspr_session_decode_many(wspr_session *const *sessions, const int *buffers, int n, struct decoder_results *decodes,
                             int max_results, int *n_results, int *decoded);
uint32_t wspr_session_fill(const wspr_session *s, int buffer);
const float *wspr_session_samples(const wspr_session *s, int buffer, int rail /* 0 = I, 1 = Q */);
/* Microseconds until the next even UTC minute, :1170-1175 (what the main loop sleeps). */
uint32_t wspr_usec_to_next_slot(long tv_sec, long tv_usec);
/* UTC time stamp of the frame being decoded: gmtime(now - 120 + 1), :307-310; for wspr_format_spot_timestamped(). */
void wspr_frame_time(long unixtime_now, int *year, int *month, int *day, int *hour, int *minute);

/* ---- recorded files and the playback print format ----------- */
/* Replaces readRawIQfile(), reference rtlsdr_wsprd.c:555-592 (.iq: interleaved f32, Q negated,
 * normalised to peak 0.5).  I/Q: 45000 floats each.  Returns complex samples read, 0 on error. */
int wspr_read_iq_file(const char *filename, float *I, float *Q);
/* Replaces readC2file(), reference rtlsdr_wsprd.c:620-667 (14-byte name, int, double dial Hz). */
int wspr_read_c2_file(const char *filename, float *I, float *Q, double *dial_hz);
/* RIFF/WAVE reader: PCM (format tag 1), 1 channel, 16 bit, 12000 Hz; chunks walked properly (unknown chunks such as LIST
 * skipped, odd sizes padded); reads min(data samples, cap); a short data chunk yields what the file holds.
 * Returns samples read, 0 on any error or any other format.  For wspr_audio_to_iq() / wspr_audio_batch_device(). */
size_t wspr_read_wav_file(const char *filename, int16_t *pcm, size_t cap);
/* RIFF/WAVE writer: nsamp samples as 12 000 Hz 16-bit mono PCM, exactly what wspr_read_wav_file() reads (a record of
 * wspr_synth_audio(), for one).  Returns 0; -1 if the file cannot be written.  Host code: needs no device. */
int wspr_write_wav_file(const char *filename, const int16_t *pcm, size_t nsamp);
/* Replaces writeRawIQfile(), reference rtlsdr_wsprd.c:595-617. */
int wspr_write_iq_file(const char *filename, const float *I, const float *Q);
/* Exactly what wspr_read_c2_file() reads: 14 name bytes (the file's base name, cut or padded with zeros), int type 2,
 * double dial frequency in Hz, then 45000 interleaved pairs (I, -Q) of float32.  I/Q: 45000 floats each.  Returns the
 * samples written (45000), 0 on error, like wspr_write_iq_file().  Host code: needs no device. */
int wspr_write_c2_file(const char *filename, const float *I, const float *Q, double dial_hz);
/* The "Spot : ..." line of decodeRecordedFile(), reference rtlsdr_wsprd.c:691-701. */
int wspr_format_spot(const struct decoder_results *r, char *out, size_t cap);

/* The daemon's stdout line, reference printSpots() rtlsdr_wsprd.c:447-474 (UTC frame time). */
int wspr_format_spot_timestamped(const struct decoder_results *r, int year, int month, int day, int hour,
                                 int minute, char *out, size_t cap);
/* Text of the wsprnet.org report URL, reference postSpots() rtlsdr_wsprd.c:390-397 (r == NULL: the
 * "no spot" status report) and :414-429 (one spot).  Formatting only -- nothing is sent. */
int wspr_format_wsprnet_url(const struct decoder_results *r, const struct decoder_options *opt,
                            double dial_hz, int year, int month, int day, int hour, int minute,
                            const char *app_version, char *out, size_t cap);

/* ---- the reference's other decoder entry points, GPU-backed ---------------- */
/* Replaces sync_and_demodulate(), reference wsprd/wsprd.h:76-91 (GPU-backed).  symfac is honoured (mode 2,
 * wsprd.c:250); the decoder itself always passes 50.
 * np (here, in subtract_signal() and in subtract_signal2()): a record holds at most 45 000 samples, as in the reference's
 * decoder.  np above 45 000 is treated as 45 000: id[k] and qd[k] with k >= 45 000 are neither read nor written. */
void sync_and_demodulate(float *id, float *qd, long np, unsigned char *symbols, float *freq,
                         int ifmin, int ifmax, float fstep, int *shift, int lagmin, int lagmax,
                         int lagstep, float *drift, int symfac, float *sync, int mode);
/* Replaces subtract_signal(), reference wsprd/wsprd.h:83-89 / wsprd.c:263-312 (symbol-by-symbol subtraction;
 * declared by the reference's header, never called by its decoder; GPU-backed).  np above 45 000 is treated as 45 000 (see
 * sync_and_demodulate()). */
void subtract_signal(float *id, float *qd, long np, float f0, int shift, float drift,
                     const unsigned char *channel_symbols);
/* Replaces subtract_signal2(), reference wsprd/wsprd.h:99-105 (GPU-backed).  np above 45 000 is treated as 45 000: samples
 * behind it are neither read nor written (see sync_and_demodulate()). */
void subtract_signal2(float *id, float *qd, long np, float f0, int shift, float drift,
                      const unsigned char *channel_symbols);
/* Timing of the stages of the most recent batch call, milliseconds (HIP events on the library's
 * streams / host clock, summed over the slots).  Order: [0] FFT+sync stage, [1] host bookkeeping,
 * [2] device Fano tail (K6), [3] fine sync + demod, [4] subtract, [5] host Fano, [6] total wall time,
 * then counts: [7] Fano calls, [8] Fano time-outs, [9] Fano cycles, [10] candidates refined, [11] GPU
 * waves, [12] Fano attempts left to the device tail, [13] segments decoded a second time, [14] refined
 * candidates whose result was consumed (the others: speculation cut by a subtraction), [15] subtractions;
 * then the CPU time (not wall time) the calling thread spent in the call, milliseconds: [16] all of it, by phase [17] pass
 * start (candidate lists, re-ranking), [18] wave building, [19] fine search + first rung (launches, lists, gates),
 * [20] ladder, [21] bookkeeping (unpack, re-encode, de-dup), [22] subtraction launches, [23] result hand-over;
 * then [24] decoded messages looked up in the calling thread's message cache (what a 50-bit message unpacks and
 * re-encodes to, computed once per thread and message) and [25] how many of them it answered;
 * then the ordered-statistics rescue stage (wspr_set_osd_depth(); all zero while it is off), summed like the counts:
 * [26] the stage's wall time, milliseconds (K9 and its round trips), [27] soft-symbol vectors it tried, [28] how many
 * of its results the "heard before" gate let through;
 * then the lag pruning of the fine search's full lag scan (drift-free candidates), summed like the counts: [29] candidates
 * whose losing lags a bounded coarse pass ruled out, [30] the exact single-lag evaluations those candidates took
 * instead of 33 each, [31] candidates that fell back to the whole scan (too many contenders, or a quantity the bound
 * does not cover);
 * then the block-detection stage (wspr_set_block_detection(); all zero while it is off), summed like the counts: [32] the
 * stage's wall time, milliseconds (K10, the Fano searches and their round trips), [33] soft-symbol vectors it sent to
 * Fano, [34] and [35] the decodes it made at block size 2 and 3;
 * then the Doppler-spread stage (wspr_set_spread_estimate(); both zero while it is off), summed like the counts: [36] the
 * stage's device time, milliseconds (K11 with its transfers, taken without a host wait like the subtraction's), [37] the
 * spread jobs it ran (one per spot the call's decode loops added);
 * then the list-decoding stage (wspr_set_message_list(); all zero while it is off), summed like the counts: [38] the
 * stage's wall time, milliseconds (K14 and its round trips), [39] soft-symbol vectors it matched against the list, [40]
 * the spots it accepted;
 * then the lag pruning of the drifting candidates (their own coarse pass; [29]..[31] count drift-free candidates only),
 * summed like the counts: [41] drifting candidates pruned, [42] the exact single-lag evaluations they took, [43] drifting
 * candidates that fell back to the whole scan;
 * then the spot-detail stage (wspr_set_spot_details(); both zero while it is off), summed like the counts: [44] the
 * stage's device time, milliseconds (K19 with its transfers, taken without a host wait like the spread stage's), [45] the
 * jobs it ran (one per spot the call's decode loops added).
 * Returns the number of values written (<= capacity). */
int wspr_last_timings(double *ms, int capacity);
/* Worker threads of the library's host pools alive in this process (the threads that call into the library are
 * not counted): what a rank adds to the host's load besides its callers -- 0 when its CPU share (WSPR_HOST_THREADS,
 * or the share of a node-level call) is no larger than the slots it drives. */
int wspr_host_pool_workers(void);
/* Device Fano search (K6w) over n soft-symbol vectors of 162 bytes in transmission
 * (interleaved) order, i.e. deinterleave() + fano() of reference wsprd.c:759-761 (fano.c:87-238) with
 * delta 60: the exact wave-parallel search the decoder uses, one wavefront per vector (fano_wave.h).  Outputs per
 * vector: ret (0 / -1), cycles and data[10] are the reference's; metric/maxnp are filled for decoded frames only
 * (the reference's caller reads nothing else of a failed attempt, wsprd.c:759-766).  steps (may be NULL):
 * expansion steps per vector. */
int wspr_fano_batch_device_wave(const unsigned char *symbols, int n, unsigned maxcycles, int *ret,
                                unsigned *cycles, unsigned *metric, unsigned *maxnp, unsigned char *data,
                                unsigned *steps);
/* Devices.  A host thread decodes on the HIP device that is current for it; wspr_set_device() makes
 * `device` current for the calling thread (0 on success, -1 if there is no such device).  The library keeps
 * separate contexts (streams, buffers, host pools) per device, so one process can drive all GPUs of a node
 * with one host thread (or one per lane) per device, segments split by the caller -- no collective is
 * involved. */
int wspr_device_count(void);
int wspr_set_device(int device);
/* Concurrency.  Like the reference, the library is not re-entrant within one lane -- calls made on the same lane of
 * the same device from several threads TAKE TURNS (safe, but nothing overlaps); it keeps up to sixteen independent
 * lanes (streams, buffers, host pools).  A host thread is bound to lane 0 until it calls this (returns the lane
 * actually bound, 0..15; one more lane is reserved for receiver sessions); calls made from threads bound to different
 * lanes may overlap, e.g. to start the next batch under the tail of the current one. */
int wspr_bind_thread_lane(int lane);
/* A batch of >= 128 segments is split over up to WSPR_SLOTS (default 3) concurrent pipelines ("slots") of the
 * calling thread's lane, so that one call overlaps its own host phases with its own kernels.  A service that
 * already keeps several batches in flight on different lanes gets that overlap from the lanes: this caps the
 * slots of the calling thread's later calls at n (n <= 0: no cap) and returns the number they will use. */
int wspr_set_thread_slots(int n);
/* Memory.  The library keeps the work buffers of every (device, lane, slot) it has used, sized for the largest
 * batch seen there (about 1 MB of HBM per segment).  This returns the work buffers of the CURRENT device -- all
 * lanes, device and pinned host memory -- to the driver and reports the device bytes freed; tables, streams and
 * host pools stay, and the next call allocates what it needs.  Calls in flight on that device (any lane, any
 * receiver session's feed) finish first and calls arriving meanwhile wait (since round 5; before, none was allowed
 * to be in flight).  Nothing a caller can observe lives in these buffers between calls. */
size_t wspr_release_buffers(void);
/* Scheduler tuning for crowded bands (batches of >= 256 segments per slot): the host Fano pool gives
 * every attempt `cycles_per_bit` cycles per bit; attempts still running then are finished by K6 with
 * the reference's 10000, and a segment in which one of those decodes after all is decoded again with
 * the full budget everywhere, so results never depend on this value.  Default 10000 = split off
 * (env WSPR_FANO_FAST overrides); a few hundred pays once a batch carries thousands of Fano time-outs (the
 * device tail then takes tens of milliseconds for all of them).  Returns the previous value. */
unsigned wspr_set_fano_fast_budget(unsigned cycles_per_bit);
/* Where a batch's Fano attempts run: 0 = the host pool (the north star's partition; with the budget split
 * above if set), 1 = every attempt on the device (the exact wave-parallel search, straight from the soft
 * symbols in HBM: no host Fano, nothing postponed or decoded twice), -1 = automatic (default; env
 * WSPR_FANO_DEVICE): the device for batches of >= 32 segments per pipeline when the rank has fewer than four
 * host threads or the pipeline's previous batch met more than one time-out per ten segments (a crowded band),
 * the host otherwise (single calls always).  Results are identical in every mode.  Returns the previous value. */
int wspr_set_fano_device_mode(int mode);
/* Arithmetic of the signal-processing stages, process-wide (like wspr_set_fano_device_mode()).
 *   WSPR_ARITH_EXACT (the default): every float sum and product separately rounded in the reference's order, i.e.
 *     what the reference's x86-64 build computes without FMA; bit-exact against that evaluation.
 *   WSPR_ARITH_CONTRACTED: each sum of products that clang's front end contracts in wsprd/wsprd.c under its default
 *     -ffp-contract=on becomes the fused multiply-add it makes there, and nothing else.  clang fuses within one
 *     expression, the LEFT product first: a*b + c*d -> fma(a, b, c*d), (acc + x*c) + y*s -> fma(y, s, fma(x, c, acc)),
 *     acc - x*s -> fma(-x, s, acc).  The sites, by wsprd.c line: 151 (frequency hypotheses), 180-187 (phasor
 *     recurrences), 200-207 (matched-filter sums), 211-214 (tone amplitudes), 249 (soft-symbol normalisation),
 *     378-379 / 388-389 / 408-409 (subtract_signal2: mixing, low-pass filter, write-back), 551 (FFT powers); the
 *     integer-valued products of 516, 571, 616, 663 and 754 are exact either way.  The FFT, the receiver front end
 *     and everything integer are the same in both modes, and subtract_signal() stays exact in both.
 *   The contracted mode CHANGES RESULTS, a little (tools/contract_robustness.py, profiles/contracted_robustness.json,
 *   against the exact mode): over 3 000 random scenes one of 6 880 spots is lost and one moves its dt by 64 ms (beyond
 *   the 10 ms tolerance); no call/loc/pwr changes, SNR moves by < 1e-5 dB, frequency by <= 0.1 Hz.
 *   No mode reproduces the reference's arm64 binary bit for bit: its Makefile's `CC ?= clang` leaves make's default
 *   `cc` in place, and gcc's gnu17 default -ffp-contract=fast fuses after optimisation by no rule the source text
 *   states.  The clang rule above is the one contraction the source defines and anyone can reproduce.
 * Every wspr_decode*() and wspr_session_decode*() call, sync_and_demodulate() and subtract_signal2() reads the mode
 * once, on entry, and uses it throughout (all slots, node worker threads and hash rounds of the call); a
 * WSPR_HASH_REVISIT call must run under the mode of the call it completes.  Returns the previous mode, or -1 (nothing
 * changed) for any other value. */
#define WSPR_ARITH_EXACT      0
#define WSPR_ARITH_CONTRACTED 1
int wspr_set_arithmetic(int mode);
/* Ordered-statistics decoding (OSD), an opt-in second chance for candidates on which every Fano attempt failed --
 * what current WSJT-X wsprd offers as -o; the reference (v0.5.6) predates it, so there is no reference behaviour to
 * match and the definition is this library's own (rtlsdr-wsprd_amd/csrc/kernels/osd.h; kernel K9):
 *   the 162 soft symbols s[i] are deinterleaved; h[i] = (s[i] >= 128), r[i] = |2 s[i] - 255|; the positions are sorted
 *   by r descending (ties: lower index) and, in that order, the first 50 whose columns of the code's generator are
 *   linearly independent form the most reliable basis; the codeword c_0 that agrees with h on the basis and every
 *   c_0 + (up to `depth` rows of the generator reduced to that basis) is tried -- 1, 51, 1 276, 20 876 codewords for
 *   depth 0..3 -- and the one with the smallest sum of r over the positions where it differs from h wins (ties: fewer
 *   rows, then the lexicographically smaller set of rows).
 * wspr_osd_batch_device(): that decode for n vectors of 162 soft symbols in transmission (interleaved) order, as
 * wspr_fano_batch_device_wave() takes them.  Per vector: data[11] = the winner's 50 message bits as fano() leaves its
 * decdata (the other bits zero), dist = its cost, nhard = the positions where it differs from h, order = the rows
 * added to c_0.  Returns 0; -1 without a usable device, for a depth outside 0..3 or n < 0; n == 0 does nothing.
 *
 * wspr_set_osd_depth(): process-wide, -1 = off (the default), 0..3 = the depth of a rescue stage in every decode call
 * (read once per call, on entry, like wspr_set_arithmetic(); a WSPR_HASH_REVISIT call must run under the depth of the
 * call it completes).  Returns the previous value; any other argument changes nothing and returns -2.  While it is on:
 *   - the Fano budget split (wspr_set_fano_fast_budget) is off for the call -- results never depended on it;
 *   - a candidate that was worth the jitter ladder, decoded on none of its rungs and whose FIRST soft-symbol vector
 *     passed the sync/rms gate of wsprd.c:758 has that vector decoded as above;
 *   - the result counts only if it is a type-1 message (CALL GRID dBm) whose callsign the hash memory already holds at
 *     that callsign's slot, i.e. a station HEARD BEFORE; otherwise the candidate stays undecoded (no spot, nothing
 *     stored, nothing subtracted).  An accepted one is a decode like any other -- spot, store, subtraction -- reported
 *     with jitter 0 and cycles 0: the Fano search never reports fewer than 81 cycles, so cycles == 0 marks an OSD spot.
 * What to expect: with usehashtable = 0 the hash memory is the call's own and starts empty, so the stage can only
 * confirm a call that the SAME segment already decoded (a second copy at another frequency, or on a later pass).  The
 * mode pays with usehashtable = 1 on a receiver that hears the same stations slot after slot: hashtable.txt then
 * carries the calls from call to call, and within a batch the gate's look-up is ordered exactly like a type-3 look-up
 * (segment k sees what segments < k stored; wspr_decode_batch_hashed() and rtlsdr-wsprd_amd/dist.py likewise).
 * An unknown call is never reported by this stage; a known call can be reported falsely only if noise lands on a
 * codeword of one of the few hundred stored calls (tools/osd_sensitivity.py measures both). */
int wspr_osd_batch_device(const unsigned char *symbols, int n, int depth, unsigned char *data, unsigned *dist,
                          unsigned *nhard, unsigned *order);
int wspr_set_osd_depth(int depth);
/* Noncoherent block detection, the demodulator behind what current WSJT-X wsprd offers as -B; the reference (v0.5.6)
 * predates it, so there is no reference behaviour to match and the definition is this library's own, shaped after
 * WSJT-X's noncoherent_sequence_detection() (rtlsdr-wsprd_amd/csrc/kernels/blockdemod.h; kernel K10).  For one hypothesis
 * (freq, shift, drift) and a block size B of 1, 2 or 3 symbols:
 *   the four tones' matched-filter sums of every symbol are those of sync_and_demodulate() mode 2 (wsprd.c:200-207, same
 *   phasor tables, same order, same guard 0 < k < np), kept as complex numbers (is, qs) instead of magnitudes; for each
 *   block of B consecutive symbols and each of its 2^B data-bit sequences (the first symbol's bit the most significant) the
 *   B sums of the tones that sequence sends (tone = sync bit + 2 * data bit) are added coherently, each rotated back by
 *   the phase its tone has gained over the symbols before it in the block (the table's recurrence one step past its last
 *   entry):  xi += is*cm + qs*sm;  xq += qs*cm - is*sm;  (cm, sm) <- (cf*cm - sf*sm, sf*cm + cf*sm), from (1, 0);
 *   p = sqrt(xi*xi + xq*xq).  A symbol's soft value is the largest p among the sequences in which its bit is 1 minus the
 *   largest among those in which it is 0; normalisation and quantisation (symfac 50) are mode 2's.
 * In the contracted arithmetic the statements fuse by the clang rule of wspr_set_arithmetic(), as written above.
 * At B = 1 this is mode 2's vector bit for bit (on finite input), in both arithmetic modes.
 *
 * wspr_block_demod_batch(): host rows as wspr_decode_batch() takes them (nseg rows of `samples` floats, seg_stride
 * apart) and n hypotheses; symbols[n][3][162] receives, per hypothesis, the vectors of B = 1, 2, 3 in transmission
 * (interleaved) order, as wspr_fano_batch_device_wave() takes them.  It obeys wspr_set_arithmetic().  Returns 0; -1 with
 * nothing written without a usable device, for samples > 45000 or < 0, n < 0, an item whose seg lies outside the batch or
 * whose freq or drift is not finite; n == 0 does nothing.
 *
 * wspr_set_block_detection(): process-wide, 1 = off (the default), 2 or 3 = the largest block size of a stage that every
 * decode call runs after the jitter ladder (read once per call, on entry, like wspr_set_osd_depth(); a WSPR_HASH_REVISIT
 * call must run under the setting of the call it completes).  Returns the previous value; any other argument changes
 * nothing and returns -2.  While it is on:
 *   - the Fano budget split (wspr_set_fano_fast_budget) is off for the call -- results never depended on it;
 *   - a candidate that was worth the jitter ladder (sync > minsync1) and decoded on none of its rungs is walked again:
 *     for B = 2 .. maxblock, and for the rungs in the reference's ladder order (quickmode: jitter 0 only), the vector of
 *     (B, rung) goes to the Fano search if the rung's mode-2 sync and the vector's own rms pass the gate of wsprd.c:758;
 *     the first success in (B, rung) order wins;
 *   - a success is a decode like any other -- spot, hash store, subtraction, de-duplication, loop exits -- reported with
 *     the rung's jitter and Fano's cycles; the spot record has no room for B (the record of wspr_set_spot_details() has);
 *   - with wspr_set_osd_depth() on as well this stage runs first, and the ordered-statistics stage sees only what it left
 *     undecoded (and uses the rung-0 vector of block size 1, as without this stage).
 * What to expect: on a stable channel the larger blocks raise the quality of the soft symbols of a weak signal without
 * any prior knowledge -- the Fano search validates a vector like any other, so no "heard before" gate is needed; drift or
 * fading across a block lowers it.  On 24 synthetic single-signal segments at -30 dB (tests/synth.py, seeds 5000..5023,
 * one pass, no subtraction) the plain decoder finds 6 and the stage's rule, stated on the CPU (tests/block_lib.py walk()),
 * adds most of the rest with no false message, and none on noise (tools/block_rescue_seeds.py prints the table).  No gain
 * is promised beyond that measured table (tools/block_sensitivity.py takes the curve).  A failing candidate costs up to
 * 43 more demodulations and 86 more Fano searches.  The stage is OFF by default, and bench.py measures the default. */
typedef struct {
    int32_t seg;      /* row of the batch */
    float   freq;     /* Hz relative to 1500 Hz, as sync_and_demodulate() takes *freq */
    int32_t shift;    /* samples, jitter included */
    float   drift;    /* Hz over the frame */
} wspr_block_item;
int wspr_block_demod_batch(const float *idat, const float *qdat, int nseg, int samples, size_t seg_stride,
                           const wspr_block_item *items, int n, unsigned char *symbols);
int wspr_set_block_detection(int maxblock);
/* A Doppler-spread figure per spot (kernel K11): how wide the received carrier is once the decode's own modulation has
 * been wiped off -- what FST4W reports with every decode and what users of WSPR spots as an ionospheric probe ask for.
 * The reference has no such figure, so the definition is this library's own (rtlsdr-wsprd_amd/csrc/kernels/spread.h;
 * tests/helpers/spread_check.c is its serial form).  For one job (seg, f0, shift, drift, symbols[162]) over a row of np
 * samples:
 *   1. Phase: phi is the synthesiser's recurrence as stated at wspr_synth_tx above -- phi = 0.0, and for symbol i, sample
 *      j: use phi, then phi += dphi_i, the same double expression with the same f0, drift and symbols; run as written,
 *      not replaced by a prefix sum.  (sn, cs) = the synthesiser's sine and cosine of phi (synth_math.h).
 *   2. Wipe: n = 256 i + j, k = shift + n: zr = (double)I[k]*cs + (double)Q[k]*sn, zi = (double)Q[k]*cs - (double)I[k]*sn,
 *      unfused doubles; both are zero where k < 0 or k >= np.
 *   3. Block sums: y[b], b = 0 .. 1295 = the sum of z over samples 32b .. 32b+31, each rail summed in double in sample
 *      order from 0.0 and rounded once to float.
 *   4. Spectrum: y zero-padded to 2 048 points, complex float32 radix-2 decimation-in-frequency transform with twiddles
 *      (float)cos(2 pi m/2048), (float)(-sin(2 pi m/2048)) from the host libm, no fused multiply-add; P[j] = re*re + im*im
 *      in float, separately rounded, j = -1024 .. 1023 the bin's signed index, bin j at j * D, D = 375/32/2048 Hz
 *      (0.00572 Hz).
 *   5. Width, in double, the order of additions part of the definition: bins in chunks of 16 consecutive j, a chunk
 *      summed serially from 0.0 in rising j, chunk totals accumulated serially in rising chunk order.  nz = the 40 chunks
 *      covering 640 <= |j| <= 959 (negative side first, from j = -959 and from j = 640) / 640.  Signal region j = -512 ..
 *      511 (64 chunks), Q[j] = (double)P[j] - nz, tot = their accumulated total.  For q = 0.25, 0.5, 0.75: the first chunk
 *      whose running total reaches q*tot, in it the first bin whose running sum reaches it, f_q = (j - 0.5 + (q*tot -
 *      C_before)/Q[j]) * D.  w50 = (float)(f_75 - f_25): the width that holds the middle half of the carrier's power;
 *      f50 = (float)f_50: the carrier's median offset from f0; ratio = (float)(largest P[j] of the signal region / nz).
 *      valid = 1 if nz > 0, tot > 0, the three crossings exist and every number involved is finite; otherwise valid = 0
 *      and the three floats are 0.
 * wspr_set_arithmetic() does not touch any of this: it is a measurement, not part of the reference's arithmetic.
 * What to expect: a Gaussian Doppler spectrum of standard deviation s gives w50 = 1.349 s, without bias down to the decode
 * threshold; a carrier that is not spread at all gives the FLOOR of about 0.005 Hz (one bin of the 110.6 s the frame
 * lasts).  ONE SPOT'S FIGURE SCATTERS BY TENS OF PERCENT (about +-30 %: that is 110 s of data, not the estimator), so
 * use medians over spots.  Residual drift -- the decoder's drift is a whole number of Hz per frame -- or a wrong drift
 * estimate widens the figure like a spread does; so does a wrong message (a false decode).
 *
 * wspr_spread_batch(): host rows as wspr_block_demod_batch() takes them and n jobs; out[i] receives job i's figures and
 * echoes its f0 / shift / drift.  A frame may hang off either end of the row, or miss it (valid = 0).  Returns 0; -1 with
 * NOTHING WRITTEN without a usable device, for samples outside 0 .. 45000, n < 0, a seg outside the batch, a symbol > 3,
 * a non-finite f0 or drift, or |f0| + |drift|/2 > 1000 Hz; n == 0 does nothing.
 *
 * wspr_set_spread_estimate(): process-wide, 0 = off (the default), 1 = on; read once per decode call, on entry, like
 * wspr_set_osd_depth().  Returns the previous value; any other argument changes nothing and returns -2.  While it is on,
 * every decode that ADDS A SPOT (not a duplicate, not beyond the 100 uniques, not a loop exit) gets one job, built from
 * the decode's refined freq / shift / drift and the symbols its message re-encodes to (valid = 0 if that fails), and run
 * BEFORE that decode is subtracted: on the IQ the candidate was decoded from, the signal still in it and every earlier
 * subtraction applied.  Spots, hash memory and IQ are what they are with the stage off.
 *
 * wspr_last_spreads(): the records of the calling thread's most recent decode call, in the layout of that call's `decodes`
 * array -- entry s * max_results + i belongs to spot i of segment s (entry i for wspr_decode()); entries beyond
 * n_results[s] are zero.  Returns the number of entries written (nseg * max_results; for wspr_decode(), *n_results), or -1
 * if the stage was off for that call, the capacity is too small, or the call was of a family that does not record them.
 * Recorded: wspr_decode(), wspr_decode_batch(), wspr_decode_batch_device(), wspr_decode_batch_hashed() (a segment decoded
 * again reports its final round's figures) and wspr_selftest().  NOT recorded, -1 afterwards: wspr_decode_batch_node(),
 * wspr_decode_batch_node_device(), wspr_session_decode() and wspr_session_decode_many(), and a call that failed.  The
 * stage is OFF by default, and bench.py measures the default. */
typedef struct {
    int32_t seg;                    /* row of the batch */
    float   f0;                     /* Hz relative to 1500 Hz, centre of the four tones */
    int32_t shift;                  /* row index of the frame's first sample; may be negative */
    float   drift;                  /* Hz over the frame */
    unsigned char symbols[162];     /* channel symbols 0..3 of the message, e.g. from get_wspr_channel_symbols() */
    unsigned char pad[2];
} wspr_spread_item;
typedef struct {
    float   w50, f50, ratio;        /* Hz, Hz, peak over noise floor; all 0 unless valid */
    int32_t valid;
    float   f0;                     /* the job: what the figure was taken with */
    int32_t shift;
    float   drift;
    int32_t pad;
} wspr_spread;
int wspr_spread_batch(const float *idat, const float *qdat, int nseg, int samples, size_t seg_stride,
                      const wspr_spread_item *items, int n, wspr_spread *out);
int wspr_set_spread_estimate(int on);
int wspr_last_spreads(wspr_spread *spreads, int capacity);
/* List decoding against known messages (kernel K14), an opt-in second chance that uses the strongest prior a receiver
 * farm has: the full text of what it decoded in the last hours -- WSPR beacons repeat the same 50 bits slot after slot.
 * Correlating a failed candidate's soft symbols with the code word of every listed message is maximum-likelihood decoding
 * over that list (JT65's "deep search", FT8's a-priori decoding).  The reference has nothing of the kind, so the definition
 * is this library's own (rtlsdr-wsprd_amd/csrc/kernels/listmatch.h; tests/helpers/list_check.c is its serial form), all
 * of it integer:
 *   entry    a message text that get_wspr_channel_symbols() encodes on an empty hash memory and whose 11-byte decdata (as
 *            fano() leaves it; obtained by decoding the noise-free code word) unpacks on an empty hash memory, WITHOUT a hash
 *            look-up, to a canonical text that encodes to the same 162 symbols: message types 1 and 2 ("K1JT FN20 0" is
 *            held as "K1JT FN20 00"); a type-3 text "<...>" is refused.  c[i] = 2 * (symbols[i] >> 1) - 1, i = 0 .. 161 in
 *            transmission (interleaved) order; nothing is deinterleaved in this stage.
 *   vector   162 soft symbols s[i] in transmission order, as wspr_fano_batch_device_wave() and wspr_osd_batch_device() take
 *            them; v[i] = 2 s[i] - 255 (odd, never 0: the reliabilities of the ordered-statistics stage, signed).
 *   score    S(m) = sum of c_m[i] * v[i] (int32) = R - 2 D, R = sum |v[i]|, D = the ordered-statistics cost of that code word.
 *   winner   the largest S, ties to the lower list index; second = the largest S among all OTHER entries (INT32_MIN for a
 *            list of one); V = sum of v[i]^2 (at most 10 534 050).
 *   gate     accepted iff S1 > 0 and 256 * S1^2 >= zmin16^2 * V (int64): z = S1 / sqrt(V) >= zmin16 / 16.  z cannot exceed
 *            sqrt(162) = 12.73, hence zmin16 = 1 .. 203.
 *
 * wspr_set_message_list(): process-wide, off by default.  messages[0 .. n) are the texts; n == 0 or messages == NULL
 * switches the stage off (returns 0).  Entries whose 50 bits repeat an earlier entry are dropped, the first occurrence
 * kept; returns the number of entries KEPT.  Returns -1 with a line on stderr naming the first offending index and CHANGES
 * NOTHING (the list in force stays in force) for a text that does not qualify, n < 0, n > WSPR_LIST_MAX or zmin16 outside
 * 1 .. 203.  A decode call reads the list once, on entry, as an immutable snapshot (like wspr_set_osd_depth(); the worker
 * threads of a node-level call inherit it), so the setter may run beside decode calls; a WSPR_HASH_REVISIT call must run
 * under the list (the very wspr_set_message_list() call) and zmin16 of the call it completes, and is refused otherwise.
 * Every device context uploads the table (196 bytes per entry) on first use and replaces it when the list changes.
 * wspr_message_list_entry(): what entry `index` of the list in force holds -- canonical text, decdata, channel symbols (any
 * of the three may be NULL); -1 outside the list or with no list.
 * wspr_list_match_batch_device(): K14 for n host vectors of 162 soft symbols against the list in force; out[i] = (winner,
 * S1, second, V) of vector i, the gate left to the caller.  Returns 0; -1 with NOTHING WRITTEN without a usable device,
 * without a list or for n < 0; n == 0 does nothing.
 *
 * While a list is set, every decode call runs the stage:
 *   - the Fano budget split (wspr_set_fano_fast_budget) is off for the call -- results never depended on it;
 *   - every candidate that was worth the jitter ladder (sync > minsync1) and decoded on none of its rungs -- nor in the
 *     block-detection stage if that is on -- has its FIRST (rung-0) soft-symbol vector matched against the list.  The
 *     sync/rms gate of wsprd.c:758 is NOT applied (it would remove about a third of the candidates this stage can use);
 *     the list gate above replaces it and is decided at once, without a hash look-up;
 *   - the stage runs AFTER the block-detection stage and BEFORE the ordered-statistics stage, which sees what it left;
 *   - an accepted candidate is a decode like any other -- spot, hash store, subtraction, de-duplication, loop exits,
 *     spread job -- reported with jitter 0 and CYCLES 1: the Fano search never reports fewer than 81 cycles and 0 marks an
 *     ordered-statistics spot, so cycles == 1 marks a list spot.
 * What to expect.  The stage reports ONLY listed messages, and what it reports is the list's text: A LISTED STATION THAT
 * CHANGED ITS POWER (same call and locator, another dBm figure: code words that differ only through the last message
 * bits) CAN BE REPORTED WITH ITS LISTED POWER.  Measured on one MI355X (tools/list_sensitivity.py, profiles/
 * list_sensitivity.json; 2 048 synthetic single-signal segments per point, 8 192 entries): with the sent message absent and
 * only that neighbour listed, 3 of the 1 041 vectors matched at -30 dB were reported as the neighbour at zmin16 = 96 (15 at
 * 88, 1 at 104), none at -27 dB, where Fano decodes the true message.  With the sent messages listed the decoded share at
 * zmin16 = 96 goes from 0.00 / 0.05 / 0.43 / 0.86 (stage off) to 0.33 / 0.76 / 0.92 / 0.93 at -32 / -31 / -30 / -29 dB,
 * the same for 512 and 8 192 entries; the call's time does not change beyond its scatter, and K14 alone takes 0.15 ms for
 * 2 048 vectors x 8 192 entries, 0.89 ms x 65 536.
 * Recommended zmin16: 96 (z >= 6.0).  The Gaussian bound on a false accept per matched vector is M * Q(6.0) = 6e-5 for a
 * full list of M = 65 536 entries; measured against that bound for the run's own M x vectors: noise alone 0 spots (1
 * vector), unlisted messages 0 spots on 1 013 vectors (bound 0.008), a crowded scene of strong listed signals 0 on 68 (bound
 * 0.0005) -- at 88 and 104 alike, so 96 stands.  The power confusion above is no noise event (the code words share all but
 * the last message bits) and no tested threshold brings it under that bound: keep the list current.  The stage is OFF by
 * default, and bench.py measures the default. */
#define WSPR_LIST_MAX 65536
typedef struct { int32_t index, score, second, v2; } wspr_list_match;   /* winner, S1, S2, V */
int wspr_set_message_list(const char *const *messages, int n, int zmin16);
int wspr_message_list_entry(int index, char text[23], unsigned char decdata[11], unsigned char symbols[162]);
int wspr_list_match_batch_device(const unsigned char *symbols, int n, wspr_list_match *out);
/* Decode-quality figures and provenance per spot (kernel K19): which pass and which stage made a spot, and how well the
 * soft-symbol vector that decoded agrees with the code word it decoded to -- what the extended spot tables of receiver
 * farms carry besides sync, dt, drift, cycles and jitter, and what a farm filters false spots by before upload.  The
 * reference reports none of this, so the definition is this library's own (rtlsdr-wsprd_amd/csrc/kernels/spot_quality.h;
 * tests/helpers/spot_quality_check.c is its serial form), all of it integer.  THE FIGURES DESCRIBE THE VECTOR THAT DECODED,
 * NOT THE CHANNEL.  A job is one vector of 162 soft symbols s[i] in transmission (interleaved) order, as
 * wspr_fano_batch_device_wave() and wspr_osd_batch_device() take them, plus decdata[11] as fano() leaves it:
 *   code word  c[i] in {0, 1}, i = 0 .. 161 in transmission order: the data bits of the code word that encode() +
 *              interleave() make of the 50 message bits of decdata followed by 31 zero tail bits (whatever decdata holds
 *              beyond bit 49 is not read).  The code word, not a re-encoding of the unpacked text: it exists for every decode
 *              and needs no hash memory.
 *   h, v, r    h[i] = (s[i] >= 128), v[i] = 2 s[i] - 255, r[i] = |v[i]|: the conventions of the ordered-statistics and of
 *              the list stage.
 *   nhard      the number of i with h[i] != c[i]: the hard errors.
 *   dist       the sum of r[i] over those i.  For the winner of wspr_osd_batch_device() these two are its nhard and dist.
 *   rsum       the sum of r[i] over all i.  rsum - 2 * dist is the score of that code word in wspr_list_match.
 *   v2         the sum of v[i]^2: v2 of wspr_list_match.
 *   metric     the sum over i of mettab[c[i]][s[i]] (int32), mettab = wspr_fano_metric_table(): the PATH METRIC.  For a vector
 *              on which fano() succeeds it is what fano() returns in *metric, that unsigned word read as int32 (gamma is
 *              signed inside the search; a decode through many wrong symbols ends below zero).
 * wspr_spot_quality_batch_device(): K19 for n host vectors (n x 162 bytes) and their n x 11 bytes of decdata; out[i] = the
 * figures of job i.  Returns 0; -1 with NOTHING WRITTEN without a usable device, for n < 0 or a missing array; n == 0 does
 * nothing.  wspr_set_arithmetic() does not touch any of this.
 *
 * wspr_set_spot_details(): process-wide, 0 = off (the default), 1 = on; read once per decode call, on entry, like
 * wspr_set_spread_estimate().  Returns the previous value; any other argument changes nothing and returns -2.  While it is
 * on, every decode that ADDS A SPOT (not a duplicate, not beyond the 100 uniques, not a loop exit) gets one job, built on
 * the vector that decoded it -- the rung's vector for a decode of the jitter ladder, the (block size, rung) vector for a
 * decode of the block-detection stage, the FIRST (rung-0) vector for a list or an ordered-statistics decode -- read where it
 * lies in device memory and queued behind the wave without a host wait.  Spots, hash memory, IQ and every other output are
 * byte for byte what they are with the stage off; it works together with wspr_set_spread_estimate().
 *
 * wspr_last_spot_details(): the records of the calling thread's most recent decode call, in the layout of that call's
 * `decodes` array, exactly as wspr_last_spreads() hands out its records -- entry s * max_results + i belongs to spot i of
 * segment s (entry i for wspr_decode()); entries beyond n_results[s] are zero.  Returns the number of entries written
 * (nseg * max_results; for wspr_decode(), *n_results), or -1 if the stage was off for that call, the capacity is too small,
 * or the call was of a family that does not record them.  Recorded: wspr_decode(), wspr_decode_batch(),
 * wspr_decode_batch_device(), wspr_decode_batch_hashed() (a segment decoded again reports its final round's records) and
 * wspr_selftest().  NOT recorded, -1 afterwards: wspr_decode_batch_node(), wspr_decode_batch_node_device(),
 * wspr_session_decode() and wspr_session_decode_many(), and a call that failed.  The stage is OFF by default, and bench.py
 * measures the default. */
typedef struct {
    int32_t nhard, dist, rsum, v2, metric;
} wspr_spot_quality;                /* 20 bytes */
typedef struct {
    int32_t nhard, dist, rsum, v2, metric;   /* the figures of the vector that decoded; all 0 unless valid */
    uint8_t pass;                   /* the decode pass, 0-based */
    uint8_t stage;                  /* WSPR_STAGE_*: which stage made the decode */
    uint8_t block;                  /* block size of the demodulation: 1, or 2 / 3 for the block-detection stage */
    uint8_t valid;                  /* 1 once the figures are filed */
    int32_t cand;                   /* index in that pass's candidate list (strongest first) */
    int32_t pad;
} wspr_spot_detail;                 /* 32 bytes */
#define WSPR_STAGE_LADDER 1         /* the reference's own decode: a rung of the jitter ladder */
#define WSPR_STAGE_BLOCK2 2         /* block detection, block size 2 */
#define WSPR_STAGE_BLOCK3 3         /* block detection, block size 3 */
#define WSPR_STAGE_LIST   4         /* list decoding */
#define WSPR_STAGE_OSD    5         /* ordered-statistics decoding */
int wspr_spot_quality_batch_device(const unsigned char *symbols, const unsigned char *decdata, int n,
                                   wspr_spot_quality *out);
int wspr_set_spot_details(int on);
int wspr_last_spot_details(wspr_spot_detail *details, int capacity);
/* The "Spot : ..." line of wspr_format_spot() followed by six columns of the spot's record, each after one blank:
 *   pass (%1d)  stage (%1d, WSPR_STAGE_*)  block (%1d)  nhard (%3d)  dist (%5d)  metric (%6d)
 * e.g. "Spot : -21.04   0.11  14.097100  0  K1JT   FN20 20 0 1 1  23  1467   4012".  The project's own format: it does not
 * claim to be the layout of any other program's spot file.  Returns what snprintf() returns: the length of the whole line,
 * of which at most cap - 1 characters and the terminating NUL were written.  Host code: needs no device. */
int wspr_format_spot_extended(const struct decoder_results *r, const wspr_spot_detail *d, char *out, size_t cap);
/* Library / device description, e.g. for bench logs. */
const char *wspr_mi355x_version(void);
int wspr_device_ready(void);        /* 1 if a HIP device and the kernels are usable */

/* ---- message layer, same names as the reference exports ------------------- */
/* reference wsprd/wsprsim_utils.h:1-9 */
char get_locator_character_code(char ch);
char get_callsign_character_code(char ch);
long unsigned int pack_grid4_power(char const *grid4, int power);
long unsigned int pack_call(char const *callsign);
void pack_prefix(char *callsign, int32_t *n, int32_t *m, int32_t *nadd);
void interleave(unsigned char *sym);
int  get_wspr_channel_symbols(char *message, char *hashtab, char *loctab, unsigned char *symbols);
/* reference wsprd/wsprd_utils.h:32-42 */
void unpack50(signed char *dat, int32_t *n1, int32_t *n2);
int  unpackcall(int32_t ncall, char *call);
int  unpackgrid(int32_t ngrid, char *grid);
int  unpackpfx(int32_t nprefix, char *call);
void deinterleave(unsigned char *sym);
int  doublecomp(const void *elem1, const void *elem2);
int  floatcomp(const void *elem1, const void *elem2);
int  unpk_(signed char *message, char *hashtab, char *loctab, char *call_loc_pow, char *call,
           char *loc, char *pwr, char *callsign);
/* reference wsprd/fano.h:14-28 */
int  fano(unsigned int *metric, unsigned int *cycles, unsigned int *maxnp, unsigned char *data,
          unsigned char *symbols, unsigned int nbits, int mettab[2][256], int delta,
          unsigned int maxcycles);
int  encode(unsigned char *symbols, unsigned char *data, unsigned int nbytes);
extern unsigned char Partab[];
/* reference wsprd/nhash.h:3 */
uint32_t nhash(const void *key, size_t length, uint32_t initval);
/* The soft-decision metric tables, reference wsprd/metric_tables.h:8 (a data symbol of the reference's wsprd.o;
 * rows = Es/No 0, 3, 6, 9 dB and a fifth row whose last eight entries are uninitialised-memory values in the
 * reference source -- kept as they are).  wspr_decode uses row 2 only (wsprd.c:471-472). */
extern float metric_tables[5][256];
/* the integer branch-metric table wspr_decode derives at wsprd/wsprd.c:467-473 */
void wspr_fano_metric_table(int mettab[2][256]);

#ifdef __cplusplus
}
#endif
#endif /* WSPR_MI355X_H */
