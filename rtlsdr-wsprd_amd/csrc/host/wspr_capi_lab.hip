// C ABI of libwspr_mi355x_lab.so only (declared in include/wspr_mi355x_bench.h): stage-level parity hooks, kernel
// timings, calibration kernels and the front end's CU share.  Empty in the product build.
#ifdef WSPR_LAB
#include <cstdint>
#include <cstring>
#include <cmath>
#include <exception>
#include <stdexcept>
#include <vector>

#include "wspr_capi_impl.h"
#include "wspr_context_impl.h"

using wspr::Context;
using namespace wspr::capi;

extern "C" {

int wspr_stage_fft_bank(const float* idat, const float* qdat, int nseg, int samples, size_t seg_stride,
                        float* ps_out) {
    LaneTurn lane_turn;
    try {
        Context& c = Context::get();
        const int blocks = 4 * (samples / wspr::kFftSize) - 1;
        c.load_host(idat, qdat, nseg, samples, seg_stride);
        float* ps = c.ps_buffer(nseg);
        wspr::launch_fft_bank(c.work_i(nseg), c.work_q(nseg), nullptr, nseg, samples, ps, c.tables(), c.stream(),
                              wspr::call_arith());
        std::vector<float> h((size_t)nseg * wspr::kPsBins * wspr::kPsTPitch);
        HIP_TRY(hipMemcpyAsync(h.data(), ps, h.size() * 4, hipMemcpyDeviceToHost, c.stream()));
        c.sync();
        memset(ps_out, 0, (size_t)nseg * wspr::kFftSize * blocks * sizeof(float));
        for (int s = 0; s < nseg; ++s)
            for (int t = 0; t < blocks; ++t)
                for (int b = 0; b < wspr::kPsBins; ++b)
                    ps_out[((size_t)s * wspr::kFftSize + (b + wspr::kPsBin0)) * blocks + t] =
                        h[((size_t)s * wspr::kPsBins + b) * wspr::kPsTPitch + t];
        return blocks;
    } catch (const std::exception& e) { return fail("wspr_stage_fft_bank", e); }
}

int wspr_stage_candidates(const float* idat, const float* qdat, int nseg, int samples, size_t seg_stride,
                          int coarse, int maxdrift, struct cand* cand_out, int* npk_out, float* noise_out,
                          float* smspec_out) {
    LaneTurn lane_turn;
    try {
        Context& c = Context::get();
        c.load_host(idat, qdat, nseg, samples, seg_stride);
        TempDev t_noise((size_t)nseg * 4), t_sm((size_t)nseg * wspr::kSmooth * 4);
        float *d_noise = t_noise.as<float>(), *d_sm = t_sm.as<float>();
        c.run_fft_sync(nseg, samples, maxdrift, coarse != 0, nullptr, nseg, d_noise, d_sm);
        std::vector<int> npk;
        std::vector<wspr::DevCand> cd;
        c.fetch_candidates(nseg, npk, cd);
        if (noise_out) HIP_TRY(hipMemcpy(noise_out, d_noise, (size_t)nseg * 4, hipMemcpyDeviceToHost));
        if (smspec_out) HIP_TRY(hipMemcpy(smspec_out, d_sm, (size_t)nseg * wspr::kSmooth * 4, hipMemcpyDeviceToHost));
        for (int s = 0; s < nseg; ++s) {
            npk_out[s] = npk[s];
            for (int j = 0; j < wspr::kMaxCand; ++j) {
                struct cand o = {0, 0, 0, 0, 0};
                if (j < npk[s]) {
                    const wspr::DevCand& v = cd[(size_t)s * wspr::kMaxCand + j];
                    o.freq = v.freq; o.snr = v.snr; o.shift = v.shift; o.drift = v.drift; o.sync = v.sync;
                }
                cand_out[(size_t)s * wspr::kMaxCand + j] = o;
            }
        }
        return 0;
    } catch (const std::exception& e) { return fail("wspr_stage_candidates", e); }
}

int wspr_stage_candidates_ps(const float* ps, int nseg, int blocks, int coarse, int maxdrift, const int* active, int nactive,
                             const float* cand_freq, const int* cand_n, int k3_kernel, struct cand* cand_out, int* npk_out,
                             float* noise_out, float* smspec_out) {
    LaneTurn lane_turn;
    try {
        if (!ps || !cand_out || !npk_out || nseg < 1 || blocks < 1 || blocks > wspr::kMaxBlocks || maxdrift < 0 ||
            k3_kernel < 0 || k3_kernel > 2 || (active && (nactive < 0 || nactive > nseg)) || (!cand_freq != !cand_n))
            throw std::invalid_argument("argument out of range");
        Context& c = Context::get();
        Context::Impl& d = *c.d;
        const size_t seg_floats = (size_t)wspr::kPsBins * wspr::kPsTPitch;
        // the device layout with every float it does not define set to NaN (all bits one): the pitch columns and, in a
        // short record, the columns from `blocks` on
        std::vector<float> h((size_t)nseg * seg_floats);
        memset(h.data(), 0xff, h.size() * 4);
        for (int s = 0; s < nseg; ++s)
            for (int b = 0; b < wspr::kPsBins; ++b)
                memcpy(h.data() + (size_t)s * seg_floats + (size_t)b * wspr::kPsTPitch,
                       ps + ((size_t)s * wspr::kFftSize + (b + wspr::kPsBin0)) * blocks, (size_t)blocks * 4);
        // the lists as the picker leaves them (shift, drift and sync zero); the peaks fall by a factor of two from one
        // candidate to the next, so that the host re-rank of fetch_candidates() keeps the caller's order
        std::vector<wspr::DevCand> hc;
        std::vector<int> hn;
        if (cand_freq) {
            wspr::DevCand none;
            memset(&none, 0xff, sizeof none);
            hc.assign((size_t)nseg * wspr::kMaxCand, none);
            hn.assign(cand_n, cand_n + nseg);
            for (int s = 0; s < nseg; ++s) {
                if (hn[s] < 0 || hn[s] > wspr::kMaxCand) throw std::invalid_argument("candidate count out of range");
                for (int j = 0; j < hn[s]; ++j) {
                    wspr::DevCand& v = hc[(size_t)s * wspr::kMaxCand + j];
                    v.freq = cand_freq[(size_t)s * wspr::kMaxCand + j];
                    const int if0 = (int)((double)v.freq / (375.0 / 256.0 / 2.0) + 256.0);     // as K3 derives it
                    // K3 stages bins if0 - 6 .. if0 + 4 and the spectrogram holds bins 100 .. 410 for it (the picker's
                    // +-110 Hz window): nothing outside may be asked for
                    if (!(if0 >= 106 && if0 <= 406)) throw std::invalid_argument("candidate outside the picker's window");
                    v.peak = exp2f((float)(100 - j));
                    v.snr = (float)(10.0 * (double)log10f(v.peak) - (double)26.3f);
                    v.shift = 0; v.drift = 0.0f; v.sync = 0.0f;
                    v.bin = if0 - 51;
                }
            }
        }
        std::vector<int> act;
        if (active) {
            act.assign(active, active + nactive);
            for (int s : act) if (s < 0 || s >= nseg) throw std::invalid_argument("active segment out of range");
        }
        const int nact = active ? nactive : nseg;

        float* d_ps = c.ps_buffer(nseg);
        wspr::DevCand* d_cand = static_cast<wspr::DevCand*>(d.cand.need((size_t)nseg * wspr::kMaxCand * sizeof(wspr::DevCand)));
        int* d_npk = static_cast<int*>(d.npk.need((size_t)nseg * 4));
        float* d_avg = static_cast<float*>(d.psavg.need((size_t)nseg * wspr::kPsStride * 4));
        TempDev t_noise((size_t)nseg * 4), t_sm((size_t)nseg * wspr::kSmooth * 4), t_act((size_t)std::max(nact, 1) * 4);
        float *d_noise = t_noise.as<float>(), *d_sm = t_sm.as<float>();
        int* d_act = active ? t_act.as<int>() : nullptr;
        hipStream_t st = c.stream();
        HIP_TRY(hipMemcpyAsync(d_ps, h.data(), h.size() * 4, hipMemcpyHostToDevice, st));
        // what a segment outside the active list keeps: an empty list and NaN noise / smspec, or the caller's list untouched
        HIP_TRY(hipMemsetAsync(d_avg, 0xff, (size_t)nseg * wspr::kPsStride * 4, st));
        HIP_TRY(hipMemsetAsync(d_noise, 0xff, (size_t)nseg * 4, st));
        HIP_TRY(hipMemsetAsync(d_sm, 0xff, (size_t)nseg * wspr::kSmooth * 4, st));
        if (cand_freq) {
            HIP_TRY(hipMemcpyAsync(d_cand, hc.data(), hc.size() * sizeof(wspr::DevCand), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_npk, hn.data(), (size_t)nseg * 4, hipMemcpyHostToDevice, st));
        } else {
            HIP_TRY(hipMemsetAsync(d_cand, 0xff, (size_t)nseg * wspr::kMaxCand * sizeof(wspr::DevCand), st));
            HIP_TRY(hipMemsetAsync(d_npk, 0, (size_t)nseg * 4, st));
        }
        if (active && nact > 0) HIP_TRY(hipMemcpyAsync(d_act, act.data(), (size_t)nact * 4, hipMemcpyHostToDevice, st));
        if (!cand_freq) {
            wspr::launch_time_average(d_ps, d_act, nact, blocks, d_avg, st);
            wspr::launch_pick_peaks(d_ps, d_act, nact, blocks, d_avg, d_cand, d_npk, d_noise, d_sm, c.tables(), st, true);
        }
        if (coarse) wspr::launch_coarse_sync(d_ps, d_act, nact, blocks, d_cand, d_npk, maxdrift, c.tables(), st, k3_kernel);
        std::vector<int> npk;
        std::vector<wspr::DevCand> cd;
        c.fetch_candidates(nseg, npk, cd);
        if (noise_out) HIP_TRY(hipMemcpy(noise_out, d_noise, (size_t)nseg * 4, hipMemcpyDeviceToHost));
        if (smspec_out) HIP_TRY(hipMemcpy(smspec_out, d_sm, (size_t)nseg * wspr::kSmooth * 4, hipMemcpyDeviceToHost));
        for (int s = 0; s < nseg; ++s) {
            npk_out[s] = npk[s];
            for (int j = 0; j < wspr::kMaxCand; ++j) {
                struct cand o = {0, 0, 0, 0, 0};
                if (j < npk[s]) {
                    const wspr::DevCand& v = cd[(size_t)s * wspr::kMaxCand + j];
                    o.freq = v.freq; o.snr = v.snr; o.shift = v.shift; o.drift = v.drift; o.sync = v.sync;
                }
                cand_out[(size_t)s * wspr::kMaxCand + j] = o;
            }
        }
        return 0;
    } catch (const std::exception& e) { return fail("wspr_stage_candidates_ps", e); }
}

int wspr_bench_fft_sync(const void* d_idat, const void* d_qdat, int nseg, int samples, size_t seg_stride, int iters,
                        double* ms) {
    LaneTurn lane_turn;
    try {
        Context& c = Context::get();
        c.load_device(d_idat, d_qdat, nseg, samples, seg_stride);
        return c.bench_fft_sync(nseg, samples, iters, ms);
    } catch (const std::exception& e) { return fail("wspr_bench_fft_sync", e); }
}

int wspr_bench_valu(const void* d_idat, const void* d_qdat, int nseg, int samples, size_t seg_stride, int iters,
                    double* ms) {
    LaneTurn lane_turn;
    try {
        Context& c = Context::get();
        c.load_device(d_idat, d_qdat, nseg, samples, seg_stride);
        // WSPR_BENCH_LAG_DRIFT (a measurement switch): before the stages below, the mode-0 lag scan of up to 2 048 drifting
        // candidates of the batch as launch sets alone -> ms[5] = whole scan, ms[6] = pruned scan (ms), ms[7] = candidates
        double dr[6] = {0};
        const bool drift_sets = wspr::lab_env("WSPR_BENCH_LAG_DRIFT") != nullptr;
        if (drift_sets) c.bench_lag_drift(nseg, samples, dr);
        const int r = c.bench_valu(nseg, samples, iters, ms);
        if (drift_sets) { ms[5] = dr[0]; ms[6] = dr[1]; ms[7] = dr[2]; }
        return r;
    } catch (const std::exception& e) { return fail("wspr_bench_valu", e); }
}

int wspr_calib_copy(const void* d_src, void* d_dst, size_t nfloats, int iters) {
    try {
        Context& c = Context::get();
        for (int i = 0; i < iters; ++i) wspr::launch_calib_copy((const float*)d_src, (float*)d_dst, nfloats, c.stream());
        c.sync();
        return 0;
    } catch (const std::exception& e) { return fail("wspr_calib_copy", e); }
}

int wspr_calib_copy16(const void* d_src, void* d_dst, size_t nfloats, int iters, int variant, double* ms) {
    try {
        if ((nfloats & 3) || ((uintptr_t)d_src & 15) || ((uintptr_t)d_dst & 15)) return -1;
        Context& c = Context::get();
        hipEvent_t e0, e1;
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, c.stream()));
        for (int i = 0; i < iters; ++i) wspr::launch_calib_copy16((const float*)d_src, (float*)d_dst, nfloats, c.stream(), variant);
        HIP_TRY(hipEventRecord(e1, c.stream()));
        HIP_TRY(hipEventSynchronize(e1));
        float t = 0;
        HIP_TRY(hipEventElapsedTime(&t, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        if (ms) *ms = iters > 0 ? t / iters : 0.0;
        return 0;
    } catch (const std::exception& e) { return fail("wspr_calib_copy16", e); }
}

int wspr_calib_valu(int launches, double* tflops) {
    try {
        Context& c = Context::get();
        TempDev out(64);
        hipEvent_t e0, e1;
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        wspr::launch_calib_valu((float*)out.p, 256, c.stream());                  // settle the clocks
        HIP_TRY(hipEventRecord(e0, c.stream()));
        double flops = 0;
        for (int i = 0; i < launches; ++i) flops += wspr::launch_calib_valu((float*)out.p, 2048, c.stream());
        HIP_TRY(hipEventRecord(e1, c.stream()));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        if (tflops) *tflops = flops / (ms * 1e-3) / 1e12;
        return 0;
    } catch (const std::exception& e) { return fail("wspr_calib_valu", e); }
}

int wspr_set_front_end_cus(int ncus) {
    return wspr::front_end_cus().exchange(ncus < 0 ? 0 : ncus);
}

void wspr_fano_host_handovers(unsigned long long* on_pool, unsigned long long* one_by_one) {
    if (on_pool) *on_pool = wspr::fano_handovers(0).load();
    if (one_by_one) *one_by_one = wspr::fano_handovers(1).load();
}

int wspr_bench_decimate(const void* d_raw, size_t bytes_per_seg, int nseg, void* d_idat, void* d_qdat, int iters,
                        double* ms) {
    LaneTurn lane_turn;
    try {
        return Context::get().bench_decimate(d_raw, bytes_per_seg, nseg, (float*)d_idat, (float*)d_qdat, iters, ms);
    } catch (const std::exception& e) { return fail("wspr_bench_decimate", e); }
}

int wspr_calib_read(const void* d_raw, size_t bytes_per_seg, int nseg, int iters, double* ms) {
    try {
        return Context::get().bench_decimate(d_raw, bytes_per_seg, nseg, nullptr, nullptr, iters, ms);
    } catch (const std::exception& e) { return fail("wspr_calib_read", e); }
}

}  // extern "C"
#endif  // WSPR_LAB
