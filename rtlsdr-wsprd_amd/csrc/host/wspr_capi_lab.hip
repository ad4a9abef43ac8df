// C ABI of libwspr_mi355x_lab.so only (declared in include/wspr_mi355x_bench.h): stage-level parity hooks, kernel
// timings, calibration kernels and the front end's CU share.  Empty in the product build.
#ifdef WSPR_LAB
#include <cstdint>
#include <cstring>
#include <exception>
#include <vector>

#include "wspr_capi_impl.h"

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
        return c.bench_valu(nseg, samples, iters, ms);
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
