// Driver of tests/test_gpu_lag_coarse.py: runs the mode-0 lag scan of a case file through the PRODUCTION launchers, once
// with the lag pruning (and lag_coarse_kernel's audit output) and once as the whole scan, and dumps every buffer.  It
// judges nothing: the assertions live in the test (tests/lag_audit_lib.py describes both file formats).  Exit status: 0,
// 1 = a HIP error (nothing is started after one), 2 = the case file is unusable.  Includes the kernel file itself.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -I rtlsdr-wsprd_amd/csrc/kernels tools/lagprune_check.hip -o tools/lagprune_check.bin
//
// Case file (little endian): int32 magic 0x3143504c, nseg, nruns; 164 bytes: the sync vector (162) + 2 of padding;
// float I[nseg][kIqStride], Q[nseg][kIqStride]; then per run: int32 np, arith, nitems, n_shared, n_own;
// FineState items[nitems] (pad is set here: item i reads table i); int32 list_shared[n_shared], list_own[n_own].
// Output file, per run: int32 nitems, n_shared, n_own, scratch_bytes; float tabs[nitems][2048]; FineState after A, after B;
// float sync_A[nitems][33], sync_B; float pw_A[nitems][33][162][4], pw_B; the pruning's scratch (masks: nitems x 8 bytes,
// exact list: 4 n_shared ints, fallback list: n_shared ints); int32 counts[4]; float audit[nitems][33][7].
// With a third argument "drift" the pruned run also prunes the drifting candidates (LagPrune::drift) and every run's dump
// ends with int32 counts[4..7] (drifting candidates: exact evaluations, fallbacks, pruned, unused); their lists are in the
// scratch dump behind the drift-free ones (lag_prune_scratch_bytes() in k4_lag_prune.h gives the layout).
// Every output buffer starts as bytes of 0xa5 (as a float: -2.87e-16), so what no kernel wrote can be told.
#include "../rtlsdr-wsprd_amd/csrc/kernels/k4_demod.hip"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace wspr;
#define OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
#define NEED(c) do { if (!(c)) { fprintf(stderr, "case file: %s (line %d)\n", #c, __LINE__); return 2; } } while (0)

constexpr int kSentinel = 0xa5;

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool wr(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

// device buffer -> output file
static int dump(FILE* out, const void* dev, size_t bytes, std::vector<char>& host) {
    host.resize(bytes);
    OK(hipMemcpy(host.data(), dev, bytes, hipMemcpyDeviceToHost));
    if (!wr(out, host.data(), bytes)) { fprintf(stderr, "short write\n"); return 2; }
    return 0;
}
#define DUMP(dev, bytes) do { const int r_ = dump(out, dev, bytes, host); if (r_) return r_; } while (0)

int main(int argc, char** argv) {
    if (argc != 3 && !(argc == 4 && !strcmp(argv[3], "drift"))) { fprintf(stderr, "usage: %s case.bin out.bin [drift]\n", argv[0]); return 2; }
    const bool drift = argc == 4;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    NEED(in && out);
    int head[3];
    unsigned char pr3[164];
    NEED(rd(in, head, sizeof head) && rd(in, pr3, sizeof pr3));
    const int nseg = head[1], nruns = head[2];
    NEED(head[0] == 0x3143504c && nseg >= 1 && nseg <= 8 && nruns >= 1 && nruns <= 16);
    const size_t niq = (size_t)nseg * kIqStride;
    std::vector<float> I(niq), Q(niq);
    NEED(rd(in, I.data(), niq * 4) && rd(in, Q.data(), niq * 4));

    float *dI, *dQ;
    unsigned char* dpr3;
    OK(hipMalloc(&dI, niq * 4)); OK(hipMalloc(&dQ, niq * 4)); OK(hipMalloc(&dpr3, sizeof pr3));
    OK(hipMemcpy(dI, I.data(), niq * 4, hipMemcpyHostToDevice)); OK(hipMemcpy(dQ, Q.data(), niq * 4, hipMemcpyHostToDevice));
    OK(hipMemcpy(dpr3, pr3, sizeof pr3, hipMemcpyHostToDevice));
    DeviceTables t{};
    t.sync = dpr3;
    std::vector<char> host;

    for (int run = 0; run < nruns; ++run) {
        int rh[5];
        NEED(rd(in, rh, sizeof rh));
        const int np = rh[0], arith = rh[1], n = rh[2], n_shared = rh[3], n_own = rh[4];
        NEED(np >= 1 && np <= kMaxSamples && (arith == 0 || arith == 1) && n >= 1 && n <= 256);
        NEED(n_shared >= 1 && n_own >= 0 && n_shared + n_own <= n);
        std::vector<FineState> items(n);
        std::vector<int> lists(n_shared + n_own);
        NEED(rd(in, items.data(), (size_t)n * sizeof(FineState)) && rd(in, lists.data(), lists.size() * 4));
        std::vector<char> seen(n, 0);
        for (size_t i = 0; i < lists.size(); ++i) {             // every entry an item, none twice, drift as its list says
            const int it = lists[i];
            NEED(it >= 0 && it < n && !seen[it]);
            seen[it] = 1;
            NEED((items[it].drift == 0.0f) == (i < (size_t)n_shared));
        }
        for (int i = 0; i < n; ++i) {
            NEED(items[i].seg >= 0 && items[i].seg < nseg && items[i].shift_coarse > -100000 && items[i].shift_coarse < 100000);
            items[i].pad = i;
        }

        const size_t nrow = (size_t)n * kLpLags, pw_bytes = nrow * kNSymD * 16, scratch_bytes = lag_prune_scratch_bytes(n);
        const size_t audit_bytes = nrow * kLpAuditStride * 4, tab_bytes = (size_t)n * 2048 * 4;
        FineState *itA, *itB;
        int *dls, *dlo, *counts;
        float *tabs, *pwA, *pwB, *syA, *syB, *audit;
        void* scratch;
        OK(hipMalloc(&itA, n * sizeof(FineState))); OK(hipMalloc(&itB, n * sizeof(FineState)));
        OK(hipMalloc(&dls, lists.size() * 4 + 4)); OK(hipMalloc(&counts, 32)); OK(hipMalloc(&tabs, tab_bytes));
        OK(hipMalloc(&pwA, pw_bytes)); OK(hipMalloc(&pwB, pw_bytes)); OK(hipMalloc(&syA, nrow * 4)); OK(hipMalloc(&syB, nrow * 4));
        OK(hipMalloc(&audit, audit_bytes)); OK(hipMalloc(&scratch, scratch_bytes));
        dlo = dls + n_shared;
        OK(hipMemcpy(itA, items.data(), n * sizeof(FineState), hipMemcpyHostToDevice));
        OK(hipMemcpy(itB, items.data(), n * sizeof(FineState), hipMemcpyHostToDevice));
        OK(hipMemcpy(dls, lists.data(), lists.size() * 4, hipMemcpyHostToDevice));
        OK(hipMemset(tabs, kSentinel, tab_bytes)); OK(hipMemset(pwA, kSentinel, pw_bytes)); OK(hipMemset(pwB, kSentinel, pw_bytes));
        OK(hipMemset(syA, kSentinel, nrow * 4)); OK(hipMemset(syB, kSentinel, nrow * 4)); OK(hipMemset(audit, kSentinel, audit_bytes));
        OK(hipMemset(scratch, kSentinel, scratch_bytes)); OK(hipMemset(counts, kSentinel, 32));
        OK(hipDeviceSynchronize());

        // A: the pruned scan, as wspr_pipeline.hip runs it, with the audit output
        LagPrune prune{scratch, counts, nullptr, audit};
        prune.drift = drift;
        OK(hipMemsetAsync(counts, 0, (drift ? 8 : 4) * 4, 0));
        launch_phasor_tables(itA, n, 0, tabs, 0, arith);
        launch_demod_tiled(dI, dQ, np, itA, n, dls, n_shared, dlo, n_own, 0, kLpLags, 8, 0.0f, tabs, pwA, syA, nullptr, nullptr, t,
                           0, arith, &prune);
        OK(hipGetLastError());
        NEED(prune.mask != nullptr);
        launch_pick_lag(itA, n, syA, kLpLags, 8, 0, prune.mask);
        OK(hipGetLastError());
        OK(hipDeviceSynchronize());
        // B: the whole scan on copies of the items
        launch_demod_tiled(dI, dQ, np, itB, n, dls, n_shared, dlo, n_own, 0, kLpLags, 8, 0.0f, tabs, pwB, syB, nullptr, nullptr, t,
                           0, arith, nullptr);
        OK(hipGetLastError());
        launch_pick_lag(itB, n, syB, kLpLags, 8, 0);
        OK(hipGetLastError());
        OK(hipDeviceSynchronize());

        const int oh[4] = {n, n_shared, n_own, (int)scratch_bytes};
        if (!wr(out, oh, sizeof oh)) return 2;
        DUMP(tabs, tab_bytes);
        DUMP(itA, n * sizeof(FineState)); DUMP(itB, n * sizeof(FineState));
        DUMP(syA, nrow * 4); DUMP(syB, nrow * 4);
        DUMP(pwA, pw_bytes); DUMP(pwB, pw_bytes);
        DUMP(scratch, scratch_bytes); DUMP(counts, 16); DUMP(audit, audit_bytes);
        if (drift) DUMP(counts + 4, 16);
        OK(hipFree(itA)); OK(hipFree(itB)); OK(hipFree(dls)); OK(hipFree(counts)); OK(hipFree(tabs)); OK(hipFree(pwA));
        OK(hipFree(pwB)); OK(hipFree(syA)); OK(hipFree(syB)); OK(hipFree(audit)); OK(hipFree(scratch));
    }
    if (fclose(out) != 0) return 2;
    printf("lagprune_check: %d runs\n", nruns);
    return 0;
}
