// Driver of tests/test_gpu_fine.py: runs the fine search of a case file -- mode 0 (lag scan), mode 1 (frequency scan) with
// the first rung, and the 43 lags of the jitter ladder -- through the PRODUCTION launchers, in the order of
// DecodeRun::refine_and_first_rung() / remaining_rungs() (wspr_pipeline.hip; what they do with the vectors afterwards is
// the Fano walk of host/wspr_fano_walk.h, not run here), and dumps every buffer.  It judges nothing:
// the assertions live in the test (tests/fine_lib.py describes both file formats).  Exit status: 0, 1 = a HIP error
// (nothing is started after one), 2 = the case file is unusable.  Includes the kernel file itself.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -I rtlsdr-wsprd_amd/csrc/kernels tools/fine_check.hip -o tools/fine_check.bin
//
// Case file (little endian): int32 magic 0x31434e46, nseg, nruns; 164 bytes: the sync vector (162) + 2 of padding;
// float I[nseg][kIqStride], Q[nseg][kIqStride]; then per run: int32 np, arith, lagstep, nlag, flags, nitems; float minsync1;
// FineState items[nitems].  flags: 1 = run mode 0 (else the scan starts from the items as they are), 2 = with the lag pruning,
// 4 = hand mode 0's amplitude block to the frequency scan (else null: every centre hypothesis is summed), 8 = run the ladder.
// pad and the two launch lists are assigned here as plan_tables() of wspr_pipeline.hip assigns them.
// Output file, per run: int32 nitems, n_shared, n_own, nlag; int32 list_shared[n_shared], list_own[n_own];
// FineState as launched, after mode 0, after mode 1, as given to the ladder (nitems each); float sync0[nitems][nlag];
// uint64 mask[nitems] (the pruning's; bytes of 0xa5 when it did not prune); float pw0[nitems][nlag][162][4];
// float pwf[n_shared + n_own][5][162][4] (slots: list_shared, then list_own); rung 0: float sync[nitems], rms[nitems],
// uint8 sym[nitems][162]; ladder: float sync[nitems][43], rms[nitems][43], uint8 sym[nitems][43][162].
// Every output buffer starts as bytes of 0xa5 (as a float: -2.87e-16), so what no kernel wrote can be told.
#include "../rtlsdr-wsprd_amd/csrc/kernels/k4_demod.hip"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace wspr;
#define OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
#define NEED(c) do { if (!(c)) { fprintf(stderr, "case file: %s (line %d)\n", #c, __LINE__); return 2; } } while (0)

constexpr int kSentinel = 0xa5;
enum { kRunMode0 = 1, kPrune = 2, kHandLagBlock = 4, kLadder = 8 };

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

// plan_tables() of wspr_pipeline.hip: pad = a dense table index over the drift-free items; lists = [shared | own at n]
static size_t plan(std::vector<FineState>& items, std::vector<int>& lists, int* n_shared, int* n_own) {
    const int n = (int)items.size();
    size_t next = 0;
    int ns = 0, no = 0;
    for (int i = 0; i < n; ++i) {
        items[i].pad = (int)next;
        if (items[i].drift != 0.0f) { lists[n + no++] = i; }
        else                        { next += 1; lists[ns++] = i; }
    }
    *n_shared = ns;
    *n_own = no;
    return next;
}

// a device buffer of `bytes` filled with the sentinel
static int fresh(void** p, size_t bytes) {
    OK(hipMalloc(p, bytes ? bytes : 16));
    OK(hipMemset(*p, kSentinel, bytes ? bytes : 16));
    return 0;
}
#define FRESH(p, bytes) do { const int r_ = fresh(reinterpret_cast<void**>(&(p)), bytes); if (r_) return r_; } while (0)

int main(int argc, char** argv) {
    // a third argument "drift": the pruned scan also prunes the drifting candidates (LagPrune::drift); the dump format is the same
    if (argc != 3 && !(argc == 4 && !strcmp(argv[3], "drift"))) { fprintf(stderr, "usage: %s case.bin out.bin [drift]\n", argv[0]); return 2; }
    const bool drift = argc == 4;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    NEED(in && out);
    int head[3];
    unsigned char pr3[164];
    NEED(rd(in, head, sizeof head) && rd(in, pr3, sizeof pr3));
    const int nseg = head[1], nruns = head[2];
    NEED(head[0] == 0x31434e46 && nseg >= 1 && nseg <= 8 && nruns >= 1 && nruns <= 16);
    const size_t niq = (size_t)nseg * kIqStride;
    std::vector<float> I(niq), Q(niq);
    NEED(rd(in, I.data(), niq * 4) && rd(in, Q.data(), niq * 4));

    float *dI, *dQ;
    unsigned char* dpr3;
    int* djit;
    // the production jitter table (wspr_context.hip): 0, -3, 3, -6, ... ; the first rung reads entry 0
    int jitter[kMaxLags];
    for (int idt = 0; idt < kMaxLags; ++idt) { const int ii = (idt + 1) / 2; jitter[idt] = 3 * ((idt % 2 == 1) ? -ii : ii); }
    OK(hipMalloc(&dI, niq * 4)); OK(hipMalloc(&dQ, niq * 4)); OK(hipMalloc(&dpr3, sizeof pr3)); OK(hipMalloc(&djit, sizeof jitter));
    OK(hipMemcpy(dI, I.data(), niq * 4, hipMemcpyHostToDevice)); OK(hipMemcpy(dQ, Q.data(), niq * 4, hipMemcpyHostToDevice));
    OK(hipMemcpy(dpr3, pr3, sizeof pr3, hipMemcpyHostToDevice)); OK(hipMemcpy(djit, jitter, sizeof jitter, hipMemcpyHostToDevice));
    DeviceTables t{};
    t.sync = dpr3;
    std::vector<char> host;

    for (int run = 0; run < nruns; ++run) {
        int rh[6];
        float minsync1;
        NEED(rd(in, rh, sizeof rh) && rd(in, &minsync1, 4));
        const int np = rh[0], arith = rh[1], lagstep = rh[2], nlag = rh[3], flags = rh[4], n = rh[5];
        NEED(np >= 1 && np <= kMaxSamples && (arith == 0 || arith == 1) && n >= 1 && n <= 64 && flags >= 0 && flags < 16);
        NEED((lagstep == 8 && nlag == 33) || (lagstep == 16 && nlag == 17));
        NEED((flags & kRunMode0) || !(flags & (kPrune | kHandLagBlock)));     // no lag block without a lag scan
        std::vector<FineState> items(n);
        NEED(rd(in, items.data(), (size_t)n * sizeof(FineState)));
        for (int i = 0; i < n; ++i) {
            NEED(items[i].seg >= 0 && items[i].seg < nseg && items[i].shift_coarse > -100000 && items[i].shift_coarse < 100000);
            NEED(items[i].shift > -100000 && items[i].shift < 100000);
        }
        std::vector<int> lists(2 * n);
        int n_shared = 0, n_own = 0;
        const size_t ntabs = plan(items, lists, &n_shared, &n_own);

        const size_t item_bytes = (size_t)n * sizeof(FineState);
        const size_t pw_bytes = (size_t)n * kMaxLags * kNSymD * 16, pw0_bytes = (size_t)n * nlag * kNSymD * 16;
        const size_t pwf_bytes = (size_t)n * kNFreq * kNSymD * 16, tab_bytes = std::max(ntabs, (size_t)n * kNFreq) * 2048 * 4;
        const size_t scratch_bytes = lag_prune_scratch_bytes(n);
        FineState* d_items;
        int *d_lists, *counts;
        float *tabs, *tabs1, *pw, *pwf, *scr, *sync0, *sync_r0, *rms_r0, *sync_l, *rms_l;
        unsigned char *sym_r0, *sym_l;
        void* scratch;
        OK(hipMalloc(&d_items, item_bytes)); OK(hipMalloc(&d_lists, 2 * n * 4));
        FRESH(counts, 32); FRESH(tabs, tab_bytes); FRESH(tabs1, tab_bytes); FRESH(pw, pw_bytes); FRESH(pwf, pwf_bytes);
        FRESH(scr, (size_t)n * kNFreq * 4); FRESH(sync0, (size_t)n * kMaxLags * 4); FRESH(sync_r0, (size_t)n * 4);
        FRESH(rms_r0, (size_t)n * 4); FRESH(sym_r0, (size_t)n * kNSymD); FRESH(sync_l, (size_t)n * kMaxLags * 4);
        FRESH(rms_l, (size_t)n * kMaxLags * 4); FRESH(sym_l, (size_t)n * kMaxLags * kNSymD); FRESH(scratch, scratch_bytes);
        OK(hipMemcpy(d_items, items.data(), item_bytes, hipMemcpyHostToDevice));
        OK(hipMemcpy(d_lists, lists.data(), 2 * n * 4, hipMemcpyHostToDevice));
        OK(hipDeviceSynchronize());

        const int oh[4] = {n, n_shared, n_own, nlag};
        if (!wr(out, oh, sizeof oh) || !wr(out, lists.data(), n_shared * 4) || !wr(out, lists.data() + n, n_own * 4)) return 2;
        DUMP(d_items, item_bytes);

        // mode 0: the lag scan and its pick
        LagPrune prune{scratch, counts, nullptr};
        prune.drift = drift;
        if (flags & kRunMode0) {
            OK(hipMemsetAsync(counts, 0, 8 * 4, 0));
            launch_phasor_tables(d_items, n, 0, tabs, 0, arith);
            launch_demod_tiled(dI, dQ, np, d_items, n, d_lists, n_shared, d_lists + n, n_own, 0, nlag, lagstep, 0.0f, tabs, pw,
                               sync0, nullptr, nullptr, t, 0, arith, (flags & kPrune) ? &prune : nullptr);
            OK(hipGetLastError());
            launch_pick_lag(d_items, n, sync0, nlag, lagstep, 0, prune.mask);
            OK(hipGetLastError());
            OK(hipDeviceSynchronize());
        }
        DUMP(d_items, item_bytes);
        const bool masked = prune.mask != nullptr;
        if (!masked) OK(hipMemset(scratch, kSentinel, scratch_bytes));
        // mode 1 and the first rung; the frequency scan reads its centre out of the lag block, so it writes elsewhere
        launch_freq_scan_and_first_rung(dI, dQ, np, d_items, d_lists, n_shared, d_lists + n, n_own, lagstep, minsync1, djit, tabs1,
                                        pwf, scr, sync_r0, sym_r0, rms_r0, t, 0, (flags & kHandLagBlock) ? pw : nullptr, nlag,
                                        arith);
        OK(hipGetLastError());
        OK(hipDeviceSynchronize());
        DUMP(d_items, item_bytes);
        OK(hipMemcpy(items.data(), d_items, item_bytes, hipMemcpyDeviceToHost));
        plan(items, lists, &n_shared, &n_own);                  // remaining_rungs() plans the items it takes on again
        OK(hipMemcpy(d_items, items.data(), item_bytes, hipMemcpyHostToDevice));
        OK(hipMemcpy(d_lists, lists.data(), 2 * n * 4, hipMemcpyHostToDevice));
        DUMP(d_items, item_bytes);
        DUMP(sync0, (size_t)n * nlag * 4); DUMP(scratch, (size_t)n * 8); DUMP(pw, pw0_bytes);
        DUMP(pwf, pwf_bytes);
        DUMP(sync_r0, (size_t)n * 4); DUMP(rms_r0, (size_t)n * 4); DUMP(sym_r0, (size_t)n * kNSymD);

        // the ladder: all 43 lags shift - 63 + 3 r of the items the gate lets through
        if (flags & kLadder) {
            launch_phasor_tables(d_items, n, 2, tabs, 0, arith);
            launch_demod_tiled(dI, dQ, np, d_items, n, d_lists, n_shared, d_lists + n, n_own, 2, kMaxLags, 3, minsync1, tabs, pw,
                               sync_l, sym_l, rms_l, t, 0, arith);
            OK(hipGetLastError());
            OK(hipDeviceSynchronize());
        }
        DUMP(sync_l, (size_t)n * kMaxLags * 4); DUMP(rms_l, (size_t)n * kMaxLags * 4); DUMP(sym_l, (size_t)n * kMaxLags * kNSymD);
        OK(hipFree(d_items)); OK(hipFree(d_lists)); OK(hipFree(counts)); OK(hipFree(tabs)); OK(hipFree(tabs1)); OK(hipFree(pw));
        OK(hipFree(pwf)); OK(hipFree(scr)); OK(hipFree(sync0)); OK(hipFree(sync_r0)); OK(hipFree(rms_r0)); OK(hipFree(sym_r0));
        OK(hipFree(sync_l)); OK(hipFree(rms_l)); OK(hipFree(sym_l)); OK(hipFree(scratch));
    }
    if (fclose(out) != 0) return 2;
    printf("fine_check: %d runs\n", nruns);
    return 0;
}
