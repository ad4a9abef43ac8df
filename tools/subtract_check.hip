// Driver of tests/test_gpu_k7_table.py: runs the coherent subtraction (K7) of a case file through the PRODUCTION
// launch_subtract(), once per run, and dumps the whole scratch -- every job's PhaseTable as sub_runs_wave_kernel left it and
// the halos the even tiles saved -- and the rows.  It judges nothing: the assertions live in the test (tests/subtract_lib.py
// describes both file formats).  Exit status: 0, 1 = a HIP error (nothing is started after one), 2 = the case file is
// unusable.  Includes the kernel file itself, so that PhaseTable is visible.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -I rtlsdr-wsprd_amd/csrc/kernels tools/subtract_check.hip -o tools/subtract_check.bin
//
// Case file (little endian): int32 magic 0x31374b53, nseg, nruns; float I[nseg][kIqStride], Q[nseg][kIqStride]; then per
// run: int32 np, arith, njobs; SubJob jobs[njobs].  Every run starts from the rows of the file.  Each job of a run has a
// segment of its own (the subtraction is in place; the decoder never queues two jobs on one row in one launch either).
// Output file, per run: int32 njobs, nseg, scratch_floats, table_floats; float scratch[scratch_floats]; float I[nseg][kIqStride],
// Q[nseg][kIqStride] after the launch.  The scratch starts as bytes of 0xa5, so what no kernel wrote can be told.
// The low-pass tables are subtract_lpf_tables() of wspr_device.h, what the context uploads.
#include "../rtlsdr-wsprd_amd/csrc/kernels/k7_subtract.hip"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace wspr;
#define OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
#define NEED(c) do { if (!(c)) { fprintf(stderr, "case file: %s (line %d)\n", #c, __LINE__); return 2; } } while (0)

constexpr int kSentinel = 0xa5;
constexpr int kMaxJobs = 8, kMaxSeg = 8, kMaxRuns = 64;
// sub_fir_fused_kernel indexes PhaseTable::runs with 16-bit numbers it reads from the table.  A table whose first_run was
// left unwritten (the sentinel) would send those reads up to 65 535 runs past a table's start: the scratch is followed by
// that much readable padding, so that a wrong table ends in a failing comparison and never in a read outside the allocation.
constexpr size_t kGuardBytes = (size_t)65536 * sizeof(PhaseRun);

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
    if (argc != 3) { fprintf(stderr, "usage: %s case.bin out.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    NEED(in && out);
    int head[3];
    NEED(rd(in, head, sizeof head));
    const int nseg = head[1], nruns = head[2];
    NEED(head[0] == 0x31374b53 && nseg >= 1 && nseg <= kMaxSeg && nruns >= 1 && nruns <= kMaxRuns);
    const size_t niq = (size_t)nseg * kIqStride;
    std::vector<float> I(niq), Q(niq);
    NEED(rd(in, I.data(), niq * 4) && rd(in, Q.data(), niq * 4));

    std::vector<float> lpf(kLpfTaps), part(kLpfTaps);
    subtract_lpf_tables(lpf.data(), part.data());
    const size_t scratch_floats = subtract_scratch_floats(kMaxJobs);
    float *dI, *dQ, *dlpf, *dpart, *scratch;
    SubJob* djobs;
    OK(hipMalloc(&dI, niq * 4)); OK(hipMalloc(&dQ, niq * 4)); OK(hipMalloc(&dlpf, kLpfTaps * 4)); OK(hipMalloc(&dpart, kLpfTaps * 4));
    OK(hipMalloc(&djobs, kMaxJobs * sizeof(SubJob))); OK(hipMalloc(&scratch, scratch_floats * 4 + kGuardBytes));
    OK(hipMemcpy(dlpf, lpf.data(), kLpfTaps * 4, hipMemcpyHostToDevice));
    OK(hipMemcpy(dpart, part.data(), kLpfTaps * 4, hipMemcpyHostToDevice));
    DeviceTables t{};
    t.lpf = dlpf;
    t.lpf_part = dpart;
    std::vector<char> host;

    for (int run = 0; run < nruns; ++run) {
        int rh[3];
        NEED(rd(in, rh, sizeof rh));
        const int np = rh[0], arith = rh[1], njobs = rh[2];
        // np <= kMaxSamples < kIqStride: the kernel's only guard is 0 < k < np
        NEED(np >= 1 && np <= kMaxSamples && (arith == 0 || arith == 1) && njobs >= 1 && njobs <= kMaxJobs);
        std::vector<SubJob> jobs(njobs);
        NEED(rd(in, jobs.data(), (size_t)njobs * sizeof(SubJob)));
        bool seen[kMaxSeg] = {};
        for (const SubJob& j : jobs) {                           // every job a row of its own; k = shift + n cannot wrap
            NEED(j.seg >= 0 && j.seg < nseg && !seen[j.seg] && j.shift > -100000 && j.shift < 100000);
            seen[j.seg] = true;
        }
        const size_t used = subtract_scratch_floats(njobs);
        OK(hipMemcpy(dI, I.data(), niq * 4, hipMemcpyHostToDevice)); OK(hipMemcpy(dQ, Q.data(), niq * 4, hipMemcpyHostToDevice));
        OK(hipMemcpy(djobs, jobs.data(), (size_t)njobs * sizeof(SubJob), hipMemcpyHostToDevice));
        OK(hipMemset(scratch, kSentinel, scratch_floats * 4 + kGuardBytes));
        OK(hipDeviceSynchronize());

        launch_subtract(dI, dQ, np, djobs, njobs, scratch, t, 0, arith);
        OK(hipGetLastError());
        OK(hipDeviceSynchronize());

        const int oh[4] = {njobs, nseg, (int)used, (int)kTableFloats};
        if (!wr(out, oh, sizeof oh)) return 2;
        DUMP(scratch, used * 4);
        DUMP(dI, niq * 4); DUMP(dQ, niq * 4);
    }
    OK(hipFree(dI)); OK(hipFree(dQ)); OK(hipFree(dlpf)); OK(hipFree(dpart)); OK(hipFree(djobs)); OK(hipFree(scratch));
    if (fclose(out) != 0) return 2;
    printf("subtract_check: %d runs\n", nruns);
    return 0;
}
