// Test helper: the exact jump-ahead of the float phase accumulator (csrc/kernels/phase_runs.h, used by
// the GPU subtraction) compiled for the host, next to the plain serial walk of wsprd.c:340-351.
#include <vector>
#include "../../rtlsdr-wsprd_amd/csrc/kernels/phase_runs.h"

// dphi: nsym floats.  Returns the number of runs (or -1), the number of samples whose reconstructed phase
// differs from the serial walk in *mismatches (bit compare), and the walk itself in phi_out if not null.
// max_runs <= 0: the product's table size.  When the table overflows the per-symbol fallback is checked.
extern "C" int phase_runs_check(const float* dphi, int nsym, int sps_log2, long* mismatches, float* phi_out, int max_runs) {
    const int sps = 1 << sps_log2;
    if (max_runs <= 0) max_runs = wspr::kPhaseMaxRuns;
    std::vector<wspr::PhaseRun> runs(max_runs);
    std::vector<uint16_t> first(nsym + 1);
    std::vector<float> sym_phi(nsym);
    const int nr = wspr::phase_runs_build([&](int i) { return dphi[i]; }, nsym, sps, runs.data(), max_runs,
                                          first.data(), sym_phi.data());
    long bad = 0;
    volatile float phi = 0.0f;                 // volatile: one rounded float addition per step, as compiled in the reference
    for (int i = 0; i < nsym; ++i)
        for (int j = 0; j < sps; ++j) {
            const int n = i * sps + j;
            const float ref = phi;
            if (phi_out) phi_out[n] = ref;
            const float got = nr >= 0 ? wspr::phase_at(runs.data(), first.data(), sps_log2, n)
                                      : wspr::phase_from_symbol(sym_phi[i], dphi[i], j);
            if (wspr::pr_bits(got) != wspr::pr_bits(ref)) ++bad;
            phi = ref + dphi[i];
        }
    *mismatches = bad;
    return nr;
}

// The chained form (phase_runs_build_chained, what sub_runs_kernel does with a wave) must produce the SAME tables as
// the serial builder: returns the number of differing table entries (runs, first_run, sym_phi), -1 if the run
// counts differ.
extern "C" long phase_runs_chained_diff(const float* dphi, int nsym, int sps_log2, int max_runs, int width) {
    const int sps = 1 << sps_log2;
    if (max_runs <= 0) max_runs = wspr::kPhaseMaxRuns;
    std::vector<wspr::PhaseRun> ra(max_runs), rb(max_runs);
    std::vector<uint16_t> fa(nsym + 1), fb(nsym + 1);
    std::vector<float> pa(nsym), pb(nsym);
    const int na = wspr::phase_runs_build([&](int i) { return dphi[i]; }, nsym, sps, ra.data(), max_runs, fa.data(), pa.data());
    const int nb = wspr::phase_runs_build_chained([&](int i) { return dphi[i]; }, nsym, sps, rb.data(), max_runs, fb.data(),
                                                  pb.data(), width);
    if (na != nb) return -1;
    long bad = 0;
    for (int i = 0; i < nsym; ++i) bad += wspr::pr_bits(pa[i]) != wspr::pr_bits(pb[i]);
    if (na >= 0) {
        for (int i = 0; i <= nsym; ++i) bad += fa[i] != fb[i];
        for (int r = 0; r < na; ++r)
            bad += ra[r].start != rb[r].start || ra[r].m0 != rb[r].m0 || ra[r].q != rb[r].q || ra[r].e != rb[r].e;
    }
    return bad;
}

// The serial builder's result in the layout of the device's PhaseTable (k7_subtract.hip): runs[kPhaseMaxRuns], sym_phi[nsym],
// first_run[nsym + 2].  Entries the builder does not write are left as the caller set them; when the runs do not fit,
// first_run[0] becomes 0xffff as on the device (and -1 is returned, else the number of runs).
extern "C" int phase_runs_table(const float* dphi, int nsym, int sps_log2, wspr::PhaseRun* runs, float* sym_phi,
                                uint16_t* first_run) {
    const int nr = wspr::phase_runs_build([&](int i) { return dphi[i]; }, nsym, 1 << sps_log2, runs, wspr::kPhaseMaxRuns,
                                          first_run, sym_phi);
    if (nr < 0) first_run[0] = 0xffffu;
    return nr;
}

// Every sample's phase from such a table, with the selection sub_fir_fused_kernel makes: the run that holds the sample
// (phase_at), or phase_from_symbol when first_run[0] == 0xffff.  Returns the number of samples skipped because the table
// names a run outside [0, kPhaseMaxRuns) or an empty range -- a table no builder may leave (phi_out keeps its value there).
extern "C" long phase_table_eval(const wspr::PhaseRun* runs, const float* sym_phi, const float* dphi,
                                 const uint16_t* first_run, int nsym, int sps_log2, float* phi_out) {
    const int sps = 1 << sps_log2;
    const bool dense = first_run[0] == 0xffffu;
    long skipped = 0;
    for (int i = 0; i < nsym; ++i) {
        const bool usable = dense || (first_run[i] < first_run[i + 1] && first_run[i + 1] <= wspr::kPhaseMaxRuns);
        for (int j = 0; j < sps; ++j) {
            const int n = i * sps + j;
            if (!usable) { ++skipped; continue; }
            phi_out[n] = dense ? wspr::phase_from_symbol(sym_phi[i], dphi[i], j) : wspr::phase_at(runs, first_run, sps_log2, n);
        }
    }
    return skipped;
}
