// K4, the lag pruning's kernels.  A part of k4_demod.hip's translation unit and of no other: included there once, behind
// ToneAcc and sys_load_checked(), which it uses; launch_demod_tiled() in that file launches what is here.
#pragma once
namespace wspr {
namespace {
// -----------------------------------------------------------------------------
// Lag pruning (mode 0: 33 lags, step 8) of a DRIFT-FREE candidate.
//
// Mode 0 returns the first-maximum lag and its sync only, so the 32 losing lags need only be PROVED to lose.  The
// reference reads nothing but the magnitudes p_t = |sum_j x[k + j] tab_t[j]| (wsprd.c:211-218), and a magnitude does not
// care at which phase the phasor starts: up to rounding and the table's recurrence error
//     p_t(u) = | sum_{n = 8u}^{8u + 255} z_t[n] |,   z_t[n] = x[k0 + n] e^{-i theta_t n},   u = 32 s + m
// -- ONE mixed-down stream per tone under a sliding window, which at lag step 8 is the sum of 32 consecutive 8-sample
// block sums: about 7 % of the scan's arithmetic, none of it bit-exact.
//   lag_coarse_kernel   a workgroup per candidate forms sync~(m) for the 33 lags that way together with a rigorous
//                       bound eps(m) on |sync(m) - sync~(m)| (DESIGN.md section 4 derives it term by term); the lags with
//                       sync~(m) + eps(m) >= max_m' (sync~(m') - eps(m')) are the CONTENDERS -- every first maximum of the
//                       exact scan is among them.  At most kLpCap contenders: they go to the exact list; more, or a
//                       quantity the bound cannot vouch for: the candidate goes to the fallback list;
//   lag_exact_kernel<., false>   the reference's 256-tap sums of ONE (candidate, lag) per workgroup, lane = symbol;
//   demod_lagsys_kernel the whole strided scan for the fallback list (its count read from device memory; k4_demod.hip);
//   lag_metric_list_kernel   folds the (candidate, lag) rows those two wrote; pick_lag_kernel reads contenders only.
// Lists and counts live in device memory and the follow-up grids are sized for the worst case (surplus workgroups
// leave at once), so the wave needs no host wait in between.
// Audit output (LagPrune::audit, null in the product and the lab library): what the proof of DESIGN.md section 4 talks
// about lives in LDS and is gone after the launch, so with a non-null `audit` lane m of the final stage also stores
// kLpAuditStride floats at audit[(item * 33 + m) * kLpAuditStride]: sync~(m), eps(m) as the contender rule reads it, totp~,
// ss~, T~ (the float, before its inflation), delta_tab, and 1.0f / 0.0f = the lag was / was not flagged bad (a seventh
// float, not a sign bit).  tools/lagprune_check.hip dumps them, tests/test_gpu_lag_coarse.py holds them against float64.
constexpr int kLpLags = 33;
constexpr int kLpCap = 4;                           // contenders a pruned candidate may have
constexpr int kCoSyms = 27;                         // symbols per chunk of the coarse pass; 6 chunks
constexpr int kCoChunks = kNSymD / kCoSyms;
constexpr int kCoThreads = 256;
constexpr int kCoOut = 32 * kCoSyms;                // window sums per chunk (+ one: lag 32 of its last symbol)
constexpr int kCoWork = kCoOut / 8 + 1;             // threads per tone pair that form window sums, eight consecutive ones each
constexpr int kCoBlocks = kCoOut + 40;              // block sums a chunk stages
constexpr int kCoPitch = 1024;                      // floats per staged array: index v + v / 8 (stride 9 per thread)
static_assert(kCoChunks * kCoSyms == kNSymD && 2 * kCoWork <= kCoThreads && kCoBlocks + kCoBlocks / 8 < kCoPitch, "coarse tiling");
constexpr int kCoRed = 19;                          // per-thread partials: totp and ss of 8 lags, of lag 32, and T
static_assert(kCoThreads * kCoRed <= 8 * kCoPitch, "the partials reuse the block sums' memory");

__device__ __forceinline__ int co_idx(int v) { return v + (v >> 3); }
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// The constants of eps(m); one line each in DESIGN.md section 4 ("The bound of the lag pruning")
constexpr double kLpU = 5.9604644775390625e-8;                         // 2^-24
constexpr double kLpGammaRef = 514 * kLpU / (1 - 514 * kLpU);          // (a) the reference's serial sum: 514 roundings
constexpr double kLpCoarse = 64 * kLpU;                                // (c) the coarse pass' own rounding
constexpr double kLpTInflate = 1 + 256 * kLpU;                         // T~ is itself a rounded sum of positive terms
constexpr double kLpGammaFold = 648 * kLpU / (1 - 648 * kLpU) + 700 * kLpU / (1 - 700 * kLpU);   // (d) both folds
constexpr double kLpAbs = 1e-15;                                       // underflow in squares, roots and products
constexpr double kLpTotpFloor = 1e-9, kLpTCeil = 1e18;                 // outside: the standard model does not hold
constexpr int kLpAuditStride = 7;                                      // floats per (item, lag) of the audit output

// The final stage of both coarse passes (lag_coarse_kernel, lag_coarse_drift_fold_kernel): eps(m), the contender rule and
// the lists of ONE candidate.  Every thread of the workgroup calls it (it holds the stage's barriers); thread m < 33 brings
// the float sums of lag m: totp~, ss~, T~ (before its inflation) and delta_tab.  This is the part DESIGN.md section 4 proves
// sound, and it exists once.
struct LpDecision {                                                    // the stage's shared state: one per workgroup
    float sy[kLpLags], ep[kLpLags];
    int bad[kLpLags];
    unsigned long long mask;
    int base;
};

__device__ __forceinline__ void lp_decide(LpDecision& dec, int item, int tid, float totp, float ss, float tm, float dtab,
                                          float* __restrict__ sync_out, int* __restrict__ counts,
                                          int* __restrict__ exact_list, int* __restrict__ fb_list,
                                          unsigned long long* __restrict__ mask_out, float* __restrict__ audit) {
    if (tid < kLpLags) {
        const int m = tid;
        // eps(m), in double from the float sums
        const double T = (double)tm * kLpTInflate, S = (double)totp, dt = (double)dtab + 1e-12;
        const double kappa = dt + (kLpGammaRef + 3 * kLpU * (1 + kLpGammaRef)) * (1 + dt) + kLpCoarse;
        const double E = 4 * kappa * T + kLpGammaFold * (S + 4 * kappa * T) + kLpAbs;
        const double r = fabs((double)ss) / S;
        const double eps = (E * (1 + r) / (S - E) + 4 * kLpU * (1 + r)) * (1 + 1e-6);
        const float sy = ss / totp;
        const bool ok = (S >= kLpTotpFloor) && (S > 4 * E) && (T < kLpTCeil) && (eps == eps) && (eps < 1.0) && (sy == sy) &&
                        (fabsf(sy) <= 2.0f);
        dec.sy[m] = sy;
        const float ep = (float)(eps * (1 + 1e-6)) + 1e-9f;
        dec.ep[m] = ep;
        dec.bad[m] = ok ? 0 : 1;
        if (audit) {
            float* __restrict__ a = audit + ((size_t)item * kLpLags + m) * kLpAuditStride;
            a[0] = sy; a[1] = ep; a[2] = totp; a[3] = ss; a[4] = tm; a[5] = dtab; a[6] = ok ? 0.0f : 1.0f;
        }
    }
    __syncthreads();
    if (tid == 0) {
        bool bad = false;
        float lo = -3.0e38f;
        for (int m = 0; m < kLpLags; ++m) {
            bad |= dec.bad[m] != 0;
            // sync~ - eps and sync~ + eps rounded outwards (one ulp of a value below 4 is under 5e-7)
            const float l = dec.sy[m] - dec.ep[m] - 1e-6f;
            lo = l > lo ? l : lo;
        }
        unsigned long long mask = 0;
        int n = 0;
        for (int m = 0; m < kLpLags; ++m)
            if (dec.sy[m] + dec.ep[m] + 1e-6f >= lo) { mask |= 1ull << m; ++n; }
        if (bad || n > kLpCap || n == 0) {
            fb_list[atomicAdd(&counts[1], 1)] = item;
            mask = (1ull << kLpLags) - 1;
            dec.base = -1;
        } else {
            dec.base = atomicAdd(&counts[0], n);
            atomicAdd(&counts[2], 1);
        }
        mask_out[item] = mask;
        dec.mask = mask;
    }
    __syncthreads();
    if (dec.base >= 0 && tid < kLpLags) {
        const unsigned long long mask = dec.mask, bit = 1ull << tid;
        if (mask & bit) exact_list[dec.base + __builtin_popcountll(mask & (bit - 1))] = item * 64 + tid;
        else sync_out[(size_t)item * kLpLags + tid] = -3.0e38f;        // never read (pick_lag_kernel's mask), and cannot win
    }
}

__global__ __launch_bounds__(kCoThreads)
void lag_coarse_kernel(const float* __restrict__ dI, const float* __restrict__ dQ, int np,
                       const FineState* __restrict__ items, const int* __restrict__ item_list, int nitems,
                       const float* __restrict__ tabs, const unsigned char* __restrict__ pr3, float* __restrict__ sync_out,
                       int* __restrict__ counts, int* __restrict__ exact_list, int* __restrict__ fb_list,
                       unsigned long long* __restrict__ mask_out, float* __restrict__ audit) {
    __shared__ double2 e3d[4][8], e2d[4][32], ead[4][16], ebd[4][11];      // e^{i theta n}: n = j, 8 j, 256 j, 4096 j
    __shared__ float2 e3f[4][8], e2f[4][32], e1f[4][164];                  // in float: n = j, 8 j, 256 j
    __shared__ float Bs[8][kCoPitch];                                      // block sums: real parts of the 4 tones, imaginary parts
    float (*Bre)[kCoPitch] = Bs, (*Bim)[kCoPitch] = Bs + 4;
    __shared__ float tedge[64];
    __shared__ float dmax_s[kCoThreads];
    __shared__ LpDecision dec;
    // candidates that follow each other in the list (the same segment's) go to the same XCD, behind one L2
    const int per_xcd = (nitems + 7) >> 3;
    const int pos = ((int)blockIdx.x & 7) * per_xcd + ((int)blockIdx.x >> 3);
    if (((int)blockIdx.x >> 3) >= per_xcd || pos >= nitems) return;
    const int item = item_list[pos], tid = threadIdx.x;
    const FineState st = items[item];
    const float* __restrict__ xi = dI + (size_t)st.seg * kIqStride;
    const float* __restrict__ xq = dQ + (size_t)st.seg * kIqStride;
    const int k0 = st.shift_coarse - 128;
    const float4* __restrict__ gtab = reinterpret_cast<const float4*>(tabs) + (size_t)st.pad * 512;

    // theta_t: the float phasor_table_kernel seeds the table with, widened; theta * n is exact in double (24 + 16 bits)
    for (int e = tid; e < 4 * 67; e += kCoThreads) {
        const int t = e / 67, i = e - 67 * t;
        const double theta = (double)tone_dphi(st.freq_coarse, st.drift, 0, t);
        const double n = i < 8 ? i : i < 40 ? 8 * (i - 8) : i < 56 ? 256 * (i - 40) : 4096 * (i - 56);
        double sn, cs;
        sincos(theta * n, &sn, &cs);
        const double2 v = make_double2(cs, sn);
        if (i < 8) e3d[t][i] = v; else if (i < 40) e2d[t][i - 8] = v; else if (i < 56) ead[t][i - 40] = v; else ebd[t][i - 56] = v;
    }
    __syncthreads();
    for (int e = tid; e < 4 * 204; e += kCoThreads) {
        const int t = e / 204, i = e - 204 * t;
        if (i < 8) e3f[t][i] = make_float2((float)e3d[t][i].x, (float)e3d[t][i].y);
        else if (i < 40) e2f[t][i - 8] = make_float2((float)e2d[t][i - 8].x, (float)e2d[t][i - 8].y);
        else {
            const int w = i - 40;
            const double2 v = cmul(ead[t][w & 15], ebd[t][w >> 4]);
            e1f[t][w] = make_float2((float)v.x, (float)v.y);
        }
    }
    // (b) delta_tab: the table's largest distance from the ideal phasor, measured on the table the exact sums read
    float dmax = 0.0f;
    for (int j = tid; j < kSps; j += kCoThreads) {
        const float4 c4 = gtab[2 * j], s4 = gtab[2 * j + 1];
        const float tc[4] = {c4.x, c4.y, c4.z, c4.w}, ts[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double2 id = cmul(e3d[t][j & 7], e2d[t][j >> 3]);
            const double dc = (double)tc[t] - id.x, ds = (double)ts[t] - id.y;
            const float d = (float)(sqrt(dc * dc + ds * ds) * (1 + 1e-6));
            dmax = (d > dmax || d != d) ? d : dmax;                    // a NaN in the table stays
        }
    }
    dmax_s[tid] = dmax;
    if (tid < 64) tedge[tid] = 0.0f;

    float acc_tp[8], acc_ss[8], acc_tp32 = 0.0f, acc_ss32 = 0.0f, tall = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; ++r) acc_tp[r] = acc_ss[r] = 0.0f;
    for (int c = 0; c < kCoChunks; ++c) {
        const int s0 = kCoSyms * c, v0 = 32 * s0;
        __syncthreads();                                               // tables ready / the previous chunk consumed
        // block sums B_t[v] = e^{-i theta_t 8 v} sum_j x[k0 + 8 v + j] e^{-i theta_t j}, one block per thread and round
#pragma unroll 2
        for (int v = tid; v < kCoBlocks; v += kCoThreads) {
            const int gv = v0 + v, k = k0 + 8 * gv;
            float xI[8], xQ[8], tb = 0.0f;
            if (k > 0 && k + 8 <= np) {                                // the whole block inside the record: 16-byte loads
                typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
                const f4u a = *reinterpret_cast<const f4u*>(xi + k), b = *reinterpret_cast<const f4u*>(xi + k + 4);
                const f4u c4 = *reinterpret_cast<const f4u*>(xq + k), d = *reinterpret_cast<const f4u*>(xq + k + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { xI[j] = a[j]; xI[4 + j] = b[j]; xQ[j] = c4[j]; xQ[4 + j] = d[j]; }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    xI[j] = sys_load_checked(xi, k + j, np);           // wsprd.c:199: 0 < k < np
                    xQ[j] = sys_load_checked(xq, k + j, np);
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) tb += fabsf(xI[j]) + fabsf(xQ[j]);
            // T: every block once (chunks overlap by 40 blocks); the first and last 32 blocks belong to some lags only
            if (v < kCoOut || (c == kCoChunks - 1 && v < kCoOut + 32)) {
                if (gv < 32) tedge[gv] = tb;
                else if (gv >= 32 * kNSymD) tedge[32 + gv - 32 * kNSymD] = tb;
                else tall += tb;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float re = 0.0f, im = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float2 e = e3f[t][j];
                    re = __builtin_fmaf(xI[j], e.x, __builtin_fmaf(xQ[j], e.y, re));
                    im = __builtin_fmaf(xQ[j], e.x, __builtin_fmaf(-xI[j], e.y, im));
                }
                const float2 a1 = e1f[t][gv >> 5], a2 = e2f[t][gv & 31];
                const float ca = a1.x * a2.x - a1.y * a2.y, sa = a1.x * a2.y + a1.y * a2.x;
                Bre[t][co_idx(v)] = re * ca + im * sa;
                Bim[t][co_idx(v)] = im * ca - re * sa;
            }
        }
        __syncthreads();
        // window sums W(u) = B[u] + .. + B[u + 31] for eight consecutive u: the 25 blocks they share, then each one's own
        if (tid < 2 * kCoWork) {
            // thread = (tone pair, g): tones (0, 1) or (2, 3) of the window sums 8 g .. 8 g + 7
            const int pair = tid >= kCoWork ? 1 : 0, g = tid - kCoWork * pair;
            float tp[8], cm[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) tp[r] = cm[r] = 0.0f;
#pragma unroll 1
            for (int t = 2 * pair; t < 2 * pair + 2; ++t) {
                float w[2][8];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float* __restrict__ b = (h ? Bim[t] : Bre[t]) + 9 * g;        // co_idx(8 g + i) = 9 g + i + i / 8
                    float mid = b[co_idx(7)];
#pragma unroll
                    for (int i = 8; i < 32; ++i) mid += b[co_idx(i)];
                    float suf = 0.0f, pre = 0.0f, sfx[8], pfx[8];
                    sfx[7] = 0.0f;
#pragma unroll
                    for (int r = 6; r >= 0; --r) { suf += b[co_idx(r)]; sfx[r] = suf; }
                    pfx[0] = 0.0f;
#pragma unroll
                    for (int r = 1; r < 8; ++r) { pre += b[co_idx(31 + r)]; pfx[r] = pre; }
#pragma unroll
                    for (int r = 0; r < 8; ++r) w[h][r] = (sfx[r] + mid) + pfx[r];
                }
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const float p = __builtin_amdgcn_sqrtf(w[0][r] * w[0][r] + w[1][r] * w[1][r]);      // v_sqrt_f32: one ulp, in (c)
                    tp[r] += p;
                    cm[r] += (t & 1) ? p : -p;                          // (p1 + p3) - (p0 + p2), wsprd.c:216
                }
            }
            // u = 32 s0 + 8 g + r: symbol s0 + g / 4 at lag 8 (g % 4) + r, and (r = 0, g % 4 = 0) the symbol
            // before it at lag 32
            const int sl = g >> 2;
            if (sl < kCoSyms) {
                const float sg = pr3[s0 + sl] ? 1.0f : -1.0f;
#pragma unroll
                for (int r = 0; r < 8; ++r) { acc_tp[r] += tp[r]; acc_ss[r] += sg * cm[r]; }
            }
            if ((g & 3) == 0 && sl > 0) {
                acc_tp32 += tp[0];
                acc_ss32 += (pr3[s0 + sl - 1] ? 1.0f : -1.0f) * cm[0];
            }
        }
    }
    __syncthreads();
    float* __restrict__ red = &Bs[0][0];                               // [kCoThreads][kCoRed]
#pragma unroll
    for (int r = 0; r < 8; ++r) { red[kCoRed * tid + r] = acc_tp[r]; red[kCoRed * tid + 8 + r] = acc_ss[r]; }
    red[kCoRed * tid + 16] = acc_tp32;
    red[kCoRed * tid + 17] = acc_ss32;
    red[kCoRed * tid + 18] = tall;
    __syncthreads();
    // lag m = tid: its sums from the threads' partials, delta_tab from theirs
    float totp = 0.0f, ss = 0.0f, tm = 0.0f, dtab = 0.0f;
    if (tid < kLpLags) {
        const int m = tid;
        if (m < 32) {
            for (int pair = 0; pair < 2; ++pair)
                for (int g = (m >> 3) + kCoWork * pair; g < kCoWork - 1 + kCoWork * pair; g += 4) {
                    totp += red[kCoRed * g + (m & 7)];
                    ss += red[kCoRed * g + 8 + (m & 7)];
                }
        } else {
            for (int pair = 0; pair < 2; ++pair)
                for (int g = 4 + kCoWork * pair; g < kCoWork + kCoWork * pair; g += 4) {
                    totp += red[kCoRed * g + 16];
                    ss += red[kCoRed * g + 17];
                }
        }
        for (int i = 0; i < kCoThreads; ++i) {
            tm += red[kCoRed * i + 18];
            const float d = dmax_s[i];
            dtab = (d > dtab || d != d) ? d : dtab;
        }
        for (int v = m; v < 32; ++v) tm += tedge[v];                   // blocks m .. m + 5183 carry lag m's windows
        for (int v = 0; v < m; ++v) tm += tedge[32 + v];
    }
    lp_decide(dec, item, tid, totp, ss, tm, dtab, sync_out, counts, exact_list, fb_list, mask_out, audit);
}

// The reference's sums of ONE (candidate, lag) of the exact list: lane = symbol (162 of 192 lanes), the samples through a
// chunked tile as in freq_scalar_kernel; amplitudes into the lag scan's block.  One workgroup per entry of the list; the grid
// is sized for the longest list and surplus workgroups leave at once.  The four tone phasors: the candidate's one table (tabs)
// through the scalar cache; kDrift: no stored table (tabs is null), the lane runs its symbol's four recurrences (wsprd.c:158-188)
// in registers, seeded as demod_drift_kernel seeds its table lanes: bytewise the rows that kernel writes.
// Same operations per accumulator as demod_kernel => identical bits.
constexpr int kLxThreads = 192;
constexpr int kLxChunk = 16;
constexpr int kLxPerThread = (kNSymD * kLxChunk + kLxThreads - 1) / kLxThreads;      // 14 samples staged per thread and chunk

template <bool kFma, bool kDrift>
__global__ __launch_bounds__(kLxThreads)
void lag_exact_kernel(const float* __restrict__ dI, const float* __restrict__ dQ, int np,
                      const FineState* __restrict__ items, const int* __restrict__ counts,
                      const int* __restrict__ exact_list, const float* __restrict__ tabs, float4* __restrict__ pw_out) {
    __shared__ float2 tile[kNSymD][kLxChunk + 1];
    if ((int)blockIdx.x >= counts[0]) return;
    const int code = exact_list[blockIdx.x], item = code >> 6, m = code & 63, tid = threadIdx.x;
    const FineState st = items[item];
    const float* __restrict__ xi = dI + (size_t)st.seg * kIqStride;
    const float* __restrict__ xq = dQ + (size_t)st.seg * kIqStride;
    const int lag = st.shift_coarse - 128 + 8 * m;
    const float4* __restrict__ gt = kDrift ? nullptr : reinterpret_cast<const float4*>(tabs) +
                                                       (size_t)__builtin_amdgcn_readfirstlane(st.pad) * 512;
    const bool working = tid < kNSymD;
    float2 nxt[kLxPerThread];
    auto fetch = [&](int c) {
#pragma unroll
        for (int u = 0; u < kLxPerThread; ++u) {
            const int e = u * kLxThreads + tid, row = e / kLxChunk, col = e & (kLxChunk - 1);
            const int k = lag + kSps * row + kLxChunk * c + col;
            const bool ok = (e < kNSymD * kLxChunk) && (k > 0) && (k < np);     // wsprd.c:199; zero-fill == skip
            nxt[u] = ok ? make_float2(xi[k], xq[k]) : make_float2(0.0f, 0.0f);
        }
    };
    fetch(0);
    v2f cd01 = {1.0f, 1.0f}, cd23 = cd01, sd01 = {0.0f, 0.0f}, sd23 = sd01;
    if (kDrift && working) {
        float dphi = tone_dphi(st.freq_coarse, st.drift, tid, 0);
        cd01.x = glibc_cosf(dphi); sd01.x = glibc_sinf(dphi);
        dphi = tone_dphi(st.freq_coarse, st.drift, tid, 1);
        cd01.y = glibc_cosf(dphi); sd01.y = glibc_sinf(dphi);
        dphi = tone_dphi(st.freq_coarse, st.drift, tid, 2);
        cd23.x = glibc_cosf(dphi); sd23.x = glibc_sinf(dphi);
        dphi = tone_dphi(st.freq_coarse, st.drift, tid, 3);
        cd23.y = glibc_cosf(dphi); sd23.y = glibc_sinf(dphi);
    }
    v2f c01 = {1.0f, 1.0f}, c23 = c01, s01 = {0.0f, 0.0f}, s23 = s01;
    ToneAcc<kFma> acc;
    acc.clear();
    for (int c = 0; c < kSps / kLxChunk; ++c) {
        __syncthreads();                                             // the previous chunk has been consumed
#pragma unroll
        for (int u = 0; u < kLxPerThread; ++u) {
            const int e = u * kLxThreads + tid;
            if (e < kNSymD * kLxChunk) tile[e / kLxChunk][e & (kLxChunk - 1)] = nxt[u];
        }
        __syncthreads();
        if (c + 1 < kSps / kLxChunk) fetch(c + 1);
        if (working) {
#pragma unroll 8
            for (int jj = 0; jj < kLxChunk; ++jj) {
                if constexpr (!kDrift) {
                    const int j = kLxChunk * c + jj;
                    acc.step(tile[tid][jj], gt[2 * j], gt[2 * j + 1]);
                } else {
                    if (c + jj > 0) {
                        if constexpr (kFma) {
                            phasor_step<kFma>(c01, s01, cd01, sd01);
                            phasor_step<kFma>(c23, s23, cd23, sd23);
                        } else {
                            // the exact phasor_step() of both pairs with the eight products formed first (freq_drift_kernel)
                            const v2f a01 = c01 * cd01, b01 = s01 * sd01, e01 = c01 * sd01, d01 = s01 * cd01;
                            const v2f a23 = c23 * cd23, b23 = s23 * sd23, e23 = c23 * sd23, d23 = s23 * cd23;
                            c01 = a01 - b01; s01 = e01 + d01;
                            c23 = a23 - b23; s23 = e23 + d23;
                        }
                    }
                    acc.step(tile[tid][jj], make_float4(c01.x, c01.y, c23.x, c23.y), make_float4(s01.x, s01.y, s23.x, s23.y));
                }
            }
        }
    }
    if (working) pw_out[((size_t)item * kLpLags + m) * kNSymD + tid] = acc.amplitudes();
}

// -----------------------------------------------------------------------------
// Lag pruning (mode 0: 33 lags, step 8) of a DRIFTING candidate (LagPrune::drift; DESIGN.md section 4, "The bound for
// drifting candidates").
//
// The identity holds per symbol with that symbol's frequency: with theta = the float tone_dphi(freq_coarse, drift, s, t),
//     p_t(s, m) = | sum_{b = m}^{m + 31} B[b] |,   B[b] = sum_{j < 8} x[k0 + 256 s + 8 b + j] e^{-i theta (8 b + j)},  b = 0 .. 63
// -- a symbol's 33 lags touch the 512 samples from 256 s on, mixed once per tone with that symbol's frequency.
//   lag_coarse_drift_kernel        a wave = 16 symbols x 4 tones of one candidate, lane = (symbol, tone): the lane forms its 64
//                                  block sums in registers (packed (re, im) pairs), the 33 window sums from them as
//                                  lag_coarse_kernel does (25 shared terms + 7 + 7), the magnitudes, and its table bound
//                                  delta_{s,t}; the wave folds them in lane order into totp~(m), ss~(m) and the largest delta
//                                  -> part[position][wave][kCdPart].  No barrier but the fold's, no atomics.
//   lag_coarse_drift_fold_kernel   a workgroup per candidate: T~(m) from the samples, the 11 waves' partials in wave order,
//                                  then lp_decide(): the final stage lag_coarse_kernel ends with.
//   lag_exact_kernel<., true>      the exact sums with the lane's four phasor recurrences in registers.
//   demod_drift_kernel<., true>    the whole drift scan over the fallback list (its count read from device memory; k4_demod.hip).
// The phasors: e^{i theta} from one double sincos, its powers by double complex products (<= 20 in a row: 1e-14 with the 511-fold
// angle error of the sincos), each rounded ONCE to float: in-block e^{i theta j}, anchors e^{i theta 8 b0} and e^{i theta 64 b1},
// multiplied in float per block (b = 8 b1 + b0) -- the roundings of lag_coarse_kernel's e3f, e2f, e1f, so term (c) keeps 64u.
// delta_{s,t} is MEASURED (method (ii) of DESIGN.md): a drifting candidate has no stored table, so the lane runs the table's float
// recurrence itself, under the call's arithmetic policy, next to a double one.  The a priori bound 255 (rho + 3u)(1 + 1e-4),
// rho = |w - e^{i theta}| (tests/lag_drift_lib.py: delta_bound) is five times the measured 1.1e-5 and sent 13 % of the drifting
// candidates of configs[2]-shaped segments over the cap of four contenders; measured, 10 % (profiles/lag_prune_drift_bound.json).
constexpr int kCdSyms = 16;                                            // symbols per wave
constexpr int kCdWaves = (kNSymD + kCdSyms - 1) / kCdSyms;             // 11 waves per candidate; the last one holds 2 symbols
constexpr int kCdPart = 2 * kLpLags + 2;                               // floats per wave: totp~[33], ss~[33], delta, spare

// One lane's block sums and window magnitudes -> ps[m][lane]; kChecked: the reference's bounds test per sample (a wave that
// hangs over the record).  Eight blocks at a time, and the windows 8 g .. 8 g + 7 (blocks 8 g .. 8 g + 38) as soon as their last
// block exists, so that at most 40 block sums are alive; the scheduling barriers keep the compiler from forming all 64 first
// (it then spilled 3 000 dwords).
template <bool kChecked>
__device__ __forceinline__ void cd_lane(const float* __restrict__ xi, const float* __restrict__ xq, int np, int kb,
                                        const float2 (&e3)[8], const float2 (&a0)[8], const float2 (&a1)[8],
                                        float (*__restrict__ ps)[64 + 1], int lane, bool live) {
    v2f B[64];
#pragma unroll
    for (int b1 = 0; b1 < 8; ++b1) {
#pragma unroll
        for (int b0 = 0; b0 < 8; ++b0) {
            const int k = kb + 8 * (8 * b1 + b0);
            float xI[8], xQ[8];
            if constexpr (kChecked) {
                // wsprd.c:199: 0 < k < np; the loads are unconditional (clamped) and masked as integers, so that no branch
                // per sample is formed
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int kk = k + j, kc = min(max(kk, 0), np - 1), keep = (kk > 0 && kk < np) ? -1 : 0;
                    xI[j] = __builtin_bit_cast(float, __builtin_bit_cast(int, xi[kc]) & keep);
                    xQ[j] = __builtin_bit_cast(float, __builtin_bit_cast(int, xq[kc]) & keep);
                }
            } else {
                typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
                const f4u a = *reinterpret_cast<const f4u*>(xi + k), c = *reinterpret_cast<const f4u*>(xi + k + 4);
                const f4u d = *reinterpret_cast<const f4u*>(xq + k), e = *reinterpret_cast<const f4u*>(xq + k + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { xI[j] = a[j]; xI[4 + j] = c[j]; xQ[j] = d[j]; xQ[4 + j] = e[j]; }
            }
            // (re, im) += (xQ, -xI) sin + (xI, xQ) cos: x e^{-i theta j} as two packed fmas
            v2f z = {0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                z = fused((v2f){xQ[j], -xI[j]}, (v2f){e3[j].y, e3[j].y}, z);
                z = fused((v2f){xI[j], xQ[j]}, (v2f){e3[j].x, e3[j].x}, z);
            }
            const float2 p = a1[b1], q = a0[b0];
            const float ca = p.x * q.x - p.y * q.y, sa = p.x * q.y + p.y * q.x;
            B[8 * b1 + b0] = (v2f){z.x * ca + z.y * sa, z.y * ca - z.x * sa};
            if (b0 & 1) __builtin_amdgcn_sched_barrier(0);           // the loads of two blocks in flight
        }
        if (b1 >= 4) {
            // window sums W(m) = B[m] + .. + B[m + 31], eight consecutive m: the 25 blocks they share, then each one's own
            const int g = b1 - 4;
            v2f mid = B[8 * g + 7];
#pragma unroll
            for (int i = 8; i < 32; ++i) mid = mid + B[8 * g + i];
            v2f suf = {0.0f, 0.0f}, pre = {0.0f, 0.0f}, sfx[8], pfx[8];
            sfx[7] = suf;
#pragma unroll
            for (int r = 6; r >= 0; --r) { suf = suf + B[8 * g + r]; sfx[r] = suf; }
            pfx[0] = pre;
#pragma unroll
            for (int r = 1; r < 8; ++r) { pre = pre + B[8 * g + 31 + r]; pfx[r] = pre; }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const v2f w = (sfx[r] + mid) + pfx[r];
                const float pm = __builtin_amdgcn_sqrtf(w.x * w.x + w.y * w.y);      // v_sqrt_f32: one ulp, in (c)
                ps[8 * g + r][lane] = live ? pm : 0.0f;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    v2f w = B[32];
#pragma unroll
    for (int i = 1; i < 32; ++i) w = w + B[32 + i];
    const float pm = __builtin_amdgcn_sqrtf(w.x * w.x + w.y * w.y);
    ps[32][lane] = live ? pm : 0.0f;
}

template <bool kFma>
__global__ __launch_bounds__(64)
void lag_coarse_drift_kernel(const float* __restrict__ dI, const float* __restrict__ dQ, int np,
                             const FineState* __restrict__ items, const int* __restrict__ item_list,
                             const unsigned char* __restrict__ pr3, float* __restrict__ part) {
    __shared__ float ps[kLpLags][64 + 1];
    __shared__ float sg_s[64], dl_s[64];
    const int pos = blockIdx.y, wave = blockIdx.x, lane = threadIdx.x;
    const FineState st = items[item_list[pos]];
    const float* __restrict__ xi = dI + (size_t)st.seg * kIqStride;
    const float* __restrict__ xq = dQ + (size_t)st.seg * kIqStride;
    const int sym_l = kCdSyms * wave + (lane >> 2), tone = lane & 3;
    const bool live = sym_l < kNSymD;                                  // the last wave's spare lanes repeat symbol 161 and add 0
    const int sym = live ? sym_l : kNSymD - 1;
    const int kb = st.shift_coarse - 128 + kSps * sym;

    const float thf = tone_dphi(st.freq_coarse, st.drift, sym, tone);
    double s1, c1;
    sincos((double)thf, &s1, &c1);
    // (b) delta_{s,t}: the table the exact sums read -- demod_drift_kernel's recurrence under this arithmetic policy, from the
    // same seeds -- against a double recurrence (255 double complex products: < 1e-12, added by the fold kernel)
    float delta;
    {
        const float cd = glibc_cosf(thf), sd = glibc_sinf(thf);
        float c = 1.0f, s = 0.0f;
        double2 r = make_double2(1.0, 0.0);
        const double2 z1 = make_double2(c1, s1);
        double d2max = 0.0;
#pragma unroll 4
        for (int j = 1; j < kSps; ++j) {
            phasor_step<kFma>(c, s, cd, sd);
            r = cmul(r, z1);
            const double dc = (double)c - r.x, ds = (double)s - r.y, d2 = dc * dc + ds * ds;
            d2max = (d2 > d2max || d2 != d2) ? d2 : d2max;             // a NaN stays, and flags the candidate
        }
        delta = (float)(sqrt(d2max) * (1 + 1e-6));
    }
    float2 e3[8], a0[8], a1[8];
    {
        const double2 z1 = make_double2(c1, s1);
        double2 z = make_double2(1.0, 0.0), z4 = z;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            e3[j] = make_float2((float)z.x, (float)z.y);
            if (j == 4) z4 = z;
            z = cmul(z, z1);
        }
        const double2 z8 = cmul(z4, z4);
        z = make_double2(1.0, 0.0);
#pragma unroll
        for (int j = 0; j < 8; ++j) { a0[j] = make_float2((float)z.x, (float)z.y); z = cmul(z, z8); }
        const double2 z64 = z;
        z = make_double2(1.0, 0.0);
#pragma unroll
        for (int j = 0; j < 8; ++j) { a1[j] = make_float2((float)z.x, (float)z.y); z = cmul(z, z64); }
    }

    // the wave's lanes read kb .. kb + 511 each
    const bool inside = kb > 0 && kb + 2 * kSps <= np;
    if (__all(inside)) cd_lane<false>(xi, xq, np, kb, e3, a0, a1, ps, lane, live);
    else cd_lane<true>(xi, xq, np, kb, e3, a0, a1, ps, lane, live);
    // (p1 + p3) - (p0 + p2), signed by the symbol's sync bit (wsprd.c:216-217)
    sg_s[lane] = ((tone & 1) ? 1.0f : -1.0f) * (pr3[sym] ? 1.0f : -1.0f);
    dl_s[lane] = delta;
    __syncthreads();
    float* __restrict__ out = part + ((size_t)pos * kCdWaves + wave) * kCdPart;
    if (lane < kLpLags) {
        float totp = 0.0f, ss = 0.0f;
        for (int l = 0; l < 64; ++l) {
            const float p = ps[lane][l];
            totp += p;
            ss += sg_s[l] * p;
        }
        out[lane] = totp;
        out[kLpLags + lane] = ss;
    } else if (lane == kLpLags) {
        float dmax = 0.0f;
        for (int l = 0; l < 64; ++l) {
            const float d = dl_s[l];
            dmax = (d > dmax || d != d) ? d : dmax;
        }
        out[2 * kLpLags] = dmax;
    }
}

constexpr int kCfThreads = 256;
constexpr int kCfBlocks = 32 * kNSymD + 32;                            // 8-sample blocks under a candidate's 33 lags

__global__ __launch_bounds__(kCfThreads)
void lag_coarse_drift_fold_kernel(const float* __restrict__ dI, const float* __restrict__ dQ, int np,
                                  const FineState* __restrict__ items, const int* __restrict__ item_list,
                                  const float* __restrict__ part, float* __restrict__ sync_out, int* __restrict__ counts,
                                  int* __restrict__ exact_list, int* __restrict__ fb_list,
                                  unsigned long long* __restrict__ mask_out, float* __restrict__ audit) {
    __shared__ float tedge[64], tsum[kCfThreads], tsum2[16];
    __shared__ LpDecision dec;
    const int pos = blockIdx.x, tid = threadIdx.x;
    const int item = item_list[pos];
    const FineState st = items[item];
    const float* __restrict__ xi = dI + (size_t)st.seg * kIqStride;
    const float* __restrict__ xq = dQ + (size_t)st.seg * kIqStride;
    const int k0 = st.shift_coarse - 128;
    // T: every block once; the first and last 32 blocks belong to some lags only
    float tall = 0.0f;
    for (int v = tid; v < kCfBlocks; v += kCfThreads) {
        const int k = k0 + 8 * v;
        float tb = 0.0f;
        if (k > 0 && k + 8 <= np) {
            typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
            const f4u a = *reinterpret_cast<const f4u*>(xi + k), b = *reinterpret_cast<const f4u*>(xi + k + 4);
            const f4u c = *reinterpret_cast<const f4u*>(xq + k), d = *reinterpret_cast<const f4u*>(xq + k + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) tb += fabsf(a[j]) + fabsf(c[j]);
#pragma unroll
            for (int j = 0; j < 4; ++j) tb += fabsf(b[j]) + fabsf(d[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) tb += fabsf(sys_load_checked(xi, k + j, np)) + fabsf(sys_load_checked(xq, k + j, np));
        }
        if (v < 32) tedge[v] = tb;
        else if (v >= 32 * kNSymD) tedge[32 + v - 32 * kNSymD] = tb;
        else tall += tb;
    }
    tsum[tid] = tall;
    __syncthreads();
    if (tid < 16) {                                                    // a term passes 16 + 21 + 16 + 16 + 32 adds: < 256
        float s = 0.0f;
        for (int i = 0; i < 16; ++i) s += tsum[16 * tid + i];
        tsum2[tid] = s;
    }
    __syncthreads();
    // lag m = tid: the 11 waves' partials in wave order, the largest delta_{s,t} of the candidate for delta_tab
    float totp = 0.0f, ss = 0.0f, tm = 0.0f, dtab = 0.0f;
    if (tid < kLpLags) {
        const int m = tid;
        const float* __restrict__ pp = part + (size_t)pos * kCdWaves * kCdPart;
        for (int w = 0; w < kCdWaves; ++w) {
            totp += pp[w * kCdPart + m];
            ss += pp[w * kCdPart + kLpLags + m];
            const float d = pp[w * kCdPart + 2 * kLpLags];
            dtab = (d > dtab || d != d) ? d : dtab;
        }
        for (int i = 0; i < 16; ++i) tm += tsum2[i];
        for (int v = m; v < 32; ++v) tm += tedge[v];                   // blocks m .. m + 5183 carry lag m's windows
        for (int v = 0; v < m; ++v) tm += tedge[32 + v];
    }
    lp_decide(dec, item, tid, totp, ss, tm, dtab, sync_out, counts, exact_list, fb_list, mask_out, audit);
}

// demod_metric_kernel (mode 0) over the rows the pruned scan filled: the exact list, then 33 lags per fallback candidate
__global__ __launch_bounds__(64)
void lag_metric_list_kernel(const float4* __restrict__ pw, const int* __restrict__ counts, const int* __restrict__ exact_list,
                            const int* __restrict__ fb_list, float* __restrict__ sync_out,
                            const unsigned char* __restrict__ pr3) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, ne = counts[0], nf = counts[1];
    int item, m;
    if (idx < ne) {
        const int code = exact_list[idx];
        item = code >> 6; m = code & 63;
    } else {
        const int j = idx - ne;
        if (j >= kLpLags * nf) return;
        item = fb_list[j / kLpLags]; m = j % kLpLags;
    }
    const size_t row = (size_t)item * kLpLags + m;
    const float4* __restrict__ P = pw + row * kNSymD;
    sync_out[row] = sync_metric([&](int k) { return P[k]; }, pr3);
}

size_t lag_prune_shared_bytes(int nitems) {
    return ((size_t)nitems * 8 + (size_t)nitems * (kLpCap + 1) * 4 + 15) & ~(size_t)15;
}
}  // namespace

// [contender masks | exact list | fallback list] of the drift-free candidates, then, for the drifting ones (LagPrune::drift),
// [exact list: kLpCap x nitems | fallback list: nitems | the coarse waves' partial sums: nitems x kCdWaves x kCdPart floats]
size_t lag_prune_scratch_bytes(int nitems) {
    return lag_prune_shared_bytes(nitems) + (((size_t)nitems * (kLpCap + 1 + kCdWaves * kCdPart) * 4 + 15) & ~(size_t)15);
}
}  // namespace wspr
