// K19 -- the decode-quality figures of a spot on the device: N jobs of (soft-symbol vector, decdata).
//
// The definition is in spot_quality.h (there is no reference code for these figures; tests/helpers/spot_quality_check.c is
// the serial statement the kernel is held to, field for field).  One wavefront per job, kJobsPerGroup jobs per workgroup;
// a lane owns the transmission positions lane, lane + 64, lane + 128 (the last one for lanes 0 .. 33 only):
//   code bits  every lane forms the 50 message bits from the job's decdata (seven wave-uniform bytes) and, for each of its
//              positions, the coder output that is sent there: where[] (162 bytes, built by the host from the message
//              layer's own interleave()) names the output, the encoder's state is a shift of the message, parity by
//              population count
//   symbols    read where they lie: symbols + offsets[job] * 162, three byte loads per lane, 64 consecutive bytes each
//   metric     metric0[c ? 255 - s : s]: row 0 of the Fano metric table, the 256 shorts the Fano wave (K6w) reads
//   sums       five butterfly reductions over the wave; lane 0 writes the 20 bytes
// No atomics, no scratch, no LDS; all integer, so no arithmetic mode touches it.  Expected load is a few jobs per segment.
#include "wspr_device.h"
#include "spot_quality.h"

namespace wspr {
namespace {

using namespace spotq;

constexpr int kJobsPerGroup = 4, kThreads = 64 * kJobsPerGroup;

__global__ __launch_bounds__(kThreads)
void spot_quality_kernel(const unsigned char* __restrict__ symbols, const int* __restrict__ offsets,
                         const unsigned char* __restrict__ decdata, int n, const short* __restrict__ metric0,
                         const unsigned char* __restrict__ where, SpotQuality* __restrict__ out) {
    const int lane = threadIdx.x & 63, job = blockIdx.x * kJobsPerGroup + (threadIdx.x >> 6);
    if (job >= n) return;                                   // the whole wave leaves: the butterflies below see 64 lanes
    const unsigned char* __restrict__ s = symbols + (size_t)offsets[job] * kN;
    const uint64_t m = message_bits(decdata + (size_t)job * 11);
    int nhard = 0, dist = 0, rsum = 0, v2 = 0, metric = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int i = lane + 64 * q;
        if (i < kN) {
            const int sv = (int)s[i];
            const int c = (int)code_bit(m, (int)where[i]);
            const int v = value(sv), r = v < 0 ? -v : v;
            const int miss = ((sv >= 128) ? 1 : 0) != c;
            nhard += miss;
            dist += miss ? r : 0;
            rsum += r;
            v2 += v * v;
            metric += (int)metric0[c ? 255 - sv : sv];
        }
    }
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) {
        nhard += __shfl_xor(nhard, step, 64);
        dist += __shfl_xor(dist, step, 64);
        rsum += __shfl_xor(rsum, step, 64);
        v2 += __shfl_xor(v2, step, 64);
        metric += __shfl_xor(metric, step, 64);
    }
    if (lane == 0) {
        SpotQuality r;
        r.nhard = nhard; r.dist = dist; r.rsum = rsum; r.v2 = v2; r.metric = metric;
        out[job] = r;
    }
}

}  // namespace

void launch_spot_quality(const unsigned char* symbols, const int* offsets, const unsigned char* decdata, int n,
                         const short* metric0, const unsigned char* where, SpotQuality* out, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(spot_quality_kernel, dim3((n + kJobsPerGroup - 1) / kJobsPerGroup), dim3(kThreads), 0, st, symbols,
                       offsets, decdata, n, metric0, where, out);
}

}  // namespace wspr
