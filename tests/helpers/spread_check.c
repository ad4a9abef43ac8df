// TEST INFRASTRUCTURE ONLY: the Doppler-spread figure (K11, rtlsdr-wsprd_amd/csrc/kernels/spread.h) in plain serial code --
// the definition the kernel is compared with, word for word.  It calls the functions of spread.h and synth_math.h (which
// are C++ headers: tests/spread_lib.py compiles this file with g++ -x c++ -O2 -ffp-contract=off) and nothing of the
// product library.
#include <stdlib.h>
#include <string.h>

#include "spread.h"

using namespace wspr;
using namespace wspr::spread;

extern "C" {

// One job over a row of np samples.  out4: w50, f50, ratio (float bits) and valid, as the kernel stores them.  power (may
// be null): P[j] for j = -1024 .. 1023 in that order.  Returns 0.
int spread_check(const float* I, const float* Q, long np, float f0, int shift, float drift, const unsigned char* symbols,
                 uint32_t* out4, float* power) {
    static float tw[2 * kTwiddles];
    static int have_tw = 0;
    if (!have_tw) { spread_twiddles(tw); have_tw = 1; }
    float* re = (float*)calloc(2 * kFft, sizeof(float));
    if (!re) return -1;
    float* im = re + kFft;
    const long sh = clamp_shift(shift);
    double phi = 0.0;
    for (int b = 0; b < kBlocks; ++b) {
        const int i = b / (kSynthSps / kBlockLen);
        const double dphi = synth_dphi(f0, drift, i, symbols[i]);
        float xi[kBlockLen], xq[kBlockLen];
        for (int s = 0; s < kBlockLen; ++s) {
            const long k = sh + (long)b * kBlockLen + s;
            const int in = k >= 0 && k < np;
            xi[s] = in ? I[k] : 0.0f;
            xq[s] = in ? Q[k] : 0.0f;
        }
        phi = spread_block(xi, xq, phi, dphi, &re[b], &im[b]);       // the serial recurrence straight through
    }
    for (int st = 0; st < kStages; ++st)
        for (int t = 0; t < kTwiddles; ++t) spread_butterfly(re, im, tw, st, t);
    if (power)
        for (int j = -kFft / 2; j < kFft / 2; ++j) power[j + kFft / 2] = spread_power(re, im, j);
    double noise[kNoiseChunks], sig[kSignalChunks];
    float maxp[kSignalChunks];
    for (int c = 0; c < kNoiseChunks; ++c) noise[c] = spread_noise_chunk(re, im, c);
    const double nz = spread_noise_floor(noise);
    for (int c = 0; c < kSignalChunks; ++c) sig[c] = spread_signal_chunk(re, im, c, nz, &maxp[c]);
    const Result r = spread_width(re, im, sig, maxp, nz);
    memcpy(&out4[0], &r.w50, 4);
    memcpy(&out4[1], &r.f50, 4);
    memcpy(&out4[2], &r.ratio, 4);
    out4[3] = (uint32_t)r.valid;
    free(re);
    return 0;
}

}  // extern "C"
