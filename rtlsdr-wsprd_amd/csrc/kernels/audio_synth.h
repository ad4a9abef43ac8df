// K17, the 12 kHz audio scene synthesiser (wspr_synth_audio*(), include/wspr_mi355x.h): THE DEFINITION, shared by the
// kernel (k17_audio_synth.hip) and by the serial checker (tests/helpers/audio_synth_check.cpp).  From "symbols, frequency,
// time, level, drift" to the 16-bit records K12 (audio_front.h) and K15 (audio_blank.h) take: 12 000 samples per second,
// the WSPR band centred on 1 500 Hz, 8 192 samples per symbol (12000/8192 = 375/256 baud).  It runs under K8's contract
// (synth_math.h): every function is a fixed sequence of correctly rounded IEEE-754 double operations in the order
// written, compiled with -ffp-contract=off on both sides, so a CPU reproduces every sample bit for bit.
//
// For record s of nsamp samples (0 .. 1 440 000), global segment S = seg_index0 + s, output sample k is formed in this order:
//   1. acc = 0.0, or (double)pcm[k] with the accumulate flag (the bit of K8's call: a test signal onto recorded audio).
//   2. If noise_sigma > 0: acc = acc + (double)n_k.  ONE synth_gauss(seed, S, m, 0x80000000u, noise_sigma, &a, &b) draw per
//      PAIR of samples, m = k >> 1: sample 2m takes a, sample 2m + 1 takes b.  Counter word 1 = 0x80000000 names a stream of
//      its own (K8's noise uses 0, K13's impulses 1 + 2q + p), and nothing is carried between samples: a record's noise
//      does not depend on how a job is split.
//   3. For each transmission of the segment IN LIST ORDER: acc = acc + (double)amp * cs, cs = synth_sincos()'s cosine of
//        phi = P_i + (double)j * dphi_i                    for sample j (0 .. 8191) of symbol i, with
//        dphi_i = audio_synth_dphi()                       (below), and
//        P_0 = 0.0, P_{i+1} = P_i + 8192.0 * dphi_i        -- 162 dependent adds, run as written (audio_synth_phases()).
//      Unlike K8 there is no serial chain inside a symbol: phi is one multiply and one add per sample.
//      Its output index is k = first + 8192 i + j, first = audio_synth_first(t0); indices outside [0, nsamp) are dropped, so
//      a frame may hang off either end of the record.
//   4. audio_synth_quantise(): above 32767.0 the sample is 32767, below -32768.0 it is -32768, and either counts as
//      clipped; otherwise round to nearest, ties to even.  n_clipped[s] is the record's count.
// amp and noise_sigma are in PCM units (LSB).
//
// THE LEVEL CONVENTION.  Real white noise of standard deviation sigma at 12 000 samples per second spreads sigma^2 over
// 6 000 Hz, so it has power sigma^2 * 2500/6000 in the 2 500 Hz the decoder's SNR refers to; a cosine of amplitude amp has
// power amp^2 / 2.  A signal at `snr` dB (the decoder's convention) is therefore amp = sigma * sqrt(5000/6000) *
// 10^(snr/20).  The scenes of tests/audio_lib.py are that with sigma = 2000 * sqrt(2.4).
//
// RANGE.  synth_sincos() is valid for |phi| < 2^20 * pi/2 rad.  The last sample of a frame has phi below
// 2 pi * f_max * 1 327 104 / 12 000 with f_max = 1500 + |f0| + |drift|/2 + 1.5 * 12000/8192 Hz (the audio carrier, the
// offset, the largest drift term at i = 0 or 161, the outermost tone: 2.2 Hz), so f_max may reach
// 2^20 * (pi/2) * 12000 / (2 pi * 1327104) = 2 370.4 Hz.  |f0| + |drift|/2 <= 800 Hz keeps f_max at 2 302.2 Hz; a call
// beyond that is refused.  (The rounding of the 162 phase adds is below 1e-9 rad and does not enter.)
#pragma once
#include <stdint.h>

#include "pcm_quantise.h"
#include "synth_math.h"

namespace wspr {

constexpr int kAudioSynthSps = 8192;                                   // samples of a symbol
constexpr int kAudioSynthSigLen = kSynthNsym * kAudioSynthSps;         // 1 327 104 samples of one transmission
constexpr int kAudioSynthMaxSamples = 1440000;                         // samples of a record (120 s)
constexpr int kAudioSynthFirstClamp = 4000000;                         // |first| beyond this: the frame misses the record
constexpr double kAudioSynthMaxHz = 800.0;                             // |f0| + |drift|/2 beyond this is refused
constexpr double kAudioSynthMaxLevel = 1.0e6;                          // |amp| and noise_sigma beyond this are refused
constexpr uint32_t kAudioSynthNoiseStream = 0x80000000u;               // Philox counter word 1 of the audio noise
// phi / (pi/2) of a frame's last sample stays below 2^20: 4 * f_max * samples / rate
static_assert(4.0 * (1500.0 + kAudioSynthMaxHz + 1.5 * 12000.0 / 8192.0) * kAudioSynthSigLen / 12000.0 < 1048576.0,
              "the phase of a frame's last sample leaves the range of synth_sincos()");
static_assert(kAudioSynthFirstClamp > kAudioSynthMaxSamples + kAudioSynthSigLen &&
              kAudioSynthFirstClamp + kAudioSynthSigLen + kAudioSynthMaxSamples < 0x7fffffff / 2,
              "a clamped first index misses every record, and the index arithmetic stays in an int");

// phase increment per sample of symbol i
WSPR_HD double audio_synth_dphi(float f0, float drift, int i, unsigned char symbol) {
    const double df = 12000.0 / 8192.0;
    const double fd = ((double)drift / 2.0) * ((double)i - 81.0) / 81.0;
    return (2.0 * 3.14159265358979323846) * (1 / 12000.0) * (((1500.0 + (double)f0) + fd) + ((double)symbol - 1.5) * df);
}
// P[i] and dphi[i], i = 0 .. 161, of one transmission: the 162 dependent adds
WSPR_HD void audio_synth_phases(float f0, float drift, const unsigned char* symbols, double* P, double* dphi, int stride) {
    double p = 0.0;
    for (int i = 0; i < kSynthNsym; ++i) {
        const double d = audio_synth_dphi(f0, drift, i, symbols[i]);
        P[(long)i * stride] = p;
        dphi[(long)i * stride] = d;
        p = p + 8192.0 * d;
    }
}
// output index of sample 0 of a transmission: floor(t0 * 12000), clamped so that a far-away frame simply misses the record
WSPR_HD int audio_synth_first(float t0) {
    const double q = __builtin_floor((double)t0 * 12000.0);
    return q > (double)kAudioSynthFirstClamp ? kAudioSynthFirstClamp
                                             : (q < -(double)kAudioSynthFirstClamp ? -kAudioSynthFirstClamp : (int)q);
}
// step 4; *clipped is incremented for a sample that leaves the 16-bit range
WSPR_HD int16_t audio_synth_quantise(double acc, int* clipped) { return pcm_quantise(acc, clipped); }

}  // namespace wspr
