"""ctypes bindings of the IQ-to-audio checker (tests/helpers/iq_audio_check.c: the contract of wspr_iq_to_audio*() in plain
serial C over rtlsdr-wsprd_amd/csrc/kernels/iq_audio.h), built on demand; a float64 numpy statement of the same definition
as a second, independent one; the rows the stage's tests share.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import audio_lib as al
import oracle_lib as ol
import synth

INTERP = 32                     # output samples per input sample
NP_MAX = 45000
K = 255
TILE = 2048                     # outputs per workgroup of the kernel (IQ_AUDIO_TILE): 64 inputs
GAIN = 32768.0                  # the inverse of K12's 2^-15
SENTINEL = 0x7A5A

_lib = None
_SRC = os.path.join(ol.ROOT, "tests", "helpers", "iq_audio_check.c")
_FLAGS = ["-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I",
          os.path.join(ol.ROOT, "rtlsdr-wsprd_amd", "csrc", "kernels")]


def checker():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="wspr_iqaudio_"), "libiqaudiocheck.so")
        # -mfma only makes fmaf() one instruction instead of a call of the C library's (correctly rounded either way)
        fast = ["-mfma"] if ol.cpu_has_fma() else []
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared"] + _FLAGS + fast + ["-o", out, _SRC, "-lm"], check=True)
        X = C.CDLL(out)
        X.iq_audio_check_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_float, C.c_void_p,
                                          C.c_size_t, C.c_void_p]
        X.iq_audio_check_rows.restype = C.c_int
        X.iq_audio_check_quantise.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        X.iq_audio_check_quantise.restype = None
        X.iq_audio_check_tile.restype = C.c_int
        _lib = X
    return _lib


def sanitizer_program(directory):
    """The checker as a stand-alone program (its own main) under AddressSanitizer and UBSan: the path of the executable."""
    exe = os.path.join(str(directory), "iq_audio_check_asan")
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DIQ_AUDIO_CHECK_MAIN"] +
                   _FLAGS + ["-o", exe, _SRC, "-lm"], check=True)
    return exe


def check_rows(I, Q, np_=None, gain=GAIN, pcm=None, pcm_stride=None):
    """The checker on float32 rows [nseg, stride] (or one row), of which the first np_ samples count.  pcm: records to write
    into (copied), else fresh ones of pcm_stride (default 32 np_) samples filled with SENTINEL.
    Returns (rc, records int16 [nseg, pcm_stride], n_clipped int32 [nseg], pre-filled with -7)."""
    I = np.ascontiguousarray(I, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    if I.ndim == 1:
        I, Q = I[None, :], Q[None, :]
    nseg, stride = I.shape
    np_ = stride if np_ is None else int(np_)
    if pcm is None:
        pcm_stride = INTERP * np_ if pcm_stride is None else int(pcm_stride)
        out = np.full((nseg, pcm_stride), SENTINEL, np.int16)
    else:
        out = np.array(pcm, np.int16).reshape(nseg, -1).copy()
        pcm_stride = out.shape[1]
    count = np.full(max(nseg, 1), -7, np.int32)
    rc = checker().iq_audio_check_rows(ol.ptr(I), ol.ptr(Q), nseg, np_, stride, gain, ol.ptr(out), pcm_stride, ol.ptr(count))
    return rc, out, count[:nseg]


def quantise(p):
    """iq_audio_quantise() on float64 values: (int16 samples, clipped count)."""
    p = np.ascontiguousarray(p, np.float64)
    out = np.zeros(p.size, np.int16)
    n = C.c_int(-1)
    checker().iq_audio_check_quantise(ol.ptr(p), int(p.size), ol.ptr(out), C.addressof(n))
    return out, int(n.value)


def impulse_record(m0, np_, rail, gain=GAIN):
    """What the definition gives for a unit impulse at input m0 of rail 0 = I, 1 = Q: quantise(16 gain g[n - 32 m0]), straight
    from the committed bit patterns (audio_lib.taps()) -- no loop over m, no checker.  16 g is exact in float32 and the
    product with the gain is formed in double, as the definition forms it."""
    g = al.taps()[rail]
    n = np.arange(INTERP * np_)
    k = n - INTERP * m0
    inside = np.abs(k) <= K
    y = np.zeros(n.size, np.float32)
    y[inside] = np.float32(16.0) * g[k[inside] + K]
    p = y.astype(np.float64) * float(np.float32(gain))
    return np.clip(np.rint(p), -32768, 32767).astype(np.int16), int(((p > 32767.0) | (p < -32768.0)).sum())


def numpy_rows(I, Q, gain=GAIN):
    """A float64 statement of the definition for finite rows [nseg, np]: zero-stuff by 32, convolve with the tables as
    float64, scale, np.rint, clip.  No fmaf, no skipped steps (the taps there are zero and the input is finite), no shared
    header.  Returns int16 [nseg, 32 np]."""
    gi, gq = (t.astype(np.float64) for t in al.taps())
    I = np.atleast_2d(np.asarray(I, np.float64))
    Q = np.atleast_2d(np.asarray(Q, np.float64))
    out = np.zeros((I.shape[0], INTERP * I.shape[1]), np.int16)
    for s in range(I.shape[0]):
        up_i = np.zeros(INTERP * I.shape[1])
        up_q = np.zeros(INTERP * I.shape[1])
        up_i[::INTERP], up_q[::INTERP] = I[s], Q[s]
        # full[n + 255] = sum_m g[n - 32 m] x[m]
        y = 16.0 * (np.convolve(up_i, gi) + np.convolve(up_q, gq))[K:K + up_i.size]
        out[s] = np.clip(np.rint(y * float(np.float32(gain))), -32768, 32767).astype(np.int16)
    return out


def tone_rows(freqs, amp, np_):
    """Rows of the phasors amp e^{+j 2 pi f m / 375}: (I, Q float32 [len(freqs), np_], z complex128 of the float32 rows)."""
    m = np.arange(np_)
    z = amp * np.exp(2j * np.pi * np.asarray(freqs, np.float64)[:, None] * m[None, :] / 375.0)
    I, Q = z.real.astype(np.float32), z.imag.astype(np.float32)
    return I, Q, I.astype(np.float64) + 1j * Q.astype(np.float64)


def odd_rows(np_, seed):
    """Three rows of np_ samples within +-0.4 with the values a float row can hold sprinkled in: NaN, +-Inf, denormals,
    1e30 and -0.0, at the row's first and last samples among others."""
    rng = np.random.default_rng(seed)
    I = rng.uniform(-0.4, 0.4, (3, np_)).astype(np.float32)
    Q = rng.uniform(-0.4, 0.4, (3, np_)).astype(np.float32)
    odd = [np.nan, np.inf, -np.inf, 1e-42, -1e-45, 1e30, -1e30, -0.0, 3e38]
    for s in range(3):
        for j, v in enumerate(odd):
            if np_ == 0:
                break
            at = [0, np_ - 1, np_ // 2, (7 * j + 3 * s) % np_, (64 * j + 63 + s) % np_][(j + s) % 5]
            (I if (j + s) & 1 else Q)[s, at] = np.float32(v)
    return I, Q


# ---- the three scenes of audio_lib (messages, SNRs, offsets, times) as IQ rows by tests/synth.py ---------------------------
@functools.lru_cache(maxsize=None)
def scene(k):
    """Scene k as the decoder's rows: synth.py's signal model and noise (unit power in 2 500 Hz) and the receiver's
    normalisation, for audio_lib.scene_items(k).  (I, Q) float32 [45000], read-only.  The seeds are ones under which these
    rows, decoded AS THEY ARE by the CPU oracle, meet the tolerances test_audio_checker.py states for its scenes: the
    decoder's own scatter of dt at -22 and -26 dB reaches 0.1 s (8300 + k: -0.101 s in scene 1, 8320 + k: +0.112 s in
    scene 2, before any audio is involved)."""
    rng = np.random.default_rng(8310 + k)
    sigma = np.sqrt((375.0 / 2500.0) / 2.0)
    I = rng.normal(0.0, sigma, synth.NS)
    Q = rng.normal(0.0, sigma, synth.NS)
    for msg, snr, f0, t0 in al.scene_items(k):
        ok, sym = ol.channel_symbols(msg)
        assert ok, msg
        si, sq = synth.tone_signal(sym, f0, t0, 10.0 ** (snr / 20.0))
        I += si
        Q += sq
    I, Q = synth.normalise(I.astype(np.float32), Q.astype(np.float32))
    I.setflags(write=False)
    Q.setflags(write=False)
    return I, Q


@functools.lru_cache(maxsize=None)
def scene_record(k):
    """The checker's record of scene k at gain 32768: (pcm int16 [1 440 000] read-only, n_clipped)."""
    rc, pcm, count = check_rows(*scene(k))
    assert rc == 0
    pcm.setflags(write=False)
    return pcm[0], int(count[0])


@functools.lru_cache(maxsize=None)
def scene_spots(k, loop):
    """The CPU oracle's spots of scene k: of its rows as they are, or (loop) of K12's checker rows, normalised, of
    scene_record(k)."""
    if not loop:
        I, Q = scene(k)
        return ol.decode(I, Q)[0]
    I, Q = al.check_rows(scene_record(k)[0], normalise=1)
    return ol.decode(I[0], Q[0])[0]
