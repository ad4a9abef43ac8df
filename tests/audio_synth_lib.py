"""ctypes bindings of the audio scene synthesiser's checker (tests/helpers/audio_synth_check.cpp: the contract of
wspr_synth_audio*() in plain serial C++ over rtlsdr-wsprd_amd/csrc/kernels/audio_synth.h and synth_math.h), built on demand;
a numpy restatement of the noise-free waveform as a second, independent statement; the scenes the synthesiser's tests share.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import math
import os
import subprocess
import tempfile

import numpy as np

import audio_lib as al
import oracle_lib as ol
import synth_lib as sl

ACCUMULATE = 1
SPS = al.SPS
SIGLEN = 162 * SPS              # 1 327 104 samples of one transmission
TILE = 2048                     # samples per workgroup of the kernel (kAudioSynthTile)
PER_THREAD = 8                  # samples per thread
SENTINEL = 0x7A5A
SIGMA = 2000.0 * math.sqrt(2.4)  # the noise of audio_lib.audio_scene() in PCM units

_lib = None
_SRC = os.path.join(ol.ROOT, "tests", "helpers", "audio_synth_check.cpp")
_INC = os.path.join(ol.ROOT, "rtlsdr-wsprd_amd", "csrc", "kernels")
_FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-I", _INC]


def checker():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="wspr_asynth_"), "libaudiosynthcheck.so")
        subprocess.run(["g++", "-O2", "-fPIC", "-shared"] + _FLAGS + ["-o", out, _SRC], check=True)
        X = C.CDLL(out)
        X.audio_synth_check_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int,
                                              C.c_void_p, C.c_size_t, C.c_void_p]
        X.audio_synth_check_batch.restype = C.c_int
        X.audio_synth_check_quantise.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        X.audio_synth_check_quantise.restype = None
        X.audio_synth_check_first.argtypes = [C.c_float]
        X.audio_synth_check_first.restype = C.c_int
        X.audio_synth_check_gauss.argtypes = [C.c_uint64, C.c_longlong, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
        X.audio_synth_check_gauss.restype = None
        _lib = X
    return _lib


def sanitizer_program(directory):
    """The checker as a stand-alone program (its own main) under AddressSanitizer and UBSan: the path of the executable."""
    exe = os.path.join(str(directory), "audio_synth_check_asan")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DAUDIO_SYNTH_CHECK_MAIN"] + _FLAGS + ["-o", exe, _SRC], check=True)
    return exe


def round8(n):
    return (n + 7) & ~7


def check_batch(items, nseg, nsamp, seg_index0=0, sigma=0.0, seed=0, flags=0, rows=None, stride=None):
    """The checker on nseg records [nseg, stride] (given rows are copied; they matter with ACCUMULATE; fresh rows are filled
    with SENTINEL).  Returns (rc, rows, n_clipped)."""
    stride = (round8(nsamp) if stride is None else int(stride)) if rows is None else np.asarray(rows).shape[-1]
    if rows is None:
        out = np.full((nseg, stride), SENTINEL, np.int16)
    else:
        out = np.array(rows, np.int16).reshape(nseg, stride).copy()
    count = np.full(max(nseg, 1), -1, np.int32)
    arr = sl.tx_list(items)
    rc = checker().audio_synth_check_batch(C.addressof(arr), len(items), nseg, seg_index0, int(nsamp), sigma, seed, flags,
                                           ol.ptr(out), stride, ol.ptr(count))
    return rc, out, count[:nseg]


def quantise(acc):
    """audio_synth_quantise() on float64 values: (int16 samples, clipped count)."""
    acc = np.ascontiguousarray(acc, np.float64)
    out = np.zeros(acc.size, np.int16)
    n = C.c_int(-1)
    checker().audio_synth_check_quantise(ol.ptr(acc), int(acc.size), ol.ptr(out), C.addressof(n))
    return out, int(n.value)


def first_index(t0):
    return int(checker().audio_synth_check_first(t0))


def gauss(seed, S, m, sigma):
    """The float32 pair (a, b) of sample pair m of global segment S."""
    a, b = C.c_float(0), C.c_float(0)
    checker().audio_synth_check_gauss(seed, S, m, sigma, C.addressof(a), C.addressof(b))
    return a.value, b.value


def philox_pairs(seed, S, m, stream=0x80000000):
    """Philox-4x32-10 restated with numpy for counters (m[i], stream, S low, S high) under the seed's key, and the
    Box-Muller of the contract in float64: (a, b) of unit variance for each m.  Independent of synth_math.h."""
    m = np.asarray(m, np.uint64)
    mask = np.uint64(0xFFFFFFFF)
    c0, c1 = m & mask, np.full(m.shape, stream, np.uint64)
    c2, c3 = np.full(m.shape, S & 0xFFFFFFFF, np.uint64), np.full(m.shape, (S >> 32) & 0xFFFFFFFF, np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    u = (c0.astype(np.float64) * 4294967296.0 + c1.astype(np.float64) + 1.0) * 2.0 ** -64
    rad = np.sqrt(-2.0 * np.log(u))
    theta = (c2.astype(np.float64) + 0.5) * (2.0 * np.pi / 4294967296.0)
    return rad * np.cos(theta), rad * np.sin(theta)


def amp_of(snr_db, sigma):
    """The level convention, stated here on its own: sigma^2 * 2500/6000 is the noise power in 2 500 Hz, amp^2/2 the signal's."""
    return sigma * math.sqrt(2.0 * 2500.0 / 6000.0) * 10.0 ** (snr_db / 20.0)


@functools.lru_cache(maxsize=None)
def symbols(msg):
    ok, sym = ol.channel_symbols(msg)
    assert ok, msg
    return tuple(int(v) for v in sym)


def item(seg, msg, f0, t0, amp, drift=0.0):
    return (seg, f0, t0, amp, drift, symbols(msg))


def numpy_record(items, nsamp):
    """The noise-free record of `items` (all of one segment) by an independent formulation: phases as a cumulative sum in
    the widest float numpy has, numpy's cos, np.rint.  No shared header, no serial phase table, no magic-number rounding."""
    wide = np.longdouble
    acc = np.zeros(nsamp, wide)
    two_pi = 2 * np.arccos(wide(-1))
    for _, f0, t0, amp, drift, sym in items:
        f0, t0, amp, drift = (float(np.float32(v)) for v in (f0, t0, amp, drift))
        i = np.arange(162)
        f = wide(1500.0) + wide(f0) + wide(drift) / 2 * (i - 81) / wide(81) + (np.asarray(sym, wide) - wide(1.5)) * (wide(12000) / 8192)
        dphi = two_pi * f / wide(12000)
        start = np.concatenate(([wide(0)], np.cumsum(dphi * 8192)[:-1]))
        first = math.floor(t0 * 12000.0)
        lo, hi = max(0, first), min(nsamp, first + SIGLEN)
        if lo >= hi:
            continue
        n = np.arange(lo - first, hi - first)
        phi = start[n >> 13] + (n & 8191) * dphi[n >> 13]
        acc[lo:hi] += wide(amp) * np.cos(phi)
    return np.clip(np.rint(acc), -32768, 32767).astype(np.int16)


# ---- the three audio_lib scenes through the synthesiser: audio_lib's messages, offsets, times and SNRs at its noise level ----
def scene_items(k, seg=0):
    return [item(seg, msg, f0, t0, amp_of(snr, SIGMA)) for msg, snr, f0, t0 in al.scene_items(k)]


SCENE_SEED = 8100


@functools.lru_cache(maxsize=None)
def scene(k):
    """The checker's record of scene k, as global segment k under SCENE_SEED -- row k of one batch call for the three, made
    here as a call of its own (read-only): (pcm, n_clipped)."""
    rc, rows, count = check_batch(scene_items(k), 1, al.NSAMP, seg_index0=k, sigma=SIGMA, seed=SCENE_SEED)
    assert rc == 0
    rows.setflags(write=False)
    return rows[0], int(count[0])


@functools.lru_cache(maxsize=None)
def scene_oracle(k):
    """The CPU oracle's spots for K12's checker rows (normalised) of scene(k)."""
    I, Q = al.check_rows(scene(k)[0], normalise=1)
    return ol.decode(I[0], Q[0])[0]
