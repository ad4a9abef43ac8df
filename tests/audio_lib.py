"""ctypes bindings of the audio front end's checker (tests/helpers/audio_check.c: the contract of wspr_audio_*() in plain
serial C over rtlsdr-wsprd_amd/csrc/kernels/audio_front.h), built on demand, and the audio scene generator the front
end's tests share.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os
import subprocess
import tempfile
import wave

import numpy as np

import oracle_lib as ol

RATE = 12000
NSAMP = 1440000                 # 120 s
NOUT = 45000
NTAPS = 511
DECIM = 32
SPS = 8192                      # audio samples per WSPR symbol: 12000 / 8192 = 375 / 256 baud
DIAL_HZ = 144489000             # oracle_lib.default_options()

_lib = None


def checker():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="wspr_audio_"), "libaudiocheck.so")
        # -mfma only makes fmaf() one instruction instead of a call of the C library's (correctly rounded either way)
        fast = ["-mfma"] if ol.cpu_has_fma() else []
        subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall"] + fast +
                       ["-I", os.path.join(ol.ROOT, "rtlsdr-wsprd_amd", "csrc", "kernels"), "-shared", "-o", out,
                        os.path.join(ol.ROOT, "tests", "helpers", "audio_check.c"), "-lm"], check=True)
        X = C.CDLL(out)
        X.audio_check_rows.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        X.audio_check_rows.restype = C.c_int
        X.audio_check_taps.argtypes = [C.c_void_p, C.c_void_p]
        X.audio_check_tile.restype = C.c_int
        _lib = X
    return _lib


def tile():
    """The kernel's outputs per workgroup (AUDIO_FRONT_TILE)."""
    return int(checker().audio_check_tile())


def taps():
    """(gI, gQ): the committed tables as float32 arrays of 511, index k + 255."""
    gi = np.zeros(NTAPS, np.float32)
    gq = np.zeros(NTAPS, np.float32)
    checker().audio_check_taps(ol.ptr(gi), ol.ptr(gq))
    return gi, gq


def n_out(nsamp):
    return min((nsamp + DECIM - 1) // DECIM, NOUT)


def check_rows(pcm, nsamp=None, normalise=0, out_stride=NOUT):
    """The checker on int16 records [nseg, stride] (or one record), of which the first nsamp samples count.
    Returns (I, Q) as float32 [nseg, out_stride]."""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    if pcm.ndim == 1:
        pcm = pcm[None, :]
    nseg, stride = pcm.shape
    nsamp = stride if nsamp is None else int(nsamp)
    I = np.full((nseg, out_stride), np.nan, np.float32)
    Q = np.full((nseg, out_stride), np.nan, np.float32)
    rc = checker().audio_check_rows(ol.ptr(pcm), stride, nsamp, nseg, ol.ptr(I), ol.ptr(Q), out_stride, int(normalise))
    assert rc == 0, rc
    return I, Q


# ---- impulses: 16384 at one sample of an otherwise silent record ---------------------------------------------------
IMPULSES = (0, 1, 31, 32, 255, 256, -1)


def impulse_rows(nsamp):
    """(pcm [7, nsamp], expected I, expected Q): 16384 at one sample of each row; the expected rows straight from the table."""
    gi, gq = taps()
    pcm = np.zeros((len(IMPULSES), nsamp), np.int16)
    ei = np.zeros((len(IMPULSES), NOUT), np.float32)
    eq = np.zeros((len(IMPULSES), NOUT), np.float32)
    for r, n in enumerate(IMPULSES):
        n = n % nsamp
        pcm[r, n] = 16384
        for m in range(n_out(nsamp)):
            if abs(n - 32 * m) <= 255:
                ei[r, m] = np.float32(0.5) * gi[n - 32 * m + 255]
                eq[r, m] = np.float32(0.5) * gq[n - 32 * m + 255]
    return pcm, ei, eq


# ---- audio scenes ---------------------------------------------------------------------------------------------------
# (message, f0 Hz from 1 500 Hz, t0 s) of the three signals every scene holds, and the SNR of each scene
SIGNALS = [("K1JT FN20 20", -104.3, 2.0), ("W1AW FN31 37", 21.7, 1.4), ("G4ABC IO91 23", 107.9, 2.9)]
SCENE_SNRS = [-15.0, -22.0, -26.0]
SCENE_MESSAGES = [["K1JT FN20 20", "W1AW FN31 37", "G4ABC IO91 23"],
                  ["VA2GKA FN35 30", "JA1XYZ PM95 10", "K9AN EN50 33"],
                  ["DL0ABC JO62 27", "VK2AB QF56 40", "ZS6BKW KG33 17"]]


def audio_scene(items, seed):
    """One record of NSAMP int16 samples: for each (message, snr dB in 2 500 Hz, f0, t0) continuous-phase 4-FSK at
    1500 + f0 Hz with SPS samples per symbol and amplitude sqrt(2) 10^(snr/20), over real white noise of variance 2.4
    (unit power in 2 500 Hz of the 6 000 Hz the record spans); scaled by 2000, rounded, clipped to int16."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, np.sqrt(2.4), NSAMP)
    for msg, snr, f0, t0 in items:
        ok, sym = ol.channel_symbols(msg)
        assert ok, msg
        f = 1500.0 + f0 + (np.repeat(np.asarray(sym, np.float64), SPS) - 1.5) * (RATE / SPS)
        dphi = 2.0 * np.pi * f / RATE
        phi = np.concatenate(([0.0], np.cumsum(dphi)[:-1]))
        start = int(round(t0 * RATE))
        idx = start + np.arange(phi.size)
        keep = (idx >= 0) & (idx < NSAMP)
        x[idx[keep]] += np.sqrt(2.0) * 10.0 ** (snr / 20.0) * np.cos(phi[keep])
    return np.clip(np.rint(x * 2000.0), -32768, 32767).astype(np.int16)


def scene_items(k):
    return [(SCENE_MESSAGES[k][j], SCENE_SNRS[k], SIGNALS[j][1], SIGNALS[j][2]) for j in range(3)]


@functools.lru_cache(maxsize=None)
def scene(k):
    """Scene k of the three the front end's tests share (read-only)."""
    pcm = audio_scene(scene_items(k), 7100 + k)
    pcm.setflags(write=False)
    return pcm


@functools.lru_cache(maxsize=None)
def scene_rows(k, normalise):
    """The checker's rows of scene k (read-only)."""
    I, Q = check_rows(scene(k), normalise=normalise)
    I.setflags(write=False)
    Q.setflags(write=False)
    return I[0], Q[0]


@functools.lru_cache(maxsize=None)
def scene_oracle(k, normalise):
    """The CPU oracle's spots for the checker's rows of scene k."""
    I, Q = scene_rows(k, normalise)
    return ol.decode(I, Q)[0]


def spot_offset_hz(s):
    """A spot's frequency as Hz from the band centre."""
    return s.freq * 1e6 - DIAL_HZ - 1500.0


def expected_text(msg):
    c, g, p = msg.split()
    return "%s %s %02d" % (c, g, int(p))


def find_sent(spots, items):
    """For every sent (message, snr, f0, t0) the spot that carries it, or None."""
    out = []
    for msg, snr, f0, t0 in items:
        hit = [s for s in spots if s.message.decode().strip() == expected_text(msg)]
        out.append(hit[0] if hit else None)
    return out


def write_wav(path, pcm, rate=RATE, channels=1, width=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm).tobytes())
