"""What the Doppler-spread tests and tools share (tests/test_spread_checker.py, tests/test_gpu_spread.py,
tools/spread_curve.py): the serial CPU checker tests/helpers/spread_check.c behind ctypes (the definition of
rtlsdr-wsprd_amd/csrc/kernels/spread.h, built on demand), and faded single-signal scenes.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = 45000
NSYM = 162
SIGLEN = 162 * 256
DELTA = 375.0 / 32.0 / 2048.0                      # Hz per bin of the spread spectrum
GAUSS_W50 = 1.349                                  # the middle half of a Gaussian spectrum is 1.349 sigma wide

# include/wspr_mi355x.h: wspr_spread_item, wspr_spread
ITEM_DTYPE = np.dtype([("seg", "<i4"), ("f0", "<f4"), ("shift", "<i4"), ("drift", "<f4"), ("symbols", "u1", (NSYM,)),
                       ("pad", "u1", (2,))])
RESULT_DTYPE = np.dtype([("w50", "<f4"), ("f50", "<f4"), ("ratio", "<f4"), ("valid", "<i4"), ("f0", "<f4"), ("shift", "<i4"),
                         ("drift", "<f4"), ("pad", "<i4")])
assert ITEM_DTYPE.itemsize == 180 and RESULT_DTYPE.itemsize == 32


@functools.lru_cache(maxsize=None)
def checker():
    out = os.path.join(tempfile.mkdtemp(prefix="wspr_spread_"), "libspreadcheck.so")
    subprocess.run(["g++", "-x", "c++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                    "-Wno-unused-function", "-I", os.path.join(ROOT, "rtlsdr-wsprd_amd", "csrc", "kernels"), "-shared", "-o", out,
                    os.path.join(ROOT, "tests", "helpers", "spread_check.c"), "-lm"], check=True)
    X = C.CDLL(out)
    X.spread_check.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                               C.c_void_p]
    X.spread_check.restype = C.c_int
    return X


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def check_words(I, Q, f0, shift, drift, symbols, np_=None, power=False):
    """The checker on one job over the row (I, Q) of np_ samples (default: all of it): the four result words as uint32
    [4] -- w50, f50, ratio as float bits, valid[, P float32 [2048] for j = -1024 .. 1023]."""
    I = np.ascontiguousarray(I, np.float32)
    Q = np.ascontiguousarray(Q, np.float32)
    sym = np.ascontiguousarray(symbols, np.uint8)
    assert sym.size == NSYM
    out = np.zeros(4, np.uint32)
    P = np.zeros(2048, np.float32) if power else None
    rc = checker().spread_check(_ptr(I), _ptr(Q), int(I.size if np_ is None else np_), float(f0), int(shift), float(drift),
                                _ptr(sym), _ptr(out), _ptr(P) if power else None)
    assert rc == 0
    return (out, P) if power else out


def unpack_words(words):
    """(w50, f50, ratio, valid) of four result words."""
    w = np.ascontiguousarray(words, np.uint32)
    f = w.view(np.float32)
    return float(f[0]), float(f[1]), float(f[2]), int(w[3])


def check(I, Q, f0, shift, drift, symbols, np_=None):
    return unpack_words(check_words(I, Q, f0, shift, drift, symbols, np_))


def record_words(rec):
    """The four result words of wspr_spread records (numpy RESULT_DTYPE): uint32 [..., 4]."""
    r = np.asarray(rec)
    return np.ascontiguousarray(r).reshape(-1).view(np.uint32).reshape(r.shape + (8,))[..., :4]


def fading(rng, sigma_hz, n=NS):
    """A complex Gaussian process of unit mean power whose Doppler spectrum is Gaussian with standard deviation sigma_hz
    (375 samples per second); sigma_hz = 0: the constant 1."""
    if sigma_hz <= 0:
        return np.ones(n, np.complex128)
    m = 1 << int(np.ceil(np.log2(2 * n)))              # twice the length: the circular process is cut, not wrapped
    w = rng.normal(size=m) + 1j * rng.normal(size=m)
    f = np.fft.fftfreq(m, 1.0 / 375.0)
    g = np.fft.ifft(np.fft.fft(w) * np.exp(-f * f / (4.0 * sigma_hz * sigma_hz)))[:n]
    shape = np.exp(-f * f / (2.0 * sigma_hz * sigma_hz))
    return g / np.sqrt(2.0 * shape.sum() / m)          # E|g|^2 = 2 * sum(shape) / m before the scaling


def faded_segment(seed, symbols, f0, t0=2.0, snr_db=-15.0, sigma_hz=0.0, noise=True):
    """One tests/synth.py signal times fading(sigma_hz) in the noise of synth.make_segment() (power 1 in 2 500 Hz), float32
    rows, and the frame's first sample index.  noise=False: the signal alone."""
    rng = np.random.default_rng(seed)
    si, sq = synth.tone_signal(symbols, f0, t0, 10.0 ** (snr_db / 20.0))
    z = (si + 1j * sq) * fading(rng, sigma_hz)
    if noise:
        s = np.sqrt((375.0 / 2500.0) / 2.0)
        z = z + rng.normal(0.0, s, NS) + 1j * rng.normal(0.0, s, NS)
    return z.real.astype(np.float32), z.imag.astype(np.float32), int(round(t0 * 375.0))
