"""ctypes bindings of the band noise figures' checker (tests/helpers/noise_check.c: the contract of wspr_noise*() in plain
serial code over rtlsdr-wsprd_amd/csrc/kernels/noise.h), built on demand; a numpy restatement of the same definition as a
second, independent statement; the crafted rows, the window cases and the white-noise rows the tests share.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as ol

NS = 45000
BLOCK, NBLOCKS = 16, 2812
NFFT, HOP, CLASSES = 512, 256, 4
BAND_HALF, BAND, LOWEST = 221, 443, 132
PRE_USED, POST_USED, FFT_USED, NONFINITE = 1, 2, 4, 8
DEFAULT_WINDOWS = (6, 42, 2672, 2790)
LENGTHS = [0, 15, 16, 511, 512, 767, 768, 44999, 45000]
NOISE_DTYPE = np.dtype([("pre_mean", "<f4"), ("pre_trough", "<f4"), ("post_mean", "<f4"), ("post_trough", "<f4"),
                        ("fft_floor", "<f4"), ("fft_p30", "<f4"), ("nframes", "<i4"), ("flags", "<i4")])
FIGURES = ("pre_mean", "pre_trough", "post_mean", "post_trough", "fft_floor", "fft_p30")
SIGMA = float(np.sqrt((375.0 / 2500.0) / 2.0))           # tests/synth.py: noise power 1 in 2500 Hz, per rail

# (name, windows): the default twice (explicit), empty, clipped away by a short row, overlapping, the whole row, one block
WINDOW_CASES = [("default", DEFAULT_WINDOWS), ("both_empty", (0, 0, 2812, 2812)), ("empty_in_the_middle", (100, 100, 7, 7)),
                ("whole_row_twice", (0, 2812, 0, 2812)), ("overlapping", (100, 200, 150, 2812)),
                ("last_block_first_block", (2811, 2812, 0, 1)), ("clipped_by_a_short_row", (0, 40, 30, 2000))]

_lib = None
_SRC = os.path.join(ol.ROOT, "tests", "helpers", "noise_check.c")
_INC = os.path.join(ol.ROOT, "rtlsdr-wsprd_amd", "csrc", "kernels")
_FLAGS = ["-x", "c++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", _INC]


def checker():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="wspr_noise_"), "libnoisecheck.so")
        subprocess.run(["g++"] + _FLAGS + ["-O2", "-fPIC", "-shared", "-o", out, _SRC], check=True)
        X = C.CDLL(out)
        X.noise_check_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
        X.noise_check_rows.restype = C.c_int
        X.noise_check_detail.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
        X.noise_check_detail.restype = C.c_int
        X.noise_check_default_windows.argtypes = [C.c_void_p]
        X.noise_check_w2.restype = C.c_double
        w = np.zeros(4, np.int32)
        X.noise_check_default_windows(ol.ptr(w))
        assert tuple(w.tolist()) == DEFAULT_WINDOWS
        _lib = X
    return _lib


def sanitizer_program(directory):
    """The checker as a stand-alone program (its own main) under AddressSanitizer and UBSan: the path of the executable."""
    exe = os.path.join(str(directory), "noise_check_asan")
    subprocess.run(["g++"] + _FLAGS + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                       "-DNOISE_CHECK_MAIN", "-o", exe, _SRC], check=True)
    return exe


def _win(windows):
    return None if windows is None else np.array(windows, np.int32)


def check_rows(I, Q, samples, windows=None):
    """The checker on float32 rows [nseg, stride] of which the first `samples` count: a NOISE_DTYPE array [nseg]."""
    I = np.ascontiguousarray(I, np.float32)
    Q = np.ascontiguousarray(Q, np.float32)
    if I.ndim == 1:
        I, Q = I[None, :], Q[None, :]
    nseg, stride = I.shape
    out = np.zeros(nseg, NOISE_DTYPE)
    w = _win(windows)
    rc = checker().noise_check_rows(ol.ptr(I), ol.ptr(Q), nseg, int(samples), stride, None if w is None else ol.ptr(w),
                                    ol.ptr(out))
    assert rc == 0, rc
    return out


def detail(I, Q, samples, windows=None):
    """One row: (record, p[2812], a[512] for j = -256 .. 255, rank[443] for j = -221 .. 221) of the checker."""
    I = np.ascontiguousarray(I, np.float32)
    Q = np.ascontiguousarray(Q, np.float32)
    out = np.zeros(1, NOISE_DTYPE)
    p = np.zeros(NBLOCKS, np.float32)
    a = np.zeros(NFFT, np.float32)
    rank = np.zeros(BAND, np.int32)
    w = _win(windows)
    rc = checker().noise_check_detail(ol.ptr(I), ol.ptr(Q), int(samples), None if w is None else ol.ptr(w), ol.ptr(out),
                                      ol.ptr(p), ol.ptr(a), ol.ptr(rank))
    assert rc == 0, rc
    return out[0], p, a, rank


@functools.lru_cache(maxsize=None)
def tables():
    """(w[512] float32, W2) restated: the window from numpy's double cosine, W2 by a serial double sum."""
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT, dtype=np.float64) / 512.0)).astype(np.float32)
    w2 = float(np.cumsum(w.astype(np.float64) ** 2)[-1])
    return w, w2


def frames_of(n):
    return (n - NFFT) // HOP + 1 if n >= NFFT else 0


def gap_numpy(I, Q, n, windows=DEFAULT_WINDOWS):
    """The gap figure restated: (p of every whole block, pre_mean, pre_trough, post_mean, post_trough, flag bits).
    np.cumsum adds serially in double, as the definition does."""
    nblk = n // BLOCK
    x = np.asarray(I[:nblk * BLOCK], np.float64).reshape(nblk, BLOCK)
    y = np.asarray(Q[:nblk * BLOCK], np.float64).reshape(nblk, BLOCK)
    s = np.zeros(nblk)
    for k in range(BLOCK):
        s = s + (x[:, k] * x[:, k] + y[:, k] * y[:, k])
    p = (s / 16.0).astype(np.float32)
    out, flags = [], 0
    for bit, (b0, b1) in ((PRE_USED, windows[:2]), (POST_USED, windows[2:])):
        b1 = min(b1, nblk)
        if b1 > b0:
            seg = p[b0:b1]
            out += [np.float32(np.cumsum(seg.astype(np.float64))[-1] / float(b1 - b0)), seg.min()]
            flags |= bit
        else:
            out += [np.float32(0), np.float32(0)]
    return p, out[0], out[1], out[2], out[3], flags


def spectrum_float64(I, Q, n):
    """a[j], j = -256 .. 255, in float64 with numpy.fft: the float32 window values, everything else double.  Also T, the
    sum over the frames of the whole spectrum's energy (for the error bound)."""
    w, w2 = tables()
    nf = frames_of(n)
    if nf == 0:
        return np.zeros(NFFT), 0.0, 0
    idx = HOP * np.arange(nf)[:, None] + np.arange(NFFT)[None, :]
    z = (np.asarray(I, np.float64)[idx] + 1j * np.asarray(Q, np.float64)[idx]) * w.astype(np.float64)[None, :]
    P = np.abs(np.fft.fft(z, axis=1)) ** 2
    A = np.fft.fftshift(P.sum(axis=0))
    return A / nf / w2, float(P.sum()), nf


def spectrum_tolerance(a64, total, nf):
    """The largest |a - a64| the nine float32 stages can cause, per bin.  u = 2^-24.  One frame's transform computed in
    float32 by radix 2 has, norm-wise, ||dX|| <= 9 eta ||X|| with eta = mu + gamma_4 (sqrt 2 + mu) (Higham, Accuracy and
    Stability of Numerical Algorithms, 2nd ed., theorem 24.2; nine stages; mu = u the twiddles' error, gamma_4 = 4u/(1 - 4u)):
    eta < 6.7 u; the window product adds u: e = 61.3 u.  A single bin's error is at most the norm: |dX_f[j]| <= e ||X_f||.
    So |dA[j]| <= sum_f (2 |X_f[j]| e ||X_f|| + e^2 ||X_f||^2) + 4u A[j] (the two squares, their sum, the conversion)
              <= 2 e sqrt(A[j] T) + e^2 T + 4u A[j]   (Cauchy-Schwarz; T = sum_f ||X_f||^2),
    and a[j] = A[j] / nframes / W2 adds 2u a[j] for the final rounding and the float64 reference's own error."""
    w, w2 = tables()
    u = 2.0 ** -24
    e = 61.3 * u
    A = a64 * nf * w2
    return (2.0 * e * np.sqrt(A * total) + e * e * total + 4.0 * u * A) / max(nf, 1) / w2 + 2.0 * u * a64


def band_numpy(a):
    """Ranks, fft_floor and fft_p30 restated on a[512] (float32, j = -256 .. 255): a stable sort of the bit patterns."""
    band = np.ascontiguousarray(a[NFFT // 2 - BAND_HALF:NFFT // 2 + BAND_HALF + 1], np.float32)
    order = np.argsort(band.view(np.uint32), kind="stable")
    rank = np.empty(BAND, np.int32)
    rank[order] = np.arange(BAND)
    ranked = band[order]
    floor = np.float32(np.cumsum(ranked[:LOWEST].astype(np.float64))[-1] / 132.0)
    return rank, floor, ranked[LOWEST]


def has_non_finite(I, Q, n):
    bits = np.concatenate((np.asarray(I[:n], np.float32).view(np.uint32), np.asarray(Q[:n], np.float32).view(np.uint32)))
    return bool((((bits >> 23) & 0xff) == 0xff).any())


# ---- rows ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def white_rows(nrows=64, seed=4242, sigma=SIGMA):
    """(I, Q) float32 [nrows, 45000]: tests/synth.py's noise, N(0, sigma^2) per rail, nothing else.  Read-only."""
    rng = np.random.default_rng(seed)
    I = rng.normal(0, sigma, (nrows, NS)).astype(np.float32)
    Q = rng.normal(0, sigma, (nrows, NS)).astype(np.float32)
    I.setflags(write=False)
    Q.setflags(write=False)
    return I, Q


@functools.lru_cache(maxsize=None)
def random_rows(nrows=3, seed=99):
    """(I, Q) [nrows, 45000]: noise whose level changes along the row (so the troughs, the windows and the ranks have
    something to find) plus two tones; every row its own.  Read-only."""
    rng = np.random.default_rng(seed)
    t = np.arange(NS) / 375.0
    I = np.zeros((nrows, NS), np.float32)
    Q = np.zeros((nrows, NS), np.float32)
    for s in range(nrows):
        env = 0.05 + 0.2 * (1.0 + np.sin(2 * np.pi * t / (7.0 + s))) + (t > 60.0 + s) * 0.3
        z = env * (rng.normal(0, 1, NS) + 1j * rng.normal(0, 1, NS))
        z += 0.8 * np.exp(2j * np.pi * (31.7 + s) * t) + 0.1 * np.exp(-2j * np.pi * 100.2 * t)
        I[s], Q[s] = z.real.astype(np.float32), z.imag.astype(np.float32)
    I.setflags(write=False)
    Q.setflags(write=False)
    return I, Q


@functools.lru_cache(maxsize=None)
def crafted_rows():
    """[(name, I, Q)] of 45000 samples: all zeros (every bin ties: rank order is j order), a constant, a complex tone on a
    bin centre (j = 40) and one half-way between two bins (j = -60.5)."""
    n = np.arange(NS, dtype=np.float64)
    rows = [("zeros", np.zeros(NS, np.float32), np.zeros(NS, np.float32)),
            ("constant", np.full(NS, 0.25, np.float32), np.full(NS, -0.125, np.float32))]
    for name, j in (("tone_on_bin_40", 40.0), ("tone_between_bins", -60.5)):
        z = 0.5 * np.exp(2j * np.pi * j * n / 512.0)
        rows.append((name, z.real.astype(np.float32), z.imag.astype(np.float32)))
    for _, I, Q in rows:
        I.setflags(write=False)
        Q.setflags(write=False)
    return rows


def non_finite_cases(n):
    """[(name, index, value, counts)]: a NaN, a +Inf and a -Inf at sample 0, at n - 1 and at n (the last must not count)."""
    vals = (("nan", np.float32(np.nan)), ("pinf", np.float32(np.inf)), ("ninf", np.float32(-np.inf)))
    return [("%s_at_%s" % (vn, where), k, v, counts) for vn, v in vals
            for where, k, counts in (("0", 0, True), ("last", n - 1, True), ("behind", n, False))]


@functools.lru_cache(maxsize=None)
def white_noise_statistics():
    """The checker's figures over white_rows() relative to 2 sigma^2: {figure: (mean ratio, relative standard deviation)}.
    The means' scatter is ALSO known in closed form (mean_scatter()); the troughs' and the spectrum figures' is measured
    here, on the checker, once for every test that needs it."""
    I, Q = white_rows()
    rec = check_rows(I, Q, NS)
    ref = 2.0 * SIGMA * SIGMA
    return {f: (float(np.mean(rec[f].astype(np.float64) / ref)), float(np.std(rec[f].astype(np.float64) / ref, ddof=1)))
            for f in FIGURES}


def mean_scatter(blocks):
    """Relative standard deviation of the mean of |z|^2 over `blocks` blocks of white complex Gaussian noise: |z|^2 is
    exponential (mean 2 s^2, standard deviation 2 s^2), the samples are independent: 1 / sqrt(16 blocks)."""
    return 1.0 / np.sqrt(BLOCK * blocks)


def crowd_items(nseg, sigma):
    """A crowded band for the synthesiser: ten strong signals per row, +0 .. +9 dB in 2 500 Hz over noise of `sigma` per
    rail, 24 Hz apart over +-110 Hz, starting between 1.0 and 2.8 s (dt -1.0 .. +0.8): [(seg, f0, t0, amp, drift, symbols)]."""
    import synth
    items = []
    ref = 2.0 * sigma * sigma * 2500.0 / 375.0
    for s in range(nseg):
        for k in range(10):
            ok, sym = ol.channel_symbols(synth.message_for(17 * s + k))
            assert ok
            items.append((s, -110.0 + 24.0 * k + 0.7 * s, 1.0 + 0.2 * k, float(np.sqrt(ref * 10.0 ** (k / 10.0))), 0.0, sym))
    return items
