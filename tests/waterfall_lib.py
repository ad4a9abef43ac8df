"""ctypes bindings of the waterfall's checker (tests/helpers/waterfall_check.c: the contract of wspr_waterfall*() in plain
serial code over rtlsdr-wsprd_amd/csrc/kernels/waterfall.h and noise.h), built on demand; a numpy float64 restatement of the
same definition as a second, independent statement; the parameter cases, lengths and scenes the tests share.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import noise_lib as nl
import oracle_lib as ol

NS = 45000
NFFT = 512
REF_ABSOLUTE, REF_FLOOR = 0, 1
WRITTEN, NO_REF, NONFINITE = 1, 2, 8
PARAMS_DTYPE = np.dtype([("hop", "<i4"), ("tavg", "<i4"), ("j0", "<i4"), ("j1", "<i4"), ("ref_mode", "<i4"),
                         ("ref", "<f4"), ("db_min", "<f4"), ("db_step", "<f4")])
INFO_DTYPE = np.dtype([("ref", "<f4"), ("nframes", "<i4"), ("nrows", "<i4"), ("flags", "<i4")])
DEFAULTS = dict(hop=128, tavg=1, j0=-150, j1=150, ref_mode=REF_FLOOR, ref=1.0, db_min=-10.0, db_step=0.25)
HOPS, TAVGS = (128, 256), (1, 2, 3, 16)
# (-150, 150) and (-149, 150): an odd and an even number of columns, so image rows and tiles start on every byte alignment
COLUMNS = [(-256, 255), (0, 0), (-256, -256), (255, 255), (-150, 150), (-149, 150)]
SIGMA = 0.02

_lib = None
_SRC = os.path.join(ol.ROOT, "tests", "helpers", "waterfall_check.c")
_INC = os.path.join(ol.ROOT, "rtlsdr-wsprd_amd", "csrc", "kernels")
_FLAGS = ["-x", "c++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", _INC]


def checker():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="wspr_waterfall_"), "libwaterfallcheck.so")
        subprocess.run(["g++"] + _FLAGS + ["-O2", "-fPIC", "-shared", "-o", out, _SRC], check=True)
        X = C.CDLL(out)
        X.waterfall_check_default_params.argtypes = [C.c_void_p]
        X.waterfall_check_levels.argtypes = [C.c_float, C.c_float, C.c_void_p]
        X.waterfall_check_level_of_ratio.argtypes = [C.c_double, C.c_float, C.c_float]
        X.waterfall_check_level_of_ratio.restype = C.c_int
        X.waterfall_check_level.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float]
        X.waterfall_check_level.restype = C.c_int
        X.waterfall_check_shape.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        X.waterfall_check_shape.restype = C.c_int
        X.waterfall_check_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p,
                                           C.c_size_t, C.c_void_p]
        X.waterfall_check_rows.restype = C.c_int
        X.waterfall_check_detail.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]
        X.waterfall_check_detail.restype = C.c_int
        d = np.zeros(1, PARAMS_DTYPE)
        X.waterfall_check_default_params(ol.ptr(d))
        assert d.tobytes() == params().tobytes(), d
        _lib = X
    return _lib


def sanitizer_program(directory):
    """The checker as a stand-alone program (its own main) under AddressSanitizer and UBSan: the path of the executable."""
    exe = os.path.join(str(directory), "waterfall_check_asan")
    subprocess.run(["g++"] + _FLAGS + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                       "-DWATERFALL_CHECK_MAIN", "-o", exe, _SRC], check=True)
    return exe


def params(**kw):
    """A PARAMS_DTYPE array of one record: the defaults with the given fields replaced."""
    d = dict(DEFAULTS)
    assert not set(kw) - set(d), kw
    d.update(kw)
    p = np.zeros(1, PARAMS_DTYPE)
    for k, v in d.items():
        p[0][k] = v
    return p


def _pptr(p):
    return None if p is None else ol.ptr(p)


def frames_of(n, hop):
    return (n - NFFT) // hop + 1 if n >= NFFT else 0


def shape_formula(n, p=None):
    p = params() if p is None else p
    return frames_of(n, int(p[0]["hop"])) // int(p[0]["tavg"]), int(p[0]["j1"]) - int(p[0]["j0"]) + 1


def lengths(hop, tavg):
    """The row lengths of the issue, in its order (duplicates kept out)."""
    out = []
    for n in (0, 511, 512, 512 + hop - 1, 512 + hop, 512 + hop * tavg - 1, 512 + hop * tavg, 44999, 45000):
        if n not in out:
            out.append(n)
    return out


def check_shape(n, p=None):
    nrows, ncols = C.c_int(-1), C.c_int(-1)
    rc = checker().waterfall_check_shape(int(n), _pptr(p), C.addressof(nrows), C.addressof(ncols))
    return rc, int(nrows.value), int(ncols.value)


def check_rows(I, Q, samples, p=None):
    """The checker on float32 rows [nseg, stride] of which the first `samples` count: (images uint8 [nseg, nrows, ncols],
    INFO_DTYPE array [nseg])."""
    I = np.ascontiguousarray(I, np.float32)
    Q = np.ascontiguousarray(Q, np.float32)
    if I.ndim == 1:
        I, Q = I[None, :], Q[None, :]
    nseg, stride = I.shape
    nrows, ncols = shape_formula(samples, p)
    img = np.zeros((nseg, nrows, ncols), np.uint8)
    info = np.zeros(nseg, INFO_DTYPE)
    rc = checker().waterfall_check_rows(ol.ptr(I), ol.ptr(Q), nseg, int(samples), stride, _pptr(p), ol.ptr(img), nrows * ncols,
                                        ol.ptr(info))
    assert rc == 0, rc
    return img, info


def detail(I, Q, samples, p=None):
    """One row: (image [nrows, ncols], record, m float32 [nrows, ncols], P float32 [nframes, 512] for j = -256 .. 255)."""
    I = np.ascontiguousarray(I, np.float32)
    Q = np.ascontiguousarray(Q, np.float32)
    nrows, ncols = shape_formula(samples, p)
    hop = int((params() if p is None else p)[0]["hop"])
    img = np.zeros((nrows, ncols), np.uint8)
    info = np.zeros(1, INFO_DTYPE)
    m = np.zeros((nrows, ncols), np.float32)
    P = np.zeros((frames_of(samples, hop), NFFT), np.float32)
    rc = checker().waterfall_check_detail(ol.ptr(I), ol.ptr(Q), int(samples), _pptr(p), ol.ptr(img), ol.ptr(info), ol.ptr(m),
                                          ol.ptr(P))
    assert rc == 0, rc
    return img, info[0], m, P


def levels(db_min, db_step):
    """T[0 .. 255] of the checker."""
    T = np.zeros(256, np.float64)
    checker().waterfall_check_levels(float(db_min), float(db_step), ol.ptr(T))
    return T


def levels_numpy(db_min, db_step):
    """T[1 .. 255] restated with numpy's power (may differ from libm's pow in the last place)."""
    i = np.arange(1, 256, dtype=np.float64)
    return np.power(10.0, (float(np.float32(db_min)) + i * float(np.float32(db_step))) / 10.0)


def level_of_ratio(r, db_min, db_step):
    return int(checker().waterfall_check_level_of_ratio(float(r), float(db_min), float(db_step)))


def level(m, ref, db_min, db_step):
    return int(checker().waterfall_check_level(float(m), float(ref), float(db_min), float(db_step)))


def image_float64(I, Q, n, p, ref):
    """The image restated in float64 with numpy.fft: the float32 window values, everything else double, levels counted
    against levels_numpy().  No guard and no flags: for finite rows with a reference.  uint8 [nrows, ncols]."""
    w, w2 = nl.tables()
    hop, tavg, j0, j1 = (int(p[0][k]) for k in ("hop", "tavg", "j0", "j1"))
    nrows = frames_of(n, hop) // tavg
    idx = hop * np.arange(nrows * tavg)[:, None] + np.arange(NFFT)[None, :]
    z = (np.asarray(I, np.float64)[idx] + 1j * np.asarray(Q, np.float64)[idx]) * w.astype(np.float64)[None, :]
    P = np.fft.fftshift(np.abs(np.fft.fft(z, axis=1)) ** 2, axes=1)[:, j0 + 256:j1 + 257]
    m = P.reshape(nrows, tavg, -1).sum(axis=1) / tavg / w2
    T = levels_numpy(p[0]["db_min"], p[0]["db_step"])
    return np.searchsorted(T, m / float(ref), side="right").astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scene_rows(nrows=8, seed=2020):
    """(I, Q) float32 [nrows, 45000]: noise of sigma 0.02 per rail plus three tones of amplitude 0.3, 0.01 and 0.002 at
    frequencies of the row's own inside +-110 Hz.  Read-only."""
    rng = np.random.default_rng(seed)
    t = np.arange(NS) / 375.0
    z = SIGMA * (rng.normal(0, 1, (nrows, NS)) + 1j * rng.normal(0, 1, (nrows, NS)))
    for amp in (0.3, 0.01, 0.002):
        f = rng.uniform(-110, 110, nrows)
        z += amp * np.exp(2j * np.pi * f[:, None] * t[None, :])
    I, Q = z.real.astype(np.float32), z.imag.astype(np.float32)
    I.setflags(write=False)
    Q.setflags(write=False)
    return I, Q


def rows_touching(first, last, hop, tavg, nrows):
    """The image rows whose samples hop*(r*tavg) .. hop*(r*tavg + tavg - 1) + 511 overlap the samples first .. last."""
    return [r for r in range(nrows) if hop * r * tavg <= last and hop * (r * tavg + tavg - 1) + 511 >= first]
