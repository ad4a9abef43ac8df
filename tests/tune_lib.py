"""ctypes bindings of the tunable front end's checker (tests/helpers/tune_check.c: the contract of wspr_tune_u8*() in plain
serial C over rtlsdr-wsprd_amd/csrc/kernels/tune.h), built on demand; a float64 numpy statement of the same definition as a
second, independent one; tone and capture generators the stage's tests share.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import json
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as ol

FS = 2400000.0
SPO = 6400                      # input samples per output
BLOCK_BYTES = 2 * SPO
R = 800                         # vectors per output
NP_MAX = 45000
STRIDE = 45056                  # wspr_iq_stride()
MAX_BANDS = 16
TILE = 4                        # bands per pass of the kernel (k21_tune.hip: kTuneTile)
SCALE = float(np.float32(6401.0 ** 2 / (800.0 ** 2 * 8 * 16384)))

_lib = None
_SRC = os.path.join(ol.ROOT, "tests", "helpers", "tune_check.c")
_FLAGS = ["-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I",
          os.path.join(ol.ROOT, "rtlsdr-wsprd_amd", "csrc", "kernels")]


def checker():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="wspr_tune_"), "libtunecheck.so")
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared"] + _FLAGS + ["-o", out, _SRC, "-lm"], check=True)
        X = C.CDLL(out)
        X.tune_check_rows.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_int, C.c_void_p]
        X.tune_check_rows.restype = C.c_int
        X.tune_check_step.argtypes = [C.c_double, C.c_void_p]
        X.tune_check_step.restype = C.c_uint32
        X.tune_check_zy.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p]
        X.tune_check_zy.restype = None
        X.tune_check_outputs.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
        X.tune_check_outputs.restype = None
        _lib = X
    return _lib


def record(name, **figures):
    """Prints a measured figure; WSPR_TUNE_FIGURES=<file> appends it there as a JSON line (tools/tune_ab.py collects them)."""
    figures = json.loads(json.dumps(figures, default=float))
    print(name, figures)
    path = os.environ.get("WSPR_TUNE_FIGURES")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"name": name, **figures}) + "\n")


def sanitizer_program(directory):
    """The checker as a stand-alone program (its own main) under AddressSanitizer and UBSan: the path of the executable."""
    exe = os.path.join(str(directory), "tune_check_asan")
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DTUNE_CHECK_MAIN"] +
                   _FLAGS + ["-o", exe, _SRC, "-lm"], check=True)
    return exe


@functools.lru_cache(maxsize=None)
def taps():
    """The reference receiver's 33 compensation taps as float32, from the committed fixture."""
    with open(os.path.join(ol.GOLDEN, "front_end_constants.json")) as f:
        t = np.array([np.float32(x) for x in json.load(f)["zCoef"]], np.float32)
    t.setflags(write=False)
    return t


def aligned_bytes(n, fill=0):
    """n uint8 in memory that starts on a 16-byte boundary."""
    buf = np.full(n + 16, fill, np.uint8)
    off = (-buf.ctypes.data) & 15
    return buf[off:off + n]


def aligned_floats(shape):
    n = int(np.prod(shape))
    buf = np.zeros(n + 4, np.float32)
    off = ((-buf.ctypes.data) & 15) // 4
    return buf[off:off + n].reshape(shape)


def step_of(offset_hz):
    """tune_step() of the header: (step, realised offset)."""
    r = C.c_double(0.0)
    s = checker().tune_check_step(float(offset_hz), C.addressof(r))
    return int(s), float(r.value)


def check_rows(raw, steps, normalise=0, nseg=None, bytes_per_seg=None, stride=STRIDE, raw_offset=0, **kw):
    """The checker on raw rows uint8 [nseg, bytes_per_seg] (or one row).  Returns (rc, I, Q float32 [nseg * nbands, stride]
    pre-filled with NaN, n_out int32 pre-filled with -7)."""
    raw = np.asarray(raw, np.uint8)
    if raw.ndim == 1:
        raw = raw[None, :]
    nseg = raw.shape[0] if nseg is None else nseg
    bytes_per_seg = raw.shape[1] if bytes_per_seg is None else bytes_per_seg
    buf = aligned_bytes(raw.size + 16)
    buf[raw_offset:raw_offset + raw.size] = raw.ravel()
    st = None if steps is None else np.ascontiguousarray(steps, np.uint32)
    nbands = kw.get("nbands", 0 if st is None else st.size)
    rows = max(nseg, 0) * max(min(nbands, MAX_BANDS), 1)
    I, Q = aligned_floats((max(rows, 1), stride)), aligned_floats((max(rows, 1), stride))
    I[:], Q[:] = np.nan, np.nan
    n = np.full(max(rows, 1), -7, np.int32)
    rc = checker().tune_check_rows(buf.ctypes.data + raw_offset, bytes_per_seg, nseg, None if st is None else ol.ptr(st), nbands,
                                   ol.ptr(taps()), ol.ptr(I), ol.ptr(Q), stride, int(normalise), ol.ptr(n))
    return rc, I[:rows], Q[:rows], n[:rows]


def check_zy(raw, step):
    """z_v and y_v (complex arrays of Python-exact int64 parts) of one row's whole vectors under one step."""
    raw = np.ascontiguousarray(raw, np.uint8)
    nvec = raw.size // 16
    z, y = np.zeros(2 * nvec, np.int32), np.zeros(2 * nvec, np.int32)
    checker().tune_check_zy(ol.ptr(raw), nvec, int(step), ol.ptr(z), ol.ptr(y))
    return z.reshape(-1, 2).astype(np.int64), y.reshape(-1, 2).astype(np.int64)


def tables_from_numpy():
    """C and F as the definition states them, by numpy's float64: int arrays [256, 2].  (No entry lies within 1e-6 of a tie.)"""
    k = np.arange(256)
    out = []
    for turns in (256.0, 65536.0):
        e = 16384.0 * np.exp(2j * np.pi * k / turns)
        assert np.abs(np.stack((e.real, e.imag)) % 1.0 - 0.5).min() > 1e-6
        out.append(np.stack((np.floor(e.real + 0.5), np.floor(e.imag + 0.5)), axis=1).astype(np.int64))
    return out


def numpy_rows(raw, step):
    """A float64 statement of the definition for one row and one step with UNROUNDED rotors at the definition's phases (the top
    16 bits of the 32-bit phase) and no rs14: y_v = 16384 sum_k s_{8v+k} e(k step) e(8 v step), two cumulative sums sampled
    behind every 800th vector, differenced over two outputs twice, scaled, K0's taps in float64.  No shared header.  Returns
    the complex128 row of n_out samples."""
    raw = np.asarray(raw, np.uint8)
    nblk = min(raw.size // BLOCK_BYTES, NP_MAX)
    s = raw[:nblk * BLOCK_BYTES].astype(np.float64).reshape(-1, 2) - 128.0
    s = (s[:, 0] + 1j * s[:, 1]).reshape(-1, 8)
    e = lambda P: np.exp(2j * np.pi * ((np.asarray(P, np.uint64) & np.uint64(0xffffffff)) >> np.uint64(16)).astype(np.float64) / 65536.0)
    step = np.uint64(step)
    H = e(np.arange(8, dtype=np.uint64) * step)
    v = np.arange(s.shape[0], dtype=np.uint64)
    y = 16384.0 * (s @ H) * e(((np.uint64(8) * v) & np.uint64(0xffffffff)) * step)
    c = np.cumsum(np.cumsum(y))[R - 1::R]
    cp = np.concatenate((np.zeros(4, complex), c))
    d = cp[4:] - 2 * cp[2:-2] + cp[:-4]
    x = np.concatenate((np.zeros(32, complex), d * SCALE))
    t = taps().astype(np.float64)
    return np.array([np.dot(x[m:m + 33], t) for m in range(nblk)], complex) if nblk else np.zeros(0, complex)


def tone_bytes(freqs_hz, amp, nsamp, seed=0, dither=True, noise=0.0):
    """One capture: the sum of tones amp e^{+2 pi i f n / fs} (freqs_hz, amp scalars or arrays) around 128, optionally with
    +-0.5 LSB of uniform dither (which whitens the quantisation error) and Gaussian noise per rail, rounded and clipped.  uint8
    [2 nsamp], 16-byte aligned."""
    rng = np.random.default_rng(seed)
    n = np.arange(nsamp, dtype=np.float64)
    z = np.zeros(nsamp, complex)
    for f, a in zip(np.atleast_1d(freqs_hz), np.broadcast_to(np.atleast_1d(amp), np.atleast_1d(freqs_hz).shape)):
        z += a * np.exp(2j * np.pi * ((f / FS * n) % 1.0))
    x = np.stack((z.real, z.imag), axis=1) + 128.0
    if dither:
        x += rng.uniform(-0.5, 0.5, x.shape)
    if noise:
        x += rng.normal(0.0, noise, x.shape)
    out = aligned_bytes(2 * nsamp)
    out[:] = np.clip(np.floor(x + 0.5), 0, 255).astype(np.uint8).ravel()
    return out


def random_bytes(nseg, nbytes, seed, clipped=False):
    """Rows of random bytes; clipped: runs of 0x00 and 0xff sprinkled in, at the start and the end of a row among others."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (nseg, nbytes), dtype=np.uint8)
    if clipped and nbytes >= 64:
        for s in range(nseg):
            for j in range(12):
                at = [0, nbytes - 40, (977 * j + 31 * s) % (nbytes - 40)][j % 3 if j > 1 else j]
                raw[s, at:at + 5 + 3 * j] = 0x00 if (j + s) & 1 else 0xff
    return raw


def oracle_k0(raw):
    """The oracle's decimator (orc_decim_feed: pinned to the reference's compiled callback by
    tests/test_reference_pin_frontend.py) on one capture from a fresh state: complex64 row of its outputs."""
    O = ol.lib()
    raw = np.ascontiguousarray(raw, np.uint8)
    I, Q = np.zeros(NP_MAX, np.float32), np.zeros(NP_MAX, np.float32)
    st = O.orc_decim_new()
    n = O.orc_decim_feed(C.c_void_p(st), ol.ptr(raw.copy()), raw.size, ol.ptr(I), ol.ptr(Q), 0, NP_MAX)
    O.orc_decim_free(C.c_void_p(st))
    return (I[:n] + 1j * Q[:n]).astype(np.complex128)


def k21_row(raw, step):
    """The checker's row of one capture under one step, complex128 [n_out]."""
    rc, I, Q, n = check_rows(raw, [step])
    assert rc == 0
    return (I[0, :n[0]] + 1j * Q[0, :n[0]]).astype(np.complex128)


# ---- a full-length two-band capture on the device: the torch method of bench.py's synth_raw_gpu ---------------------------
def synth_two_bands_gpu(torch, dev, w, messages, f0s, t0s, step_b, seed, amp_lsb=4.0, noise_lsb=10.0, nsamp=NP_MAX * SPO):
    """One capture uint8 [2 nsamp] on the device: message 0 at -600 kHz (the band K0 extracts), message 1 at the offset whose
    oscillator step is step_b, each a 375 sps baseband frame held for 6400 samples (bench.py's config-5 model), over
    noise_lsb LSB rms of noise per rail, quantised around 127.5.  The carriers are exact: 32-bit phase accumulators."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    df, dt = 375.0 / 256.0, 1.0 / 375.0
    bbs = []
    for msg, f0, t0 in zip(messages, f0s, t0s):
        sym = w.get_wspr_channel_symbols(msg)[1].astype(np.float64)
        dphi = np.repeat(2.0 * np.pi * dt * (f0 + (sym - 1.5) * df), 256)
        phi = np.concatenate(([0.0], np.cumsum(dphi)[:-1]))
        bb = np.zeros(NP_MAX, np.complex128)
        start = int(round(t0 / dt))
        bb[start:start + 41472] = amp_lsb * np.exp(1j * phi)[:max(0, min(41472, NP_MAX - start))]
        bbs.append((torch.from_numpy(np.ascontiguousarray(bb.real)).float().to(dev),
                    torch.from_numpy(np.ascontiguousarray(bb.imag)).float().to(dev)))
    carrier = [(-(1 << 30)) & 0xffffffff, (-int(step_b)) & 0xffffffff]      # phase per sample, 2^32 = one turn
    raw = torch.empty(2 * nsamp, device=dev, dtype=torch.uint8)
    out = raw.view(nsamp, 2)
    chunk = SPO * 1500
    for c0 in range(0, nsamp, chunk):
        n = torch.arange(c0, min(nsamp, c0 + chunk), device=dev, dtype=torch.int64)
        m = torch.div(n, SPO, rounding_mode="floor")
        zr = torch.zeros(n.numel(), device=dev)
        zi = torch.zeros(n.numel(), device=dev)
        for (br, bi), cstep in zip(bbs, carrier):
            ang = ((n * cstep) & 0xffffffff).double() * (2.0 * np.pi / 4294967296.0)
            cr, ci = torch.cos(ang).float(), torch.sin(ang).float()
            xr, xi = br[m], bi[m]
            zr += xr * cr - xi * ci
            zi += xr * ci + xi * cr
        nz = torch.randn(n.numel(), 2, device=dev, generator=g) * noise_lsb
        out[c0:c0 + n.numel(), 0] = (127.5 + zr + nz[:, 0]).round().clamp(0, 255).to(torch.uint8)
        out[c0:c0 + n.numel(), 1] = (127.5 + zi + nz[:, 1]).round().clamp(0, 255).to(torch.uint8)
    return raw
