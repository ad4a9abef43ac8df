"""ctypes bindings of the synthesiser's checker (tests/helpers/synth_check.cpp: the contract of wspr_synth*() in plain
serial C++ over rtlsdr-wsprd_amd/csrc/kernels/synth_math.h), built on demand, and the scene helpers the synthesiser's
tests share.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as ol

NS = 45000
ACCUMULATE, NORMALISE = 1, 2


class Tx(C.Structure):                   # include/wspr_mi355x.h: wspr_synth_tx
    _fields_ = [("seg", C.c_int32), ("f0", C.c_float), ("t0", C.c_float), ("amp", C.c_float), ("drift", C.c_float),
                ("symbols", C.c_ubyte * 162), ("pad", C.c_ubyte * 2)]


assert C.sizeof(Tx) == 184

_lib = None


def checker():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="wspr_synth_"), "libsynthcheck.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                        "-Wno-unused-function", "-I", os.path.join(ol.ROOT, "rtlsdr-wsprd_amd", "csrc", "kernels"),
                        "-shared", "-o", out, os.path.join(ol.ROOT, "tests", "helpers", "synth_check.cpp")], check=True)
        X = C.CDLL(out)
        X.synth_check_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_size_t]
        X.synth_check_batch.restype = C.c_int
        X.synth_check_sincos.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        X.synth_check_log.argtypes = [C.c_double]
        X.synth_check_log.restype = C.c_double
        _lib = X
    return _lib


def tx_list(items):
    """items: (seg, f0, t0, amp, drift, symbols[162]) in list order -> ctypes array of wspr_synth_tx."""
    arr = (Tx * max(1, len(items)))()
    for k, (seg, f0, t0, amp, drift, sym) in enumerate(items):
        arr[k].seg, arr[k].f0, arr[k].t0, arr[k].amp, arr[k].drift = int(seg), f0, t0, amp, drift
        arr[k].symbols[:] = [int(v) for v in sym]
    return arr


def check_batch(items, nseg, seg_index0=0, sigma=0.0, seed=0, flags=0, I=None, Q=None):
    """The checker on nseg rows of 45000 floats (given rows are copied; they matter with ACCUMULATE).
    Returns (rc, I, Q)."""
    I = np.zeros((nseg, NS), np.float32) if I is None else np.array(I, np.float32).reshape(nseg, NS).copy()
    Q = np.zeros((nseg, NS), np.float32) if Q is None else np.array(Q, np.float32).reshape(nseg, NS).copy()
    arr = tx_list(items)
    rc = checker().synth_check_batch(C.addressof(arr), len(items), nseg, seg_index0, sigma, seed, flags,
                                     ol.ptr(I), ol.ptr(Q), NS)
    return rc, I, Q


def selftest_item(seg=0):
    """The reference's self-test transmission, rtlsdr_wsprd.c:736-745."""
    ok, sym = ol.channel_symbols("K1JT FN20QI 20")
    assert ok
    return (seg, 50.0, 2.0, 1.0, 0.0, sym)


def reference_noise():
    """The noise of decoderSelfTest() alone (rtlsdr_wsprd.c:706-726, :756-757): glibc rand() seeded 1, drawn I then Q per
    sample over the frame's 41 472 samples from index 750, float32; zero elsewhere."""
    libc = C.CDLL("libc.so.6")
    libc.srand(1)
    rand_max = 2147483647.0
    wgn = np.float32(0.02)
    I = np.zeros(NS, np.float32)
    Q = np.zeros(NS, np.float32)
    out = np.empty(2 * 162 * 256, np.float32)
    k = 0
    while k < out.size:
        while True:
            v1 = 2 * (libc.rand() / rand_max) - 1
            v2 = 2 * (libc.rand() / rand_max) - 1
            s = v1 * v1 + v2 * v2
            if not (s >= 1 or s == 0):
                break
        f = math.sqrt(-2 * math.log(s) / s)
        out[k] = np.float32(v1 * f) * wgn
        out[k + 1] = np.float32(v2 * f) * wgn
        k += 2
    I[750:750 + 162 * 256] = out[0::2]
    Q[750:750 + 162 * 256] = out[1::2]
    return I, Q


def libm_frame(item, base_i=None, base_q=None):
    """One transmission by the contract's statements with glibc's cos/sin (Python's math module) on the serial phases:
    the model that is independent of synth_math.h.  Over `base` rows (float32) or zero."""
    _, f0, t0, amp, drift, sym = item
    f0, t0, amp, drift = (float(np.float32(v)) for v in (f0, t0, amp, drift))
    df, dt = 375.0 / 256.0, 1 / 375.0
    I = np.zeros(NS, np.float32) if base_i is None else np.array(base_i, np.float32).copy()
    Q = np.zeros(NS, np.float32) if base_q is None else np.array(base_q, np.float32).copy()
    first = math.floor(t0 / dt)
    phi = 0.0
    for i in range(162):
        fd = (drift / 2.0) * (float(i) - 81.0) / 81.0
        dphi = 2.0 * math.pi * dt * ((f0 + fd) + (float(sym[i]) - 1.5) * df)
        for j in range(256):
            k = first + 256 * i + j
            if 0 <= k < NS:
                I[k] = np.float32(float(I[k]) + amp * math.cos(phi))
                Q[k] = np.float32(float(Q[k]) + amp * math.sin(phi))
            phi += dphi
    return I, Q
