"""ctypes bindings of the fading channel's checker (tests/helpers/fade_check.cpp: the contract of wspr_synth_faded*() in
plain serial C++ over rtlsdr-wsprd_amd/csrc/kernels/fade.h and synth_math.h), built on demand, and what the channel's
tests share.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as ol
import synth_lib as sl

NS = sl.NS
SIGLEN = 162 * 256
IDENTITY = [(1.0, 0.0, 0.0), (0.0, 0.0, 0.0)]


class Path(C.Structure):                 # include/wspr_mi355x.h: wspr_synth_path
    _fields_ = [("gain", C.c_float), ("shift", C.c_float), ("sigma", C.c_float)]


class Channel(C.Structure):              # wspr_synth_channel
    _fields_ = [("path", Path * 2)]


assert C.sizeof(Channel) == 24


@functools.lru_cache(maxsize=None)
def checker():
    out = os.path.join(tempfile.mkdtemp(prefix="wspr_fade_"), "libfadecheck.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                    "-Wno-unused-function", "-I", os.path.join(ol.ROOT, "rtlsdr-wsprd_amd", "csrc", "kernels"),
                    "-shared", "-o", out, os.path.join(ol.ROOT, "tests", "helpers", "fade_check.cpp")], check=True)
    X = C.CDLL(out)
    X.fade_check_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_size_t]
    X.fade_check_batch.restype = C.c_int
    X.fade_check_gain.argtypes = [C.c_uint64, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    X.fade_check_gain.restype = C.c_int
    X.fade_check_exp.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    X.fade_check_exp.restype = None
    X.fade_check_noise.argtypes = [C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    X.fade_check_noise.restype = None
    return X


def channel_list(channels):
    """channels: [(gain, shift, sigma), (gain, shift, sigma)] per transmission -> ctypes array of wspr_synth_channel."""
    arr = (Channel * max(1, len(channels)))()
    for k, ch in enumerate(channels):
        assert len(ch) == 2
        for p in range(2):
            arr[k].path[p].gain, arr[k].path[p].shift, arr[k].path[p].sigma = ch[p]
    return arr


def check_batch(items, channels, nseg, seg_index0=0, sigma=0.0, seed=0, flags=0, I=None, Q=None):
    """The checker on nseg rows of 45000 floats (given rows are copied; they matter with ACCUMULATE); channels=None is the
    unfaded call.  Returns (rc, I, Q)."""
    I = np.zeros((nseg, NS), np.float32) if I is None else np.array(I, np.float32).reshape(nseg, NS).copy()
    Q = np.zeros((nseg, NS), np.float32) if Q is None else np.array(Q, np.float32).reshape(nseg, NS).copy()
    arr = sl.tx_list(items)
    ch = None
    if channels is not None:
        assert len(channels) == len(items)
        ch = channel_list(channels)
    rc = checker().fade_check_batch(C.addressof(arr), C.addressof(ch) if ch is not None else None, len(items), nseg,
                                    seg_index0, sigma, seed, flags, ol.ptr(I), ol.ptr(Q), NS)
    return rc, I, Q


def gain(seed, S, q, channel, n0=0, count=SIGLEN):
    """G[n0 .. n0 + count) of the q-th transmission of global segment S: complex128."""
    ch = channel_list([channel])
    re = np.zeros(count, np.float64)
    im = np.zeros(count, np.float64)
    rc = checker().fade_check_gain(seed, S, q, C.addressof(ch), n0, count, ol.ptr(re), ol.ptr(im))
    assert rc == 0
    return re + 1j * im


def synth_exp(x):
    x = np.ascontiguousarray(x, np.float64)
    out = np.zeros_like(x)
    checker().fade_check_exp(ol.ptr(x), int(x.size), ol.ptr(out))
    return out


def noise(seed, segment, sample0, count, sigma):
    nI = np.zeros(count, np.float32)
    nQ = np.zeros(count, np.float32)
    checker().fade_check_noise(seed, segment, sample0, count, sigma, ol.ptr(nI), ol.ptr(nQ))
    return nI, nQ
