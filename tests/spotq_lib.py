"""Shared by tests/test_spot_quality_checker.py and tests/test_gpu_spot_quality.py: the serial checker of the decode-quality
figures (tests/helpers/spot_quality_check.c; the definition in rtlsdr-wsprd_amd/csrc/kernels/spot_quality.h), a numpy
statement of the four sums that need no code word, and the vectors both files use -- each computed once per process."""
import ctypes as C
import functools
import json
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as orc
import rtlsdr_wsprd_amd as w
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 162
FIELDS = ("nhard", "dist", "rsum", "v2", "metric")
# tests/scenes.py seeds whose scene holds three signals (make_scene() draws the count after the two noise rows)
THREE_SIGNAL_SEEDS = (4, 17, 34, 41)


@functools.lru_cache(maxsize=None)
def checker():
    """tests/helpers/spot_quality_check.c, compiled once per process into a scratch directory."""
    so = os.path.join(tempfile.mkdtemp(prefix="spot_quality_check_"), "spot_quality_check.so")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    os.path.join(ROOT, "tests", "helpers", "spot_quality_check.c")], check=True)
    L = C.CDLL(so)
    L.spot_quality_codeword.argtypes = [C.c_void_p, C.c_void_p]
    L.spot_quality_codeword.restype = None
    L.spot_quality_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.spot_quality_check.restype = C.c_int
    return L


@functools.lru_cache(maxsize=None)
def mettab():
    """wspr_fano_metric_table() of the product library: int32 [2, 256]."""
    mt = np.zeros((2, 256), np.int32)
    w.lib().wspr_fano_metric_table(mt.ctypes.data_as(C.c_void_p))
    mt.setflags(write=False)
    return mt


def codeword(decdata):
    """The checker's code word of one decdata (uint8 [>= 7]): uint8 [162], transmission order."""
    dec = np.zeros(11, np.uint8)
    d = np.asarray(decdata, np.uint8).ravel()[:11]
    dec[:d.size] = d
    c = np.zeros(N, np.uint8)
    checker().spot_quality_codeword(dec.ctypes.data, c.ctypes.data)
    return c


def check(symbols, decdata):
    """The checker: symbols uint8 [n, 162], decdata uint8 [n, 11] -> int32 [n, 5] (nhard, dist, rsum, v2, metric)."""
    sym = np.ascontiguousarray(symbols, np.uint8).reshape(-1, N)
    dec = np.ascontiguousarray(decdata, np.uint8).reshape(-1, 11)
    assert dec.shape[0] == sym.shape[0]
    out = np.zeros((sym.shape[0], 5), np.int32)
    assert checker().spot_quality_check(sym.ctypes.data, dec.ctypes.data, sym.shape[0], mettab().ctypes.data, out.ctypes.data) == 0
    return out


def words(rec):
    """A SPOT_QUALITY_DTYPE / SPOT_DETAIL_DTYPE array -> int32 [..., 5] in the checker's order."""
    return np.stack([np.asarray(rec[k], np.int32) for k in FIELDS], axis=-1)


def numpy_sums(symbols, code):
    """nhard, dist, rsum, v2 of the definition, stated with numpy: symbols uint8 [n, 162], code uint8 [n, 162]."""
    s = np.asarray(symbols, np.int64).reshape(-1, N)
    c = np.asarray(code, np.int64).reshape(-1, N)
    v = 2 * s - 255
    r = np.abs(v)
    miss = (s >= 128).astype(np.int64) != c
    return np.stack([miss.sum(axis=1), (r * miss).sum(axis=1), r.sum(axis=1), (v * v).sum(axis=1)], axis=1)


def random_decdata(rng, n):
    """n random 50-bit payloads as fano() leaves decdata: 11 bytes, bits 50 .. 87 zero."""
    dec = np.zeros((n, 11), np.uint8)
    dec[:, :7] = rng.integers(0, 256, (n, 7), dtype=np.uint8)
    dec[:, 6] &= 0xC0
    return dec


def edge_vectors():
    """all 0, all 255, all 127, all 128, alternating 127 / 128."""
    alt = np.where(np.arange(N) % 2 == 0, 127, 128).astype(np.uint8)
    return np.stack([np.full(N, v, np.uint8) for v in (0, 255, 127, 128)] + [alt])


def product_fano(sym_tx, maxcycles=10000):
    """deinterleave() + fano() of the product library with the decoder's constants (wsprd.c:759-761) on one vector in
    transmission order: (ret, metric, decdata uint8 [11]).  fano() hands *metric out as unsigned int; the figure is that
    word as int32 (gamma is signed inside the search and negative after many flipped symbols)."""
    L = w.lib()
    sym = np.ascontiguousarray(sym_tx, np.uint8).copy()
    L.deinterleave(sym.ctypes.data_as(C.c_void_p))
    metric, cycles, maxnp = C.c_uint(0), C.c_uint(0), C.c_uint(0)
    data = np.zeros(11, np.uint8)
    mt = mettab().copy()
    L.fano.restype = C.c_int
    ret = L.fano(C.byref(metric), C.byref(cycles), C.byref(maxnp), data.ctypes.data_as(C.c_void_p),
                 sym.ctypes.data_as(C.c_void_p), C.c_uint(81), mt.ctypes.data_as(C.c_void_p), C.c_int(60), C.c_uint(maxcycles))
    return ret, int(np.uint32(metric.value).astype(np.int32)), data


@functools.lru_cache(maxsize=None)
def fano_candidates():
    """The vectors identity (a) is tested on, uint8 [n, 162] in transmission order: the noise-free code word of every
    message of tests/golden/message_vectors.json with 0, 5, 15 and 25 symbols flipped (s -> 255 - s), and the first
    soft-symbol vector of every candidate the CPU oracle found worth the ladder in four scenes of tests/scenes.py."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "message_vectors.json")))
    rng = np.random.default_rng(1919)
    vec = []
    for e in gold["channel_symbols"]:
        if not e["ok"]:
            continue
        clean = np.array([255 if int(ch) >> 1 else 0 for ch in e["symbols"]], np.uint8)
        for flips in (0, 5, 15, 25):
            v = clean.copy()
            at = rng.choice(N, flips, replace=False)
            v[at] = 255 - v[at]
            vec.append(v)
    for seed in THREE_SIGNAL_SEEDS:
        I, Q = scenes.make_scene(seed)
        tr = orc.decode(I, Q, trace=True)[3]
        for p in range(tr.passes_run):
            for j in range(tr.n_visited[p]):
                if tr.attempts[p][j] > 0:
                    vec.append(np.array(tr.first_symbols[p][j], np.uint8))
    out = np.stack(vec)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fano_successes():
    """(vectors uint8 [m, 162], decdata uint8 [m, 11], metric int64 [m]) of the candidates on which the product's exported
    fano() returns 0."""
    vec, dec, met = [], [], []
    for v in fano_candidates():
        ret, metric, data = product_fano(v)
        if ret == 0:
            vec.append(v); dec.append(data); met.append(metric)
    out = (np.stack(vec), np.stack(dec), np.array(met, np.int64))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def kernel_jobs(n=257):
    """n jobs for the kernel against the checker: the edge vectors with random payloads, the Fano successes with their own
    decdata (small nhard), and random soft bytes with random payloads -- and the checker's answer, computed once."""
    rng = np.random.default_rng(19)
    fv, fd, _ = fano_successes()
    take = min(len(fv), 60)
    edge = edge_vectors()
    nrand = n - len(edge) - take
    vec = np.concatenate([edge, fv[:take], rng.integers(0, 256, (nrand, N), dtype=np.uint8)])
    dec = np.concatenate([random_decdata(rng, len(edge)), fd[:take], random_decdata(rng, nrand)])
    dec[0] = 0                                     # the all-zero message on the all-zero vector
    dec[1, :7] = [255] * 6 + [0xC0]                # all fifty bits set on all 255
    want = check(vec, dec)
    for a in (vec, dec, want):
        a.setflags(write=False)
    return vec, dec, want
