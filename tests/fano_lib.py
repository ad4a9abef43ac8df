"""What the tests of the device Fano search K6w share (tests/test_fano_cases_cpu.py, tests/test_gpu_fano_wave.py,
tests/test_fano_wave.py): the host emulation of the kernel's step structure (tests/helpers/fano_wave_check.cpp, built once
per process), the serial reference (the reference's own fano() from oracle/_ref where it is present, else the oracle's
orc_fano, as tests/test_gpu_parity.py chooses), and the vector sets.  Every vector here is in TRANSMISSION order, as the
demodulator emits it and as wspr_fano_batch_device_wave() takes it; the serial decoders and the emulation get it
deinterleaved.  Results are cached per (set, budget, width, capacity): computed once, shared, never modified."""
import ctypes as C
import functools
import json
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as ol
import rtlsdr_wsprd_amd as w

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES_JSON = os.path.join(ROOT, "tests", "golden", "fano_budget_edges.json")
N, NBITS, DELTA = 162, 81, 60
BUDGETS = (50, 200, 1500, 10000)
# every (width, capacity) at which the CPU tests run the emulation; the kernel is (64, 4096), and (64, 1024) / (64, 96)
# under the lab switch WSPR_FANO_WAVE_CAP
SHAPES = ((64, 4096), (64, 1024), (64, 96), (1, 1024), (7, 1024))
_REV8 = [int("{:08b}".format(i)[::-1], 2) for i in range(256)]
PERM = np.array([j for j in _REV8 if j < N])       # deinterleaved[p] = transmitted[PERM[p]]  (wsprd_utils.c:196-213)


def deinterleaved(sym):
    """One vector or a stack of vectors, transmission order -> decoder order."""
    return np.ascontiguousarray(np.asarray(sym, np.uint8)[..., PERM])


@functools.lru_cache(maxsize=None)
def emulation():
    """tests/helpers/fano_wave_check.cpp, compiled once per process."""
    so = os.path.join(tempfile.mkdtemp(prefix="fano_wave_check_"), "fano_wave_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-mpopcnt", "-shared", "-fPIC", "-o", so,
                    os.path.join(ROOT, "tests", "helpers", "fano_wave_check.cpp")], check=True)
    L = C.CDLL(so)
    L.fano_wave_host.restype = C.c_int
    return L


@functools.lru_cache(maxsize=None)
def mettab():
    """The product's branch-metric table, equal to the one the oracle derives as wsprd.c:467-473 does."""
    mt = (C.c_int * 256 * 2)()
    w.lib().wspr_fano_metric_table(mt)
    ref = (C.c_int * 256 * 2)()
    ol.lib().orc_build_mettab(ref)
    assert bytes(mt) == bytes(ref)
    return mt


def serial_decoders():
    """name -> fano() with the reference's signature: the reference's own where oracle/_ref is present, the oracle's
    restatement and the product's host routine."""
    out = {}
    R = ol.ref_lib()
    if R is not None:
        out["reference"] = R.fano
    O = ol.lib()
    O.orc_fano.restype = C.c_int
    out["oracle"] = O.orc_fano
    L = w.lib()
    L.fano.restype = C.c_int
    out["product"] = L.fano
    return out


def reference_name():
    return "reference" if ol.ref_lib() is not None else "oracle"


def serial(sym_tx, maxcycles, which=None):
    """A serial decoder on a stack of vectors: int64 array [n, 14] = ret, metric, cycles, maxnp, data[10] (metric, maxnp and
    data zeroed where ret != 0: the reference defines them for decoded frames only)."""
    fn = serial_decoders()[which or reference_name()]
    d = deinterleaved(np.atleast_2d(sym_tx))
    out = np.zeros((len(d), 14), np.int64)
    dec = (C.c_ubyte * 11)(); a = C.c_uint(); b = C.c_uint(); c = C.c_uint()
    for i, v in enumerate(d):
        s = (C.c_ubyte * N).from_buffer_copy(v.tobytes())
        r = fn(C.byref(a), C.byref(b), C.byref(c), dec, s, C.c_uint(NBITS), mettab(), C.c_int(DELTA), C.c_uint(maxcycles))
        out[i, 0], out[i, 2] = r, b.value
        if r == 0:
            out[i, 1], out[i, 3], out[i, 4:] = a.value, c.value, list(dec)[:10]
    return out


def wave(sym_tx, maxcycles, width=64, cap=4096):
    """The emulation on a stack of vectors: int64 array [n, 16] = ret, metric, cycles, maxnp, data[10], steps, maxsize
    (the largest number of pending visits after any step)."""
    fn = emulation().fano_wave_host
    d = deinterleaved(np.atleast_2d(sym_tx))
    out = np.zeros((len(d), 16), np.int64)
    dec = (C.c_ubyte * 10)(); a = C.c_uint(); b = C.c_uint(); c = C.c_uint(); st = C.c_uint(); mx = C.c_uint()
    for i, v in enumerate(d):
        s = (C.c_ubyte * N).from_buffer_copy(v.tobytes())
        r = fn(C.byref(a), C.byref(b), C.byref(c), dec, s, C.c_uint(NBITS), mettab(), C.c_int(DELTA), C.c_uint(maxcycles),
               C.c_int(width), C.c_int(cap), C.byref(st), C.byref(mx))
        out[i] = [r, a.value, b.value, c.value] + list(dec) + [st.value, mx.value]
    return out


def defined(rows):
    """The first 14 columns of wave() or of the kernel's outputs with what the reference's caller never reads zeroed, as
    serial() has it: metric, maxnp and data where ret != 0.  (A frame found at look i == budget is such a case: the search
    returns -1 and both the kernel and the emulation leave the frame's bytes in data.)"""
    out = np.array(np.atleast_2d(rows)[:, :14], np.int64)
    out[out[:, 0] != 0, 1] = 0
    out[out[:, 0] != 0, 3:] = 0
    return out


# ------------------------------------------------------------------------------------------------ the vector sets
@functools.lru_cache(maxsize=None)
def ladder_vectors():
    """The 364 vectors of tests/test_gpu_parity.py::test_wave_fano_equals_host_fano, generated as there: 360 random
    messages at twelve noise levels, then all-erasure, all-zero, all-one and alternating saturated symbols."""
    R = ol.ref_lib()
    O = ol.lib()
    enc_fn, inter = (R.encode, R.interleave) if R is not None else (O.orc_conv_encode, O.orc_interleave)
    rng = np.random.default_rng(18)
    enc = (C.c_ubyte * 176)()
    vecs = []
    for t in range(360):
        data = [int(x) for x in rng.integers(0, 256, 7)] + [0, 0, 0, 0]
        data[6] &= 0xC0
        enc_fn(enc, (C.c_ubyte * 11)(*data), C.c_uint(11))
        bits = (C.c_ubyte * 162)(*list(enc)[:162])
        inter(bits)                                          # transmission order, as the demodulator emits
        sigma = [5, 25, 40, 50, 55, 60, 65, 75, 100, 150, 400, 1000][t % 12]
        vecs.append(np.clip(np.where(np.frombuffer(bits, np.uint8) > 0, 178, 78) + rng.normal(0, sigma, 162), 0, 255).astype(np.uint8))
    vecs += [np.full(162, 128, np.uint8), np.zeros(162, np.uint8), np.full(162, 255, np.uint8),
             np.tile(np.array([0, 255], np.uint8), 81)]
    sym = np.stack(vecs)
    sym.setflags(write=False)
    return sym


@functools.lru_cache(maxsize=None)
def alternating_vectors(n=16):
    """Alternating saturated symbols with 5 % erasures: bushy trees that never decode and fill the pending-visit store
    (past 2 048 of 4 096, past 768 of 1 024, and over the edge of 96)."""
    g = np.random.default_rng(3)
    sym = np.stack([np.where(g.random(162) < 0.05, 128, np.tile([0, 255], 81)).astype(np.uint8) for _ in range(n)])
    sym.setflags(write=False)
    return sym


@functools.lru_cache(maxsize=None)
def budget_edges():
    """tests/golden/fano_budget_edges.json: a list of (symbols [162] uint8, [(maxcycles, ret, cycles, metric, decdata)]) --
    decodable vectors whose cycle count c has (c - 1) % 81 == 0, with the reference's results at maxcycles m - 1, m and
    m + 1 (m = (c - 1) / 81), and the all-zero vector at 0, 1 and 2."""
    with open(EDGES_JSON) as f:
        doc = json.load(f)
    out = []
    for v in doc["vectors"]:
        sym = np.array(v["symbols"], np.uint8)
        sym.setflags(write=False)
        out.append((sym, [(c["maxcycles"], c["ret"], c["cycles"], c["metric"], tuple(c["decdata"])) for c in v["cases"]]))
    return out


@functools.lru_cache(maxsize=None)
def main_set():
    """The ladder vectors followed by the first 16 alternating ones: what the step-for-step GPU tests run."""
    sym = np.concatenate([ladder_vectors(), alternating_vectors(16)])
    sym.setflags(write=False)
    return sym


_SETS = {"ladder": ladder_vectors, "alternating": alternating_vectors, "main": main_set}


@functools.lru_cache(maxsize=None)
def wave_of(name, maxcycles, width=64, cap=4096):
    out = wave(_SETS[name](), maxcycles, width, cap)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def serial_of(name, maxcycles, which=None):
    out = serial(_SETS[name](), maxcycles, which)
    out.setflags(write=False)
    return out


def queue_order(n, seed=4096):
    """Indices into the ladder vectors for a call of n vectors: a seeded shuffle, repeated, so that deep stacks and instant
    decodes alternate on a wave."""
    rng = np.random.default_rng(seed)
    m = len(ladder_vectors())
    return np.concatenate([rng.permutation(m) for _ in range(-(-n // m))])[:n]
