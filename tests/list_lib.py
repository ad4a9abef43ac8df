"""What the list-decoding tests share (tests/test_list_checker.py, tests/test_gpu_list.py, tools/list_*.py): the serial CPU
checker tests/helpers/list_check.c behind ctypes, an independent numpy statement of the definition in
rtlsdr-wsprd_amd/csrc/kernels/listmatch.h in 64-bit integers, the 7 600-message list and the soft-symbol vectors both suites
match against it."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import osd_lib as ol
import rtlsdr_wsprd_amd as w
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 162
NO_SECOND = -2 ** 31
S_CLEAN = 162 * 255                                    # 41 310: the score of an entry's own clean code word, z = sqrt(162)
V_MAX = 162 * 255 * 255                                # 10 534 050
FIELDS = ("index", "score", "second", "v2")


@functools.lru_cache(maxsize=None)
def checker():
    """tests/helpers/list_check.c, compiled once per process into a scratch directory."""
    so = os.path.join(tempfile.mkdtemp(prefix="list_check_"), "list_check.so")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    os.path.join(ROOT, "tests", "helpers", "list_check.c")], check=True)
    L = C.CDLL(so)
    L.list_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.list_check.restype = C.c_int
    L.list_gate.argtypes = [C.c_int32, C.c_int32, C.c_int]
    L.list_gate.restype = C.c_int
    return L


def check(entries, vectors):
    """The checker: entries uint8 [m, 162] channel symbols, vectors uint8 [n, 162] -> int32 [n, 4] (index, score, second, v2)."""
    e = np.ascontiguousarray(entries, np.uint8).reshape(-1, N)
    v = np.ascontiguousarray(vectors, np.uint8).reshape(-1, N)
    out = np.zeros((v.shape[0], 4), np.int32)
    assert checker().list_check(e.ctypes.data, e.shape[0], v.ctypes.data, v.shape[0], out.ctypes.data) == 0
    return out


def gate(score, v2, zmin16):
    return checker().list_gate(int(score), int(v2), int(zmin16))


def gate_exact(score, v2, zmin16):
    """The gate in Python's unbounded integers."""
    return int(score > 0 and 256 * int(score) ** 2 >= int(zmin16) ** 2 * int(v2))


def numpy_match(entries, vectors):
    """The definition by other means: one int64 matrix product, a stable argsort for the tie rule, `second` by masking."""
    c = 2 * (np.asarray(entries, np.int64).reshape(-1, N) >> 1) - 1
    v = 2 * np.asarray(vectors, np.int64).reshape(-1, N) - 255
    S = v @ c.T                                          # [n, m]
    out = np.zeros((v.shape[0], 4), np.int64)
    for t in range(v.shape[0]):
        order = np.argsort(-S[t], kind="stable")         # descending score, equal scores in index order
        out[t] = (order[0], S[t, order[0]], S[t, order[1]] if len(order) > 1 else NO_SECOND, (v[t] * v[t]).sum())
    return out


@functools.lru_cache(maxsize=None)
def all_messages():
    """The 7 600 messages synth.CALLS x GRIDS x POWERS, calls outermost: what tests/synth.py message_for() draws from."""
    return tuple("%s %s %d" % (c, g, p) for c in synth.CALLS for g in synth.GRIDS for p in synth.POWERS)


@functools.lru_cache(maxsize=None)
def all_symbols():
    """Channel symbols of all_messages(), uint8 [7600, 162], through the library's own encoder (pinned to the reference's
    by tests/test_reference_pin.py)."""
    out = np.zeros((len(all_messages()), N), np.uint8)
    for k, m in enumerate(all_messages()):
        ok, out[k] = w.get_wspr_channel_symbols(m)
        assert ok, m
    out.setflags(write=False)
    return out


def clean(symbols):
    """The noise-free soft symbols of an entry: 255 where its data bit is 1, else 0."""
    return np.where(np.asarray(symbols) >> 1, 255, 0).astype(np.uint8)


def tie_vector(sym_a, sym_b, x=101):
    """The clean code word of a with the positions where a and b differ set to c_a * x on one half and to -c_a * x on the
    other, so that S(a) == S(b) exactly.  Needs an even number of such positions (every v is odd: an odd number of them
    cannot cancel)."""
    ca, cb = 2 * (np.asarray(sym_a, int) >> 1) - 1, 2 * (np.asarray(sym_b, int) >> 1) - 1
    diff = np.flatnonzero(ca != cb)
    assert len(diff) % 2 == 0 and len(diff) > 0 and x % 2 == 1
    v = 255 * ca
    v[diff[0::2]] = x * ca[diff[0::2]]
    v[diff[1::2]] = -x * ca[diff[1::2]]
    s = (v + 255) // 2
    assert np.array_equal(2 * s - 255, v)
    return s.astype(np.uint8)


def even_partner(sym, a, b):
    """The first index >= b (other than a) whose code word differs from a's in an even number of positions."""
    ca = sym[a] >> 1
    for k in range(b, len(sym)):
        if k != a and int(((sym[k] >> 1) != ca).sum()) % 2 == 0:
            return k
    raise AssertionError("no partner")


# (a, b): the clean code word is a's.  Within one 32-tile, across tiles, with a member in the last, partly filled tile of
# the 7 600 (7 584 .. 7 599), and each shape once with a < b and once with b < a.
TIE_PAIRS = ((3, 17), (17, 3), (5, 40), (40, 5), (31, 32), (32, 31), (10, 300), (300, 10), (100, 7590), (7590, 100),
             (7585, 7597), (7597, 7585), (0, 1), (63, 64), (256, 20), (1, 0))


@functools.lru_cache(maxsize=None)
def tie_cases():
    """[(a, b, vector)]: b moved up to the next index at an even distance from a."""
    sym = all_symbols()
    out = []
    for a, b in TIE_PAIRS:
        b = even_partner(sym, a, b)
        out.append((a, b, tie_vector(sym[a], sym[b])))
    return out


def degenerate_vectors():
    """all 0, all 255, all 128 (S = B_m), all 127, alternating 0 / 255."""
    return np.array([[0] * N, [255] * N, [128] * N, [127] * N, [0, 255] * 81], np.uint8)


@functools.lru_cache(maxsize=None)
def match_vectors():
    """257 vectors: the degenerate ones, clean code words of entries and their complements, the tie vectors, listed code
    words under noise, and the noise ladder of osd_lib (random messages, none of them listed)."""
    sym = all_symbols()
    rng = np.random.default_rng(14)
    vec = [degenerate_vectors()]
    own = (0, 1, 31, 32, 33, 64, 256, 4000, 7599)
    vec.append(np.array([clean(sym[k]) for k in own]))
    vec.append(np.array([255 - clean(sym[k]) for k in own]))
    vec.append(np.array([t[2] for t in tie_cases()]))
    noisy = []
    for k in rng.integers(0, len(sym), 48):
        sigma = (20, 60, 120, 250)[len(noisy) % 4]
        noisy.append(np.clip(np.where(sym[k] >> 1, 178, 78) + rng.normal(0, sigma, N), 0, 255).astype(np.uint8))
    vec.append(np.array(noisy))
    have = sum(len(x) for x in vec)
    vec.append(ol.ladder_vectors(257 - have)[0])
    out = np.concatenate(vec)
    assert out.shape == (257, N)
    out.setflags(write=False)
    return out
