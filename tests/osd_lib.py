"""What the ordered-statistics tests share (tests/test_osd_checker.py, tests/test_gpu_osd.py): the serial CPU checker
tests/helpers/osd_check.cpp behind ctypes, an independent and slow numpy statement of the definition in
rtlsdr-wsprd_amd/csrc/kernels/osd.h, and the soft-symbol vectors both suites decode."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import tempfile

import numpy as np

import rtlsdr_wsprd_amd as w

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K = 162, 50
_REV8 = [int("{:08b}".format(i)[::-1], 2) for i in range(256)]
PERM = np.array([j for j in _REV8 if j < N])       # deinterleaved[p] = transmitted[PERM[p]]  (wsprd_utils.c:196-213)


def _helper(name):
    """tests/helpers/<name>.cpp compiled into a scratch directory."""
    so = os.path.join(tempfile.mkdtemp(prefix=name + "_"), name + ".so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-mpopcnt", "-ffp-contract=off", "-shared", "-fPIC", "-Wno-format-truncation",
                    "-o", so, os.path.join(ROOT, "tests", "helpers", name + ".cpp")], check=True)
    return C.CDLL(so)


@functools.lru_cache(maxsize=None)
def packed():
    """tests/helpers/osd_packed_check.cpp: the kernel's packed arithmetic (osd.h) emulated lane by lane on the host."""
    L = _helper("osd_packed_check")
    L.osd_packed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.osd_packed.restype = C.c_int
    return L


@functools.lru_cache(maxsize=None)
def checker():
    """tests/helpers/osd_check.cpp, compiled once per process."""
    L = _helper("osd_check")
    L.osd_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.osd_check.restype = C.c_int
    L.osd_gate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.osd_gate.restype = C.c_int
    return L


def check(sym_tx, depth, fn=None):
    """The checker (or fn, a routine with its signature) on one vector in transmission order: (data[11] as a tuple, dist,
    nhard, order)."""
    sym = np.ascontiguousarray(sym_tx, np.uint8)
    assert sym.shape == (N,)
    data = np.zeros(11, np.uint8)
    d, nh, o = C.c_uint(), C.c_uint(), C.c_uint()
    rc = (fn or checker().osd_check)(sym.ctypes.data, int(depth), data.ctypes.data, C.byref(d), C.byref(nh), C.byref(o))
    assert rc == 0, rc
    return tuple(int(x) for x in data), d.value, nh.value, o.value


def check_packed(sym_tx, depth):
    return check(sym_tx, depth, packed().osd_packed)


def encode_bits(data11):
    """The library's encode() (pinned to the reference's own by tests/test_reference_pin.py): first 162 outputs."""
    enc = (C.c_ubyte * 176)()
    w.lib().encode(enc, (C.c_ubyte * 11)(*[int(x) for x in data11]), C.c_uint(11))
    return np.frombuffer(enc, np.uint8)[:N].copy()


@functools.lru_cache(maxsize=None)
def generator():
    """G of the definition, [50, 162], through the library's encode()."""
    G = np.zeros((K, N), np.uint8)
    for j in range(K):
        d = [0] * 11
        d[j >> 3] = 0x80 >> (j & 7)
        G[j] = encode_bits(d)
    return G


def interleave(deint):
    tx = np.zeros(N, np.uint8)
    tx[PERM] = np.asarray(deint, np.uint8)
    return tx


def _gf2_inverse(A):
    n = A.shape[0]
    M = np.concatenate([A.astype(np.uint8) & 1, np.eye(n, dtype=np.uint8)], axis=1)
    for col in range(n):
        piv = col + int(np.argmax(M[col:, col]))
        assert M[piv, col], "singular"
        M[[col, piv]] = M[[piv, col]]
        for rrow in np.flatnonzero(M[:, col]):
            if rrow != col:
                M[rrow] ^= M[col]
    return M[:, n:]


def trials(size):
    return (1, 50, 1225, 19600)[size]                # subsets of {0..49} with exactly `size` elements


def numpy_osd(sym_tx, depth):
    """Section 1 of the definition, written for clarity and by other means than the checker: the basis from an XOR basis
    of COLUMN vectors, G~ = inverse(G[:, P]) G, every subset enumerated, the winner by a lexicographic sort."""
    G = generator().astype(np.int64)
    s = np.asarray(sym_tx, np.int64)[PERM]
    h = (s >= 128).astype(np.int64)
    r = np.abs(2 * s - 255)
    order = sorted(range(N), key=lambda i: (-int(r[i]), i))
    cols = [int("".join(str(int(b)) for b in G[:, p]), 2) for p in range(N)]
    basis, P = {}, []                                # leading bit -> reduced column vector
    for p in order:
        v = cols[p]
        while v:
            top = v.bit_length()
            if top not in basis:
                basis[top] = v
                P.append(p)
                break
            v ^= basis[top]
        if len(P) == K:
            break
    assert len(P) == K
    Ainv = _gf2_inverse(G[:, P] % 2).astype(np.int64)
    Gt = Ainv @ G % 2                                # Gt[k][P[m]] == (k == m)
    assert np.array_equal(Gt[:, P], np.eye(K, dtype=np.int64))
    c0 = h[P] @ Gt % 2
    m0 = h[P] @ Ainv % 2
    cands = []                                       # (D, |T|, T)
    for size in range(depth + 1):
        T = np.array(list(itertools.combinations(range(K), size)), np.int64).reshape(trials(size), size)
        cw = np.broadcast_to(c0, (T.shape[0], N)).copy()
        for e in range(size):
            cw ^= Gt[T[:, e]]
        D = ((cw != h) * r).sum(axis=1)
        cands += [(int(D[i]), size, tuple(int(x) for x in T[i])) for i in range(T.shape[0])]
    D, size, T = min(cands)
    msg, cw = m0.copy(), c0.copy()
    for k in T:
        msg ^= Ainv[k]
        cw ^= Gt[k]
    bits = np.zeros(88, np.uint8)
    bits[:K] = msg
    return tuple(int(x) for x in np.packbits(bits)), D, int((cw != h).sum()), size


def ladder_vectors(n, seed=33):
    """tests/test_fano_wave.py's noise ladder: random 50-bit messages, encoded, 78 / 178 plus Gaussian noise of twelve
    strengths, clipped to a byte -- in transmission order.  Returns (uint8 [n, 162], the messages uint8 [n, 11])."""
    rng = np.random.default_rng(seed)
    out, msgs = np.zeros((n, N), np.uint8), np.zeros((n, 11), np.uint8)
    for t in range(n):
        data = [int(x) for x in rng.integers(0, 256, 7)] + [0, 0, 0, 0]
        data[6] &= 0xC0
        sigma = [5, 25, 40, 50, 55, 60, 65, 70, 80, 100, 150, 400][t % 12]
        soft = np.clip(np.where(encode_bits(data) > 0, 178, 78) + rng.normal(0, sigma, N), 0, 255)
        out[t] = interleave(soft.astype(np.uint8))
        msgs[t] = data
    return out, msgs


def degenerate_vectors():
    """All-erasure and saturated vectors, and vectors of 127 / 128 only (every reliability ties at 1)."""
    rng = np.random.default_rng(7)
    v = [[128] * N, [0] * N, [255] * N, [127] * N, [127, 128] * 81, [128, 127] * 81,
         (127 + rng.integers(0, 2, N)).tolist(), (127 + rng.integers(0, 2, N)).tolist()]
    return np.array(v, np.uint8)
