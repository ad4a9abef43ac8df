"""What the block-detection tests share (tests/test_block_checker.py, tests/test_gpu_block.py, tools/block_rescue_seeds.py):
the serial CPU checker tests/helpers/block_check.c behind ctypes (built twice, CONTRACT=0/1, against the CPU oracle), the
decode loop's block stage restated over that checker and the oracle's Fano search (walk()), and the scenes both suites
use.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as ol
import synth

NSYM = 162
MINSYNC1, MINSYNC2, MINRMS = np.float32(0.10), np.float32(0.12), np.float32(52.0 * (50 / 64.0))   # wsprd.c:423-428
# the reference's jitter ladder (wsprd.c:739-747): 0, -3, +3, -6, ... +63
LADDER = [3 * (-((idt + 1) // 2) if idt % 2 else (idt + 1) // 2) for idt in range(43)]


@functools.lru_cache(maxsize=None)
def checker(flag):
    """tests/helpers/block_check.c built with -DCONTRACT=flag (0 exact, 1 contracted), cached per process."""
    ol.lib()                                              # builds oracle/liboracle.so if it is missing
    out = os.path.join(tempfile.mkdtemp(prefix="wspr_block_"), "libblock%d.so" % flag)
    subprocess.run(["gcc", "-O2", "-std=gnu17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                    "-DCONTRACT=%d" % flag, "-I", ol.ORACLE_DIR, "-shared", "-o", out,
                    os.path.join(ol.ROOT, "tests", "helpers", "block_check.c"), "-L", ol.ORACLE_DIR, "-loracle",
                    "-Wl,-rpath," + ol.ORACLE_DIR, "-lm"], check=True)
    X = C.CDLL(out)
    X.blk_demod.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p]
    X.blk_demod.restype = C.c_int
    return X


def demod(flag, I, Q, np_, freq, shift, drift, sums=False):
    """The checker on one hypothesis: (symbols uint8 [3, 162], rms float32 [3], sync float32[, sums float32 [162, 4, 4] =
    (is, qs, cf, sf) per symbol and tone])."""
    I = np.ascontiguousarray(I, np.float32)
    Q = np.ascontiguousarray(Q, np.float32)
    sym = np.zeros((3, NSYM), np.uint8)
    rms = np.zeros(3, np.float32)
    sync = C.c_float(0)
    sm = np.zeros((NSYM, 4, 4), np.float32) if sums else None
    rc = checker(flag).blk_demod(ol.ptr(I), ol.ptr(Q), int(np_), float(freq), int(shift), float(drift),
                                 ol.ptr(sm) if sums else None, ol.ptr(sym), ol.ptr(rms), C.byref(sync))
    assert rc == 0
    out = (sym, rms, np.float32(sync.value))
    return out + (sm,) if sums else out


@functools.lru_cache(maxsize=None)
def _mettab():
    mt = ((C.c_int * 256) * 2)()
    ol.lib().orc_build_mettab(mt)
    return mt


def fano(sym_tx):
    """deinterleave + the oracle's Fano search with the decoder's constants (wsprd.c:759-761): (ret, cycles, decdata[11])."""
    L = ol.lib()
    sym = (C.c_ubyte * NSYM)(*[int(x) for x in sym_tx])
    L.orc_deinterleave(sym)
    metric, cycles, maxnp = C.c_uint(0), C.c_uint(0), C.c_uint(0)
    data = (C.c_ubyte * 11)()
    ret = L.orc_fano(C.byref(metric), C.byref(cycles), C.byref(maxnp), data, sym, C.c_uint(81), _mettab(), C.c_int(60),
                     C.c_uint(10000))
    return ret, cycles.value, tuple(int(x) for x in data)


def walk(flag, I, Q, np_, freq, shift, drift, quickmode=0, maxblock=3, minsync2=MINSYNC2):
    """The block stage's rule on one candidate the plain ladder left undecoded: for B = 2 .. maxblock and the rungs in the
    ladder's order (quick mode: jitter 0 only), the vector of (B, rung) goes to Fano if the rung's mode-2 sync exceeds
    minsync2 and the vector's rms minrms; the first success wins.  Returns (block, jitter, decdata, cycles) or None."""
    rungs = LADDER[:1] if quickmode else LADDER
    vec = [demod(flag, I, Q, np_, freq, shift + j, drift) for j in rungs]
    for B in range(2, maxblock + 1):
        for j, (sym, rms, sync) in zip(rungs, vec):
            if sync > minsync2 and rms[B - 1] > MINRMS:
                ret, cycles, data = fano(sym[B - 1])
                if ret == 0:
                    return B, j, data, cycles
    return None


def unpack(data):
    """A decode's text (call_loc_pow) with empty hash tables, through the oracle's message layer."""
    L = ol.lib()
    h, l = C.create_string_buffer(32768 * 13), C.create_string_buffer(32768 * 5)
    msg = (C.c_byte * 12)(*[x - 256 if x > 127 else x for x in data], 0)
    out = [C.create_string_buffer(32) for _ in range(5)]
    L.orc_unpk(msg, h, l, *out)
    return out[0].value.decode()


def symbols_of(message):
    return ol.channel_symbols(message)[1]


@functools.lru_cache(maxsize=None)
def weak_scene(seed, snr_db=-30.0):
    """tests/synth.py make_segment(seed) with one signal at snr_db: (I, Q, the text a decode of it prints)."""
    I, Q, truth = synth.make_segment(seed, symbols_of, snr_db=snr_db)
    return I, Q, synth.expected_text(truth[0][0])


def undecoded_worth(tr, npasses=1):
    """(pass, candidate, freq, shift, drift) of every candidate an oracle trace visited, found worth the ladder and left
    undecoded."""
    out = []
    for p in range(min(tr.passes_run, npasses)):
        for j in range(tr.n_visited[p]):
            cf = tr.cand_fine[p][j]
            if tr.decoded[p][j] or not np.float32(cf.sync) > MINSYNC1:
                continue
            out.append((p, j, cf.freq, cf.shift, cf.drift))
    return out
