"""ctypes bindings of the contracted-arithmetic checker (tests/helpers/contract_dsp.c), built on demand against the CPU
oracle (oracle/liboracle.so).  contract(0) restates the oracle's arithmetic, contract(1) the fusions of
wspr_set_arithmetic(WSPR_ARITH_CONTRACTED).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as ol

_libs = {}


def contract(flag):
    """The checker built with -DCONTRACT=flag (0 or 1), cached per process."""
    if flag not in _libs:
        L = ol.lib()                                      # builds oracle/liboracle.so if it is missing
        out = os.path.join(tempfile.mkdtemp(prefix="wspr_contract_"), "libcontract%d.so" % flag)
        subprocess.run(["gcc", "-O3", "-std=gnu17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                        "-Wno-unused-function", "-DCONTRACT=%d" % flag, "-I", ol.ORACLE_DIR, "-shared", "-o", out,
                        os.path.join(ol.ROOT, "tests", "helpers", "contract_dsp.c"), "-L", ol.ORACLE_DIR, "-loracle",
                        "-Wl,-rpath," + ol.ORACLE_DIR, "-lm"], check=True)
        del L
        X = C.CDLL(out)
        X.ctr_wspr_decode_stops.argtypes = [C.c_void_p, C.c_void_p, C.c_int, ol.Options,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        X.ctr_wspr_decode_stops.restype = C.c_int
        X.ctr_sync_demod.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int,
                                     C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        X.ctr_subtract.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_int, C.c_float, C.c_void_p]
        X.ctr_fft_bank.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _libs[flag] = X
    return _libs[flag]


def decode(flag, I, Q, samples=None, opt=None, trace=False):
    """ol.decode() through the checker: (spots, residual I, Q[, trace with stop_reason / stop_cand])."""
    X = contract(flag)
    I = np.ascontiguousarray(I, dtype=np.float32).copy()
    Q = np.ascontiguousarray(Q, dtype=np.float32).copy()
    n = int(samples if samples is not None else I.size)
    opt = opt or ol.default_options()
    spots = (ol.Spot * 100)()
    nres = C.c_int(0)
    tr = ol.Trace() if trace else None
    st = ol.Stops()
    X.ctr_wspr_decode_stops(ol.ptr(I), ol.ptr(Q), n, opt, C.addressof(spots), C.addressof(nres),
                            C.addressof(tr) if trace else None, C.addressof(st))
    if trace:
        tr.stop_reason, tr.stop_cand = list(st.reason), list(st.cand)
    out = [spots[i] for i in range(nres.value)]
    return (out, I, Q, tr) if trace else (out, I, Q)


def fft_bank(flag, I, Q, n):
    blocks = ol.lib().orc_blocks_for(n)
    ps = np.zeros((512, blocks), np.float32)
    contract(flag).ctr_fft_bank(ol.ptr(I), ol.ptr(Q), C.c_int(n), ol.ptr(ps))
    return ps
