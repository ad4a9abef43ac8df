"""The contracted-arithmetic checker (tests/helpers/contract_dsp.c) and the public switch, without a GPU.

Built with CONTRACT=0 the checker must be the CPU oracle byte for byte -- spots, residual IQ, per-stage trace and stop
points -- so that its restatement of the oracle differs from the oracle only where a site's macro turns into an fma
(CONTRACT=1).  wspr_set_arithmetic() exists in the product, defaults to exact and refuses anything but 0 and 1."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import contract_lib as cl
import oracle_lib as ol
import rtlsdr_wsprd_amd as w
from test_gpu_parity import random_scenes
from test_oracle_golden import _selftest_signal

NS = 45000


def _same_decode(a, b):
    sa, ia, qa, ta = a
    sb, ib, qb, tb = b
    assert [bytes(s) for s in sa] == [bytes(s) for s in sb]
    assert ia.tobytes() == ib.tobytes() and qa.tobytes() == qb.tobytes()
    assert bytes(ta) == bytes(tb) and ta.stop_reason == tb.stop_reason and ta.stop_cand == tb.stop_cand


def _both(I, Q, n=NS, opt=None):
    return (ol.decode(I, Q, n, opt, trace=True), cl.decode(0, I, Q, n, opt, trace=True))


def test_uncontracted_checker_is_the_oracle_on_the_reference_lines():
    I, Q, n = ol.read_iq_file(os.path.join(ol.GOLDEN, "refSignalSnr0dB.iq"))
    o, c = _both(I, Q, n)
    _same_decode(o, c)
    assert len(o[0]) == 1 and ol.spot_line(o[0][0]) == "Spot :  -0.07   0.01 144.490550  0    K1JT   FN20 20"
    I, Q = _selftest_signal()
    o, c = _both(I, Q)
    _same_decode(o, c)
    assert len(o[0]) == 1


def test_uncontracted_checker_is_the_oracle_on_random_scenes():
    """The 420 random scenes of tests/test_gpu_parity.py: every spot, residual sample and trace byte."""
    I, Q = random_scenes()
    cl.contract(0)
    ol.decode(I[0], Q[0], NS)                                   # static tables initialised before the threads start
    cl.decode(0, I[0], Q[0], NS)
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        res = list(ex.map(lambda s: _both(I[s], Q[s]), range(I.shape[0])))
    spots = 0
    for s, (o, c) in enumerate(res):
        _same_decode(o, c)
        spots += len(o[0])
    assert spots > 400


def test_contracted_checker_changes_the_arithmetic_and_not_the_decode_of_the_reference_line():
    I, Q, n = ol.read_iq_file(os.path.join(ol.GOLDEN, "refSignalSnr0dB.iq"))
    ps0, ps1 = cl.fft_bank(0, I, Q, n), cl.fft_bank(1, I, Q, n)
    assert not np.array_equal(ps0, ps1) and np.allclose(ps0, ps1, rtol=1e-5, atol=1e-6)
    s0, i0, q0 = cl.decode(0, I, Q, n)
    s1, i1, q1 = cl.decode(1, I, Q, n)
    assert [s.key() for s in s1] == [s.key() for s in s0] and len(s1) == 1
    assert abs(s1[0].snr - s0[0].snr) < 0.1 and abs(s1[0].dt - s0[0].dt) < 0.01 and abs(s1[0].freq - s0[0].freq) < 1e-7
    assert not np.array_equal(i0, i1) and np.allclose(i0, i1, atol=1e-4)


def test_set_arithmetic_defaults_round_trips_and_rejects_other_modes():
    L = w.lib()
    assert (w.WSPR_ARITH_EXACT, w.WSPR_ARITH_CONTRACTED) == (0, 1)
    assert L.wspr_set_arithmetic(0) == 0                        # the default
    assert L.wspr_set_arithmetic(1) == 0
    assert L.wspr_set_arithmetic(2) == -1 and L.wspr_set_arithmetic(-1) == -1      # refused, nothing changed
    assert L.wspr_set_arithmetic(1) == 1
    assert w.wspr_set_arithmetic(0) == 1
    assert w.wspr_set_arithmetic(0) == 0
    hdr = open(os.path.join(ol.ROOT, "include", "wspr_mi355x.h")).read()
    assert "#define WSPR_ARITH_EXACT      0" in hdr and "#define WSPR_ARITH_CONTRACTED 1" in hdr
    assert hasattr(w.lab(), "wspr_set_arithmetic") if os.path.exists(w.LAB_PATH) else True
