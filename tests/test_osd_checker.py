"""Ordered-statistics decoding WITHOUT a GPU: the serial checker tests/helpers/osd_check.cpp (what the kernel K9 is held
to, tests/test_gpu_osd.py) against an independent numpy statement of the definition in
rtlsdr-wsprd_amd/csrc/kernels/osd.h, against the code itself (the returned message re-encodes to a codeword with the
reported cost), on inputs whose answer is known, and on degenerate vectors; and the message layer's "heard before"
gate, wspr::osd_accept(), over the reference's flat hash tables."""
import ctypes as C

import numpy as np
import pytest

import osd_lib as ol
import rtlsdr_wsprd_amd as w


@pytest.fixture(scope="module")
def ladder():
    return ol.ladder_vectors(40)


def test_checker_equals_the_numpy_statement(ladder):
    vec, _ = ladder
    for t in range(len(vec)):
        for depth in (0, 1, 2):
            assert ol.check(vec[t], depth) == ol.numpy_osd(vec[t], depth), (t, depth)
    for t in (0, 5, 7, 9, 11):                            # clean, near the edge, and hopeless
        assert ol.check(vec[t], 3) == ol.numpy_osd(vec[t], 3), t


def test_packed_arithmetic_of_the_kernel_equals_the_checker(ladder):
    """What K9 computes, emulated lane by lane with the packed half of osd.h (tests/helpers/osd_packed_check.cpp: 7-word
    rows, bit-plane cost, packed keys, the pair list dealt over 64 lanes), against the serial checker: the ladder, the
    degenerate vectors (every reliability ties) and random bytes, depth 0..2 on all and depth 3 on every fourth."""
    vec, _ = ladder
    rng = np.random.default_rng(5)
    every = np.concatenate([vec, ol.degenerate_vectors(), rng.integers(0, 256, (40, ol.N)).astype(np.uint8),
                            rng.integers(100, 156, (20, ol.N)).astype(np.uint8)])
    for t, v in enumerate(every):
        for depth in (0, 1, 2) + ((3,) if t % 4 == 0 else ()):
            assert ol.check_packed(v, depth) == ol.check(v, depth), (t, depth)
    assert ol.packed().osd_packed(every[0].ctypes.data, 4, None, None, None, None) == -1


def test_returned_message_reencodes_to_the_reported_codeword(ladder):
    vec, msgs = ladder
    for t in range(len(vec)):
        s = vec[t].astype(int)[ol.PERM]
        h, r = (s >= 128), np.abs(2 * s - 255)
        assert r.min() >= 1 and r.max() <= 255 and np.all(r % 2 == 1)
        for depth in (0, 2, 3):
            data, dist, nhard, order = ol.check(vec[t], depth)
            assert order <= depth and data[6] & 0x3F == 0 and data[7:] == (0, 0, 0, 0)
            cw = ol.encode_bits(data) > 0
            assert int(r[cw != h].sum()) == dist and int((cw != h).sum()) == nhard, (t, depth)
            if t % 12 < 2:                                # sigma 5 and 25 against +-50: at most a few weak errors
                assert data == tuple(int(x) for x in msgs[t]), (t, depth)


def test_errors_on_the_least_reliable_positions_cost_no_order():
    rng = np.random.default_rng(11)
    for t in range(6):
        data = [int(x) for x in rng.integers(0, 256, 7)] + [0, 0, 0, 0]
        data[6] &= 0xC0
        cw = ol.encode_bits(data)
        amp = rng.integers(50, 128, ol.N)                 # reliabilities 2 * amp - 1 >= 99 ...
        s = np.where(cw > 0, 127 + amp, 128 - amp)
        bad = rng.choice(ol.N, 20, replace=False)         # ... but 1 on twenty positions, whose decisions are all wrong
        s[bad] = np.where(cw[bad] > 0, 127, 128)
        # any other codeword differs from the sent one on a basis position (reliability >= 99 > 20 = this one's cost)
        for depth in (0, 1, 3):
            assert ol.check(ol.interleave(s), depth) == (tuple(data), 20, 20, 0), (t, depth)


def test_cost_never_grows_with_depth(ladder):
    vec, _ = ladder
    for t in range(len(vec)):
        d = [ol.check(vec[t], depth)[1] for depth in range(4)]
        assert d[0] >= d[1] >= d[2] >= d[3], (t, d)


def test_degenerate_vectors():
    deg = ol.degenerate_vectors()
    for k, v in enumerate(deg):
        for depth in (0, 1, 2):
            assert ol.check(v, depth) == ol.numpy_osd(v, depth), (k, depth)
    assert ol.check(deg[3], 3) == ol.numpy_osd(deg[3], 3)
    assert ol.check(deg[6], 3) == ol.numpy_osd(deg[6], 3)
    # all-0 / all-127 are the zero codeword as received; all-255 is no codeword (the code is not closed under complement)
    assert ol.check(deg[1], 0) == ((0,) * 11, 0, 0, 0) and ol.check(deg[3], 3) == ((0,) * 11, 0, 0, 0)
    assert ol.check(deg[2], 3)[1] > 0
    assert ol.checker().osd_check(deg[0].ctypes.data, 4, None, None, None, None) == -1
    assert ol.checker().osd_check(deg[0].ctypes.data, -1, None, None, None, None) == -1


def _decdata(text):
    """The 50 bits of a message text as the decoder leaves them: its channel symbols, noiseless, through the checker."""
    ok, sym = w.get_wspr_channel_symbols(text)
    assert ok
    data, dist, _, order = ol.check(np.where(sym >> 1, 255, 0).astype(np.uint8), 0)
    assert dist == 0 and order == 0
    return np.array(data, np.uint8)


def test_gate_accepts_only_type1_messages_of_known_calls():
    L = ol.checker()
    hashtab = np.zeros(32768 * 13, np.uint8)
    loctab = np.zeros(32768 * 5, np.uint8)

    def gate(text):
        d = _decdata(text)
        return L.osd_gate(d.ctypes.data, hashtab.ctypes.data, loctab.ctypes.data)

    def store(call):
        slot = w.lib().nhash(call.encode(), len(call), 146)
        hashtab[slot * 13:slot * 13 + len(call)] = np.frombuffer(call.encode(), np.uint8)

    assert gate("K1ABC FN42 37") == 0                     # empty table: nobody was heard before
    assert not hashtab.any() and not loctab.any()         # ... and the refusal stored nothing
    store("K1ABC")
    store("PJ4/K1ABC")
    slot = w.lib().nhash(b"G4JNT", 5, 146)                # G4JNT's slot holds ANOTHER call
    hashtab[slot * 13:slot * 13 + 5] = np.frombuffer(b"DL1XX", np.uint8)
    before = hashtab.copy()
    assert gate("K1ABC FN42 37") == 1 and gate("K1ABC JO65 10") == 1
    assert gate("W9XYZ EM12 23") == 0                     # another call
    assert gate("PJ4/K1ABC 37") == 0                      # type 2, its call known
    assert gate("<PJ4/K1ABC> FK52UD 37") == 0             # type 3, its hash known
    assert gate("G4JNT IO90 30") == 0
    # nothing was stored by any of the calls, accepted or refused: both tables as they were before the first of them
    assert np.array_equal(hashtab, before) and not loctab.any()


def test_setter_and_argument_checks_need_no_device():
    """wspr_set_osd_depth() is a process-wide setting and the argument checks of wspr_osd_batch_device() come before
    anything touches a device: both behave as the header says on a machine without one, in either library."""
    for L in (w.lib(), w.lab()):
        try:
            assert w.set_osd_depth(-1, L) == -1               # off is the default
            assert w.set_osd_depth(2, L) == -1 and w.set_osd_depth(0, L) == 2 and w.set_osd_depth(3, L) == 0
            assert w.set_osd_depth(4, L) == -2 and w.set_osd_depth(-2, L) == -2 and w.set_osd_depth(3, L) == 3
        finally:
            w.set_osd_depth(-1, L)
        sym = np.zeros(162, np.uint8)
        out = np.full(16, 0xA5, np.uint8)
        u = np.full(4, 0xA5A5A5A5, np.uint32)
        args = (out.ctypes.data, u.ctypes.data, u.ctypes.data, u.ctypes.data)
        assert L.wspr_osd_batch_device(sym.ctypes.data, 0, 3, *args) == 0             # n == 0: nothing happens
        assert L.wspr_osd_batch_device(sym.ctypes.data, 1, 4, *args) == -1            # depth outside 0..3
        assert L.wspr_osd_batch_device(sym.ctypes.data, 1, -1, *args) == -1
        assert L.wspr_osd_batch_device(sym.ctypes.data, -1, 0, *args) == -1           # n < 0
        assert np.all(out == 0xA5) and np.all(u == 0xA5A5A5A5)
