"""The decimator oracle (oracle/orc_frontend.c) against the reference's own compiled callback, without a GPU.

oracle/Makefile compiles the reference's rtlsdr_wsprd.c where it lies, behind declaration-only <rtl-sdr.h> and
<curl/curl.h> stand-ins, into oracle/_ref/librtlsdr_front_ref.so; a wrapper exports a feeder around the file-local
callback and a reader of its output buffer.  The callback's state cannot be reset, so every stream gets a fresh copy of
the library (oracle_lib.ref_front_end()).  Both sides are fed the same chunks; every output is compared bit for bit.

The tests skip only when the library is absent (a checkout where the reference was never mounted)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_parity import _raw_stream

NS = 45000


def front():
    fe = ol.ref_front_end()
    if fe is None:
        pytest.skip("oracle/_ref/librtlsdr_front_ref.so is not built (the reference is not mounted)")
    return fe


def both(raw, sizes):
    """raw u8 stream cut into chunks of the given sizes -> (oracle I, Q, fill), (reference I, Q, count)."""
    assert sum(sizes) == raw.size and all(c % 8 == 0 for c in sizes)
    fe = front()
    L = ol.lib()
    st = L.orc_decim_new()
    oi = np.zeros(NS, np.float32); oq = np.zeros(NS, np.float32)
    fill = pos = 0
    for c in sizes:
        chunk = np.ascontiguousarray(raw[pos:pos + c])
        before = chunk.copy()
        fill = L.orc_decim_feed(C.c_void_p(st), ol.ptr(chunk), c, ol.ptr(oi), ol.ptr(oq), fill, NS)
        assert fe.feed(chunk) == fill, pos
        assert np.array_equal(chunk, before)                     # neither side touched the caller's bytes
        pos += c
    L.orc_decim_free(C.c_void_p(st))
    return (oi, oq, fill), fe.outputs()


def equal(o, r, want):
    assert o[2] == r[2] == want
    assert o[0].tobytes() == r[0].tobytes() and o[1].tobytes() == r[1].tobytes()


def test_tone_and_noise_with_rail_runs():
    """The stream of test_decimator_bit_exact_vs_oracle: 0x00 runs (int8 -128, whose negation wraps) and 0xff runs."""
    rng = np.random.default_rng(11)
    nsamp = 6401 * 300 + 1000
    n = np.arange(nsamp)
    sig = 6.0 * np.exp(1j * 2 * np.pi * (-600000.0 + 40.0) / 2.4e6 * n)
    raw = np.empty(2 * nsamp, np.uint8)
    raw[0::2] = np.clip(np.round(127.5 + sig.real + rng.normal(0, 10, nsamp)), 0, 255).astype(np.uint8)
    raw[1::2] = np.clip(np.round(127.5 + sig.imag + rng.normal(0, 10, nsamp)), 0, 255).astype(np.uint8)
    raw[:64] = 0
    raw[64:128] = 255
    raw = raw[:(raw.size // 8) * 8]
    o, r = both(raw, [raw.size])
    equal(o, r, 300)
    assert np.abs(o[0][40:300]).max() > 1e6                      # the in-band tone came through


def test_zero_bytes_on_block_edges_and_hard_clipping():
    """The stream of test_decimator_block_edges_and_clipping_equal_oracle."""
    rng = np.random.default_rng(12)
    nblk = 70
    raw = _raw_stream(rng, 6401 * nblk + 3000, f0=-35.0, amp=8.0)
    for b in (1, 2, 3, 9, 10, 17, 33, 34, 35, 64):
        k = 6401 * b + int(rng.integers(-9, 10))
        raw[2 * k + int(rng.integers(0, 2))] = 0
    raw[2 * (6401 * 20 + 3000)] = 0
    lo, hi = 2 * 6401 * 40, 2 * 6401 * 43
    n = np.arange((hi - lo) // 2)
    raw[lo:hi:2] = np.clip(np.round(127.5 + 400.0 * np.cos(2 * np.pi * (-600000.0 + 20.0) / 2.4e6 * n)), 0, 255).astype(np.uint8)
    raw = raw[:(raw.size // 16) * 16]
    o, r = both(raw, [raw.size])
    equal(o, r, nblk)
    o, r = both(np.maximum(raw, 1), [raw.size])                  # the same rows without any zero byte
    equal(o, r, nblk)


def test_streamed_under_four_chunkings():
    """The stream and the chunkings of test_streaming_decimator_any_chunking_equals_oracle: the mixer phase restarts
    with every callback in the reference, and so it must in the oracle."""
    rng = np.random.default_rng(21)
    nsamp = 6401 * 90 + 3206
    raw = _raw_stream(rng, nsamp)
    raw[1000:1256] = 0
    raw[70000:70512] = 255
    nbytes = raw.size
    chunkings = [[65536] * (nbytes // 65536) + ([nbytes % 65536] if nbytes % 65536 else []), [nbytes]]
    sizes, left = [], nbytes
    while left:
        c = min(left, 16 * int(rng.integers(1, 3000)))
        sizes.append(c); left -= c
    chunkings.append(sizes)
    chunkings.append([16] * 40 + [6400 * 2 - 640] + [nbytes - 640 - (6400 * 2 - 640)])
    outs = []
    for sizes in chunkings:
        o, r = both(raw, sizes)
        equal(o, r, 90)
        outs.append(o)
    assert outs[0][0].tobytes() == outs[1][0].tobytes()          # chunks of whole 4-sample groups: the same stream


def test_a_full_length_stream_saturates_at_45000_outputs():
    """Two minutes and a little more of input, in callbacks of 65536 bytes cut from one block of tone plus noise at
    moving offsets: the integrators wrap many times over, the count stops at 45000 and later input changes nothing."""
    rng = np.random.default_rng(31)
    block = _raw_stream(rng, 8 * 65536, f0=25.0, amp=5.0)
    block[5000:5064] = 0
    block[90000:90064] = 255
    fe = front()
    L = ol.lib()
    st = L.orc_decim_new()
    oi = np.zeros(NS, np.float32); oq = np.zeros(NS, np.float32)
    ncall = 45046 * 6401 * 2 // 65536 + 1
    fill = 0
    for k in range(ncall):
        off = (k * 7919 * 8) % (block.size - 65536)
        chunk = np.ascontiguousarray(block[off:off + 65536])
        fill = L.orc_decim_feed(C.c_void_p(st), ol.ptr(chunk), 65536, ol.ptr(oi), ol.ptr(oq), fill, NS)
        count = fe.feed(chunk)
        assert count == fill, k
    L.orc_decim_free(C.c_void_p(st))
    assert ncall * 32768 // 6401 > NS + 40                        # more was offered than fits
    ri, rq, n = fe.outputs()
    assert n == fill == NS
    assert oi.tobytes() == ri.tobytes() and oq.tobytes() == rq.tobytes()
    assert np.isfinite(oi).all() and np.abs(oi[NS - 100:]).max() > 0


def test_the_compiled_receiver_passes_its_own_self_test():
    """decoderSelfTest() of the same library (rtlsdr_wsprd.c:729-789): the decoder behind it is the reference's, with
    the oracle's FFT."""
    assert front().self_test() == 1
