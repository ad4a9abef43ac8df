"""The decode-quality figures of a spot WITHOUT a GPU: the serial checker tests/helpers/spot_quality_check.c (what the
kernel K19 is held to, tests/test_gpu_spot_quality.py) against the product library's own encode() + interleave(), against
the *metric the exported fano() returns (identity (a) of rtlsdr-wsprd_amd/csrc/kernels/spot_quality.h), against a numpy
statement of the sums on vectors whose answer is known; and the text of wspr_format_spot_extended() (host code)."""
import ctypes as C

import numpy as np

import rtlsdr_wsprd_amd as w
import spotq_lib as sq


def _product_codeword(decdata):
    """encode() + interleave() of the product library on the 50 message bits of decdata and 31 zero tail bits."""
    L = w.lib()
    data = np.zeros(11, np.uint8)
    data[:7] = decdata[:7]
    data[6] &= 0xC0
    coded = np.zeros(176, np.uint8)
    L.encode(coded.ctypes.data_as(C.c_void_p), data.ctypes.data_as(C.c_void_p), C.c_uint(11))
    sym = coded[:162].copy()
    L.interleave(sym.ctypes.data_as(C.c_void_p))
    return sym


def test_code_word_is_encode_plus_interleave_of_the_product_library():
    rng = np.random.default_rng(50)
    dec = sq.random_decdata(rng, 64)
    for k in range(64):
        got, want = sq.codeword(dec[k]), _product_codeword(dec[k])
        assert set(np.unique(want)) <= {0, 1} and np.array_equal(got, want), k
    # bits beyond the fiftieth are not read: the code word is that of the 50 message bits and a zero tail
    noisy = dec[:8].copy()
    noisy[:, 6] |= 0x3F
    noisy[:, 7:] = 0xFF
    for k in range(8):
        assert np.array_equal(sq.codeword(noisy[k]), sq.codeword(dec[k]))
    assert not sq.codeword(np.zeros(11, np.uint8)).any()


def test_metric_is_what_fano_returns():
    """Identity (a): on every vector on which the exported fano() returns 0, the checker's metric on Fano's decdata is
    Fano's *metric -- gamma at the last node, the sum of the 81 branch metrics of the decoded path."""
    cand = sq.fano_candidates()
    vec, dec, metric = sq.fano_successes()
    got = sq.check(vec, dec)
    print("fano() decodes %d of %d vectors; metric %d .. %d, nhard %d .. %d" % (len(vec), len(cand), metric.min(), metric.max(),
                                                                              got[:, 0].min(), got[:, 0].max()))
    assert len(vec) >= 20
    bad = np.flatnonzero(got[:, 4] != metric)
    assert bad.size == 0, (bad[:5], got[bad[:5], 4], metric[bad[:5]])
    # Fano leaves the bits behind the fiftieth zero, and a noise-free code word has no hard error
    assert not (dec[:, 6] & 0x3F).any() and not dec[:, 7:].any()
    assert (got[:, 0] == 0).sum() >= 10 and got[:, 0].max() >= 15


def test_edge_vectors_have_the_sums_numpy_gives():
    rng = np.random.default_rng(5)
    edge = sq.edge_vectors()
    dec = sq.random_decdata(rng, 16)
    for d in dec:
        code = np.tile(sq.codeword(d), (len(edge), 1))
        got = sq.check(edge, np.tile(d, (len(edge), 1)))
        assert np.array_equal(got[:, :4], sq.numpy_sums(edge, code)), d
        ones = int(code[0].sum())
        # all 0: every one of the code word is a hard error of weight 255; all 128: every zero, weight 1
        assert tuple(got[0, :4]) == (ones, 255 * ones, 255 * 162, 255 * 255 * 162)
        assert tuple(got[1, :4]) == (162 - ones, 255 * (162 - ones), 255 * 162, 255 * 255 * 162)
        assert tuple(got[2, :4]) == (ones, ones, 162, 162) and tuple(got[3, :4]) == (162 - ones, 162 - ones, 162, 162)
        assert got[4, 2] == 162 and got[4, 3] == 162
        mt = sq.mettab()
        assert got[0, 4] == int(mt[code[0], 0].sum()) and got[3, 4] == int(mt[code[0], 128].sum())
    # random soft bytes as well, and the metric through the table
    vec = rng.integers(0, 256, (32, 162), dtype=np.uint8)
    dec = sq.random_decdata(rng, 32)
    code = np.stack([sq.codeword(d) for d in dec])
    got = sq.check(vec, dec)
    assert np.array_equal(got[:, :4], sq.numpy_sums(vec, code))
    assert np.array_equal(got[:, 4], sq.mettab()[code.astype(int), vec.astype(int)].sum(axis=1))
    out = np.full(5, 77, np.int32)
    assert sq.checker().spot_quality_check(vec.ctypes.data, dec.ctypes.data, -1, sq.mettab().ctypes.data, out.ctypes.data) == -1
    assert (out == 77).all()


def _spot(snr, dt, freq, drift, call, loc, pwr):
    r = w.decoder_results()
    r.snr, r.dt, r.freq, r.drift = snr, dt, freq, drift
    r.call, r.loc, r.pwr = call, loc, pwr
    return r


def test_extended_spot_line():
    det = np.zeros(2, w.SPOT_DETAIL_DTYPE)
    det[0] = (23, 1467, 30123, 6000000, 4012, 0, 1, 1, 1, 3, 0)
    det[1] = (0, 0, 41310, 10534050, -1234, 2, 5, 1, 1, 17, 0)
    a = _spot(-21.04, 0.11, 14.0971, 0.0, b"K1JT", b"FN20", b"20")
    b = _spot(3.5, -1.25, 144.490512, -2.0, b"PJ4/K1ABC", b"", b"37")
    want_a = "Spot : -21.04   0.11  14.097100  0    K1JT   FN20 20 0 1 1  23  1467   4012"
    want_b = "Spot :   3.50  -1.25 144.490512 -2 PJ4/K1ABC        37 2 5 1   0     0  -1234"
    for r, d, want in ((a, det[0:1], want_a), (b, det[1:2], want_b)):
        text, n = w.format_spot_extended(r, d)
        assert (text, n) == (want, len(want))
        # the line begins with wspr_format_spot()'s
        plain = C.create_string_buffer(160)
        m = w.lib().wspr_format_spot(C.byref(r), plain, 160)
        assert text[:m] == plain.value.decode() and text[m] == " "
        # a short cap: the whole length is reported, cap - 1 characters and the NUL are written, nothing behind them
        buf = C.create_string_buffer(b"\xa5" * 64, 64)
        assert w.lib().wspr_format_spot_extended(C.byref(r), d.ctypes.data_as(C.c_void_p), buf, 20) == len(want)
        assert buf.raw[:19] == want[:19].encode() and buf.raw[19] == 0 and buf.raw[20:] == b"\xa5" * 44


def test_settings_and_records_without_a_decode_call():
    """The switch is host state: it answers without a device, and no record exists before a decode call."""
    L = w.lib()
    assert w.set_spot_details(0) == 0
    assert w.set_spot_details(2) == -2 and w.set_spot_details(-1) == -2 and w.set_spot_details(0) == 0
    assert w.set_spot_details(1) == 0 and w.set_spot_details(0) == 1
    buf = np.zeros(4, w.SPOT_DETAIL_DTYPE)
    assert L.wspr_last_spot_details(buf.ctypes.data_as(C.c_void_p), 4) == -1 and not buf.view(np.uint8).any()
    assert w.SPOT_DETAIL_DTYPE.itemsize == 32 and w.SPOT_QUALITY_DTYPE.itemsize == 20
    out = np.full(5, 77, np.int32)
    sym, dec = np.zeros(162, np.uint8), np.zeros(11, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.wspr_spot_quality_batch_device(p(sym), p(dec), 0, p(out)) == 0                # n == 0 does nothing
    assert L.wspr_spot_quality_batch_device(p(sym), p(dec), -1, p(out)) == -1
    assert L.wspr_spot_quality_batch_device(None, p(dec), 1, p(out)) == -1 and (out == 77).all()
