"""The Doppler-spread figure as its definition states it (rtlsdr-wsprd_amd/csrc/kernels/spread.h through the serial checker
tests/helpers/spread_check.c): floor and centre on an unspread carrier, the width of Gaussian Doppler spectra against
1.349 sigma, what makes a figure invalid, and frames that hang off the row.  No GPU."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import spread_lib as sl

F0 = np.float32(37.25)


@functools.lru_cache(maxsize=None)
def symbols():
    ok, sym = ol.channel_symbols("K1JT FN20QI 20")
    assert ok
    return sym


@pytest.mark.parametrize("noise", [False, True])
def test_unspread_carrier_sits_on_the_floor(noise):
    """sigma = 0 with the true (f0, shift, symbols), noise-free and at -15 dB: valid, and w50 a bin wide."""
    I, Q, sh = sl.faded_segment(11, symbols(), float(F0), snr_db=-15.0, noise=noise)
    w50, f50, ratio, valid = sl.check(I, Q, F0, sh, 0.0, symbols())
    print("noise", noise, "w50", w50, "f50", f50, "ratio", ratio)
    assert valid == 1 and 0.0 < w50 < 0.02
    assert abs(f50) < 0.01 and ratio > 100.0


def test_carrier_offset_is_reported():
    """The carrier 0.03 Hz above the f0 the job names."""
    I, Q, sh = sl.faded_segment(12, symbols(), float(F0), snr_db=-15.0)
    w50, f50, ratio, valid = sl.check(I, Q, np.float32(float(F0) - 0.03), sh, 0.0, symbols())
    print("w50", w50, "f50", f50)
    assert valid == 1 and abs(f50 - 0.03) < 0.01


def test_width_follows_the_doppler_spread():
    """-15 dB, 32 seeds per point: the medians rise with sigma, and from 0.1 Hz on lie within 20 % of 1.349 sigma."""
    med = []
    for sigma in (0.0, 0.1, 0.3, 1.0):
        w = []
        for seed in range(32):
            I, Q, sh = sl.faded_segment(1000 + seed, symbols(), float(F0), snr_db=-15.0, sigma_hz=sigma)
            w50, _, _, valid = sl.check(I, Q, F0, sh, 0.0, symbols())
            assert valid == 1
            w.append(w50)
        med.append(float(np.median(w)))
        print("sigma", sigma, "median", med[-1], "min", min(w), "max", max(w), "1.349 sigma", sl.GAUSS_W50 * sigma)
    assert med[0] < med[1] < med[2] < med[3]
    for m, sigma in zip(med[1:], (0.1, 0.3, 1.0)):
        assert abs(m - sl.GAUSS_W50 * sigma) <= 0.2 * sl.GAUSS_W50 * sigma, (sigma, m)


def test_invalid_inputs_give_zero_fields():
    """All-zero rows, one NaN sample and one Inf sample: valid = 0, the three floats 0, and the checker returns."""
    I, Q, sh = sl.faded_segment(13, symbols(), float(F0))
    z = np.zeros(sl.NS, np.float32)
    cases = [(z, z)]
    for bad in (np.nan, np.inf):
        Ib = I.copy()
        Ib[sh + 20000] = bad
        cases.append((Ib, Q))
        Qb = Q.copy()
        Qb[sh + 5] = -bad
        cases.append((I, Qb))
    for a, b in cases:
        assert sl.check_words(a, b, F0, sh, 0.0, symbols()).tolist() == [0, 0, 0, 0]
    assert sl.check(I, Q, F0, sh, 0.0, symbols())[3] == 1                     # the same row without the bad sample


@pytest.mark.parametrize("np_", [45000, 44993, 30000])
def test_frame_hanging_off_the_row_is_the_zero_extended_row(np_):
    """shift = -300 and shift = np - 41 000 give what the same row gives with zeros written where it has no samples."""
    I, Q, _ = sl.faded_segment(14, symbols(), float(F0), t0=-0.8, snr_db=-5.0)          # the frame begins at -300
    I, Q = I[:np_].copy(), Q[:np_].copy()
    pad = 42000
    Iz = np.concatenate([np.zeros(pad, np.float32), I, np.zeros(pad, np.float32)])
    Qz = np.concatenate([np.zeros(pad, np.float32), Q, np.zeros(pad, np.float32)])
    for shift in (-300, np_ - 41000):
        got = sl.check_words(I, Q, F0, shift, 0.0, symbols(), np_=np_)
        want = sl.check_words(Iz, Qz, F0, shift + pad, 0.0, symbols())
        assert got.tolist() == want.tolist(), shift
    # a frame that begins at -300 still holds nearly all of the signal: a figure, not a refusal
    assert sl.check(I, Q, F0, -300, 0.0, symbols(), np_=np_)[3] == 1
    # and one that misses the row altogether has nothing to measure
    assert sl.check_words(I, Q, F0, np_ + 10, 0.0, symbols(), np_=np_).tolist() == [0, 0, 0, 0]
