"""The fading channel's definition on the CPU (no GPU needed): the serial checker tests/helpers/fade_check.cpp over the
shared headers fade.h / synth_math.h -- synth_exp() against numpy, the existing synthesiser's samples unchanged, the
identity channel, the statistics of the gain, agreement with the model the Doppler-spread figure (K11) was calibrated on,
the shift, and the library's refusals."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import fade_lib as fl
import oracle_lib as ol
import rtlsdr_wsprd_amd as w
import spread_lib as sp
import synth
import synth_lib as sl

SIGMA = float(np.float32(np.sqrt((375.0 / 2500.0) / 2.0)))      # the project's noise level (tests/synth.py)
R = 4096                                                        # realisations of the statistics, taken over S
SEED = 20261019


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _differing(a, b):
    return int((_bits(a) != _bits(b)).sum())


def _symbols(k=0):
    ok, sym = ol.channel_symbols(synth.message_for(17 + 5 * k))
    assert ok
    return sym


def exp_error():
    """(largest relative error, largest distance in ulp) of synth_exp() against numpy.exp on 200 000 points of [-40, 0],
    both ends included.  (tools/fade_sensitivity.py records the same figures in profiles/fade_channel.json.)"""
    x = np.linspace(-40.0, 0.0, 200000)
    assert x[0] == -40.0 and x[-1] == 0.0
    got, want = fl.synth_exp(x), np.exp(x)
    return float(np.max(np.abs(got - want) / want)), float(np.max(np.abs(got - want) / np.spacing(want)))


def test_synth_exp_is_within_2_to_the_minus_40_of_exp():
    """2^-40 leaves the gain 16 bits finer than the float32 sample it ends in.  exp(0) is exactly 1."""
    rel, ulp = exp_error()
    print("synth_exp: largest relative error %.3e, largest distance %.1f ulp" % (rel, ulp))
    assert rel <= 2.0 ** -40
    assert fl.synth_exp(np.array([0.0]))[0] == 1.0
    x = np.array([-40.0, -32.0, -0.5 * np.log(2.0), -1e-300])
    assert np.all(np.abs(fl.synth_exp(x) - np.exp(x)) <= 2.0 ** -40 * np.exp(x))


def test_existing_noise_and_scenes_keep_their_bits():
    """synth_noise() is now a call of the generalised Box-Muller helper: the fixture holds digests of the scenes of
    tests/test_synth_checker.py and of three noise rows, taken with synth_math.h as it was before, through both checkers."""
    pins = json.load(open(os.path.join(ol.GOLDEN, "synth_k8_pins.json")))
    scenes = [(sl.selftest_item(), 0.0)]
    k = 0
    for f0 in (-150.0, -50.0, 50.0, 150.0):
        for amp in (1.0, 0.0316, 7.3):
            scenes.append(((0, f0, 2.0 + 0.37 * (k % 3), amp, 0.0, _symbols(k)), SIGMA))
            k += 1
    ok, sym = ol.channel_symbols(synth.message_for(3))
    scenes.append(((0, 31.25, 1.1, 0.5, -3.0, sym), SIGMA))
    for n, (item, sigma) in enumerate(scenes):
        for rc, I, Q in (sl.check_batch([item], 1, seg_index0=n, sigma=sigma, seed=11),
                         fl.check_batch([item], None, 1, seg_index0=n, sigma=sigma, seed=11)):
            assert rc == 0 and hashlib.sha256(I.tobytes() + Q.tobytes()).hexdigest() == pins["scenes_seed11_sha256"][n], n
    for k, (seed, seg) in enumerate(((11, 0), (20261016, 1000), ((1 << 64) - 1, (1 << 31) - 1))):
        rc, I, Q = sl.check_batch([], 1, seg_index0=seg, sigma=SIGMA, seed=seed)
        assert rc == 0 and hashlib.sha256(I.tobytes() + Q.tobytes()).hexdigest() == pins["noise"][2 * k]
        nI, nQ = fl.noise(seed, seg, 0, 8, SIGMA)
        assert [int(v) for v in _bits(nI)] + [int(v) for v in _bits(nQ)] == pins["noise"][2 * k + 1]


def _two_tx_scene():
    return [(0, 50.0, 2.0, 0.3, 0.0, _symbols(0)), (0, -31.25, -1.0, 1.7, 2.0, _symbols(1)), (1, 120.0, 11.0, 0.05, -3.0, _symbols(2))]


@pytest.mark.parametrize("flags", [0, sl.NORMALISE, sl.ACCUMULATE])
def test_identity_channel_and_no_channel_are_the_unfaded_scene(flags):
    items = _two_tx_scene()
    rng = np.random.default_rng(4)
    fill = (None, None)
    if flags & sl.ACCUMULATE:
        fill = (rng.normal(0, 0.3, (2, sl.NS)).astype(np.float32), rng.normal(0, 0.3, (2, sl.NS)).astype(np.float32))
    rc, I, Q = sl.check_batch(items, 2, 7, SIGMA, 5, flags, *fill)
    rc1, I1, Q1 = fl.check_batch(items, [fl.IDENTITY] * 3, 2, 7, SIGMA, 5, flags, *fill)
    rc2, I2, Q2 = fl.check_batch(items, None, 2, 7, SIGMA, 5, flags, *fill)
    assert rc == 0 and rc1 == 0 and rc2 == 0
    assert I1.tobytes() == I.tobytes() and Q1.tobytes() == Q.tobytes()
    assert I2.tobytes() == I.tobytes() and Q2.tobytes() == Q.tobytes()
    # and a faded channel is not the identity
    _, I3, _ = fl.check_batch(items, [[(1.0, 0.0, 0.2), (0.0, 0.0, 0.0)]] * 3, 2, 7, SIGMA, 5, flags, *fill)
    assert _differing(I3, I) > 40000


def _ensemble(channel, n, q=0, count=1, seed=SEED):
    """G[n .. n + count) over S = 0 .. R-1: complex128 [R, count]."""
    return np.stack([fl.gain(seed, S, q, channel, n, count) for S in range(R)])


@pytest.mark.parametrize("sigma", [0.001, 0.2, 10.0])
def test_mean_power_is_the_gain_squared(sigma):
    """G[n] at a fixed n is complex Gaussian, so |G|^2 / gain^2 is exponential with mean 1 and variance 1: the mean of R
    independent realisations (S differs, so all draws do) has standard error 1 / sqrt(R); the tolerance is five of them.
    n = 0 and 41 471 are the frame's ends, where the sum reaches k < 0 and past the last sample."""
    gain = 0.5
    for n in (0, 20000, 41471):
        g = _ensemble([(gain, 0.0, sigma), (0.0, 0.0, 0.0)], n)[:, 0]
        m = float(np.mean(np.abs(g) ** 2)) / gain ** 2
        print("sigma %.3f n %5d: E|G|^2 / gain^2 = %.4f (se %.4f)" % (sigma, n, m, 1 / np.sqrt(R)))
        assert abs(m - 1.0) <= 5.0 / np.sqrt(R)


@pytest.mark.parametrize("sigma", [0.2, 1.0])
def test_autocorrelation_is_the_gaussian_spectrums(sigma):
    """Z = G[n + tau] conj(G[n]) of unit-power circular Gaussians with correlation rho has E Z = rho, E|Z|^2 = 1 + rho^2
    and E Z^2 = 2 rho^2, so Var(Re Z) = (1 + rho^2) / 2 < 1: the standard error of the mean over R is below
    1 / sqrt(R), and 5 / sqrt(R) is more than five of them.  A Gaussian Doppler spectrum of deviation sigma has
    rho(tau) = exp(-2 pi^2 sigma^2 (tau / 375)^2) = 0.607 at tau = 375 / (2 pi sigma)."""
    tau = int(round(375.0 / (2.0 * np.pi * sigma)))
    want = float(np.exp(-2.0 * np.pi ** 2 * sigma ** 2 * (tau / 375.0) ** 2))
    g = _ensemble([(1.0, 0.0, sigma), (0.0, 0.0, 0.0)], 10000, count=tau + 1)
    got = float(np.mean((g[:, tau] * np.conj(g[:, 0])).real))
    print("sigma %.1f tau %d: %.4f against %.4f" % (sigma, tau, got, want))
    assert abs(want - 0.607) < 0.005 and abs(got - want) <= 5.0 / np.sqrt(R)


def test_rails_paths_and_transmissions_are_uncorrelated():
    """Correlation coefficients of independent unit-variance quantities: Re G and Im G have variance 1/2 each, so
    2 mean(Re G Im G) has standard error 1 / sqrt(R); for two independent unit-power complex gains mean(A conj(B)) has
    variance 1/2 per part, standard error 0.71 / sqrt(R).  All within 5 / sqrt(R)."""
    one = [(1.0, 0.0, 0.2), (0.0, 0.0, 0.0)]
    a = _ensemble(one, 20000)[:, 0]
    rails = 2.0 * float(np.mean(a.real * a.imag))
    b = _ensemble([(0.0, 0.0, 0.0), (1.0, 0.0, 0.2)], 20000)[:, 0]              # the other path of the same transmission
    c = _ensemble(one, 20000, q=1)[:, 0]                                        # the same path of the next transmission
    paths, txs = np.mean(a * np.conj(b)), np.mean(a * np.conj(c))
    print("rails %.4f  paths %.4f%+.4fj  transmissions %.4f%+.4fj  (5/sqrt(R) = %.4f)"
          % (rails, paths.real, paths.imag, txs.real, txs.imag, 5 / np.sqrt(R)))
    lim = 5.0 / np.sqrt(R)
    assert abs(rails) <= lim
    assert abs(paths.real) <= lim and abs(paths.imag) <= lim and abs(txs.real) <= lim and abs(txs.imag) <= lim
    assert abs(np.mean(np.abs(b) ** 2) - 1.0) <= lim and abs(np.mean(np.abs(c) ** 2) - 1.0) <= lim    # (and they are there)
    # the realisation is a function of (seed, S, q, p) alone
    assert np.array_equal(fl.gain(SEED, 9, 1, one, 20000, 4), fl.gain(SEED, 9, 1, one, 19998, 6)[2:])
    assert not np.array_equal(fl.gain(SEED + 1, 9, 1, one, 20000, 4), fl.gain(SEED, 9, 1, one, 20000, 4))


@pytest.mark.parametrize("sigma", [0.2, 1.0])
def test_width_agrees_with_the_model_the_spread_figure_was_calibrated_on(sigma):
    """64 noise-free frames through the channel and 64 through tests/spread_lib.py fading(): the medians of K11's w50
    (spread_lib.check) differ by at most four standard errors, each sample's being 1.25 IQR / 1.349 / sqrt(64) (the
    median of a near-normal sample), combined in quadrature.  Seeds: S = 0 .. 63 of seed 20261019 here, 7000 .. 7063
    there (the first set tried)."""
    sym = _symbols(0)
    item = (0, 50.0, 2.0, 1.0, 0.0, sym)
    ours, theirs = [], []
    for k in range(64):
        rc, I, Q = fl.check_batch([item], [[(1.0, 0.0, sigma), (0.0, 0.0, 0.0)]], 1, seg_index0=k, seed=SEED)
        assert rc == 0
        w50, _, _, valid = sp.check(I[0], Q[0], np.float32(50.0), 750, 0.0, sym)
        assert valid == 1
        ours.append(w50)
        I, Q, sh = sp.faded_segment(7000 + k, sym, 50.0, snr_db=0.0, sigma_hz=sigma, noise=False)
        w50, _, _, valid = sp.check(I, Q, np.float32(50.0), sh, 0.0, sym)
        assert valid == 1
        theirs.append(w50)

    def med_se(v):
        q1, q2, q3 = np.percentile(v, [25, 50, 75])
        return float(q2), 1.25 * float(q3 - q1) / 1.349 / np.sqrt(len(v))
    (ma, sa), (mb, sb) = med_se(ours), med_se(theirs)
    print("sigma %.1f: median w50 / sigma %.3f (se %.3f) here, %.3f (se %.3f) for spread_lib.fading()"
          % (sigma, ma / sigma, sa / sigma, mb / sigma, sb / sigma))
    assert abs(ma - mb) <= 4.0 * np.hypot(sa, sb)


@pytest.mark.parametrize("shift", [0.5, -10.0, 100.0])
def test_a_shifted_specular_path_is_the_transmission_at_the_shifted_frequency(shift):
    """Noise-free, amp 1, f0 + shift exact in float32.  Both sides round one double to float32 per sample (half an ulp of a
    value below 1 each: 2^-25), and both carry a serially accumulated phase: 41 472 adds, each rounding by at most half an
    ulp of the largest phase, 2 pi (|f0 + shift| + 2.2) 41 472 / 375 rad.  The shift's own phase w * n is one
    product.  The bound is the sum of those, about 4e-7 at 60 Hz; the largest difference found is printed."""
    sym = _symbols(1)
    f0 = 50.0
    rc, I, Q = fl.check_batch([(0, f0, 1.0, 1.0, 0.0, sym)], [[(1.0, shift, 0.0), (0.0, 0.0, 0.0)]], 1)
    rc2, J, P = sl.check_batch([(0, f0 + shift, 1.0, 1.0, 0.0, sym)], 1)
    assert rc == 0 and rc2 == 0 and float(np.float32(f0 + shift)) == f0 + shift
    top = 2.0 * np.pi * (abs(f0 + shift) + 2.2) * 41472 / 375.0
    top0 = 2.0 * np.pi * (abs(f0) + 2.2) * 41472 / 375.0
    bound = 2.0 * 2.0 ** -25 + 41472 * 0.5 * (np.spacing(top) + np.spacing(top0)) + np.spacing(2.0 * np.pi * abs(shift) * 41472 / 375.0)
    d = max(float(np.max(np.abs(I.astype(np.float64) - J))), float(np.max(np.abs(Q.astype(np.float64) - P))))
    print("shift %.1f: largest difference %.3e, bound %.3e" % (shift, d, bound))
    assert np.count_nonzero(I) > 41000 and d <= bound


def test_checker_refuses_what_the_library_refuses():
    item = (0, 50.0, 2.0, 1.0, 0.0, _symbols(0))
    nan, inf = float("nan"), float("inf")
    ok = (1.0, 0.0, 0.0)
    for bad in ((nan, 0.0, 0.0), (1.0, inf, 0.0), (1.0, 0.0, nan), (1.0, 0.0, 0.0005), (1.0, 0.0, 10.5), (1.0, 0.0, -0.2),
                (1.0, 100.5, 0.0), (1.0, -101.0, 0.2), (-inf, 0.0, 0.0)):
        for ch in ([bad, ok], [ok, bad]):
            rc, I, Q = fl.check_batch([item], [ch], 1)
            assert rc == -1 and not I.any() and not Q.any(), ch
    for good in ((1.0, 100.0, 10.0), (-2.0, -100.0, 0.001), (0.0, 0.0, 0.0)):
        assert fl.check_batch([item], [[good, ok]], 1)[0] == 0


def test_library_refuses_bad_channels_before_it_looks_for_a_device(capfd):
    """Both symbols exist, and every refusal the channel adds is made by the argument checks, which precede the device:
    -1, the reason on stderr, and guard-filled rows untouched -- with or without a GPU."""
    L = w.lib()
    assert hasattr(L, "wspr_synth_faded_batch_device") and hasattr(L, "wspr_synth_faded")
    assert C.sizeof(w.wspr_synth_channel) == 24
    item = (0, 50.0, 2.0, 1.0, 0.0, _symbols(0))
    arr = w.synth_tx_list([item])
    nan, inf = float("nan"), float("inf")
    ok = (1.0, 0.0, 0.0)
    cases = [((nan, 0.0, 0.0), "not finite"), ((1.0, -inf, 0.0), "not finite"), ((1.0, 0.0, inf), "not finite"),
             ((1.0, 0.0, 0.0005), "sigma neither 0 nor within"), ((1.0, 0.0, 10.5), "sigma neither 0 nor within"),
             ((1.0, 0.0, -1.0), "sigma neither 0 nor within"), ((1.0, 100.5, 0.0), "|shift| above 100 Hz"),
             ((1.0, -100.5, 0.2), "|shift| above 100 Hz")]
    for bad, text in cases:
        for ch in ([bad, ok], [ok, bad]):
            I = np.full(45000, 123.25, np.float32)
            Q = np.full(45000, -7.5, np.float32)
            chs = w.synth_channel_list([ch])
            capfd.readouterr()
            assert L.wspr_synth_faded(C.addressof(arr), C.addressof(chs), 1, 0.0, 0, 0, ol.ptr(I), ol.ptr(Q)) == -1
            assert text in capfd.readouterr().err, (ch, text)
            assert (I == np.float32(123.25)).all() and (Q == np.float32(-7.5)).all()
            assert L.wspr_synth_faded_batch_device(C.addressof(arr), C.addressof(chs), 1, 1, 0, 0.0, 0, 0, None, None) == -1
            assert text in capfd.readouterr().err
    # what the unfaded call refuses is refused here too, channel or not
    sym = item[5].copy()
    sym[7] = 9
    bad_tx = w.synth_tx_list([item[:5] + (sym,)])
    chs = w.synth_channel_list([[ok, ok]])
    I = np.full(45000, 123.25, np.float32)
    Q = np.full(45000, -7.5, np.float32)
    for ch in (C.addressof(chs), None):
        assert L.wspr_synth_faded(C.addressof(bad_tx), ch, 1, 0.0, 0, 0, ol.ptr(I), ol.ptr(Q)) == -1
        assert "channel symbol above 3" in capfd.readouterr().err
    assert L.wspr_synth_faded(C.addressof(arr), C.addressof(chs), 1, 0.0, 0, 4, ol.ptr(I), ol.ptr(Q)) == -1
    assert (I == np.float32(123.25)).all() and (Q == np.float32(-7.5)).all()
    with pytest.raises(ValueError):
        w.wspr_synth_faded([item], [[ok]])
