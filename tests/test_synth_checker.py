"""The synthesiser's contract on the CPU (no GPU needed): the checker (tests/helpers/synth_check.cpp over the shared
maths header synth_math.h) against an independent model on glibc's cos/sin, against the reference's own self-test
signal and its decode, the statistics and the counter property of its noise, and the library's behaviour without a
device."""
import ctypes as C

import numpy as np

import oracle_lib as ol
import rtlsdr_wsprd_amd as w
import synth
import synth_lib as sl

SIGMA = float(np.float32(np.sqrt((375.0 / 2500.0) / 2.0)))      # the project's noise level (tests/synth.py)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _differing(a, b):
    return int((_bits(a) != _bits(b)).sum())


def test_checker_equals_the_glibc_model_on_every_float_sample():
    """Independent of synth_math.h: the same serial phases through glibc's cos/sin (Python's math module) and the
    contract's statements.  The checker's double sin/cos are within one ulp of glibc's (about 3 % differ in the last
    bit); after the rounding to float32 not one sample may differ."""
    scenes = [(sl.selftest_item(), 0.0)]
    k = 0
    for f0 in (-150.0, -50.0, 50.0, 150.0):
        for amp in (1.0, 0.0316, 7.3):
            ok, sym = ol.channel_symbols(synth.message_for(17 + 5 * k))
            assert ok
            scenes.append(((0, f0, 2.0 + 0.37 * (k % 3), amp, 0.0, sym), SIGMA))
            k += 1
    ok, sym = ol.channel_symbols(synth.message_for(3))
    scenes.append(((0, 31.25, 1.1, 0.5, -3.0, sym), SIGMA))             # and one with drift
    total = 0
    for n, (item, sigma) in enumerate(scenes):
        rc, base_i, base_q = sl.check_batch([], 1, seg_index0=n, sigma=sigma, seed=11)
        assert rc == 0
        rc, I, Q = sl.check_batch([item], 1, seg_index0=n, sigma=sigma, seed=11)
        assert rc == 0
        if sigma > 0:
            assert np.count_nonzero(base_i) > 44000 and _differing(base_i, I) > 40000
        mi, mq = sl.libm_frame(item, base_i[0], base_q[0])
        d = _differing(I[0], mi) + _differing(Q[0], mq)
        print("scene %d f0 %.2f amp %.4f: %d differing float samples" % (n, item[1], item[3], d))
        total += d
    assert total == 0


def test_accumulate_over_the_reference_noise_is_the_reference_self_test():
    """decoderSelfTest() (rtlsdr_wsprd.c:729-760) = its noise (glibc rand(), seed 1) + one transmission: bit for bit what
    tests/test_oracle_golden.py builds sample by sample, and the oracle prints REPORT.md:198's line for it."""
    from test_oracle_golden import _selftest_signal
    ni, nq = sl.reference_noise()
    rc, I, Q = sl.check_batch([sl.selftest_item()], 1, flags=sl.ACCUMULATE, I=ni, Q=nq)
    assert rc == 0
    ri, rq = _selftest_signal()
    assert _differing(I[0], ri) == 0 and _differing(Q[0], rq) == 0
    spots, _, _ = ol.decode(I[0], Q[0], 45000)
    s = spots[0]
    line = "Spot(%i) %6.2f %6.2f %10.6f %2d %7s %6s %2s" % (
        0, s.snr, s.dt, s.freq, int(s.drift), s.call.decode(), s.loc.decode(), s.pwr.decode())
    assert line == "Spot(0)  22.80   0.01 144.490550  0    K1JT   FN20 20"


def test_noise_free_self_test_frame_decodes():
    rc, I, Q = sl.check_batch([sl.selftest_item()], 1)
    assert rc == 0
    spots, _, _ = ol.decode(I[0], Q[0], 45000)
    assert len(spots) == 1
    s = spots[0]
    assert (s.call, s.loc, s.pwr) == (b"K1JT", b"FN20", b"20")
    assert "%.2f %.2f" % (s.snr, s.dt) == "39.02 0.01"


def test_noise_is_gaussian_white_and_uncorrelated_between_rails():
    """45 000 x 64 complex draws against N(0, sigma^2), every statistic within 4 standard errors.  With N samples per
    rail: se(mean) = sigma / sqrt(N); se(variance) = sigma^2 sqrt(2 / N); se(excess kurtosis) = sqrt(24 / N);
    se(correlation coefficient of independent series) = 1 / sqrt(N) (lag 1 within a segment row, and I against Q)."""
    nseg = 64
    rc, I, Q = sl.check_batch([], nseg, seg_index0=1000, sigma=SIGMA, seed=20261016)
    assert rc == 0
    N = float(nseg * sl.NS)
    for name, x in (("I", I.astype(np.float64)), ("Q", Q.astype(np.float64))):
        mean, var = x.mean(), x.var()
        kurt = ((x - mean) ** 4).mean() / var ** 2 - 3.0
        lag1 = ((x[:, 1:] - mean) * (x[:, :-1] - mean)).mean() / var
        print("%s: mean %.3e (se %.3e)  var/sigma^2 - 1 %.3e (se %.3e)  kurtosis %.3e (se %.3e)  lag-1 %.3e (se %.3e)"
              % (name, mean, SIGMA / np.sqrt(N), var / SIGMA ** 2 - 1, np.sqrt(2 / N), kurt, np.sqrt(24 / N), lag1, 1 / np.sqrt(N)))
        assert abs(mean) < 4 * SIGMA / np.sqrt(N)
        assert abs(var - SIGMA ** 2) < 4 * SIGMA ** 2 * np.sqrt(2 / N)
        assert abs(kurt) < 4 * np.sqrt(24 / N)
        assert abs(lag1) < 4 / np.sqrt(nseg * (sl.NS - 1.0))
    a, b = I.astype(np.float64), Q.astype(np.float64)
    rho = ((a - a.mean()) * (b - b.mean())).mean() / np.sqrt(a.var() * b.var())
    print("I/Q correlation %.3e (se %.3e)" % (rho, 1 / np.sqrt(N)))
    assert abs(rho) < 4 / np.sqrt(N)


def test_noise_is_a_pure_function_of_seed_and_segment():
    rc, a, aq = sl.check_batch([], 2, seg_index0=5, sigma=SIGMA, seed=77)
    rc2, b, bq = sl.check_batch([], 2, seg_index0=5, sigma=SIGMA, seed=77)
    assert rc == 0 and rc2 == 0 and a.tobytes() == b.tobytes() and aq.tobytes() == bq.tobytes()
    assert _differing(a[0], a[1]) > 44000                              # another segment
    assert _differing(a[0], aq[0]) > 44000                             # the other rail
    _, c, _ = sl.check_batch([], 2, seg_index0=5, sigma=SIGMA, seed=78)
    assert _differing(a, c) > 88000                                    # another seed
    _, d, _ = sl.check_batch([], 1, seg_index0=6, sigma=SIGMA, seed=77)
    assert d[0].tobytes() == a[1].tobytes()                            # segment 6 is segment 6 wherever a batch starts
    _, e, _ = sl.check_batch([], 1, seg_index0=(1 << 31) - 1, sigma=SIGMA, seed=(1 << 64) - 1)
    assert np.isfinite(e).all() and np.count_nonzero(e) > 44000


def _scene(rng, nseg, per_seg=3):
    items = []
    for seg in range(nseg):
        for _ in range(int(rng.integers(0, per_seg + 1))):
            ok, sym = ol.channel_symbols(synth.message_for(int(rng.integers(0, 1 << 20))))
            assert ok
            items.append((seg, float(rng.uniform(-100, 100)), float(rng.uniform(-1, 3)), float(10 ** rng.uniform(-1.5, 0.5)),
                          float(rng.uniform(-4, 4)), sym))
    return items


def test_a_batch_split_into_two_calls_equals_the_one_call_batch():
    rng = np.random.default_rng(5)
    items = _scene(rng, 6)
    rc, I, Q = sl.check_batch(items, 6, seg_index0=40, sigma=SIGMA, seed=9, flags=sl.NORMALISE)
    assert rc == 0
    lo = [it for it in items if it[0] < 2]
    hi = [(it[0] - 2,) + it[1:] for it in items if it[0] >= 2]
    _, I0, Q0 = sl.check_batch(lo, 2, seg_index0=40, sigma=SIGMA, seed=9, flags=sl.NORMALISE)
    _, I1, Q1 = sl.check_batch(hi, 4, seg_index0=42, sigma=SIGMA, seed=9, flags=sl.NORMALISE)
    assert np.concatenate([I0, I1]).tobytes() == I.tobytes() and np.concatenate([Q0, Q1]).tobytes() == Q.tobytes()
    assert abs(max(np.abs(I[0]).max(), np.abs(Q[0]).max()) - 0.5) < 1e-6


def test_checker_refuses_what_the_library_refuses():
    good = sl.selftest_item()
    bad_sym = good[5].copy()
    bad_sym[100] = 4
    for items, nseg, sigma in (([(0, 50.0, 2.0, 1.0, 0.0, bad_sym)], 1, 0.0), ([(1,) + good[1:]], 1, 0.0),
                               ([(1,) + good[1:], good], 2, 0.0), ([(0, float("nan"), 2.0, 1.0, 0.0, good[5])], 1, 0.0),
                               ([(0, 50.0, float("inf"), 1.0, 0.0, good[5])], 1, 0.0), ([good], 1, float("nan")),
                               ([(0, 2000.0, 2.0, 1.0, 0.0, good[5])], 1, 0.0)):
        rc, I, Q = sl.check_batch(items, nseg, sigma=sigma)
        assert rc == -1 and not I.any() and not Q.any()


def test_library_has_the_synthesiser_and_refuses_loudly():
    """The three symbols exist in the product library.  Without a device wspr_synth() returns -1 and writes nothing
    (there is no CPU fallback); with one, a call it must refuse does the same."""
    L = w.lib()
    for name in ("wspr_synth_batch_device", "wspr_synth", "wspr_selftest"):
        assert hasattr(L, name)
    assert C.sizeof(w.wspr_synth_tx) == 184
    item = sl.selftest_item()
    if L.wspr_device_ready() == 1:
        sym = item[5].copy()
        sym[7] = 9
        item = item[:5] + (sym,)
    arr = w.synth_tx_list([item])
    I = np.full(45000, 123.25, np.float32)
    Q = np.full(45000, -7.5, np.float32)
    assert L.wspr_synth(C.addressof(arr), 1, 0.0, 0, 0, ol.ptr(I), ol.ptr(Q)) == -1
    assert (I == np.float32(123.25)).all() and (Q == np.float32(-7.5)).all()
