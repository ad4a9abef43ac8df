"""The band noise figures (K16) on the CPU: the serial checker (tests/helpers/noise_check.c over
rtlsdr-wsprd_amd/csrc/kernels/noise.h) against a numpy restatement of the definition and against crafted rows, its scaling on
white noise of known sigma, and the checker under AddressSanitizer as a stand-alone program.  No GPU."""
import subprocess

import numpy as np
import pytest

import noise_lib as nl


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _compare_with_numpy(I, Q, n, windows):
    """One row: everything the restatement states exactly is compared exactly, a[j] within the derived bound."""
    rec, p, a, rank = nl.detail(I, Q, n, windows)
    nf = nl.frames_of(n)
    if nl.has_non_finite(I, Q, n):                                           # the guard: the record alone is defined
        assert rec.tobytes() == np.array([(0, 0, 0, 0, 0, 0, nf, nl.NONFINITE)], nl.NOISE_DTYPE).tobytes()
        return rec, None, None, None
    w = nl.DEFAULT_WINDOWS if windows is None else windows
    p_np, pre_mean, pre_trough, post_mean, post_trough, flags = nl.gap_numpy(I, Q, n, w)
    nblk = n // nl.BLOCK
    assert np.array_equal(_bits(p[:nblk]), _bits(p_np)) and not p[nblk:].any()
    a64, total, _ = nl.spectrum_float64(I, Q, n)
    tol = nl.spectrum_tolerance(a64, total, nf)
    assert np.all(np.abs(a.astype(np.float64) - a64) <= tol), float(np.max(np.abs(a - a64) / np.maximum(tol, 1e-300)))
    rank_np, floor, p30 = nl.band_numpy(a)
    assert np.array_equal(rank, rank_np)
    if nf:
        flags |= nl.FFT_USED
    else:
        floor = p30 = np.float32(0)
    want = (pre_mean, pre_trough, post_mean, post_trough, floor, p30, nf, flags)
    got = tuple(rec[f] for f in nl.FIGURES) + (rec["nframes"], rec["flags"])
    assert [int(_bits(x)) for x in got[:6]] == [int(_bits(x)) for x in want[:6]] and got[6:] == want[6:], (got, want)
    return rec, a, a64, tol


@pytest.mark.parametrize("n", nl.LENGTHS)
def test_checker_equals_the_numpy_restatement(n):
    I, Q = nl.random_rows()
    worst = 0.0
    for s in range(I.shape[0]):
        for name, windows in [("null", None)] + nl.WINDOW_CASES:
            rec, a, a64, tol = _compare_with_numpy(I[s, :n], Q[s, :n], n, windows)
            if nl.frames_of(n):
                worst = max(worst, float(np.max(np.abs(a - a64) / tol)))
    print("n = %d: largest |a - a64| / bound = %.3f" % (n, worst))
    # the batch call over strided rows gives the same records as row by row
    batch = nl.check_rows(I, Q, n, nl.WINDOW_CASES[4][1])
    for s in range(I.shape[0]):
        assert batch[s].tobytes() == nl.detail(I[s, :n], Q[s, :n], n, nl.WINDOW_CASES[4][1])[0].tobytes()


def test_windows_do_what_their_names_say():
    I, Q = nl.random_rows()
    by = dict(nl.WINDOW_CASES)
    full = {name: nl.check_rows(I[0], Q[0], nl.NS, w)[0] for name, w in nl.WINDOW_CASES}
    assert full["both_empty"]["flags"] == nl.FFT_USED and full["empty_in_the_middle"]["flags"] == nl.FFT_USED
    assert full["both_empty"]["pre_mean"] == 0 and full["both_empty"]["post_trough"] == 0
    assert full["whole_row_twice"]["pre_mean"] == full["whole_row_twice"]["post_mean"] > 0
    assert full["whole_row_twice"]["pre_trough"] == full["whole_row_twice"]["post_trough"] <= full["default"]["pre_trough"]
    assert full["default"].tobytes() == nl.check_rows(I[0], Q[0], nl.NS, None)[0].tobytes()
    # a row of 511 samples has 31 whole blocks: [0, 40) is clipped to [0, 31), [30, 2000) to [30, 31)
    short = nl.check_rows(I[0, :511], Q[0, :511], 511, by["clipped_by_a_short_row"])[0]
    p = nl.detail(I[0, :511], Q[0, :511], 511)[1]
    assert short["flags"] == nl.PRE_USED | nl.POST_USED and short["nframes"] == 0
    assert short["post_mean"] == short["post_trough"] == p[30] and short["pre_trough"] == p[:31].min()
    # ... and one of 480 samples has 30: the post window is clipped away
    gone = nl.check_rows(I[0, :480], Q[0, :480], 480, by["clipped_by_a_short_row"])[0]
    assert gone["flags"] == nl.PRE_USED and gone["post_mean"] == 0 and gone["post_trough"] == 0
    # the spectrum does not depend on the windows
    assert len({(r["fft_floor"], r["fft_p30"], r["nframes"]) for r in full.values()}) == 1


@pytest.mark.parametrize("row", nl.crafted_rows(), ids=[r[0] for r in nl.crafted_rows()])
def test_crafted_rows(row):
    name, I, Q = row
    rec, a, a64, tol = _compare_with_numpy(I, Q, nl.NS, None)
    _, p, _, rank = nl.detail(I, Q, nl.NS)
    mid = nl.NFFT // 2
    if name == "zeros":
        assert rank.tolist() == list(range(nl.BAND))                         # every bin ties: rank order is j order
        assert rec["flags"] == 7 and not any(rec[f] for f in nl.FIGURES)
    elif name == "constant":
        power = np.float32(0.25 * 0.25 + 0.125 * 0.125)
        assert np.all(p == power) and rec["pre_mean"] == rec["pre_trough"] == rec["post_mean"] == power
        # Hann: the sum of w is 256, so bin 0 holds power * 256^2 / W2, each neighbour a quarter of that, the rest nothing
        assert abs(float(a[mid]) * nl.tables()[1] / (256.0 ** 2 * float(power)) - 1.0) < 1e-5
        assert abs(float(a[mid + 1]) / float(a[mid]) - 0.25) < 1e-5 and a[mid + 2] < 1e-9 * a[mid]
        assert rec["fft_floor"] < 1e-9 * a[mid]
    elif name == "tone_on_bin_40":
        assert int(np.argmax(a)) - mid == 40 and rank[40 + nl.BAND_HALF] == nl.BAND - 1
        assert np.all(np.abs(p - 0.25) < 1e-6)
    else:
        top = np.argsort(a)[-2:] - mid
        assert sorted(top.tolist()) == [-61, -60] and abs(float(a[mid - 61]) / float(a[mid - 60]) - 1.0) < 1e-3
    # a short row of each: the same through the batch entry
    for n in (767, 768):
        _compare_with_numpy(I[:n], Q[:n], n, (0, 2812, 40, 48))


@pytest.mark.parametrize("n", [16, 512, 768, 45000])
def test_non_finite_samples(n):
    I0, Q0 = nl.random_rows()
    clean = nl.check_rows(I0[1, :n], Q0[1, :n], n)[0]
    assert not clean["flags"] & nl.NONFINITE
    for name, k, value, counts in nl.non_finite_cases(n):
        for rail in (0, 1):
            I = np.zeros(n + 1, np.float32)
            Q = np.zeros(n + 1, np.float32)
            I[:n], Q[:n] = I0[1, :n], Q0[1, :n]
            (I, Q)[rail][k] = value
            rec = nl.check_rows(I, Q, n)[0]
            if counts:
                assert rec["flags"] == nl.NONFINITE and rec["nframes"] == nl.frames_of(n), name
                assert not any(_bits(rec[f]) for f in nl.FIGURES), name
            else:
                assert rec.tobytes() == clean.tobytes(), name
            _compare_with_numpy(I[:n], Q[:n], n, None)


def test_checker_refuses_what_the_library_refuses():
    import oracle_lib as ol
    chk = nl.checker()
    I = np.zeros(64, np.float32)
    out = np.full(8, -7, np.int32)
    p, o = ol.ptr(I), ol.ptr(out)

    def call(nseg, n, stride, win):
        w = np.array(win, np.int32)
        return chk.noise_check_rows(p, p, nseg, n, stride, ol.ptr(w), o)
    assert call(-1, 64, 64, nl.DEFAULT_WINDOWS) == -1 and call(1, -1, 64, nl.DEFAULT_WINDOWS) == -1
    assert call(1, 64, 63, nl.DEFAULT_WINDOWS) == -1 and call(0, 45001, 45001, nl.DEFAULT_WINDOWS) == -2
    for bad in ((-1, 5, 0, 0), (5, 4, 0, 0), (0, 2813, 0, 0), (0, 0, -1, 0), (0, 0, 9, 8), (0, 0, 0, 2813)):
        assert call(1, 64, 64, bad) == -1, bad
    assert np.all(out == -7)
    assert call(1, 64, 64, (0, 2812, 2812, 2812)) == 0 and out[7] == nl.PRE_USED and out[6] == 0


def test_white_noise_scaling():
    """64 rows of N(0, sigma^2) per rail: the gap means are unbiased estimates of 2 sigma^2, within five standard deviations
    each; the spectrum figure's bias (the order statistics of "the quietest 30 % of 443 averaged bins") is MEASURED and
    printed, not asserted against a constant: README, DESIGN.md and the public header quote it."""
    I, Q = nl.white_rows()
    rec = nl.check_rows(I, Q, nl.NS)
    ref = 2.0 * nl.SIGMA ** 2
    assert np.all(rec["flags"] == 7) and np.all(rec["nframes"] == 174)
    for fig, blocks in (("pre_mean", 36), ("post_mean", 118)):
        dev = (rec[fig].astype(np.float64) / ref - 1.0) / nl.mean_scatter(blocks)
        print("%s: largest deviation %.2f standard deviations (1 sd = %.4f of 2 s^2)" % (fig, np.abs(dev).max(), nl.mean_scatter(blocks)))
        assert np.all(np.abs(dev) < 5.0)
    stats = nl.white_noise_statistics()
    for fig in nl.FIGURES:
        print("%-11s / 2 s^2: mean %.4f, standard deviation %.4f (%.2f dB, %.2f dB)" % (
            fig, stats[fig][0], stats[fig][1], 10 * np.log10(stats[fig][0]), 10 * np.log10(1 + stats[fig][1])))
    # what IS known in advance: a mean of the lowest values lies below the mean of all, the next value above it
    assert np.all(rec["fft_floor"] < rec["fft_p30"]) and np.all(rec["fft_p30"] < ref)
    assert np.all(rec["pre_trough"] < rec["pre_mean"]) and np.all(rec["post_trough"] < rec["post_mean"])
    # scaling the rows by 10 dB scales every figure by 10 dB (up to float rounding): the figures are linear powers
    k = np.float32(np.sqrt(10.0))
    loud = nl.check_rows(I[:2] * k, Q[:2] * k, nl.NS)
    for fig in nl.FIGURES:
        assert np.allclose(loud[fig] / rec[fig][:2], 10.0, rtol=1e-5)


def test_checker_under_the_address_sanitizer(tmp_path):
    """A stand-alone program with its own main (no preloading, nothing loaded into Python): rows exactly as long as the
    contract allows, lengths 0 .. 45000, five window settings, a non-finite last sample."""
    r = subprocess.run([nl.sanitizer_program(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "noise_check: ok" in r.stdout and not r.stderr.strip()
