"""The Doppler-spread figure on the device (K11, wspr_spread_batch / wspr_set_spread_estimate / wspr_last_spreads; the
definition in rtlsdr-wsprd_amd/csrc/kernels/spread.h).  Every comparison is on the four result words as bit patterns
against the serial CPU checker (tests/spread_lib.py): the kernel over host rows, the entry point's refusals, both
arithmetic modes, the stage inside the decode loop (before the subtraction, records following the spots through sort and
cut) and "off is off"."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as orc
import spread_lib as sl
import synth

pytestmark = pytest.mark.gpu
NS = 45000


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    return mod


@pytest.fixture()
def stage_off(w):
    """Whatever a test sets, the next one starts with the stage off and exact arithmetic."""
    yield
    w.set_spread_estimate(0)
    w.wspr_set_arithmetic(0)


def symbols_of(message):
    return orc.channel_symbols(message)[1]


# ---- the kernel over host rows ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows(n):
    """Five rows of n samples: a -10 dB signal, zeros, a faded -5 dB signal, and the first row with one NaN / one Inf."""
    sym = symbols_of("K1JT FN20QI 20")
    I0, Q0, truth = synth.make_segment(700 + n, symbols_of, snr_db=-10.0)
    f0, s0 = np.float32(truth[0][1]), int(round(truth[0][2] * 375))
    sym0 = symbols_of(truth[0][0])
    I2, Q2, s2 = sl.faded_segment(800 + n, sym, -61.5, t0=1.3, snr_db=-5.0, sigma_hz=0.2)
    In, Qi = I0.copy(), Q0.copy()
    In[s0 + 12345] = np.nan
    Qi[s0 + 777] = np.inf
    z = np.zeros(NS, np.float32)
    I = np.stack([I0, z, I2, In, I0])[:, :n].copy()
    Q = np.stack([Q0, z, Q2, Q0, Qi])[:, :n].copy()
    return I, Q, (f0, s0, sym0), (np.float32(-61.5), s2, sym)


@functools.lru_cache(maxsize=None)
def _scene(n, count=300):
    import rtlsdr_wsprd_amd as mod
    I, Q, (f0, s0, sym0), (f2, s2, sym2) = _rows(n)
    all0, all3 = np.zeros(162, np.uint8), np.full(162, 3, np.uint8)
    it = [(2, f2, s2, 0.0, sym2), (0, f0, s0, 0.0, sym0), (1, f0, s0, 0.0, sym0)]     # mixed row order from the start
    it += [(0, f0, sh, 0.0, sym0) for sh in (-300, 0, 1, 2, 3, n - 41000, n + 10)]
    it += [(2, f2, sh, 0.0, sym2) for sh in (-300, 0, 1, 2, 3, n - 41000, n + 10)]
    it += [(0, 150.0, s0, 4.0, sym0), (2, -150.0, s2, -4.0, sym2), (0, 150.0, s0, -4.0, sym0), (2, -150.0, s2, 4.0, sym2),
           (0, 0.0, s0, 0.0, sym0), (2, 0.0, 0, 0.0, sym2)]
    it += [(0, f0, s0, 0.0, all0), (2, f2, s2, 0.0, all3), (0, f0, s0, 1.0, all3)]
    it += [(1, 0.0, 0, 0.0, all0), (3, f0, s0, 0.0, sym0), (4, f0, s0, 0.0, sym0), (3, f0, 0, 0.0, all3), (4, f0, -300, 2.0, sym0)]
    it += [(2, np.float32(float(f2) - 0.03), s2, 0.0, sym2), (0, f0, s0 + 1, 0.0, sym0), (0, f0, -(1 << 30), 0.0, sym0),
           (0, f0, (1 << 31) - 1, 0.0, sym0)]
    rng = np.random.default_rng(n)
    while len(it) < count:
        seg = int(rng.choice([0, 0, 2, 2, 1, 3, 4]))
        f, s, sy = (f2, s2, sym2) if seg == 2 else (f0, s0, sym0)
        it.append((seg, np.float32(f + rng.choice([0.0, 0.0, 0.01, -0.2])), int(s + rng.integers(-3, 4)),
                   float(rng.choice([0.0, 0.0, 1.0, -3.0])), sy))
    items = np.zeros(count, mod.SPREAD_ITEM_DTYPE)
    for k, (seg, f, sh, dr, sy) in enumerate(it[:count]):
        items[k]["seg"], items[k]["f0"], items[k]["shift"], items[k]["drift"] = seg, f, sh, dr
        items[k]["symbols"] = sy
    want = np.stack([sl.check_words(I[x["seg"]], Q[x["seg"]], x["f0"], x["shift"], x["drift"], x["symbols"], np_=n)
                     for x in items])
    return I, Q, items, want


def _assert_equal(got, items, want, what):
    words = sl.record_words(got)
    bad = np.argwhere((words != want).any(axis=1))
    assert bad.size == 0, (what, bad[:5].ravel().tolist(), items[bad[0][0]], words[bad[0][0]], want[bad[0][0]])
    for k in ("f0", "shift", "drift"):                                          # the echo of the job
        assert got[k].tobytes() == items[k].tobytes(), (what, k)
    assert not got["pad"].any()


@pytest.mark.parametrize("n", [45000, 44993, 30000])
def test_kernel_equals_the_checker(w, stage_off, n):
    I, Q, items, want = _scene(n)
    valid = want[:, 3]
    seg = items["seg"]
    print("n", n, "valid jobs", int(valid.sum()), "of", valid.size)
    (f0, s0, sym0) = _rows(n)[2]
    true = (seg == 0) & (np.abs(items["f0"] - f0) < 0.5) & (np.abs(items["shift"].astype(np.int64) - s0) <= 3) & \
           (items["symbols"] == sym0).all(axis=1)
    assert true.sum() > 20 and valid[true].all()                                 # the signal with its own parameters
    assert not valid[np.isin(seg, (1, 3, 4))].any()                            # zero, NaN and Inf rows
    assert not valid[items["shift"] == n + 10].any() and not valid[np.abs(items["shift"].astype(np.int64)) > (1 << 29)].any()
    assert not want[valid == 0].any()                                          # valid = 0: the three floats are zero too
    for cnt in (1, 3, 65, 300):
        _assert_equal(w.spread_batch(I, Q, items[:cnt]), items[:cnt], want[:cnt], (n, cnt))
    # the jobs elsewhere in the batch do not matter: the last ones alone, and one row of the batch alone
    _assert_equal(w.spread_batch(I, Q, items[-9:]), items[-9:], want[-9:], (n, "tail"))
    only0 = items[seg == 0][:20]
    _assert_equal(w.spread_batch(I[:1], Q[:1], only0), only0, want[seg == 0][:20], (n, "row 0"))


def test_arithmetic_mode_does_not_matter(w, stage_off):
    I, Q, items, want = _scene(44993)
    for mode in (0, 1):
        w.wspr_set_arithmetic(mode)
        _assert_equal(w.spread_batch(I, Q, items[:65]), items[:65], want[:65], ("arith", mode))
    assert w.wspr_set_arithmetic(0) == 1


def test_entry_point_arguments(w):
    L = w.lib()
    I, Q, items, want = _scene(45000)
    out = np.full(2 * 8, 0xA5A5A5A5, np.uint32)

    def one(**kw):
        it = items[1:2].copy()
        for k, v in kw.items():
            if k == "symbol":
                it[0]["symbols"][v[0]] = v[1]
            else:
                it[0][k] = v
        return it

    def call(it, n=1, nseg=5, samples=NS, I=I, Q=Q):
        return L.wspr_spread_batch(orc.ptr(I), orc.ptr(Q), nseg, samples, NS, orc.ptr(it), n, orc.ptr(out))

    assert call(one(), n=0) == 0                                               # n == 0: nothing happens
    assert call(one(), n=-1) == -1
    assert call(one(seg=5)) == -1 and call(one(seg=-1)) == -1 and call(one(seg=1), nseg=1) == -1
    assert call(one(f0=np.nan)) == -1 and call(one(f0=np.inf)) == -1
    assert call(one(drift=np.nan)) == -1 and call(one(drift=-np.inf)) == -1
    assert call(one(symbol=(0, 4))) == -1 and call(one(symbol=(161, 255))) == -1
    assert call(one(f0=999.0, drift=4.0)) == -1 and call(one(f0=-1000.5)) == -1
    assert call(one(), samples=45001) == -1 and call(one(), samples=-1) == -1
    two = np.concatenate([one(), one(seg=7)])
    assert call(two, n=2) == -1                                                # one bad job refuses the whole call
    assert (out == 0xA5A5A5A5).all()                                           # ... and nothing was written by any of these
    assert call(one(f0=998.0, drift=4.0)) == 0                                 # the limit itself is inside
    assert call(one()) == 0
    assert out[:4].tolist() == want[1].tolist() and (out[8:] == 0xA5A5A5A5).all()
    # samples = 0: every frame misses the row
    assert call(one(), samples=0) == 0 and out[:4].tolist() == [0, 0, 0, 0]


# ---- the stage inside the decode loop ------------------------------------------------------------------------------------
def _decode(w, I, Q, options, max_results):
    """wspr_decode_batch() keeping the raw arrays: (bytes of the spot records per segment, spots per segment, n_results)."""
    nseg, samples = I.shape
    out = (w.decoder_results * (nseg * max_results))()
    nres = (C.c_int * nseg)()
    rc = w.lib().wspr_decode_batch(orc.ptr(I), orc.ptr(Q), nseg, samples, samples, options, C.addressof(out), max_results,
                                   C.addressof(nres), 0)
    assert rc == 0
    spots = [[out[s * max_results + i] for i in range(nres[s])] for s in range(nseg)]
    raw = [bytes(memoryview(out).cast("B")[(s * max_results) * 80:(s * max_results + nres[s]) * 80]) for s in range(nseg)]
    return raw, spots, list(nres)


def _check_records(w, I, Q, spots, rec, options):
    """Every spot's record: valid, tied to its spot (frequency, time, drift), and the checker's words on the ORIGINAL row
    with the record's own (f0, shift, drift) and the symbols of the spot's message."""
    total = 0
    for s, seg_spots in enumerate(spots):
        for i, sp in enumerate(seg_spots):
            r = rec[s, i]
            assert r["valid"] == 1, (s, i, r)
            assert abs((sp.freq - options.freq / 1e6) * 1e6 - 1500.0 - float(r["f0"])) < 1e-3
            assert abs(sp.dt - (int(r["shift"]) / 375.0 - 2.0)) < 1e-6 and sp.drift == r["drift"]
            ok, sym = w.get_wspr_channel_symbols(sp.message.decode())
            assert ok
            want = sl.check_words(I[s], Q[s], r["f0"], r["shift"], r["drift"], sym)
            assert sl.record_words(r).tolist() == want.tolist(), (s, i, sp.message, sl.unpack_words(want), r)
            total += 1
        assert not rec[s, len(seg_spots):].view(np.uint8).any()                # entries beyond n_results[s] are zero
    return total


@functools.lru_cache(maxsize=None)
def _single_signal_batch():
    segs = [synth.make_segment(9100 + k, symbols_of, snr_db=-15.0) for k in range(8)]
    return np.stack([s[0] for s in segs]), np.stack([s[1] for s in segs])


def test_decoder_with_the_stage_on(w, stage_off):
    """Default options (subtraction on, two passes): same spots, one valid record per spot, taken BEFORE the subtraction."""
    I, Q = _single_signal_batch()
    opt = w.default_options()
    off_raw, off_spots, _ = _decode(w, I, Q, opt, 8)
    assert w.last_spreads(8, 8) is None                                        # the stage was off for that call
    t = w.last_timings()
    assert t["spread_ms"] == 0 and t["spread_jobs"] == 0 and t["subtractions"] >= 8
    assert w.set_spread_estimate(1) == 0
    on_raw, spots, nres = _decode(w, I, Q, opt, 8)
    assert on_raw == off_raw and all(n >= 1 for n in nres)
    rec = w.last_spreads(8, 8)
    assert rec is not None
    t = w.last_timings()
    nspots = _check_records(w, I, Q, spots, rec, opt)
    print("spots", nspots, "spread_ms", t["spread_ms"], "subtract_ms", t["subtract_ms"], "w50", rec["w50"][:, 0].tolist())
    assert t["spread_jobs"] == nspots and t["spread_ms"] > 0
    assert w.lib().wspr_last_spreads(orc.ptr(rec), 8 * 8 - 1) == -1             # capacity too small
    # the single-segment entry point: entry i, *n_results of them
    one, _, _ = w.wspr_decode(I[0], Q[0])
    buf = np.zeros(100, w.SPREAD_DTYPE)
    assert w.lib().wspr_last_spreads(orc.ptr(buf), 100) == len(one) >= 1
    assert buf[:len(one)].tobytes() == rec[0, :len(one)].tobytes()


@functools.lru_cache(maxsize=None)
def _three_signal_batch():
    segs = [synth.make_segment(9200 + k, symbols_of, n_signals=3, snr_db=-8.0, snr_span=8.0) for k in range(4)]
    return np.stack([s[0] for s in segs]), np.stack([s[1] for s in segs])


def test_records_follow_the_spots_through_sort_and_cut(w, stage_off):
    I, Q = _three_signal_batch()
    opt = w.default_options(npasses=1, subtraction=0)
    off_raw, _, _ = _decode(w, I, Q, opt, 5)
    w.set_spread_estimate(1)
    raw, spots, nres = _decode(w, I, Q, opt, 5)
    assert raw == off_raw and nres == [3, 3, 3, 3]
    rec = w.last_spreads(4, 5)
    assert _check_records(w, I, Q, spots, rec, opt) == 12 and w.last_timings()["spread_jobs"] == 12
    for seg_spots in spots:                                                    # strongest first, as without the stage
        assert [sp.snr for sp in seg_spots] == sorted((sp.snr for sp in seg_spots), reverse=True)
    raw2, spots2, nres2 = _decode(w, I, Q, opt, 2)
    assert nres2 == [2, 2, 2, 2] and all(a == b[:160] for a, b in zip(raw2, raw))
    rec2 = w.last_spreads(4, 2)
    assert _check_records(w, I, Q, spots2, rec2, opt) == 8
    assert rec2.tobytes() == rec[:, :2].tobytes()
    assert w.last_timings()["spread_jobs"] == 12                               # every spot was measured, two per segment kept
    assert w.last_spreads(4, 5) is None                                        # the layout is the last call's


def test_switch(w, stage_off):
    assert w.set_spread_estimate(0) == 0
    assert w.set_spread_estimate(2) == -2 and w.set_spread_estimate(-1) == -2
    assert w.set_spread_estimate(0) == 0                                       # ... and changed nothing
    I, Q = _single_signal_batch()
    _decode(w, I[:2], Q[:2], w.default_options(), 4)
    assert w.last_spreads(2, 4) is None
    buf = np.zeros(8, w.SPREAD_DTYPE)
    assert w.lib().wspr_last_spreads(orc.ptr(buf), 8) == -1 and not buf.view(np.uint8).any()
    t = w.last_timings()
    assert t["spread_ms"] == 0 and t["spread_jobs"] == 0
    assert w.set_spread_estimate(1) == 0 and w.set_spread_estimate(0) == 1
