"""The band noise figures (K16) through the C ABI: every record byte for byte the serial checker's
(tests/helpers/noise_check.c) -- lengths, batch sizes, strides with garbage behind the rows, non-finite samples, crafted
rows, windows -- the refusals, the one-row call, two lanes, and end to end on the synthesiser's noise: figures that follow
the noise level, what a crowded band does to them, and a decoder that does not notice the call."""
import functools
import threading

import numpy as np
import pytest

import noise_lib as nl
import scenes

pytestmark = pytest.mark.gpu

NS = nl.NS
SENTINEL = -7


@pytest.fixture(scope="module")
def env():
    import torch
    import rtlsdr_wsprd_amd as w
    assert w.lib().wspr_device_ready() == 1
    torch.cuda.set_device(0)
    assert w.NOISE_DTYPE == nl.NOISE_DTYPE and w.noise_default_windows() == nl.DEFAULT_WINDOWS
    return torch, w, torch.device("cuda", 0), int(w.lib().wspr_iq_stride())


@functools.lru_cache(maxsize=None)
def _many_rows():
    """(I, Q) [65, 45000]: noise of a level of its own per row and a tone of its own; read-only."""
    rng = np.random.default_rng(1616)
    t = np.arange(NS) / 375.0
    level = 10.0 ** rng.uniform(-3, 0, 65)
    z = level[:, None] * (rng.normal(0, 1, (65, NS)) + 1j * rng.normal(0, 1, (65, NS)))
    z += (3.0 * level[:, None]) * np.exp(2j * np.pi * rng.uniform(-150, 150, 65)[:, None] * t[None, :])
    I, Q = z.real.astype(np.float32), z.imag.astype(np.float32)
    I.setflags(write=False)
    Q.setflags(write=False)
    return I, Q


def _garbage(shape, seed):
    """What lies behind a row: NaN, infinities and huge finite values."""
    rng = np.random.default_rng(seed)
    g = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38, -1e30, 1.0], np.float32), shape)
    return g.astype(np.float32)


def _host_rows(I, Q, n, pad):
    """Rows [nseg, >= n] in buffers of stride roundup4(n) + pad whose columns from n on are garbage."""
    nseg = I.shape[0]
    keep = max(0, min(n, I.shape[1]))
    stride = ((max(n, 0) + 3) & ~3) + pad
    hi, hq = _garbage((nseg, stride), 5), _garbage((nseg, stride), 6)
    hi[:, :keep], hq[:, :keep] = I[:, :keep], Q[:, :keep]
    return hi, hq, stride


def _device_noise(env, I, Q, n, windows=None, pad=8, nseg=None, offset=0, stride=None, out=None):
    """wspr_noise_batch_device() on rows [rows, >= n] with garbage behind n; out pre-filled with the sentinel.
    Returns (rc, records, host rows as uploaded)."""
    torch, w, dev, _ = env
    hi, hq, st = _host_rows(np.atleast_2d(I), np.atleast_2d(Q), n, pad)
    dI, dQ = torch.from_numpy(hi).to(dev), torch.from_numpy(hq).to(dev)
    rows = hi.shape[0]
    if out is None:
        out = np.zeros(rows, nl.NOISE_DTYPE)
        out.view(np.int32)[:] = SENTINEL
    w.sync_torch()
    rc, out = w.noise_batch_device(dI.data_ptr() + offset, dQ.data_ptr() + offset, rows if nseg is None else nseg, n,
                                   st if stride is None else stride, windows, out)
    return rc, out, (hi, hq)


def _same(got, want):
    return got.tobytes() == want.tobytes()


def _diff(got, want):
    bad = [s for s in range(len(want)) if got[s].tobytes() != want[s].tobytes()]
    return [(s, got[s], want[s]) for s in bad[:3]]


@pytest.mark.parametrize("n", nl.LENGTHS)
def test_lengths_and_batch_sizes_equal_the_checker(env, n):
    I, Q = _many_rows()
    want = nl.check_rows(I[:, :n] if n else I[:, :1], Q[:, :n] if n else Q[:, :1], n)
    for nseg in (1, 3, 65):
        rc, got, _ = _device_noise(env, I[:nseg], Q[:nseg], n, pad=8 if nseg != 3 or n == 0 else 0)   # (rows must exist)
        assert rc == 0 and _same(got, want[:nseg]), _diff(got, want[:nseg])
    if n == 0:
        assert not got.view(np.int32).any()                                  # records of zeros, flags 0
    if n == NS:
        assert np.all(got["flags"] == 7) and np.all(got["nframes"] == 174) and np.all(got["fft_floor"] > 0)


def test_non_finite_rows_among_clean_rows(env):
    I, Q = (x[:7].copy() for x in _many_rows())
    n = 44999
    I[1, 0] = np.nan
    Q[3, n - 1] = -np.inf
    I[4, 20000] = np.inf
    Q[5, 511] = np.nan
    I[6, n] = np.nan                                                         # behind the row: does not count
    rc, got, _ = _device_noise(env, I, Q, n)
    want = nl.check_rows(I[:, :n], Q[:, :n], n)
    assert rc == 0 and _same(got, want), _diff(got, want)
    assert got["flags"].tolist() == [7, 8, 7, 8, 8, 8, 7] and np.all(got["nframes"] == 174)
    assert not got[[1, 3, 4, 5]].view(np.int32).reshape(4, 8)[:, :6].any()
    for short in (16, 512):                                                  # the first and the last sample of short rows
        J, K = I[:3, :short + 1].copy(), Q[:3, :short + 1].copy()
        J[0, 0], K[1, short - 1], J[2, short] = np.inf, np.nan, np.nan
        rc, got, _ = _device_noise(env, J, K, short)
        want = nl.check_rows(J[:, :short], K[:, :short], short)
        assert rc == 0 and _same(got, want) and got["flags"].tolist()[:2] == [8, 8] and not got["flags"][2] & 8


def test_crafted_rows(env):
    rows = nl.crafted_rows()
    I, Q = np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows])
    for n in (NS, 768, 767):
        rc, got, _ = _device_noise(env, I, Q, n)
        want = nl.check_rows(I[:, :n], Q[:, :n], n)
        assert rc == 0 and _same(got, want), _diff(got, want)
    assert got["flags"].tolist() == [7 & ~nl.POST_USED] * 4                  # 767 samples: the post window is clipped away


@pytest.mark.parametrize("case", [("null", None)] + nl.WINDOW_CASES, ids=["null"] + [c[0] for c in nl.WINDOW_CASES])
def test_windows(env, case):
    name, windows = case
    I, Q = nl.random_rows()
    for n in (NS, 511, 480):
        rc, got, _ = _device_noise(env, I, Q, n, windows)
        want = nl.check_rows(I[:, :n], Q[:, :n], n, windows)
        assert rc == 0 and _same(got, want), (n, _diff(got, want))
    if name == "null":
        assert _same(got, nl.check_rows(I[:, :480], Q[:, :480], 480, nl.DEFAULT_WINDOWS))


def test_refusals_write_nothing(env):
    torch, w, dev, _ = env
    I, Q = nl.random_rows()

    def refused(code, n=1000, **kw):
        rc, out, _ = _device_noise(env, I, Q, n, **kw)
        assert rc == code, (rc, code, kw)
        assert np.all(out.view(np.int32) == SENTINEL), kw
    refused(-1, nseg=-1)
    refused(-1, n=-1)
    refused(-1, offset=4)                                                    # rows that are not 16-byte aligned
    refused(-1, stride=1002)                                                 # no multiple of 4 floats
    refused(-1, stride=996)                                                  # shorter than the row
    for bad in ((-1, 5, 0, 0), (5, 4, 0, 0), (0, 2813, 0, 0), (0, 0, -1, 0), (0, 0, 9, 8), (0, 0, 0, 2813)):
        refused(-1, windows=bad)
    refused(-2, n=45001)
    refused(0, nseg=0)                                                       # does nothing
    out = np.zeros(1, nl.NOISE_DTYPE)
    out.view(np.int32)[:] = SENTINEL
    assert w.lib().wspr_noise(None, None, 45001, None, out.ctypes.data) == -2
    assert w.lib().wspr_noise(None, None, 8, None, out.ctypes.data) == -1
    assert np.all(out.view(np.int32) == SENTINEL)
    with pytest.raises(RuntimeError):
        w.noise(I[0], Q[0], windows=(0, 2813, 0, 0))


def test_one_row_call_equals_row_0_of_the_batch(env):
    torch, w, dev, _ = env
    I, Q = nl.random_rows()
    for n, windows in ((NS, None), (44999, (0, 2812, 100, 200)), (767, None), (0, None)):
        rc, batch, _ = _device_noise(env, I, Q, n, windows)
        one = w.noise(I[0, :n + 1], Q[0, :n + 1], windows, samples=n)          # (one more sample than counts, unaligned)
        assert rc == 0 and one.tobytes() == batch[0].tobytes(), (n, one, batch[0])
    assert float(w.to_db(np.float32(10.0))) == 10.0 and w.to_db(np.array([0.0, 1.0])).tolist() == [-np.inf, 0.0]


def test_two_lanes_give_the_same_bytes(env):
    torch, w, dev, _ = env
    I, Q = _many_rows()
    rc, here, _ = _device_noise(env, I[:5], Q[:5], NS)
    there = {}

    def other_lane():
        torch.cuda.set_device(0)
        there["lane"] = w.lib().wspr_bind_thread_lane(3)
        there["rc"], there["out"], _ = _device_noise(env, I[:5], Q[:5], NS)
    th = threading.Thread(target=other_lane)
    th.start()
    th.join()
    assert rc == 0 and there["rc"] == 0 and there["lane"] == 3
    assert _same(here, there["out"]) and _same(here, nl.check_rows(I[:5], Q[:5], NS))


def test_default_windows_stand_clear_of_an_on_time_transmission(env):
    """wspr_selftest() sends at t0 = 2.0 s and the decoder reports dt = 0 for it ("dt = t0 - 2.0"): in these rows a
    transmission on time starts at 2.0 s and ends at 112.6 s.  The default windows end before the one and start a second
    after the other -- wsprdaemon's windows, which assume a start at 1.0 s, moved by one second."""
    import ctypes as C
    torch, w, dev, _ = env
    first = w.decoder_results()
    assert w.lib().wspr_selftest(w.default_options(), C.addressof(first)) == 1
    assert abs(first.dt) < 0.05, first.dt
    pre0, pre1, post0, post1 = w.noise_default_windows()
    end = 2.0 + 162 * 256 / 375.0
    assert 0.25 <= 16 * pre0 / 375.0 and 16 * pre1 / 375.0 <= 2.0
    assert end + 1.0 <= 16 * post0 / 375.0 and 16 * post1 / 375.0 <= 120.0 and post1 <= w.NOISE_MAX_BLOCK


# ---- end to end on the synthesiser's noise ------------------------------------------------------------------------------
S_LO = 0.02
S_HI = float(np.float32(0.02 * np.sqrt(10.0)))
NROWS = 8


@pytest.fixture(scope="module")
def synth_rows(env):
    """Noise-only rows of the synthesiser at two levels 10 dB apart (different seeds), and the quieter ones with ten strong
    signals added: {name: (device I, device Q, records, host I, host Q)}."""
    torch, w, dev, stride = env
    made = {}
    for name, sigma, seed, crowd in (("lo", S_LO, 31, False), ("hi", S_HI, 32, False), ("crowded", S_LO, 31, True)):
        dI = torch.zeros((NROWS, stride), dtype=torch.float32, device=dev)
        dQ = torch.zeros((NROWS, stride), dtype=torch.float32, device=dev)
        w.sync_torch()
        assert w.wspr_synth_batch_device(nl.crowd_items(NROWS, sigma) if crowd else [], NROWS, dI.data_ptr(), dQ.data_ptr(),
                                         noise_sigma=sigma, seed=seed) == 0
        rc, rec = w.noise_batch_device(dI.data_ptr(), dQ.data_ptr(), NROWS, NS, stride)
        assert rc == 0
        made[name] = (dI, dQ, rec, dI.cpu().numpy(), dQ.cpu().numpy())
    return made


def test_figures_follow_the_noise_level(env, synth_rows):
    """Two levels 10 dB apart give all six figures 10 dB apart, within five standard deviations of the difference of two
    independent rows' figures: sqrt(2) times the relative scatter of one -- closed form for the means, the checker's
    measured scatter on white noise (noise_lib.white_noise_statistics()) for the troughs and the spectrum figures."""
    stats = nl.white_noise_statistics()
    lo, hi = synth_rows["lo"][2], synth_rows["hi"][2]
    for name, sigma in (("lo", S_LO), ("hi", S_HI)):
        _, _, rec, hI, hQ = synth_rows[name]
        want = nl.check_rows(hI[:, :NS], hQ[:, :NS], NS)
        assert _same(rec, want), _diff(rec, want)
        assert np.all(rec["flags"] == 7)
        ratio = {f: rec[f].astype(np.float64) / (2.0 * sigma * sigma) for f in nl.FIGURES}
        print("sigma %.5f: " % sigma + ", ".join("%s %.4f +- %.4f" % (f, ratio[f].mean(), ratio[f].std(ddof=1)) for f in nl.FIGURES))
    scatter = {f: stats[f][1] / stats[f][0] for f in nl.FIGURES}
    scatter["pre_mean"], scatter["post_mean"] = nl.mean_scatter(36), nl.mean_scatter(118)
    for f in nl.FIGURES:
        d_db = 10.0 * np.log10(hi[f].astype(np.float64) / lo[f].astype(np.float64)) - 10.0
        bound = 5.0 * np.sqrt(2.0) * scatter[f] * 10.0 / np.log(10.0)
        print("%-11s: hi / lo - 10 dB = %s (bound %.3f dB)" % (f, np.round(d_db, 3).tolist(), bound))
        assert np.all(np.abs(d_db) < bound), f


def test_a_crowded_band_moves_the_figures_by_a_measured_amount(env, synth_rows):
    """Ten strong signals (+0 .. +9 dB) on the quieter rows.  What they do to the figures is MEASURED and printed (README and
    DESIGN.md quote tools/noise_ab.py's run of the same scene); asserted: the records equal the checker's, are finite and
    fully flagged.  The clean rows' relation is test_figures_follow_the_noise_level().
    Measured on an MI355X (these eight rows; profiles/noise_figure.json has 64): fft_floor +0.48 dB (+0.45 .. +0.52), fft_p30
    +0.72 dB, post_mean and post_trough +0.00 dB, pre_trough +0.00 dB in the median and up to +3.36 dB, pre_mean +10.8 dB --
    the stations of the scene that start up to a second early fill the pre window."""
    _, _, rec, hI, hQ = synth_rows["crowded"]
    clean = synth_rows["lo"][2]
    want = nl.check_rows(hI[:, :NS], hQ[:, :NS], NS)
    assert _same(rec, want), _diff(rec, want)
    assert np.all(rec["flags"] == 7) and np.all(rec["nframes"] == 174)
    for f in nl.FIGURES:
        assert np.all(np.isfinite(rec[f])) and np.all(rec[f] > 0)
        shift = 10.0 * np.log10(rec[f].astype(np.float64) / clean[f].astype(np.float64))
        print("%-11s: crowded / clean = %+.2f dB (median; %+.2f .. %+.2f)" % (f, np.median(shift), shift.min(), shift.max()))


def test_the_decoder_does_not_notice_a_noise_call(env):
    torch, w, dev, stride = env
    I, Q = scenes.make_scene(15)
    dI = torch.zeros((1, stride), dtype=torch.float32, device=dev)
    dQ = torch.zeros((1, stride), dtype=torch.float32, device=dev)
    dI[0, :NS], dQ[0, :NS] = torch.from_numpy(I).to(dev), torch.from_numpy(Q).to(dev)
    dec = w.BatchDecoder(1)

    def spots():
        w.sync_torch()
        dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)
        return [scenes.spot_record(s) for s in dec.spots(0)]
    before = spots()
    rc, rec = w.noise_batch_device(dI.data_ptr(), dQ.data_ptr(), 1, NS, stride)
    one = w.noise(I, Q)
    assert rc == 0 and rec[0].tobytes() == one.tobytes() == nl.check_rows(I, Q, NS)[0].tobytes()
    after = spots()
    assert before and after == before
    assert np.array_equal(dI.cpu().numpy()[0, :NS].view(np.uint32), I.view(np.uint32))      # the rows are only read
