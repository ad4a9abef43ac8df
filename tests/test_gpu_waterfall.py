"""The waterfall (K20) through the C ABI: every image and every info record byte for byte the serial checker's
(tests/helpers/waterfall_check.c) -- lengths, batch sizes, hops, averaging, column ranges that start tiles on every byte
alignment, both reference modes, strides with garbage behind the rows and sentinels behind the images, huge, denormal and
non-finite samples -- floor mode against the noise figures' call, the refusals, the one-row call, two lanes, and end to end
on a scene of the synthesiser."""
import functools
import threading

import numpy as np
import pytest

import noise_lib as nl
import scenes
import waterfall_lib as wl

pytestmark = pytest.mark.gpu

NS = wl.NS
SENTINEL = 0xa5
INFO_SENTINEL = -7


@pytest.fixture(scope="module")
def env():
    import torch
    import rtlsdr_wsprd_amd as w
    assert w.lib().wspr_device_ready() == 1
    torch.cuda.set_device(0)
    assert w.WATERFALL_INFO_DTYPE == wl.INFO_DTYPE and w.WATERFALL_PARAMS_DTYPE == wl.PARAMS_DTYPE
    return torch, w, torch.device("cuda", 0), int(w.lib().wspr_iq_stride())


@functools.lru_cache(maxsize=None)
def _many_rows():
    """(I, Q) [65, 45000]: noise of a level of its own per row (three decades) and a tone of its own; read-only."""
    rng = np.random.default_rng(2020)
    t = np.arange(NS) / 375.0
    level = 10.0 ** rng.uniform(-3, 0, 65)
    z = level[:, None] * (rng.normal(0, 1, (65, NS)) + 1j * rng.normal(0, 1, (65, NS)))
    z += (30.0 * level[:, None]) * np.exp(2j * np.pi * rng.uniform(-150, 150, 65)[:, None] * t[None, :])
    I, Q = z.real.astype(np.float32), z.imag.astype(np.float32)
    I.setflags(write=False)
    Q.setflags(write=False)
    return I, Q


def _garbage(shape, seed):
    """What lies behind a row: NaN, infinities and huge finite values."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38, -1e30, 1.0], np.float32), shape).astype(np.float32)


def _host_rows(I, Q, n, pad):
    """Rows [nseg, >= n] in buffers of stride roundup4(n) + pad whose columns from n on are garbage."""
    nseg = I.shape[0]
    keep = max(0, min(n, I.shape[1]))
    stride = ((max(n, 0) + 3) & ~3) + pad
    hi, hq = _garbage((nseg, stride), 5), _garbage((nseg, stride), 6)
    hi[:, :keep], hq[:, :keep] = I[:, :keep], Q[:, :keep]
    return hi, hq, stride


def _device_waterfall(env, I, Q, n, p=None, pad=8, ipad=32, nseg=None, offset=0, stride=None, img_offset=0, img_stride=None,
                      shape_n=None):
    """wspr_waterfall_batch_device() on rows [rows, >= n] with garbage behind n; images in a buffer of stride
    roundup16(nrows * ncols) + ipad filled with the sentinel, info pre-filled with its sentinel.
    Returns (rc, image buffer uint8 [rows, img stride], info, (nrows, ncols))."""
    torch, w, dev, _ = env
    hi, hq, st = _host_rows(np.atleast_2d(I), np.atleast_2d(Q), n, pad)
    dI, dQ = torch.from_numpy(hi).to(dev), torch.from_numpy(hq).to(dev)
    rows = hi.shape[0]
    try:
        nrows, ncols = wl.shape_formula(max(0, min(n if shape_n is None else shape_n, NS)), p)
    except Exception:
        nrows, ncols = 348, 512
    if ncols < 1 or nrows < 0:
        nrows, ncols = 348, 512
    ist = ((nrows * ncols + 15) & ~15) + ipad
    d_img = torch.full((rows, ist), SENTINEL, dtype=torch.uint8, device=dev)
    info = np.zeros(rows, wl.INFO_DTYPE)
    info.view(np.int32)[:] = INFO_SENTINEL
    w.sync_torch()
    rc, info = w.waterfall_batch_device(dI.data_ptr() + offset, dQ.data_ptr() + offset, rows if nseg is None else nseg, n,
                                        st if stride is None else stride, d_img.data_ptr() + img_offset,
                                        ist if img_stride is None else img_stride, None if p is None else p[0], info)
    torch.cuda.synchronize()
    return rc, d_img.cpu().numpy(), info, (nrows, ncols)


def _equal(got_buf, got_info, shape, want_img, want_info):
    """The images' bytes, the sentinel behind them and the records."""
    nrows, ncols = shape
    nseg = want_img.shape[0]
    used = nrows * ncols
    assert got_info.tobytes() == want_info.tobytes(), (got_info[:3], want_info[:3])
    got = got_buf[:nseg, :used].reshape(nseg, nrows, ncols)
    if not np.array_equal(got, want_img):
        s, r, c = (int(x[0]) for x in np.nonzero(got != want_img))
        raise AssertionError("%d pixels differ; the first: image %d row %d column %d: %d, the checker %d" %
                             (np.count_nonzero(got != want_img), s, r, c, got[s, r, c], want_img[s, r, c]))
    assert np.all(got_buf[:nseg, used:] == SENTINEL)                         # everything behind the image is left alone


@functools.lru_cache(maxsize=None)
def _want(n, hop, tavg, cols, mode, nseg=3):
    """The checker on the first nseg of the 65 rows, once per case."""
    I, Q = _many_rows()
    p = wl.params(hop=hop, tavg=tavg, j0=cols[0], j1=cols[1], ref_mode=mode, ref=1e-3)
    k = max(n, 1)
    img, info = wl.check_rows(I[:nseg, :k], Q[:nseg, :k], n, p)
    return p, img, info


@pytest.mark.parametrize("hop", wl.HOPS)
@pytest.mark.parametrize("tavg", wl.TAVGS)
def test_images_and_records_equal_the_checker(env, hop, tavg):
    """Every length of the issue with 3 rows, every column range and both modes; the full row also with 1 row, and 65 rows of
    5 003 samples (65 full rows are test_65_full_rows()).  NOT the full product: of the twelve (columns, mode) combinations a full row
    meets three per (hop, tavg) case -- over the eight cases every combination meets a full row once, not with every hop and
    tavg -- to keep a case within seconds; the short lengths run all twelve.  A tile of the kernel is
    max(1, 16 / tavg) image rows: 348, 174, 116, 87 and 58 rows are no multiples of 16, 8 or 5."""
    I, Q = _many_rows()
    combos = [(cols, mode) for cols in wl.COLUMNS for mode in (wl.REF_FLOOR, wl.REF_ABSOLUTE)]
    turn = wl.TAVGS.index(tavg) * 2 + wl.HOPS.index(hop)
    for n in wl.lengths(hop, tavg):
        full = n >= 44999
        for k, (cols, mode) in enumerate(combos):
            if full and (k + turn) % 4:                                      # the full rows: three of the twelve combinations per case
                continue
            p, img, info = _want(n, hop, tavg, cols, mode)
            rc, buf, got, shape = _device_waterfall(env, I[:3], Q[:3], n, p, pad=0 if (k & 1 and n) else 8, ipad=16 + 16 * (k % 3))
            assert rc == 0
            _equal(buf, got, shape, img[:3], info[:3])
            if n < 512:
                assert shape[0] == 0 and np.all(got["nrows"] == 0) and np.all(got["flags"] == (wl.NO_REF if mode == wl.REF_FLOOR else 0))
    wide = (wl.COLUMNS[4 + turn % 2], (wl.REF_FLOOR, wl.REF_ABSOLUTE)[(turn // 2) % 2])    # 301 or 300 columns
    for nseg, n, (cols, mode) in ((1, NS, combos[turn % 12]), (65, 5003, wide)):
        p, img, info = _want(n, hop, tavg, cols, mode, nseg)
        rc, buf, got, shape = _device_waterfall(env, I[:nseg], Q[:nseg], n, p)
        assert rc == 0 and shape[0] == ((348 if hop == 128 else 174) if n == NS else (n - 512) // hop + 1) // tavg
        _equal(buf, got, shape, img[:nseg], info[:nseg])
        assert np.all(got["flags"] == wl.WRITTEN) and np.all(got["ref"] > 0)


def test_65_full_rows(env):
    I, Q = _many_rows()
    p, img, info = _want(NS, 128, 1, (-150, 150), wl.REF_FLOOR, 65)
    rc, buf, got, shape = _device_waterfall(env, I, Q, NS, p)
    assert rc == 0 and shape == (348, 301)
    _equal(buf, got, shape, img, info)
    assert np.all(got["flags"] == wl.WRITTEN) and len(set(got["ref"].tolist())) == 65


def test_default_parameters_are_null(env):
    I, Q = _many_rows()
    rc, buf, got, shape = _device_waterfall(env, I[:2], Q[:2], NS, None)
    img, info = wl.check_rows(I[:2], Q[:2], NS, None)
    assert rc == 0 and shape == (348, 301)
    _equal(buf, got, shape, img, info)
    p = wl.params()
    rc, buf2, got2, _ = _device_waterfall(env, I[:2], Q[:2], NS, p)
    assert rc == 0 and np.array_equal(buf, buf2) and got.tobytes() == got2.tobytes()


def _special_rows(hop, tavg):
    """Twelve rows: 0 of 1e30 (every power overflows), 1 of denormals (every power underflows), 2 .. 8 with one non-finite
    sample -- at the first and at the last sample of tile 3 of the kernel, just before and just behind that tile, at sample 0,
    at the last sample a complete row uses and behind it (no complete row uses that one) -- 9 clean, 10 with a stretch of
    garbage, 11 clean.  Returns (I, Q, places)."""
    I, Q = (x[:12].copy() for x in _many_rows())
    R = max(1, 16 // tavg)
    nrows = wl.frames_of(NS, hop) // tavg
    tile = 3
    first = hop * (tile * R * tavg)
    last = hop * ((tile + 1) * R * tavg - 1) + 511
    used = hop * (nrows * tavg - 1) + 512
    assert 0 < first and last + 1 < used < NS
    I[0] *= np.float32(1e30) / np.abs(I[0]).max()
    Q[0] *= np.float32(1e30) / np.abs(Q[0]).max()
    I[1] = (I[1] * np.float32(1e-38)) * np.float32(1e-3)
    Q[1] = (Q[1] * np.float32(1e-38)) * np.float32(1e-3)
    I[2, first] = np.inf
    Q[3, last] = np.nan
    I[4, first - 1] = -np.inf
    Q[5, last + 1] = np.inf
    I[6, 0] = np.nan
    Q[7, used - 1] = -np.inf
    I[8, used] = np.nan
    Q[10, 20000:20700] = np.nan
    return I, Q, dict(R=R, nrows=nrows, tile=tile, first=first, last=last, used=used)


def _special_claims(mode, hop, tavg, img, info, at):
    """What the definition says about the rows of _special_rows(), on images [12, nrows, ncols] and their records."""
    nrows, R, tile = at["nrows"], at["R"], at["tile"]
    if mode == wl.REF_ABSOLUTE:
        nonfinite = [bool(f & wl.NONFINITE) for f in info["flags"]]
        assert nonfinite == [False, False, True, True, True, True, True, True, False, False, True, False]
        white = [np.nonzero(np.all(img[s] == 255, axis=1))[0].tolist() for s in range(12)]
        assert white[2] == wl.rows_touching(at["first"], at["first"], hop, tavg, nrows) and white[2][-1] == tile * R
        assert white[3] == wl.rows_touching(at["last"], at["last"], hop, tavg, nrows) and white[3][0] == (tile + 1) * R - 1
        assert white[4][-1] == tile * R - 1 and white[5][0] == (tile + 1) * R and white[6][0] == 0
        assert white[7] == [nrows - 1] and white[8] == [] and white[9] == [] and white[11] == []
        assert white[10] == wl.rows_touching(20000, 20699, hop, tavg, nrows)
        assert np.all(img[0] == 255) and not img[1].any()                    # +Inf over a finite reference; 0 below every threshold
    else:
        assert [int(f) for f in info["flags"][2:9]] == [wl.WRITTEN | wl.NO_REF | wl.NONFINITE] * 7
        assert not img[2:9].any() and not info["ref"][2:9].any()


@pytest.mark.parametrize("hop,tavg", [(128, 1), (256, 1), (128, 3), (256, 16)])
def test_huge_denormal_and_non_finite_samples(env, hop, tavg):
    I, Q, at = _special_rows(hop, tavg)
    for mode in (wl.REF_ABSOLUTE, wl.REF_FLOOR):
        p = wl.params(hop=hop, tavg=tavg, ref_mode=mode, ref=1e-3, j0=-149, j1=150)
        want_img, want_info = wl.check_rows(I, Q, NS, p)
        rc, buf, got, shape = _device_waterfall(env, I, Q, NS, p)
        assert rc == 0
        _equal(buf, got, shape, want_img, want_info)
        _special_claims(mode, hop, tavg, buf[:, :shape[0] * shape[1]].reshape(12, shape[0], shape[1]), got, at)


def test_floor_mode_is_the_noise_call_and_touches_nothing(env):
    torch, w, dev, stride = env
    I, Q = _many_rows()
    nseg = 5
    dI = torch.zeros((nseg, stride), dtype=torch.float32, device=dev)
    dQ = torch.zeros((nseg, stride), dtype=torch.float32, device=dev)
    dI[:, :NS], dQ[:, :NS] = torch.from_numpy(I[:nseg].copy()).to(dev), torch.from_numpy(Q[:nseg].copy()).to(dev)
    scene_i, scene_q = scenes.make_scene(15)
    dI[0, :NS], dQ[0, :NS] = torch.from_numpy(scene_i).to(dev), torch.from_numpy(scene_q).to(dev)
    before_i, before_q = dI.cpu().numpy().copy(), dQ.cpu().numpy().copy()
    dec = w.BatchDecoder(1)

    def spots():
        w.sync_torch()
        dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)
        return [scenes.spot_record(s) for s in dec.spots(0)]
    spots_before = spots()
    for n in (NS, 44999, 1000):
        w.sync_torch()
        rc, k16_before = w.noise_batch_device(dI.data_ptr(), dQ.data_ptr(), nseg, n, stride)
        assert rc == 0
        nrows, ncols = w.waterfall_shape(n)
        ist = (nrows * ncols + 15) & ~15
        d_img = torch.zeros((nseg, ist), dtype=torch.uint8, device=dev)
        w.sync_torch()
        rc, info = w.waterfall_batch_device(dI.data_ptr(), dQ.data_ptr(), nseg, n, stride, d_img.data_ptr(), ist)
        assert rc == 0 and info["ref"].tobytes() == k16_before["fft_p30"].tobytes() and np.all(info["flags"] == wl.WRITTEN)
        rc, k16_after = w.noise_batch_device(dI.data_ptr(), dQ.data_ptr(), nseg, n, stride)
        assert rc == 0 and k16_after.tobytes() == k16_before.tobytes()
        assert k16_before.tobytes() == nl.check_rows(before_i[:, :n], before_q[:, :n], n).tobytes()
    spots_after = spots()
    assert spots_before and spots_after == spots_before
    assert np.array_equal(dI.cpu().numpy().view(np.uint32), before_i.view(np.uint32))       # the rows are only read
    assert np.array_equal(dQ.cpu().numpy().view(np.uint32), before_q.view(np.uint32))


def test_refusals_write_nothing(env):
    torch, w, dev, _ = env
    I, Q = (x[:2] for x in _many_rows())
    nan, inf = float("nan"), float("inf")

    def refused(code, n=1000, **kw):
        p = wl.params(**{k: kw.pop(k) for k in list(kw) if k in wl.DEFAULTS})
        rc, buf, info, _ = _device_waterfall(env, I, Q, n, p, **kw)
        assert rc == code, (rc, code, kw, p)
        assert np.all(buf == SENTINEL) and np.all(info.view(np.int32) == INFO_SENTINEL), (kw, p)
    refused(-1, nseg=-1)
    refused(-1, n=-1)
    refused(-2, n=45001)
    refused(-1, offset=4)                                                    # rows that are not 16-byte aligned
    refused(-1, stride=1002)                                                 # no multiple of 4 floats
    refused(-1, stride=996)                                                  # shorter than the row
    refused(-1, img_offset=8)                                                # images that are not 16-byte aligned
    refused(-1, img_stride=4 * 301 + 8)                                      # no multiple of 16 (1000 samples: 4 rows of 301)
    refused(-1, img_stride=1200)                                             # a multiple of 16 below 4 * 301
    for kw in (dict(hop=0), dict(hop=64), dict(hop=512), dict(tavg=0), dict(tavg=17), dict(j0=-257), dict(j1=256), dict(j0=9, j1=8),
               dict(ref_mode=2), dict(ref_mode=-1), dict(ref_mode=0, ref=0.0), dict(ref_mode=0, ref=-1.0), dict(ref_mode=0, ref=nan),
               dict(ref_mode=0, ref=inf), dict(db_min=nan), dict(db_min=-61.0), dict(db_min=61.0), dict(db_step=nan),
               dict(db_step=0.04), dict(db_step=4.1), dict(db_step=inf)):
        refused(-1, shape_n=0, **kw)
    refused(0, nseg=0)                                                       # does nothing
    # no info records: straight through the library (the wrapper would make some)
    p = wl.params()
    d_rows = torch.zeros((1, 1024), dtype=torch.float32, device=dev)
    d_img = torch.full((1, 2048), SENTINEL, dtype=torch.uint8, device=dev)
    w.sync_torch()
    assert w.lib().wspr_waterfall_batch_device(d_rows.data_ptr(), d_rows.data_ptr(), 1, 1000, 1024, p.ctypes.data, d_img.data_ptr(),
                                               2048, None) == -1
    torch.cuda.synchronize()
    assert np.all(d_img.cpu().numpy() == SENTINEL)
    with pytest.raises(RuntimeError):
        w.waterfall(I[0], Q[0], samples=45001)


def test_one_row_call_equals_row_0_of_the_batch(env):
    torch, w, dev, _ = env
    I, Q = _many_rows()
    cases = ((NS, None), (44999, wl.params(hop=256, tavg=3, j0=-149, j1=150, ref_mode=wl.REF_ABSOLUTE, ref=1e-3)),
             (767, wl.params(hop=128, tavg=2)), (640, wl.params(j0=0, j1=0)), (511, None), (0, None))
    for n, p in cases:
        rc, buf, info, shape = _device_waterfall(env, I[:2], Q[:2], n, p)
        img, one = w.waterfall(I[0, :n + 1], Q[0, :n + 1], None if p is None else p[0], samples=n)    # (one more sample than counts, unaligned)
        assert rc == 0 and img.shape == shape and one.tobytes() == info[0].tobytes(), (n, one, info[0])
        assert np.array_equal(img.reshape(-1), buf[0, :shape[0] * shape[1]])
        want_img, want_info = wl.check_rows(I[:1, :max(n, 1)], Q[:1, :max(n, 1)], n, p)
        assert np.array_equal(img, want_img[0]) and one.tobytes() == want_info[0].tobytes()


def test_two_lanes_give_the_same_bytes(env):
    torch, w, dev, _ = env
    I, Q = _many_rows()
    rc, here, here_info, shape = _device_waterfall(env, I[:5], Q[:5], NS)
    there = {}

    def other_lane():
        torch.cuda.set_device(0)
        there["lane"] = w.lib().wspr_bind_thread_lane(3)
        there["rc"], there["buf"], there["info"], _ = _device_waterfall(env, I[:5], Q[:5], NS)
    th = threading.Thread(target=other_lane)
    th.start()
    th.join()
    assert rc == 0 and there["rc"] == 0 and there["lane"] == 3
    assert np.array_equal(here, there["buf"]) and here_info.tobytes() == there["info"].tobytes()
    img, info = wl.check_rows(I[:5], Q[:5], NS)
    _equal(here, here_info, shape, img, info)


def test_end_to_end_a_transmission_shows_where_it_is(env):
    """One transmission of the synthesiser at f0 = +50 Hz, t0 = 2.0 s, +10 dB in 2 500 Hz over noise of sigma 0.02, default
    parameters: its four tones lie at 50 +- 2.2 Hz, bins 65.3 .. 71.3, from 2.0 s to 112.6 s.  Every image row that lies wholly
    inside 2.7 s .. 111.9 s has its brightest pixel in bins 64 .. 72."""
    import oracle_lib as ol
    import synth
    torch, w, dev, stride = env
    sigma = 0.02
    ok, sym = ol.channel_symbols(synth.message_for(20))
    assert ok
    amp = float(np.sqrt(2.0 * sigma * sigma * 2500.0 / 375.0 * 10.0))
    dI = torch.zeros((1, stride), dtype=torch.float32, device=dev)
    dQ = torch.zeros((1, stride), dtype=torch.float32, device=dev)
    w.sync_torch()
    assert w.wspr_synth_batch_device([(0, 50.0, 2.0, amp, 0.0, sym)], 1, dI.data_ptr(), dQ.data_ptr(), noise_sigma=sigma, seed=20) == 0
    nrows, ncols = w.waterfall_shape()
    ist = (nrows * ncols + 15) & ~15
    d_img = torch.zeros((1, ist), dtype=torch.uint8, device=dev)
    rc, info = w.waterfall_batch_device(dI.data_ptr(), dQ.data_ptr(), 1, NS, stride, d_img.data_ptr(), ist)
    torch.cuda.synchronize()
    assert rc == 0 and info[0]["flags"] == wl.WRITTEN and (info[0]["nframes"], info[0]["nrows"]) == (348, 348)
    img = d_img.cpu().numpy()[0, :nrows * ncols].reshape(nrows, ncols)
    hI, hQ = dI.cpu().numpy()[:, :NS], dQ.cpu().numpy()[:, :NS]
    want_img, want_info = wl.check_rows(hI, hQ, NS)
    assert np.array_equal(img, want_img[0]) and info.tobytes() == want_info.tobytes()
    inside = [r for r in range(nrows) if 128 * r >= 2.7 * 375 and 128 * r + 511 <= 111.9 * 375]
    assert len(inside) > 300
    brightest = np.argmax(img[inside], axis=1) - 150                         # column c is bin c - 150
    assert np.all((brightest >= 64) & (brightest <= 72)), brightest[(brightest < 64) | (brightest > 72)]
    assert abs(float(info[0]["ref"]) / (2 * sigma * sigma) - 0.957) < 0.06   # the floor: fft_p30 of white noise (K16's figure)
