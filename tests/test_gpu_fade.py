"""The synthesiser's fading channel on the device (K13) through the C ABI: bit for bit the serial checker
(tests/helpers/fade_check.cpp) on a scene that takes every branch, split invariance, the identity channel, the host entry,
refusals that leave the rows alone, and one faded segment generated, decoded and measured without leaving the device."""
import ctypes as C
import functools

import numpy as np
import pytest

import fade_lib as fl
import oracle_lib as ol
import synth
import synth_lib as sl

pytestmark = pytest.mark.gpu

NS = 45000
SIGMA = float(np.float32(np.sqrt((375.0 / 2500.0) / 2.0)))
NSEG, SEG0, SEED = 3, 5, 20261019
NONE = (0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def env():
    import torch
    import rtlsdr_wsprd_amd as w
    assert w.lib().wspr_device_ready() == 1
    torch.cuda.set_device(0)
    return torch, w, torch.device("cuda", 0), int(w.lib().wspr_iq_stride())


def _sym(k):
    ok, sym = ol.channel_symbols(synth.message_for(40 + 7 * k))
    assert ok
    return sym


def _scene7():
    """Three segments, the middle one empty: the six transmissions the channel's branches ask for and a seventh, so that q
    reaches 3.  A frame at t0 = 2 s crosses every 4 096-sample tile edge of the row."""
    items = [(0, 50.0, 2.0, 0.5, 0.0, _sym(0)), (0, -80.0, 2.0, 0.3, 1.5, _sym(1)), (0, 130.5, 1.3, 0.7, 0.0, _sym(2)),
             (0, -140.0, 2.5, 0.2, 0.0, _sym(6)),
             (2, -20.0, -3.0, 1.0, 0.0, _sym(3)), (2, 75.25, 12.0, 0.4, -2.0, _sym(4)), (2, 0.0, 2.0, 0.6, 0.0, _sym(5))]
    channels = [[(1.0, 0.0, 0.2), (0.5, 0.5, 0.0)],          # Rayleigh plus a shifted specular path
                fl.IDENTITY,
                [(1.0, 0.0, 10.0), NONE],                    # L = 4: the LDS staging at its largest
                [(0.7, -0.25, 0.05), (0.7, 0.25, 0.05)],     # (the seventh)
                [(1.0, 0.0, 0.001), NONE],                   # the frame hangs off the start; L exceeds the frame
                [(0.8, 1.0, 0.3), (0.6, -1.0, 1.0)],         # off the end, two diffuse paths, shifted both ways
                [NONE, (1.0, 0.0, 0.5)]]                     # path 0 skipped
    return items, channels


@functools.lru_cache(maxsize=None)
def _fill():
    rng = np.random.default_rng(12)
    return rng.normal(0, 0.3, (NSEG, NS)).astype(np.float32), rng.normal(0, 0.3, (NSEG, NS)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(flags):
    """The checker's rows for the scene, computed once per flag combination and left unchanged."""
    items, channels = _scene7()
    fill = _fill() if flags & sl.ACCUMULATE else (None, None)
    rc, I, Q = fl.check_batch(items, channels, NSEG, SEG0, SIGMA, SEED, flags, *fill)
    assert rc == 0
    I.setflags(write=False)
    Q.setflags(write=False)
    return I, Q


def _device(env, items, channels, nseg, seg0=0, sigma=0.0, seed=0, flags=0, fill=None, faded=True):
    """wspr_synth_faded_batch_device() (or the unfaded call) on fresh device rows, pad columns 7.0 (filled from `fill` =
    (I, Q) host rows of 45000 where given): (rc, I, Q, pad columns of I and Q)."""
    torch, w, dev, stride = env
    hi = np.full((nseg, stride), 7.0, np.float32)
    hq = np.full((nseg, stride), 7.0, np.float32)
    if fill is not None:
        hi[:, :NS], hq[:, :NS] = fill
    dI = torch.from_numpy(hi).to(dev)
    dQ = torch.from_numpy(hq).to(dev)
    w.sync_torch()
    if faded:
        rc = w.wspr_synth_faded_batch_device(items, channels, nseg, dI.data_ptr(), dQ.data_ptr(), seg0, sigma, seed, flags)
    else:
        rc = w.wspr_synth_batch_device(items, nseg, dI.data_ptr(), dQ.data_ptr(), seg0, sigma, seed, flags)
    gi, gq = dI.cpu().numpy(), dQ.cpu().numpy()
    return rc, gi[:, :NS], gq[:, :NS], (gi[:, NS:], gq[:, NS:])


@pytest.mark.parametrize("flags", [0, sl.NORMALISE, sl.ACCUMULATE, sl.ACCUMULATE | sl.NORMALISE])
def test_every_float_equals_the_checker(env, flags):
    items, channels = _scene7()
    fill = _fill() if flags & sl.ACCUMULATE else None
    rc, I, Q, pad = _device(env, items, channels, NSEG, SEG0, SIGMA, SEED, flags, fill)
    ci, cq = _reference(flags)
    assert rc == 0
    d = [int((I[s].view(np.uint32) != ci[s].view(np.uint32)).sum() + (Q[s].view(np.uint32) != cq[s].view(np.uint32)).sum())
         for s in range(NSEG)]
    print("flags %d: differing floats per segment %s" % (flags, d))
    assert d == [0, 0, 0]
    if flags & sl.ACCUMULATE:
        assert (pad[0] == 7.0).all() and (pad[1] == 7.0).all()                  # columns from 45000 on are left alone
    else:
        assert not pad[0].any() and not pad[1].any()


def test_three_calls_of_one_segment_equal_one_call_of_three(env):
    items, channels = _scene7()
    ci, cq = _reference(0)
    for s in range(NSEG):
        keep = [k for k, it in enumerate(items) if it[0] == s]
        rc, I, Q, _ = _device(env, [(0,) + items[k][1:] for k in keep], [channels[k] for k in keep], 1, SEG0 + s, SIGMA, SEED)
        assert rc == 0 and I[0].tobytes() == ci[s].tobytes() and Q[0].tobytes() == cq[s].tobytes(), s


def test_identity_channel_and_no_channel_equal_the_unfaded_call(env):
    items, _ = _scene7()
    rc, I, Q, _ = _device(env, items, None, NSEG, SEG0, SIGMA, SEED, sl.NORMALISE, faded=False)
    rc1, I1, Q1, _ = _device(env, items, [fl.IDENTITY] * len(items), NSEG, SEG0, SIGMA, SEED, sl.NORMALISE)
    rc2, I2, Q2, _ = _device(env, items, None, NSEG, SEG0, SIGMA, SEED, sl.NORMALISE)
    assert rc == 0 and rc1 == 0 and rc2 == 0 and I[0].any()
    assert I1.tobytes() == I.tobytes() and Q1.tobytes() == Q.tobytes()
    assert I2.tobytes() == I.tobytes() and Q2.tobytes() == Q.tobytes()


def test_host_entry_is_row_zero_of_the_batch_entry(env):
    torch, w, dev, stride = env
    items, channels = _scene7()
    keep = [k for k, it in enumerate(items) if it[0] == 0]
    items, channels = [items[k] for k in keep], [channels[k] for k in keep]
    base = tuple(x[:1] for x in _fill())
    for flags in (0, sl.NORMALISE, sl.ACCUMULATE):
        fill = base if flags & sl.ACCUMULATE else None
        rc, I, Q, _ = _device(env, items, channels, 1, 0, SIGMA, 42, flags, fill)
        hi, hq = w.wspr_synth_faded(items, channels, SIGMA, 42, flags, *(tuple(x[0] for x in fill) if fill else (None, None)))
        assert rc == 0 and hi.tobytes() == I[0].tobytes() and hq.tobytes() == Q[0].tobytes()


def test_refused_calls_leave_the_rows_untouched(env):
    torch, w, dev, stride = env
    items, channels = _scene7()
    nan, inf = float("nan"), float("inf")
    ok = (1.0, 0.0, 0.0)
    bad_sym = items[0][5].copy()
    bad_sym[161] = 4

    def with_channel(k, ch):
        return items, channels[:k] + [ch] + channels[k + 1:]
    cases = [with_channel(0, [(nan, 0.0, 0.0), ok]), with_channel(6, [ok, (1.0, inf, 0.0)]), with_channel(2, [(1.0, 0.0, nan), ok]),
             with_channel(3, [(1.0, 0.0, 0.0005), ok]), with_channel(4, [ok, (1.0, 0.0, 10.5)]), with_channel(5, [(1.0, 0.0, -0.2), ok]),
             with_channel(1, [(1.0, 100.5, 0.0), ok]), with_channel(6, [ok, (0.0, -100.5, 0.2)]),
             ([items[0][:5] + (bad_sym,)] + items[1:], channels),                # and what the unfaded call refuses
             ([(3,) + items[-1][1:]], [channels[-1]]),
             (items[::-1], channels[::-1])]
    for its, chs in cases:
        rc, I, Q, pad = _device(env, its, chs, NSEG, SEG0, SIGMA, SEED)
        assert rc == -1, chs
        assert (I == 7.0).all() and (Q == 7.0).all() and (pad[0] == 7.0).all() and (pad[1] == 7.0).all(), chs
    for kw in (dict(sigma=nan), dict(flags=4)):
        rc, I, Q, pad = _device(env, items, channels, NSEG, SEG0, kw.get("sigma", SIGMA), SEED, kw.get("flags", 0))
        assert rc == -1 and (I == 7.0).all() and (Q == 7.0).all()
    L = w.lib()
    arr, chs = w.synth_tx_list(items), w.synth_channel_list(channels)
    dI = torch.full((NSEG, stride), 7.0, device=dev)
    dQ = torch.full((NSEG, stride), 7.0, device=dev)
    w.sync_torch()
    a, c = C.addressof(arr), C.addressof(chs)
    assert L.wspr_synth_faded_batch_device(a, c, -1, NSEG, 0, 0.0, 0, 0, dI.data_ptr(), dQ.data_ptr()) == -1
    assert L.wspr_synth_faded_batch_device(a, c, len(items), NSEG, 0, 0.0, 0, 0, dI.data_ptr() + 4, dQ.data_ptr()) == -1
    assert L.wspr_synth_faded_batch_device(a, c, len(items), NSEG, 0, 0.0, 0, 0, None, dQ.data_ptr()) == -1
    assert bool((dI == 7.0).all()) and bool((dQ == 7.0).all())
    hi = np.full(NS, 7.0, np.float32)
    hq = np.full(NS, 7.0, np.float32)
    one = w.synth_channel_list([[(1.0, 0.0, 11.0), ok]])
    assert L.wspr_synth_faded(a, C.addressof(one), 1, 0.0, 0, 0, ol.ptr(hi), ol.ptr(hq)) == -1
    assert (hi == 7.0).all() and (hq == 7.0).all()
    # and the library is in working order afterwards
    rc, I, Q, _ = _device(env, items, channels, NSEG, SEG0, SIGMA, SEED)
    assert rc == 0 and I.tobytes() == _reference(0)[0].tobytes()


def test_faded_segment_is_decoded_and_measured_on_the_device(env):
    """"K1JT FN20QI 20" at -10 dB in 2 500 Hz through one Rayleigh path of sigma = 0.1 Hz, seed 1, normalised: the CPU
    oracle decodes the checker's row (seed 1 was the first tried); the device's row is that row, decodes to the same
    message, its Doppler-spread record is valid, and its w50 is above that of the same scene through the identity channel."""
    torch, w, dev, stride = env
    ok, sym = ol.channel_symbols("K1JT FN20QI 20")
    assert ok
    item = (0, 50.0, 2.0, float(10.0 ** (-10.0 / 20.0)), 0.0, sym)
    faded = [[(1.0, 0.0, 0.1), NONE]]
    rc, ci, cq = fl.check_batch([item], faded, 1, 0, SIGMA, 1, sl.NORMALISE)
    ref, _, _ = ol.decode(ci[0], cq[0], NS)
    assert rc == 0 and [(s.call, s.loc, s.pwr) for s in ref] == [(b"K1JT", b"FN20", b"20")]
    dI = torch.zeros(1, stride, device=dev)
    dQ = torch.zeros(1, stride, device=dev)
    w.sync_torch()
    dec = w.BatchDecoder(1, 8)
    w50 = []
    prev = w.set_spread_estimate(1)
    try:
        for ch in (faded, [fl.IDENTITY]):
            assert w.wspr_synth_faded_batch_device([item], ch, 1, dI.data_ptr(), dQ.data_ptr(), 0, SIGMA, 1, sl.NORMALISE) == 0
            if ch is faded:
                assert dI.cpu().numpy()[0, :NS].tobytes() == ci[0].tobytes()
            dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)
            spots = dec.spots(0)
            assert [(s.call, s.loc, s.pwr) for s in spots] == [(b"K1JT", b"FN20", b"20")]
            rec = w.last_spreads(1, 8)
            assert rec is not None and rec["valid"][0, 0] == 1
            w50.append(float(rec["w50"][0, 0]))
    finally:
        w.set_spread_estimate(prev)
    print("w50 faded %.4f Hz, identity %.4f Hz" % tuple(w50))
    assert w50[0] > w50[1]
