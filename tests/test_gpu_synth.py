"""The device synthesiser (K8) through the C ABI: bit for bit the checker (tests/helpers/synth_check.cpp), the
reference's self-test with the generator on the device, residency (generated rows decoded without visiting the host),
and refused calls that leave the rows alone."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import synth
import synth_lib as sl

pytestmark = pytest.mark.gpu

NS = 45000
SIGMA = float(np.float32(np.sqrt((375.0 / 2500.0) / 2.0)))
REPORT_LINE = "Spot(0)  22.80   0.01 144.490550  0    K1JT   FN20 20"          # REPORT.md:198


@pytest.fixture(scope="module")
def env():
    import torch
    import rtlsdr_wsprd_amd as w
    assert w.lib().wspr_device_ready() == 1
    torch.cuda.set_device(0)
    return torch, w, torch.device("cuda", 0), int(w.lib().wspr_iq_stride())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _differing(a, b):
    return int((_bits(a) != _bits(b)).sum())


def _message(rng, seg):
    kind = int(rng.integers(0, 4))
    if kind == 0:
        return synth.station_message(int(rng.integers(0, 8)), 0)                # type 2
    if kind == 1:
        return synth.station_message(int(rng.integers(0, 8)), 1)                # type 3
    return synth.message_wide(int(rng.integers(0, 1 << 40)))                    # type 1


def _random_scene(rng, nseg, max_tx=10):
    """0 .. max_tx transmissions per segment, types 1-3, drift -4 .. 4, t0 -1 .. 3 s (frames leave both ends of the row;
    now and then far outside it), amplitudes over 40 dB."""
    items = []
    for seg in range(nseg):
        for _ in range(int(rng.integers(0, max_tx + 1))):
            ok, sym = ol.channel_symbols(_message(rng, seg))
            assert ok
            t0 = float(rng.uniform(-1, 3))
            if rng.integers(0, 12) == 0:
                t0 = float(rng.choice([-115.0, -109.9, 118.0, 125.0]))
            drift = 0.0 if rng.integers(0, 4) == 0 else float(rng.uniform(-4, 4))
            items.append((seg, float(rng.uniform(-160, 160)), t0, float(10 ** rng.uniform(-1.5, 0.5)), drift, sym))
    return items


def _device_batch(env, items, nseg, seg_index0=0, sigma=0.0, seed=0, flags=0, fill=None):
    """wspr_synth_batch_device() on fresh device rows (filled from `fill` = (I, Q) host rows of 45000, pad columns 7.0):
    returns (rc, I, Q, pad columns of I and Q)."""
    torch, w, dev, stride = env
    hi = np.full((nseg, stride), 7.0, np.float32)
    hq = np.full((nseg, stride), 7.0, np.float32)
    if fill is not None:
        hi[:, :NS], hq[:, :NS] = fill
    dI = torch.from_numpy(hi).to(dev)
    dQ = torch.from_numpy(hq).to(dev)
    w.sync_torch()
    rc = w.wspr_synth_batch_device(items, nseg, dI.data_ptr(), dQ.data_ptr(), seg_index0, sigma, seed, flags)
    gi, gq = dI.cpu().numpy(), dQ.cpu().numpy()
    return rc, gi[:, :NS], gq[:, :NS], (gi[:, NS:], gq[:, NS:])


def test_self_test_frame_equals_the_checker(env):
    item = sl.selftest_item()
    rc, I, Q, pad = _device_batch(env, [item], 1)
    _, ci, cq = sl.check_batch([item], 1)
    assert rc == 0 and _differing(I, ci) == 0 and _differing(Q, cq) == 0
    assert not pad[0].any() and not pad[1].any()                                 # the whole row is written
    rc, I, Q, _ = _device_batch(env, [item], 1, sigma=0.02, seed=1)
    _, ci, cq = sl.check_batch([item], 1, sigma=0.02, seed=1)
    assert rc == 0 and _differing(I, ci) == 0 and _differing(Q, cq) == 0


def test_random_scenes_equal_the_checker_bit_for_bit(env):
    """208 random segments in 8 calls: every flag combination, sigma = 0 and > 0, several seeds and batch origins."""
    rng = np.random.default_rng(20261016)
    total = 0
    for call in range(8):
        nseg = 26
        flags = call % 4
        sigma = 0.0 if call in (1, 6) else float(SIGMA * 10 ** rng.uniform(-1, 0.3))
        seed = int(rng.integers(0, 1 << 63)) * 2 + 1
        seg0 = int(rng.integers(0, 1 << 30))
        items = _random_scene(rng, nseg)
        fill = None
        if flags & sl.ACCUMULATE:
            fill = (rng.normal(0, 0.3, (nseg, NS)).astype(np.float32), rng.normal(0, 0.3, (nseg, NS)).astype(np.float32))
        rc, I, Q, pad = _device_batch(env, items, nseg, seg0, sigma, seed, flags, fill)
        crc, ci, cq = sl.check_batch(items, nseg, seg0, sigma, seed, flags, *(fill or (None, None)))
        assert rc == 0 and crc == 0
        d = _differing(I, ci) + _differing(Q, cq)
        print("call %d: %d transmissions, flags %d, sigma %.3f: %d differing samples" % (call, len(items), flags, sigma, d))
        assert d == 0
        if flags & sl.ACCUMULATE:
            assert (pad[0] == 7.0).all() and (pad[1] == 7.0).all()              # columns from 45000 on are left alone
        else:
            assert not pad[0].any() and not pad[1].any()
        total += nseg
    assert total >= 200


def test_host_entry_is_row_zero_of_the_batch_entry(env):
    torch, w, dev, stride = env
    rng = np.random.default_rng(3)
    items = _random_scene(rng, 1, 6) or [sl.selftest_item()]
    base = (rng.normal(0, 0.1, (1, NS)).astype(np.float32), rng.normal(0, 0.1, (1, NS)).astype(np.float32))
    for flags in (0, sl.NORMALISE, sl.ACCUMULATE):
        fill = base if flags & sl.ACCUMULATE else None
        rc, I, Q, _ = _device_batch(env, items, 1, 0, SIGMA, 42, flags, fill)
        hi, hq = w.wspr_synth(items, SIGMA, 42, flags, *(tuple(x[0] for x in fill) if fill else (None, None)))
        assert rc == 0 and hi.tobytes() == I[0].tobytes() and hq.tobytes() == Q[0].tobytes()


def test_split_batch_equals_one_call(env):
    rng = np.random.default_rng(8)
    items = _random_scene(rng, 12, 4)
    rc, I, Q, _ = _device_batch(env, items, 12, 700, SIGMA, 5, sl.NORMALISE)
    lo = [it for it in items if it[0] < 5]
    hi = [(it[0] - 5,) + it[1:] for it in items if it[0] >= 5]
    rc0, I0, Q0, _ = _device_batch(env, lo, 5, 700, SIGMA, 5, sl.NORMALISE)
    rc1, I1, Q1, _ = _device_batch(env, hi, 7, 705, SIGMA, 5, sl.NORMALISE)
    assert rc == 0 and rc0 == 0 and rc1 == 0
    assert np.concatenate([I0, I1]).tobytes() == I.tobytes() and np.concatenate([Q0, Q1]).tobytes() == Q.tobytes()


def test_reference_self_test_with_the_generator_on_the_device(env):
    """The reference's -t: its own noise (glibc rand(), through accumulate), the transmission added by the device, decoded
    by wspr_decode(): REPORT.md:198's line.  And wspr_selftest(), the same with the library's own noise."""
    torch, w, dev, stride = env
    ni, nq = sl.reference_noise()
    I, Q = w.wspr_synth([sl.selftest_item()], 0.0, 0, sl.ACCUMULATE, ni, nq)
    spots, _, _ = w.wspr_decode(I, Q, NS)
    s = spots[0]
    line = "Spot(%i) %6.2f %6.2f %10.6f %2d %7s %6s %2s" % (
        0, s.snr, s.dt, s.freq, int(s.drift), s.call.decode(), s.loc.decode(), s.pwr.decode())
    assert line == REPORT_LINE
    rc, first = w.wspr_selftest()
    assert rc == 1 and (first.call, first.loc, first.pwr) == (b"K1JT", b"FN20", b"20")
    assert w.lib().wspr_selftest(w.default_options(), None) == 1


def test_generated_rows_are_decoded_without_visiting_the_host(env):
    """256 ten-signal segments generated into HBM and decoded there; every spot field equals the oracle's decode of the
    checker's rows."""
    from concurrent.futures import ThreadPoolExecutor
    torch, w, dev, stride = env
    nseg = 256
    rng = np.random.default_rng(99)
    items = []
    for seg in range(nseg):
        for k, f0 in enumerate(np.linspace(-100, 100, 10) + rng.uniform(-2, 2, 10)):
            ok, sym = ol.channel_symbols(synth.message_wide(int(rng.integers(0, 1 << 40))))
            assert ok
            items.append((seg, float(f0), float(2.0 + rng.uniform(-1, 1)), float(10 ** (-(10 + 2 * k) / 20.0)), 0.0, sym))
    dI = torch.zeros(nseg, stride, device=dev)
    dQ = torch.zeros(nseg, stride, device=dev)
    w.sync_torch()
    assert w.wspr_synth_batch_device(items, nseg, dI.data_ptr(), dQ.data_ptr(), 0, SIGMA, 31337, sl.NORMALISE) == 0
    dec = w.BatchDecoder(nseg, 32)
    dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)
    rc, ci, cq = sl.check_batch(items, nseg, 0, SIGMA, 31337, sl.NORMALISE)
    assert rc == 0
    ref = [ol.decode(ci[0], cq[0], NS)[0]]                                       # (the oracle's tables are built by now)
    with ThreadPoolExecutor(8) as pool:
        ref += list(pool.map(lambda s: ol.decode(ci[s], cq[s], NS)[0], range(1, nseg)))

    def tup(x):
        return (x.message, x.call, x.loc, x.pwr, x.cycles, x.jitter, x.drift, x.sync, x.dt, x.freq)
    n_spots = 0
    for s in range(nseg):
        got = dec.spots(s)
        assert [tup(x) for x in got] == [tup(x) for x in ref[s]], s
        assert all(abs(a.snr - b.snr) < 1e-4 for a, b in zip(got, ref[s]))
        n_spots += len(got)
    print("residency: %d spots in %d segments" % (n_spots, nseg))
    assert n_spots > 5 * nseg


def test_refused_calls_leave_the_rows_untouched(env):
    torch, w, dev, stride = env
    good = sl.selftest_item()
    bad_sym = good[5].copy()
    bad_sym[161] = 4
    nan, inf = float("nan"), float("inf")
    cases = [
        dict(items=[good[:5] + (bad_sym,)]),                                   # a symbol > 3
        dict(items=[(2,) + good[1:]]),                                         # seg outside the batch
        dict(items=[(-1,) + good[1:]]),
        dict(items=[(1,) + good[1:], good]),                                   # unsorted
        dict(items=[(0, nan, 2.0, 1.0, 0.0, good[5])]),
        dict(items=[(0, 50.0, inf, 1.0, 0.0, good[5])]),
        dict(items=[(0, 50.0, 2.0, -inf, 0.0, good[5])]),
        dict(items=[(0, 50.0, 2.0, 1.0, nan, good[5])]),
        dict(items=[good], sigma=nan),
        dict(items=[good], sigma=inf),
        dict(items=[good], flags=4),
        dict(items=[(0, 1500.0, 2.0, 1.0, 0.0, good[5])]),                     # beyond the phase reduction's range
    ]
    for c in cases:
        rc, I, Q, pad = _device_batch(env, c["items"], 2, 0, c.get("sigma", 0.0), 1, c.get("flags", 0))
        assert rc == -1, c
        assert (I == 7.0).all() and (Q == 7.0).all() and (pad[0] == 7.0).all() and (pad[1] == 7.0).all(), c
    L = w.lib()
    arr = w.synth_tx_list([good])
    dI = torch.full((2, stride), 7.0, device=dev)
    dQ = torch.full((2, stride), 7.0, device=dev)
    w.sync_torch()
    assert L.wspr_synth_batch_device(C.addressof(arr), -1, 2, 0, 0.0, 0, 0, dI.data_ptr(), dQ.data_ptr()) == -1   # negative counts
    assert L.wspr_synth_batch_device(C.addressof(arr), 1, -2, 0, 0.0, 0, 0, dI.data_ptr(), dQ.data_ptr()) == -1
    assert L.wspr_synth_batch_device(C.addressof(arr), 1, 2, 0, 0.0, 0, 0, dI.data_ptr() + 4, dQ.data_ptr()) == -1    # misaligned
    assert bool((dI == 7.0).all()) and bool((dQ == 7.0).all())
    hi = np.full(NS, 7.0, np.float32)
    hq = np.full(NS, 7.0, np.float32)
    bad = w.synth_tx_list([good[:5] + (bad_sym,)])
    assert L.wspr_synth(C.addressof(bad), 1, 0.0, 0, 0, ol.ptr(hi), ol.ptr(hq)) == -1
    assert (hi == 7.0).all() and (hq == 7.0).all()
    # and the library is in working order afterwards
    rc, I, Q, _ = _device_batch(env, [good], 2)
    assert rc == 0 and I[0].any() and not I[1].any()
