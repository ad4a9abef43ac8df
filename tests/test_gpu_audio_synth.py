"""The 12 kHz audio scene synthesiser (K17) through the C ABI: records and clip counts byte for byte the serial checker's
(tests/helpers/audio_synth_check.cpp) at every length around a thread's vector, a symbol and the kernel's tile, frames that
hang off either end, split invariance, clipping, the host entry point, the refusals, and the whole chain on the device:
K17 -> K12 -> decoder against the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import audio_lib as al
import audio_synth_lib as asl

pytestmark = pytest.mark.gpu

NS = 45000
T = asl.TILE
MSG = al.SCENE_MESSAGES
LENGTHS = [0, 1, 7, 8, 9, 8191, 8192, 8193, 3 * 8192 + 5, T - 1, T, T + 1, 2 * T + 3]


@pytest.fixture(scope="module")
def env():
    import torch
    import rtlsdr_wsprd_amd as w
    assert w.lib().wspr_device_ready() == 1
    torch.cuda.set_device(0)
    return torch, w, torch.device("cuda", 0), int(w.lib().wspr_iq_stride())


def _t0(first):
    """A t0 whose first index is `first`: the middle of that sample (float32 resolves 1e-5 s at 110 s: an eighth of a sample)."""
    t0 = float(np.float32((first + 0.5) / 12000.0))
    assert asl.first_index(t0) == first, first
    return t0


def _prefill(nseg, nsamp, pad, seed):
    """Rows of round8(nsamp) + pad samples: random samples within +-20000, SENTINEL behind round8(nsamp)."""
    width = asl.round8(nsamp) + pad
    rows = np.random.default_rng(seed).integers(-20000, 20001, (nseg, width)).astype(np.int16)
    rows[:, asl.round8(nsamp):] = asl.SENTINEL
    return rows


def _device(env, items, nseg, nsamp, rows, seg_index0=0, sigma=0.0, seed=0, flags=0, count=True, **kw):
    """wspr_synth_audio_batch_device() on a device copy of `rows`: (rc, rows afterwards, n_clipped pre-filled with -7)."""
    torch, w, dev, _ = env
    d = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    n = np.full(max(nseg, 1), -7, np.int32)
    w.sync_torch()
    rc = w.synth_audio_batch_device(items, kw.get("nseg_arg", nseg), kw.get("nsamp_arg", nsamp), d.data_ptr() + kw.get("offset", 0),
                                    kw.get("stride", rows.shape[1]), seg_index0, sigma, seed, flags, n if count else None)
    return rc, d.cpu().numpy(), n[:nseg]


def _both(env, items, nseg, nsamp, rows, **kw):
    """The device and the checker on the same rows: asserts that records, padding, sentinels and counts are equal."""
    rc, got, count = _device(env, items, nseg, nsamp, rows, **kw)
    crc, want, ccount = asl.check_batch(items, nseg, nsamp, rows=rows, **kw)
    assert rc == 0 and crc == 0
    bad = int((got != want).sum())
    print("nsamp %d: %d of %d samples differ, clipped %s (checker %s)" % (nsamp, bad, got.size, count.tolist(), ccount.tolist()))
    assert np.array_equal(got, want)
    assert np.array_equal(count, ccount)
    return got, count


def _short_scene():
    """Two records: a frame that began 0.3 s before the record and one whose first sample is the record's sixth over noise; a
    drifting one at another offset."""
    return [asl.item(0, MSG[0][0], -104.3, -0.3, 9000.0), asl.item(0, MSG[0][1], 21.7, _t0(5), 7000.0, -2.0),
            asl.item(1, MSG[0][2], 107.9, _t0(-8192 * 3 - 4), 9000.0, 3.0)]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nsamp", LENGTHS)
def test_lengths_equal_the_checker(env, nsamp, accumulate):
    rows = _prefill(2, nsamp, 24, 100 + nsamp)
    got, count = _both(env, _short_scene(), 2, nsamp, rows, sigma=300.0, seed=5, flags=accumulate, seg_index0=7)
    r8 = asl.round8(nsamp)
    assert (got[:, r8:] == asl.SENTINEL).all()                                  # the columns behind are untouched
    if accumulate:
        assert np.array_equal(got[:, nsamp:r8], rows[:, nsamp:r8])              # from nsamp on: kept
    else:
        assert not got[:, nsamp:r8].any()                                        # ... or zero
    if nsamp >= 8:
        assert (got[:, :nsamp] != rows[:, :nsamp]).any()


def test_frame_edges_on_thread_and_tile_edges(env):
    """Three records, five transmissions in one and none in another.  Frame starts, symbol boundaries and frame ends inside a
    thread's eight samples (2051, 10243, 4100) and on a tile's first sample (4096, 12288, 6143 + 1); a frame that ends
    before the record and one that starts behind it; two transmissions at the same f0 in one record."""
    nsamp = 7 * T + 77
    items = [asl.item(0, MSG[1][0], 33.3, _t0(T + 3), 5000.0, 1.0),            # first sample 2051, symbol boundary 10243
             asl.item(0, MSG[1][1], 33.3, _t0(2 * T), 5000.0),                 # the same f0; first 4096, boundary 12288
             asl.item(0, MSG[1][2], -60.0, _t0(2 * T + 5 - asl.SIGLEN), 5000.0, -3.0),   # last sample 4100
             asl.item(0, MSG[2][0], 80.0, -115.0, 5000.0),                     # ends 52 898 samples before the record
             asl.item(0, MSG[2][1], -80.0, 10.0, 5000.0),                      # starts at 120 000, behind the record
             asl.item(2, MSG[2][2], 150.0, _t0(3 * T - asl.SIGLEN), 5000.0),   # last sample 6143
             asl.item(2, MSG[0][0], -150.0, _t0(-5), 5000.0, 2.0)]             # first sample 5 before the record
    got, count = _both(env, items, 3, nsamp, _prefill(3, nsamp, 8, 1), sigma=200.0, seed=11)
    rc, quiet, _ = asl.check_batch([], 3, nsamp, sigma=200.0, seed=11)
    assert rc == 0 and np.array_equal(got[1, :nsamp], quiet[1, :nsamp])         # record 1: noise alone
    # the far-away frames add nothing: the record without them is the same
    rc, without, _ = asl.check_batch(items[:3], 3, nsamp, sigma=200.0, seed=11)
    assert rc == 0 and np.array_equal(got[0, :nsamp], without[0, :nsamp])
    # list order is part of the contract: the swapped list is what the checker makes of the swapped list
    swapped = [items[1], items[0]] + items[2:]
    _both(env, swapped, 3, nsamp, _prefill(3, nsamp, 8, 1), sigma=200.0, seed=11)


def test_split_invariance_on_the_device(env):
    nsamp = T + 100
    def scene(seg0):
        return [asl.item(s - seg0, MSG[s % 3][s % 2], 20.0 * s - 30.0, 0.01 * s - 0.02, 6000.0, s - 1.5)
                for s in range(seg0, 4) for _ in range(1 + (s & 1))]
    rc4, rows4, c4 = _device(env, scene(0), 4, nsamp, _prefill(4, nsamp, 8, 2), sigma=2500.0, seed=99)
    rc2, rows2, c2 = _device(env, scene(2), 2, nsamp, _prefill(2, nsamp, 8, 3), sigma=2500.0, seed=99, seg_index0=2)
    assert rc4 == 0 and rc2 == 0
    assert np.array_equal(rows4[2:, :asl.round8(nsamp)], rows2[:, :asl.round8(nsamp)]) and np.array_equal(c4[2:], c2)
    assert not np.array_equal(rows4[0, :nsamp], rows4[2, :nsamp])


def test_clipping_counts_equal_the_checker(env):
    nsamp = 2 * T + 3
    items = [asl.item(0, MSG[0][0], 12.5, -1.0, 40000.0), asl.item(1, MSG[0][1], -12.5, _t0(T - 2), -40000.0, 1.0)]
    rows = _prefill(2, nsamp, 8, 4)
    got, count = _both(env, items, 2, nsamp, rows, sigma=3000.0, seed=21)
    assert count[0] > nsamp // 10 and 0 < count[1] < count[0]
    assert (got[:, :nsamp] == 32767).any() and (got[:, :nsamp] == -32768).any()
    rc, again, untouched = _device(env, items, 2, nsamp, rows, sigma=3000.0, seed=21, count=False)       # n_clipped == NULL
    assert rc == 0 and np.array_equal(again, got) and (untouched == -7).all()


def _tup(s):
    return (s.message, s.call, s.loc, s.pwr, s.cycles, s.jitter, s.drift, s.sync, s.snr, s.dt, s.freq)


def _same_as_oracle(got, ref):
    """every field equal, snr to 1e-4 dB (tests/test_gpu_audio.py's equality)"""
    g = [_tup(x) for x in got]
    r = [_tup(x) for x in ref]
    return [t[:8] + t[9:] for t in g] == [t[:8] + t[9:] for t in r] and all(abs(a[8] - b[8]) < 1e-4 for a, b in zip(g, r))


def test_scenes_to_spots_on_the_device(env):
    """One full-length record per audio_lib scene, the whole chain on the device: K17 -> K12 -> the decoder."""
    torch, w, dev, stride = env
    items = [it for k in range(3) for it in asl.scene_items(k, seg=k)]
    d_pcm = torch.full((3, al.NSAMP), asl.SENTINEL, dtype=torch.int16, device=dev)
    dI = torch.full((3, stride), float("nan"), dtype=torch.float32, device=dev)
    dQ = torch.full((3, stride), float("nan"), dtype=torch.float32, device=dev)
    clipped = np.full(3, -7, np.int32)
    w.sync_torch()
    assert w.synth_audio_batch_device(items, 3, al.NSAMP, d_pcm.data_ptr(), al.NSAMP, 0, asl.SIGMA, asl.SCENE_SEED, 0, clipped) == 0
    assert w.audio_batch_device(d_pcm.data_ptr(), al.NSAMP, al.NSAMP, 3, dI.data_ptr(), dQ.data_ptr(), 1) == 0
    dec = w.BatchDecoder(3, 32)
    dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)
    pcm = d_pcm.cpu().numpy()
    for k in range(3):
        want, wclip = asl.scene(k)
        assert np.array_equal(pcm[k], want[:al.NSAMP]) and clipped[k] == wclip, k
        assert _same_as_oracle(dec.spots(k), asl.scene_oracle(k)), k
        assert all(s is not None for s in al.find_sent(dec.spots(k), al.scene_items(k))), k


@pytest.mark.parametrize("nsamp", [0, 1001, 2 * T + 3])
def test_host_entry_point_is_row_zero_of_the_batch_call(env, nsamp):
    torch, w, dev, stride = env
    items = [it for it in _short_scene() if it[0] == 0]
    for flags in (0, asl.ACCUMULATE):
        rows = _prefill(1, nsamp, 8, 6)
        rc, got, count = _device(env, items, 1, nsamp, rows, sigma=20000.0, seed=3, flags=flags)
        pcm, clipped = w.synth_audio(items, nsamp=nsamp, noise_sigma=20000.0, seed=3, flags=flags, pcm=rows[0, :nsamp])
        assert rc == 0 and np.array_equal(pcm, got[0, :nsamp]) and clipped == count[0]
        assert nsamp == 0 or clipped > 0


def test_refusals_leave_rows_and_counts_untouched(env):
    torch, w, dev, stride = env
    nsamp = 4096
    good = [it for it in _short_scene() if it[0] == 0]
    rows = _prefill(2, nsamp, 104, 8)
    cases = [(good, dict(offset=2), -1), (good, dict(offset=8), -1),           # misaligned d_pcm
             (good, dict(stride=4100), -1), (good, dict(stride=4088), -1),      # no multiple of 8; below nsamp
             (good, dict(nseg_arg=-1), -1), (good, dict(nsamp_arg=-1), -1),
             (good, dict(nsamp_arg=1440001, stride=1440008, nseg_arg=1), -2),
             (good, dict(flags=2), -1), (good, dict(sigma=-1.0), -1), (good, dict(sigma=float("nan")), -1),
             ([asl.item(0, MSG[0][0], 800.5, 0.0, 100.0)], {}, -1),
             ([asl.item(0, MSG[0][0], 0.0, 0.0, 2.0e6)], {}, -1),
             ([asl.item(2, MSG[0][0], 0.0, 0.0, 100.0)], {}, -1),
             ([(0, 0.0, 0.0, 100.0, 0.0, tuple([4] * 162))], {}, -1)]
    for items, kw, want in cases:
        kw = dict(dict(sigma=10.0, seed=1), **kw)
        rc, got, count = _device(env, items, 2, nsamp, rows, **kw)
        assert rc == want, (kw, rc)
        assert np.array_equal(got, rows) and (count == -7).all(), kw
    pcm = np.full(nsamp, 0x1234, np.int16)
    n = C.c_int(-7)
    arr = w.synth_tx_list(good)
    assert w.lib().wspr_synth_audio(C.addressof(arr), len(good), nsamp, 10.0, 1, 4, pcm.ctypes.data, C.addressof(n)) == -1
    assert (pcm == 0x1234).all() and n.value == -7
    rc, got, count = _device(env, [], 2, nsamp, rows, nseg_arg=0)                 # nseg == 0 does nothing
    assert rc == 0 and np.array_equal(got, rows) and (count == -7).all()
    rc, got, count = _device(env, good, 2, 0, rows, sigma=10.0)               # nsamp == 0 writes no sample, counts are zero
    assert rc == 0 and np.array_equal(got, rows) and count.tolist() == [0, 0]
