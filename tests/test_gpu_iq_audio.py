"""IQ to audio (K18) through the C ABI: records and clip counts byte for byte the serial checker's
(tests/helpers/iq_audio_check.c) at every length around a block, the kernel's tile and a full row, with every kind of value
a float row can hold, split invariance, the host entry point, the refusals, a WAV file, and the whole loop on the device:
K8 -> K18 -> K12 -> decoder against the decode of the K8 rows themselves."""
import ctypes as C

import numpy as np
import pytest

import audio_lib as al
import iq_audio_lib as iq
import oracle_lib as ol
import synth_lib as sl

pytestmark = pytest.mark.gpu

NS = 45000
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 2 * 64 + 3, NS]
SIGMA = float(np.float32(np.sqrt((375.0 / 2500.0) / 2.0)))       # K8's noise of unit power in 2 500 Hz


@pytest.fixture(scope="module")
def env():
    import torch
    import rtlsdr_wsprd_amd as w
    assert w.lib().wspr_device_ready() == 1
    torch.cuda.set_device(0)
    return torch, w, torch.device("cuda", 0), int(w.lib().wspr_iq_stride())


def _rows(nseg, np_, seed, amp=0.4):
    """Random rows of np_ samples within +-amp in rows of round4(np_) + 8 floats; NaN behind np_ (it must not be read)."""
    rng = np.random.default_rng(seed)
    width = ((np_ + 3) & ~3) + 8
    I = np.full((nseg, width), np.nan, np.float32)
    Q = np.full((nseg, width), np.nan, np.float32)
    I[:, :np_] = rng.uniform(-amp, amp, (nseg, np_))
    Q[:, :np_] = rng.uniform(-amp, amp, (nseg, np_))
    return I, Q


def _prefill(nseg, np_, pad, seed):
    """Records of 32 np_ + pad samples: random samples within +-20000, SENTINEL behind 32 np_."""
    pcm = np.random.default_rng(seed).integers(-20000, 20001, (nseg, 32 * np_ + pad)).astype(np.int16)
    pcm[:, 32 * np_:] = iq.SENTINEL
    return pcm


def _device(env, I, Q, np_, pcm, gain=iq.GAIN, count=True, **kw):
    """wspr_iq_to_audio_batch_device() on device copies of the rows and records: (rc, records afterwards, n_clipped
    pre-filled with -7, the rows afterwards)."""
    torch, w, dev, _ = env
    nseg = I.shape[0]
    dI, dQ = torch.from_numpy(np.ascontiguousarray(I)).to(dev), torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    d = torch.from_numpy(np.ascontiguousarray(pcm)).to(dev)
    n = np.full(max(nseg, 1), -7, np.int32)
    w.sync_torch()
    rc = w.iq_to_audio_batch_device(dI.data_ptr() + kw.get("i_offset", 0), dQ.data_ptr() + kw.get("q_offset", 0),
                                    kw.get("nseg_arg", nseg), kw.get("np_arg", np_), kw.get("stride", I.shape[1]),
                                    d.data_ptr() + kw.get("offset", 0), kw.get("pcm_stride", pcm.shape[1]), gain,
                                    n if count else None)
    return rc, d.cpu().numpy(), n[:nseg], (dI.cpu().numpy(), dQ.cpu().numpy())


def _both(env, I, Q, np_, pcm, gain=iq.GAIN):
    """The device and the checker on the same rows: asserts that records, sentinels, counts and the input are equal."""
    rc, got, count, (aI, aQ) = _device(env, I, Q, np_, pcm, gain)
    crc, want, ccount = iq.check_rows(I, Q, np_, gain, pcm=pcm)
    assert rc == 0 and crc == 0
    bad = int((got != want).sum())
    print("np %d, gain %g: %d of %d samples differ, clipped %s (checker %s)" % (np_, gain, bad, got.size, count.tolist(), ccount.tolist()))
    assert np.array_equal(got, want)
    assert np.array_equal(count, ccount)
    assert np.array_equal(aI.view(np.uint32), I.view(np.uint32)) and np.array_equal(aQ.view(np.uint32), Q.view(np.uint32))
    return got, count


@pytest.mark.parametrize("np_", LENGTHS)
def test_lengths_equal_the_checker(env, np_):
    I, Q = _rows(3, np_, 200 + np_)
    pcm = _prefill(3, np_, 24, 300 + np_)
    got, count = _both(env, I, Q, np_, pcm)
    assert (got[:, 32 * np_:] == iq.SENTINEL).all()                              # the columns behind are untouched
    if np_:
        assert (got[:, :32 * np_] != pcm[:, :32 * np_]).any() and np.abs(got[:, :32 * np_].astype(np.int32)).max() > 4000


@pytest.mark.parametrize("gain", [iq.GAIN, 0.0, -32768.0, 3.0e6])
@pytest.mark.parametrize("np_", [17, 2 * 64 + 3, 400])              # 400: tiles with no step outside the row
def test_odd_values_and_gains_equal_the_checker(env, np_, gain):
    """NaN, +-Inf, denormals, 1e30, 3e38 and -0.0 at a row's first and last samples, on tile edges and elsewhere."""
    I, Q = _rows(3, np_, 42)
    I[:, :np_], Q[:, :np_] = iq.odd_rows(np_, 40 + np_)
    got, count = _both(env, I, Q, np_, _prefill(3, np_, 8, 41), gain)
    assert (count > 0).all()                                                   # NaN counts at every gain
    if gain == 3.0e6:
        assert (count > 32 * np_ // 2).all() and (got == 32767).any() and (got == -32768).any()
    if gain == 0.0:
        assert not got[:, :32 * np_].any()


def test_denormal_rows_are_not_flushed(env):
    """A row of denormals alone, seen through a gain of 3e38: the multiply-adds keep them as the checker's fmaf does."""
    tiny = np.full((1, 72), 1e-38, np.float32)
    got, count = _both(env, tiny, -tiny, 65, _prefill(1, 65, 8, 5), 3e38)
    assert got[:, :32 * 65].any() and not count.any()


def test_one_call_equals_two(env):
    np_ = 2 * 64 + 3
    I, Q = _rows(5, np_, 10)                                                   # rows 3 and 4 stay random; a stride of 140
    I[:3, :np_], Q[:3, :np_] = iq.odd_rows(np_, 9)
    pcm = _prefill(5, np_, 8, 11)
    rc5, all5, c5, _ = _device(env, I, Q, np_, pcm, 50000.0)
    rc2, lo, c2, _ = _device(env, I[:2], Q[:2], np_, pcm[:2], 50000.0)
    rc3, hi, c3, _ = _device(env, I[2:], Q[2:], np_, pcm[2:], 50000.0)
    assert rc5 == 0 and rc2 == 0 and rc3 == 0
    assert np.array_equal(all5, np.concatenate((lo, hi))) and np.array_equal(c5, np.concatenate((c2, c3)))
    assert c5.sum() > 0 and not np.array_equal(all5[3], all5[4])


@pytest.mark.parametrize("np_", [0, 1001, NS])
def test_host_entry_point_is_row_zero_of_the_batch_call(env, np_):
    torch, w, dev, stride = env
    I, Q = _rows(1, np_, 60 + np_, amp=0.6)
    rc, got, count, _ = _device(env, I, Q, np_, _prefill(1, np_, 8, 61))
    pcm, clipped = w.iq_to_audio(I[0], Q[0], samples=np_)
    assert rc == 0 and pcm.size == 32 * np_ and np.array_equal(pcm, got[0, :32 * np_]) and clipped == count[0]
    assert np_ == 0 or clipped > 0                                             # an amplitude of 0.6 at gain 32768 clips


def test_refusals_leave_records_and_counts_untouched(env):
    torch, w, dev, stride = env
    np_ = 128
    I, Q = _rows(2, np_, 70)                                                   # rows of 136 floats
    pcm = _prefill(2, np_, 104, 71)                                             # records of 4200 samples
    cases = [(dict(i_offset=4), -1), (dict(q_offset=8), -1), (dict(offset=2), -1), (dict(offset=8), -1),      # misaligned
             (dict(stride=134), -1), (dict(stride=124), -1),                    # no multiple of 4; below samples
             (dict(pcm_stride=4100), -1), (dict(pcm_stride=4088), -1),          # no multiple of 8; below 32 * samples
             (dict(nseg_arg=-1), -1), (dict(np_arg=-1), -1),
             (dict(np_arg=45001, stride=45004, pcm_stride=1440032, nseg_arg=1), -2),
             (dict(gain=float("nan")), -1), (dict(gain=float("inf")), -1), (dict(gain=float("-inf")), -1)]
    for kw, want in cases:
        gain = kw.pop("gain", iq.GAIN)
        rc, got, count, _ = _device(env, I, Q, np_, pcm, gain, **kw)
        assert rc == want, (kw, rc)
        assert np.array_equal(got, pcm) and (count == -7).all(), kw
    out = np.full(32 * np_, 0x1234, np.int16)
    n = C.c_int(-7)
    for args, want in (((I[0].ctypes.data, Q[0].ctypes.data, np_, float("nan")), -1),
                       ((I[0].ctypes.data, Q[0].ctypes.data, -1, 1.0), -1), ((I[0].ctypes.data, Q[0].ctypes.data, 45001, 1.0), -2)):
        assert w.lib().wspr_iq_to_audio(*args, out.ctypes.data, C.addressof(n)) == want
        assert (out == 0x1234).all() and n.value == -7
    rc, got, count, _ = _device(env, I, Q, np_, pcm, nseg_arg=0)                 # nseg == 0 does nothing
    assert rc == 0 and np.array_equal(got, pcm) and (count == -7).all()
    rc, got, count, _ = _device(env, I, Q, 0, pcm)                               # samples == 0 writes no sample, counts are zero
    assert rc == 0 and np.array_equal(got, pcm) and count.tolist() == [0, 0]
    rc, got, count, _ = _device(env, I, Q, np_, pcm, count=False)                # n_clipped == NULL
    assert rc == 0 and (count == -7).all() and not np.array_equal(got, pcm)


def test_a_record_survives_a_wav_file(env, tmp_path):
    torch, w, dev, stride = env
    I, Q = _rows(1, 1001, 80)
    pcm, clipped = w.iq_to_audio(I[0], Q[0], samples=1001)
    w.write_wav_file(tmp_path / "slot.wav", pcm)
    back = w.read_wav_file(tmp_path / "slot.wav")
    assert back.size == 32 * 1001 and np.array_equal(back, pcm) and clipped == 0 and pcm.any()


# ---- the loop on the device -------------------------------------------------------------------------------------------------
LOOP_SNRS = [(-6.0, -12.0, -18.0), (-18.0, -10.0, -14.0), (-15.0, -18.0, -9.0), (-12.0, -16.0, -18.0)]


def _loop_items():
    items, sent = [], []
    for seg in range(4):
        for j, (name, f0, t0) in enumerate(al.SIGNALS):
            msg = al.SCENE_MESSAGES[(seg + j) % 3][j]
            ok, sym = ol.channel_symbols(msg)
            assert ok
            snr = LOOP_SNRS[seg][j]
            f, t = f0 * (1.0 - 0.05 * seg), t0 - 0.2 * seg                      # inside the +-110 Hz the decoder searches
            items.append((seg, f, t, 10.0 ** (snr / 20.0), 0.0, sym))
            sent.append((seg, msg, snr, f, t))
    return items, sent


def _tup(s):
    return (s.message, s.call, s.loc, s.pwr, s.cycles, s.jitter, s.drift, s.sync, s.snr, s.dt, s.freq)


def test_k8_scenes_survive_k18_and_k12_on_the_device(env):
    """Four K8 scenes of three signals at -6 .. -18 dB, normalised, decoded as they are and after K18 (gain 32768) -> K12
    (normalise = 1), without a sample leaving the device.
    1. The loop's spots are the CPU oracle's of the same chain in the checkers (K8's, K18's, K12's): every field equal, snr
       to 1e-4 dB -- the equality tests/test_gpu_audio_synth.py's scenes-to-spots test holds its device chain to.
    2. The loop's messages are those of the rows decoded as they are; between the two, f, dt and snr of every spot stay
       within the 0.15 Hz, 0.1 s and 0.5 dB tests/test_audio_checker.py states for scenes (on the CPU the same loop moved
       neither f nor dt and the snr by 0.05 dB: the filters' edges beyond +-150 Hz, taken twice, lower the noise estimate)."""
    torch, w, dev, stride = env
    items, sent = _loop_items()
    dI = torch.zeros(4, stride, device=dev)
    dQ = torch.zeros(4, stride, device=dev)
    d_pcm = torch.full((4, al.NSAMP), iq.SENTINEL, dtype=torch.int16, device=dev)
    bI = torch.full((4, stride), float("nan"), dtype=torch.float32, device=dev)
    bQ = torch.full((4, stride), float("nan"), dtype=torch.float32, device=dev)
    clipped = np.full(4, -7, np.int32)
    w.sync_torch()
    assert w.wspr_synth_batch_device(items, 4, dI.data_ptr(), dQ.data_ptr(), 0, SIGMA, 1818, sl.NORMALISE) == 0
    direct = w.BatchDecoder(4, 32)
    direct.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)
    assert w.iq_to_audio_batch_device(dI.data_ptr(), dQ.data_ptr(), 4, NS, stride, d_pcm.data_ptr(), al.NSAMP, iq.GAIN, clipped) == 0
    assert w.audio_batch_device(d_pcm.data_ptr(), al.NSAMP, al.NSAMP, 4, bI.data_ptr(), bQ.data_ptr(), 1) == 0
    loop = w.BatchDecoder(4, 32)
    loop.decode_ptr(bI.data_ptr(), bQ.data_ptr(), NS, stride)
    # the same chain in the checkers
    rc, cI, cQ = sl.check_batch(items, 4, 0, SIGMA, 1818, sl.NORMALISE)
    assert rc == 0
    crc, cpcm, cclip = iq.check_rows(cI, cQ)
    assert crc == 0 and np.array_equal(d_pcm.cpu().numpy(), cpcm) and np.array_equal(clipped, cclip)
    kI, kQ = al.check_rows(cpcm, normalise=1)
    print("clipped per record: %s" % clipped.tolist())
    for seg in range(4):
        got, was = loop.spots(seg), direct.spots(seg)
        ref = ol.decode(kI[seg], kQ[seg])[0]
        g, r = [_tup(x) for x in got], [_tup(x) for x in ref]
        assert [t[:8] + t[9:] for t in g] == [t[:8] + t[9:] for t in r], seg
        assert all(abs(a[8] - b[8]) < 1e-4 for a, b in zip(g, r)), seg
        assert sorted(s.message for s in got) == sorted(s.message for s in was), seg
        mine = [x for x in sent if x[0] == seg]
        found = al.find_sent(got, [x[1:] for x in mine])
        before = al.find_sent(was, [x[1:] for x in mine])
        for s, d, (_, msg, snr, f0, t0) in zip(found, before, mine):
            assert s is not None and d is not None, (seg, msg)
            print("seg %d %-16s snr %+.2f (direct %+.2f, sent %+.1f)  df %+.4f Hz  ddt %+.4f s" %
                  (seg, msg, s.snr, d.snr, snr, (s.freq - d.freq) * 1e6, s.dt - d.dt))
            assert abs(s.freq - d.freq) * 1e6 <= 0.15 and abs(s.dt - d.dt) <= 0.1 and abs(s.snr - d.snr) <= 0.5
