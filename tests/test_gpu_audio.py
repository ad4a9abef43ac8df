"""The 12 kHz audio front end (K12) through the C ABI: rows bit for bit the serial checker's (tests/helpers/audio_check.c),
every length around the kernel's tile, the refusals, and WAV file -> device -> decoder against the CPU oracle."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import audio_lib as al
import oracle_lib as ol

pytestmark = pytest.mark.gpu

NS = 45000
NROWS = 5
T = al.tile()
LENGTHS = [0, 1, 31, 32, 33, 255, 256, 511, 512, T * 32 - 1, T * 32, T * 32 + 1, 3 * T * 32 + 17, 1439999, 1440000]


@pytest.fixture(scope="module")
def env():
    import torch
    import rtlsdr_wsprd_amd as w
    assert w.lib().wspr_device_ready() == 1
    torch.cuda.set_device(0)
    return torch, w, torch.device("cuda", 0), int(w.lib().wspr_iq_stride())


@functools.lru_cache(maxsize=None)
def random_records():
    """NROWS full-scale random records, -32768 and 32767 included (read-only)."""
    pcm = np.random.default_rng(2024).integers(-32768, 32768, (NROWS, al.NSAMP)).astype(np.int16)
    pcm[:, 5] = -32768
    pcm[:, 6] = 32767
    pcm.setflags(write=False)
    return pcm


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _device_rows(env, pcm, nsamp=None, normalise=0, pad=64, ptr_offset=0, stride=None, nseg=None):
    """wspr_audio_batch_device() on records [nseg, >= nsamp]: device rows of round8(nsamp) + pad samples, the padding 0x7FFF,
    outputs pre-filled with NaN.  Returns (rc, I, Q) with the whole stride."""
    torch, w, dev, ostride = env
    pcm = np.asarray(pcm, np.int16)
    rows = pcm.shape[0]
    nsamp = pcm.shape[1] if nsamp is None else nsamp
    keep = max(0, min(nsamp, pcm.shape[1]))
    width = ((keep + 7) & ~7) + pad
    host = np.full((rows, width), 0x7FFF, np.int16)
    host[:, :keep] = pcm[:, :keep]
    d_pcm = torch.from_numpy(host).to(dev)
    dI = torch.full((rows, ostride), float("nan"), dtype=torch.float32, device=dev)
    dQ = torch.full((rows, ostride), float("nan"), dtype=torch.float32, device=dev)
    w.sync_torch()
    rc = w.audio_batch_device(d_pcm.data_ptr() + ptr_offset, width if stride is None else stride, nsamp,
                              rows if nseg is None else nseg, dI.data_ptr(), dQ.data_ptr(), normalise)
    return rc, dI.cpu().numpy(), dQ.cpu().numpy()


def _same_rows(got, want):
    """The first 45000 columns equal bit for bit, the rest of the stride +0.0f."""
    return np.array_equal(_bits(got[:, :NS]), _bits(want[:, :NS])) and not _bits(got[:, NS:]).any()


@pytest.mark.parametrize("nsamp", LENGTHS)
def test_lengths_equal_the_checker(env, nsamp):
    pcm = random_records()[:, :max(nsamp, 8)]
    rc, I, Q = _device_rows(env, pcm, nsamp)
    ci, cq = al.check_rows(pcm, nsamp)
    assert rc == 0
    bad = int((_bits(I[:, :NS]) != _bits(ci)).sum() + (_bits(Q[:, :NS]) != _bits(cq)).sum())
    print("nsamp %d: %d outputs, %d words differ" % (nsamp, al.n_out(nsamp), bad))
    assert _same_rows(I, ci) and _same_rows(Q, cq)
    n = al.n_out(nsamp)
    assert not _bits(I[:, n:]).any() and not _bits(Q[:, n:]).any()            # zero from n_out to the stride


def test_row_contents_equal_the_checker(env):
    n = 3 * T * 32 + 17
    rows = np.zeros((4, n), np.int16)
    rows[0] = random_records()[0, :n]
    rows[1] = 32767
    rows[2] = -32768
    rc, I, Q = _device_rows(env, rows)
    ci, cq = al.check_rows(rows)
    assert rc == 0 and _same_rows(I, ci) and _same_rows(Q, cq)
    assert not _bits(I[3]).any() and not _bits(Q[3]).any()                   # zeros in, +0.0f out


@pytest.mark.parametrize("nsamp", [1000, 1440000])
def test_impulses_equal_the_table(env, nsamp):
    pcm, ei, eq = al.impulse_rows(nsamp)
    rc, I, Q = _device_rows(env, pcm)
    assert rc == 0 and _same_rows(I, ei) and _same_rows(Q, eq)


def test_normalisation_is_the_receivers_rule(env):
    n = T * 32 + 4001
    rows = np.zeros((3, n), np.int16)
    rows[0] = random_records()[1, :n]
    rows[1] = al.scene(0)[:n]
    rc, I, Q = _device_rows(env, rows, normalise=1)
    ci, cq = al.check_rows(rows)
    assert rc == 0
    for s in range(3):
        peak = max(np.float32(1e-24), np.abs(ci[s]).max(), np.abs(cq[s]).max())
        scale = np.float32(0.5 / float(peak))
        assert np.array_equal(_bits(I[s, :NS]), _bits(ci[s] * scale)) and np.array_equal(_bits(Q[s, :NS]), _bits(cq[s] * scale))
        assert not _bits(I[s, NS:]).any() and not _bits(Q[s, NS:]).any()
    assert abs(float(max(np.abs(I[0]).max(), np.abs(Q[0]).max())) - 0.5) < 1e-6      # peak * (float)(0.5 / peak): 0.5 to an ulp
    assert not _bits(I[2]).any() and not _bits(Q[2]).any()                   # a zero row stays zero
    ni, nq = al.check_rows(rows, normalise=1)
    assert _same_rows(I, ni) and _same_rows(Q, nq)


def test_arithmetic_mode_does_not_touch_the_front_end(env):
    torch, w, dev, stride = env
    rows = random_records()[:2, :T * 32 + 777]
    ci, cq = al.check_rows(rows)
    prev = w.wspr_set_arithmetic(w.WSPR_ARITH_CONTRACTED)
    try:
        rc, I, Q = _device_rows(env, rows)
    finally:
        w.wspr_set_arithmetic(prev)
    assert rc == 0 and _same_rows(I, ci) and _same_rows(Q, cq)


@pytest.mark.parametrize("nsamp", [0, 1000, 1440000])
def test_host_entry_point_is_row_zero_of_the_batch_call(env, nsamp):
    torch, w, dev, stride = env
    pcm = random_records()[2:3, :max(nsamp, 8)]
    for normalise in (0, 1):
        rc, I, Q = _device_rows(env, pcm, nsamp, normalise=normalise)
        hi, hq, n = w.audio_to_iq(pcm[0, :nsamp], normalise)
        assert rc == 0 and n == al.n_out(nsamp)
        assert np.array_equal(_bits(hi), _bits(I[0, :NS])) and np.array_equal(_bits(hq), _bits(Q[0, :NS]))


def test_refusals_leave_the_outputs_alone(env):
    torch, w, dev, stride = env
    pcm = random_records()[:2, :4096]
    cases = [(dict(ptr_offset=2), -1),                        # misaligned d_pcm
             (dict(ptr_offset=8), -1),
             (dict(stride=4100), -1),                         # stride not a multiple of 8
             (dict(stride=4088), -1),                         # stride < nsamp
             (dict(nseg=-1), -1),
             (dict(nsamp=-1), -1),
             (dict(nsamp=1440001, stride=1440008, nseg=1), -2)]
    for kw, want in cases:
        rc, I, Q = _device_rows(env, pcm, **kw)
        assert rc == want, (kw, rc)
        assert np.isnan(I).all() and np.isnan(Q).all(), kw
    with pytest.raises(RuntimeError):
        w.audio_to_iq(np.zeros(1440001, np.int16))
    rc, I, Q = _device_rows(env, pcm, nseg=0)                 # nseg == 0 does nothing
    assert rc == 0 and np.isnan(I).all() and np.isnan(Q).all()


def _tup(s):
    return (s.message, s.call, s.loc, s.pwr, s.cycles, s.jitter, s.drift, s.sync, s.snr, s.dt, s.freq)


def _same_as_oracle(got, ref):
    """every field equal, snr to 1e-4 dB (the tolerance the decoder's own tests state)"""
    g = [_tup(x) for x in got]
    r = [_tup(x) for x in ref]
    return [t[:8] + t[9:] for t in g] == [t[:8] + t[9:] for t in r] and all(abs(a[8] - b[8]) < 1e-4 for a, b in zip(g, r))


def test_wav_files_to_spots(env, tmp_path):
    torch, w, dev, stride = env
    recs = []
    for k in range(3):
        al.write_wav(tmp_path / ("slot%d.wav" % k), al.scene(k))
        recs.append(w.read_wav_file(tmp_path / ("slot%d.wav" % k)))
        assert np.array_equal(recs[k], al.scene(k))
    d_pcm = torch.from_numpy(np.stack(recs)).to(dev)
    dI = torch.full((3, stride), float("nan"), dtype=torch.float32, device=dev)
    dQ = torch.full((3, stride), float("nan"), dtype=torch.float32, device=dev)
    w.sync_torch()
    assert w.audio_batch_device(d_pcm.data_ptr(), al.NSAMP, al.NSAMP, 3, dI.data_ptr(), dQ.data_ptr(), 1) == 0
    I, Q = dI.cpu().numpy(), dQ.cpu().numpy()
    dec = w.BatchDecoder(3, 32)
    dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)
    for k in range(3):
        ci, cq = al.scene_rows(k, 1)
        assert np.array_equal(_bits(I[k, :NS]), _bits(ci)) and np.array_equal(_bits(Q[k, :NS]), _bits(cq))
        ref = al.scene_oracle(k, 1)
        assert _same_as_oracle(dec.spots(k), ref), k
        assert all(s is not None for s in al.find_sent(dec.spots(k), al.scene_items(k))), k


def test_an_audio_call_leaves_the_decoder_as_it_was(env):
    torch, w, dev, stride = env
    I, Q, n = ol.read_iq_file(os.path.join(ol.ROOT, "tests", "golden", "refSignalSnr0dB.iq"))
    before, bi, bq = w.wspr_decode(I, Q, n)
    count = len(w.last_timings())
    rc, _, _ = _device_rows(env, random_records()[:2, :40000], normalise=1)
    w.audio_to_iq(random_records()[0, :5000])
    after, ai, aq = w.wspr_decode(I, Q, n)
    assert rc == 0 and len(before) == 1 and [_tup(s) for s in after] == [_tup(s) for s in before]
    assert np.array_equal(_bits(ai), _bits(bi)) and np.array_equal(_bits(aq), _bits(bq))
    assert len(w.last_timings()) == count == len(w.TIMING_NAMES)
