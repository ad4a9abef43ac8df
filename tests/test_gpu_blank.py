"""The impulse-noise blanker (K15) through the C ABI: rows and counts byte for byte the serial checker's
(tests/helpers/blank_check.c), every length around the block and every setting, the crafted cases, the fused call against
checker blanker + checker front end bit for bit, the refusals, and spiky audio -> device -> decoder against the CPU oracle."""
import functools
import os

import numpy as np
import pytest

import audio_lib as al
import blank_lib as bl
import oracle_lib as ol

pytestmark = pytest.mark.gpu

NS = 45000
LENGTHS = [0, 1, 2, 8191, 8192, 8193, 8196, 16383, 16385, 24581]
THRS = [16, 96, 4096]
GUARDS = [0, 1, 4, 64]


@pytest.fixture(scope="module")
def env():
    import torch
    import rtlsdr_wsprd_amd as w
    assert w.lib().wspr_device_ready() == 1
    torch.cuda.set_device(0)
    return torch, w, torch.device("cuda", 0), int(w.lib().wspr_iq_stride())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _to_device(env, pcm, nsamp, pad):
    """Records [rows, >= nsamp] in a sentinel-filled device buffer of stride round8(nsamp) + pad."""
    torch, w, dev, _ = env
    pcm = np.asarray(pcm, np.int16)
    keep = max(0, min(nsamp, pcm.shape[1]))
    width = bl.round8(keep) + pad
    host = np.full((pcm.shape[0], width), bl.SENTINEL, np.int16)
    host[:, :keep] = pcm[:, :keep]
    return torch.from_numpy(host).to(dev), width


def _device_blank(env, pcm, nsamp, thr16, guard, pad_in=24, pad_out=16, in_offset=0, out_offset=0, in_stride=None,
                  out_stride=None, nseg=None, d_in=None):
    """wspr_audio_blank_batch_device() on records [rows, >= nsamp]: input stride round8(nsamp) + pad_in, output stride
    round8(nsamp) + pad_out, both buffers filled with the sentinel, n_blanked pre-filled with -7.
    Returns (rc, out with the whole stride, n_blanked)."""
    torch, w, dev, _ = env
    rows = np.asarray(pcm).shape[0]
    if d_in is None:
        d_in, win = _to_device(env, pcm, nsamp, pad_in)
    else:
        win = d_in.shape[1]
    wout = bl.round8(max(0, min(nsamp, np.asarray(pcm).shape[1]))) + pad_out
    d_out = torch.full((rows, wout), bl.SENTINEL, dtype=torch.int16, device=dev)
    count = np.full(rows, -7, np.int32)
    w.sync_torch()
    rc = w.audio_blank_batch_device(d_in.data_ptr() + in_offset, win if in_stride is None else in_stride, nsamp,
                                    rows if nseg is None else nseg, thr16, guard, d_out.data_ptr() + out_offset,
                                    wout if out_stride is None else out_stride, count)
    return rc, d_out.cpu().numpy(), count


def _same_pcm(got, want, nsamp):
    """Columns 0 .. round8(nsamp) - 1 the checker's (zeros from nsamp on), the sentinel behind them."""
    r8 = bl.round8(nsamp)
    return np.array_equal(got[:, :r8], want[:, :r8]) and not got[:, nsamp:r8].any() and np.all(got[:, r8:] == bl.SENTINEL)


@pytest.mark.parametrize("nsamp", LENGTHS)
def test_lengths_and_settings_equal_the_checker(env, nsamp):
    rows = bl.random_rows(nsamp, 500 + nsamp)
    d_in, _ = _to_device(env, rows, nsamp, 24)
    for thr16 in THRS:
        for guard in GUARDS:
            rc, out, count = _device_blank(env, rows, nsamp, thr16, guard, d_in=d_in)
            want, n = bl.check_rows(rows, nsamp, thr16, guard)
            assert rc == 0 and _same_pcm(out, want, nsamp), (thr16, guard)
            assert count.tolist() == n.tolist(), (thr16, guard)
    print("nsamp %d: blanked at (96, 4): %s" % (nsamp, bl.check_rows(rows, nsamp, 96, 4)[1].tolist()))


def test_a_full_length_spiky_record_equals_the_checker(env):
    pcm = bl.e2e_scene(50)[None, :]
    rc, out, count = _device_blank(env, pcm, al.NSAMP, bl.THR, bl.GUARD)
    want, n = bl.scene_blanked(50)
    assert rc == 0 and _same_pcm(out, want[None, :], al.NSAMP) and count[0] == n
    assert 0.03 < n / al.NSAMP < 0.06


@pytest.mark.parametrize("case", bl.crafted_cases(), ids=[c[0] for c in bl.crafted_cases()])
def test_crafted_cases(env, case):
    name, pcm, thr16, guard, want, counts = case
    nsamp = pcm.shape[1]
    rc, out, count = _device_blank(env, pcm, nsamp, thr16, guard, pad_in=16, pad_out=16)
    assert rc == 0 and np.array_equal(out[:, :nsamp], want) and count.tolist() == counts
    assert not out[:, nsamp:bl.round8(nsamp)].any()
    assert np.all(out[:, bl.round8(nsamp):] == bl.SENTINEL)                 # what lies behind roundup8(nsamp) survives


def test_the_highest_threshold_copies_a_scene(env):
    rc, out, count = _device_blank(env, al.scene(0)[None, :], al.NSAMP, 4096, 64)
    assert rc == 0 and count[0] == 0 and np.array_equal(out[0, :al.NSAMP], al.scene(0))


def _device_fused(env, pcm, nsamp, thr16, guard, normalise, pad=40, nseg=None, ptr_offset=0, stride=None):
    """wspr_audio_blanked_batch_device(); outputs pre-filled with NaN, n_blanked with -7.  Returns (rc, I, Q, n_blanked)."""
    torch, w, dev, ostride = env
    rows = np.asarray(pcm).shape[0]
    d_in, win = _to_device(env, pcm, nsamp, pad)
    dI = torch.full((rows, ostride), float("nan"), dtype=torch.float32, device=dev)
    dQ = torch.full((rows, ostride), float("nan"), dtype=torch.float32, device=dev)
    count = np.full(rows, -7, np.int32)
    w.sync_torch()
    rc = w.audio_blanked_batch_device(d_in.data_ptr() + ptr_offset, win if stride is None else stride, nsamp,
                                      rows if nseg is None else nseg, thr16, guard, dI.data_ptr(), dQ.data_ptr(), normalise, count)
    return rc, dI.cpu().numpy(), dQ.cpu().numpy(), count


def _same_rows(got, want):
    """The first 45000 columns equal bit for bit, the rest of the stride +0.0f."""
    return np.array_equal(_bits(got[:, :NS]), _bits(want[:, :NS])) and not _bits(got[:, NS:]).any()


@functools.lru_cache(maxsize=None)
def _short_rows():
    """130 records of 8200 samples (two blocks, the second of 8 samples): quiet noise with spikes, each record its own."""
    rng = np.random.default_rng(77)
    rows = rng.integers(-400, 401, (130, 8200)).astype(np.int16)
    rows[rng.integers(0, 300, rows.shape) == 0] = 32767
    rows[rng.integers(0, 300, rows.shape) == 0] = -32768
    rows.setflags(write=False)
    return rows


@pytest.mark.parametrize("normalise", [0, 1])
def test_fused_call_equals_checker_blanker_then_checker_front_end(env, normalise):
    rows = _short_rows()                                            # 130 records: the chunk boundary at 128 is crossed
    rc, I, Q, count = _device_fused(env, rows, 8200, bl.THR, bl.GUARD, normalise)
    blanked, n = bl.check_rows(rows, 8200, bl.THR, bl.GUARD)
    ci, cq = al.check_rows(blanked, 8200, normalise=normalise)
    assert rc == 0 and count.tolist() == n.tolist() and n.min() > 0
    assert _same_rows(I, ci) and _same_rows(Q, cq)
    assert len({int(x) for x in n}) > 20                            # the records differ: a row in the wrong place would show


def test_fused_call_at_the_highest_threshold_is_the_plain_front_end(env):
    torch, w, dev, ostride = env
    pcm = al.scene(0)[None, :]
    rc, I, Q, count = _device_fused(env, pcm, al.NSAMP, 4096, 64, 1, pad=0)
    d_pcm = torch.from_numpy(np.array(pcm)).to(dev)
    pI = torch.full((1, ostride), float("nan"), dtype=torch.float32, device=dev)
    pQ = torch.full((1, ostride), float("nan"), dtype=torch.float32, device=dev)
    w.sync_torch()
    assert w.audio_batch_device(d_pcm.data_ptr(), al.NSAMP, al.NSAMP, 1, pI.data_ptr(), pQ.data_ptr(), 1) == 0
    assert rc == 0 and count[0] == 0
    assert np.array_equal(_bits(I), _bits(pI.cpu().numpy())) and np.array_equal(_bits(Q), _bits(pQ.cpu().numpy()))


@pytest.mark.parametrize("nsamp", [0, 8200, 1440000])
def test_host_entry_point_is_row_zero_of_the_batch_call(env, nsamp):
    torch, w, dev, stride = env
    pcm = bl.e2e_scene(50)[None, :max(nsamp, 8)]
    for normalise in (0, 1):
        rc, I, Q, count = _device_fused(env, pcm, nsamp, bl.THR, bl.GUARD, normalise)
        hi, hq, n, blanked = w.audio_to_iq_blanked(pcm[0, :nsamp], bl.THR, bl.GUARD, normalise)
        assert rc == 0 and n == al.n_out(nsamp) and blanked == count[0] and (blanked > 0 or nsamp == 0)
        assert np.array_equal(_bits(hi), _bits(I[0, :NS])) and np.array_equal(_bits(hq), _bits(Q[0, :NS]))


def test_refusals_leave_the_outputs_alone(env):
    torch, w, dev, stride = env
    pcm = bl.random_rows(4096, 5)[:2]
    blank_cases = [(dict(in_offset=2), -1),                    # misaligned d_pcm
                   (dict(in_offset=8), -1),
                   (dict(out_offset=8), -1),                   # misaligned d_out
                   (dict(in_stride=4100), -1),                 # strides that are no multiple of 8
                   (dict(out_stride=4100), -1),
                   (dict(in_stride=4088), -1),                 # strides below nsamp
                   (dict(out_stride=4088), -1),
                   (dict(nseg=-1), -1),
                   (dict(nsamp=-1), -1),
                   (dict(thr16=15), -1), (dict(thr16=4097), -1), (dict(guard=-1), -1), (dict(guard=65), -1),
                   (dict(nsamp=1440001, in_stride=1440008, out_stride=1440008, nseg=1), -2)]
    for kw, want in blank_cases:
        args = dict(nsamp=4096, thr16=bl.THR, guard=bl.GUARD)
        args.update(kw)
        rc, out, count = _device_blank(env, pcm, **args)
        assert rc == want, (kw, rc)
        assert np.all(out == bl.SENTINEL) and np.all(count == -7), kw
    # in place, eight samples on, and an output that starts inside the input's last row (the buffer is four rows long, so
    # that every one of these outputs would lie inside it)
    d_big, win = _to_device(env, np.concatenate((pcm, pcm)), 4096, 24)
    before = d_big.cpu().numpy()
    count = np.full(2, -7, np.int32)
    w.sync_torch()
    for shift in (0, 16, 2 * win + 32):
        assert w.audio_blank_batch_device(d_big.data_ptr(), win, 4096, 2, bl.THR, bl.GUARD, d_big.data_ptr() + shift, win, count) == -1
    assert np.array_equal(d_big.cpu().numpy(), before) and np.all(count == -7)
    rc, out, count = _device_blank(env, pcm, 4096, bl.THR, bl.GUARD, nseg=0)         # nseg == 0 does nothing
    assert rc == 0 and np.all(out == bl.SENTINEL) and np.all(count == -7)
    rc, out, count = _device_blank(env, pcm, 0, bl.THR, bl.GUARD)                    # nsamp == 0 writes no sample
    assert rc == 0 and np.all(out == bl.SENTINEL) and count.tolist() == [0, 0]

    fused_cases = [(dict(ptr_offset=2), -1), (dict(ptr_offset=8), -1), (dict(stride=4100), -1), (dict(stride=4088), -1),
                   (dict(nseg=-1), -1), (dict(nsamp=-1), -1),
                   (dict(thr16=15), -1), (dict(thr16=4097), -1), (dict(guard=-1), -1), (dict(guard=65), -1),
                   (dict(nsamp=1440001, stride=1440008, nseg=1), -2)]
    for kw, want in fused_cases:
        args = dict(nsamp=4096, thr16=bl.THR, guard=bl.GUARD, normalise=1)
        args.update(kw)
        rc, I, Q, count = _device_fused(env, pcm, **args)
        assert rc == want, (kw, rc)
        assert np.isnan(I).all() and np.isnan(Q).all() and np.all(count == -7), kw
    rc, I, Q, count = _device_fused(env, pcm, 4096, bl.THR, bl.GUARD, 1, nseg=0)
    assert rc == 0 and np.isnan(I).all() and np.isnan(Q).all() and np.all(count == -7)
    rc, I, Q, count = _device_fused(env, pcm, 0, bl.THR, bl.GUARD, 1)                # nsamp == 0 writes zero rows
    assert rc == 0 and not _bits(I).any() and not _bits(Q).any() and count.tolist() == [0, 0]
    for thr16, guard, n in ((15, 4, 100), (96, 65, 100), (96, 4, 1440001)):
        with pytest.raises(RuntimeError):
            w.audio_to_iq_blanked(np.zeros(n, np.int16), thr16, guard)


def _tup(s):
    return (s.message, s.call, s.loc, s.pwr, s.cycles, s.jitter, s.drift, s.sync, s.snr, s.dt, s.freq)


def _same_as_oracle(got, ref):
    """every field equal, snr to 1e-4 dB (the tolerance the decoder's own tests state)"""
    g = [_tup(x) for x in got]
    r = [_tup(x) for x in ref]
    return [t[:8] + t[9:] for t in g] == [t[:8] + t[9:] for t in r] and all(abs(a[8] - b[8]) < 1e-4 for a, b in zip(g, r))


def test_spiky_audio_to_spots(env):
    """50 bursts per second over three signals at -20 dB: through the blanker all three are decoded, the spots the oracle's
    on the checker's rows; through the plain front end none of them is."""
    torch, w, dev, stride = env
    pcm = bl.e2e_scene(50)
    items = bl.dirty_items()
    d_pcm = torch.from_numpy(np.stack((pcm, pcm))).to(dev)
    dI = torch.full((2, stride), float("nan"), dtype=torch.float32, device=dev)
    dQ = torch.full((2, stride), float("nan"), dtype=torch.float32, device=dev)
    count = np.full(1, -7, np.int32)
    w.sync_torch()
    assert w.audio_blanked_batch_device(d_pcm.data_ptr(), al.NSAMP, al.NSAMP, 1, bl.THR, bl.GUARD, dI.data_ptr(), dQ.data_ptr(),
                                        1, count) == 0
    assert w.audio_batch_device(d_pcm[1].data_ptr(), al.NSAMP, al.NSAMP, 1, dI[1].data_ptr(), dQ[1].data_ptr(), 1) == 0
    assert count[0] == bl.scene_blanked(50)[1]
    dec = w.BatchDecoder(2, 32)
    dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), NS, stride)
    for row, blanked in ((0, True), (1, False)):
        if blanked:
            assert _same_as_oracle(dec.spots(row), bl.scene_oracle(50, True))
        found = al.find_sent(dec.spots(row), items)
        print("blanker %s: %s" % ("on" if blanked else "off", [s.message for s in found if s is not None]))
        assert [s is not None for s in found] == [blanked] * 3


def test_a_blanker_call_leaves_the_decoder_as_it_was(env):
    torch, w, dev, stride = env
    I, Q, n = ol.read_iq_file(os.path.join(ol.ROOT, "tests", "golden", "refSignalSnr0dB.iq"))
    before, bi, bq = w.wspr_decode(I, Q, n)
    count = len(w.last_timings())
    rows = bl.random_rows(40000, 9)
    rc, _, _ = _device_blank(env, rows, 40000, bl.THR, bl.GUARD)
    rc2, _, _, _ = _device_fused(env, rows, 40000, bl.THR, bl.GUARD, 1)
    w.audio_to_iq_blanked(rows[1, :5000], bl.THR, bl.GUARD)
    after, ai, aq = w.wspr_decode(I, Q, n)
    assert rc == 0 and rc2 == 0 and len(before) == 1 and [_tup(s) for s in after] == [_tup(s) for s in before]
    assert np.array_equal(_bits(ai), _bits(bi)) and np.array_equal(_bits(aq), _bits(bq))
    assert len(w.last_timings()) == count == len(w.TIMING_NAMES)
