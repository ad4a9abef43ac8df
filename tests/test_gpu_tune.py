"""The tunable multi-band front end (K21) through the C ABI: rows bit for bit the serial checker's
(tests/helpers/tune_check.c) at every length around a block and the filter's start-up, for band counts around the kernel's band
tile, several segments, the exact and the extreme steps, clipped bytes, duplicates and both normalise settings; the host entry
point; the refusals; and one full-length capture with two bands decoded end to end beside the K0 path."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import synth
import tune_lib as tl

pytestmark = pytest.mark.gpu

BLK = tl.BLOCK_BYTES
LENGTHS = [0, 8, 6392, 6400, 6408, 6400 * 37, 6400 * 40 + 3208]       # samples; 37: the first output with a full FIR history
EDGE_STEPS = [0, 1 << 30, 3 << 30, 1 << 31, 1, (1 << 32) - 1]


@pytest.fixture(scope="module")
def env():
    import torch
    import rtlsdr_wsprd_amd as w
    assert w.lib().wspr_device_ready() == 1
    torch.cuda.set_device(0)
    assert int(w.lib().wspr_iq_stride()) == tl.STRIDE
    return torch, w, torch.device("cuda", 0)


def _odd_steps(n, seed):
    return [int(x) | 1 for x in np.random.default_rng(seed).integers(0, 1 << 32, n)]


def _device(env, raw, steps, normalise=0, **kw):
    """wspr_tune_u8_batch_device() on a device copy of raw [nseg, bytes_per_seg]: (rc, I, Q [rows + 1, stride] afterwards,
    pre-filled with NaN; the extra row must stay NaN)."""
    torch, w, dev = env
    nseg, bps = raw.shape
    nb = len(steps) if steps is not None else 1
    rows = nseg * min(nb, tl.MAX_BANDS) + 1
    d = torch.from_numpy(np.ascontiguousarray(raw).ravel()).to(dev) if raw.size else torch.zeros(16, dtype=torch.uint8, device=dev)
    dI = torch.full((rows, tl.STRIDE), float("nan"), device=dev)
    dQ = torch.full((rows, tl.STRIDE), float("nan"), device=dev)
    w.sync_torch()
    if "nbands" in kw:                                                    # the raw call: a count that is not len(steps)
        st = np.ascontiguousarray(steps, np.uint32)
        rc = w.lib().wspr_tune_u8_batch_device(d.data_ptr(), bps, nseg, ol.ptr(st), kw["nbands"], dI.data_ptr(), dQ.data_ptr(), normalise)
    else:
        rc = w.tune_u8_batch_device(d.data_ptr() + kw.get("raw_offset", 0), kw.get("bytes_per_seg", bps), kw.get("nseg", nseg), steps,
                                    dI.data_ptr() + kw.get("i_offset", 0), dQ.data_ptr(), normalise)
    return rc, dI.cpu().numpy(), dQ.cpu().numpy()


def _both(env, raw, steps, normalise=0):
    """The device and the checker on the same rows: asserts that every float of every row is the same bit pattern."""
    rc, gI, gQ = _device(env, raw, steps, normalise)
    crc, wI, wQ, n = tl.check_rows(raw, steps, normalise)
    assert rc == 0 and crc == 0
    rows = wI.shape[0]
    bad = int((gI[:rows].view(np.uint32) != wI.view(np.uint32)).sum() + (gQ[:rows].view(np.uint32) != wQ.view(np.uint32)).sum())
    print("%d x %d bytes, %d bands, normalise %d: %d of %d floats differ" % (raw.shape + (len(steps), normalise, bad, 2 * wI.size)))
    assert bad == 0
    assert np.isnan(gI[rows]).all() and np.isnan(gQ[rows]).all()           # nothing behind the last row
    return gI[:rows], gQ[:rows], n


def test_taps_are_the_fixtures(env):
    _, w, _ = env
    t = np.zeros(33, np.float32)
    r = C.c_int(0)
    w.lib().wspr_front_end_constants(ol.ptr(t), C.byref(r))
    assert np.array_equal(t.view(np.uint32), tl.taps().view(np.uint32))


@pytest.mark.parametrize("nsamp", LENGTHS)
def test_lengths_equal_the_checker(env, nsamp):
    raw = tl.random_bytes(1, 2 * nsamp, 500 + nsamp % 89)
    gI, gQ, n = _both(env, raw, [0x12345677, 1 << 30])
    assert (n == nsamp // 6400).all() and not gI[:, nsamp // 6400:].any() and not gQ[:, nsamp // 6400:].any()
    if nsamp >= 6400:
        assert gI[:, :nsamp // 6400].any() and not np.array_equal(gI[0], gI[1])


@pytest.mark.parametrize("nbands", [1, 2, tl.TILE + 1, 16])
@pytest.mark.parametrize("normalise", [0, 1])
def test_band_counts_and_steps_equal_the_checker(env, nbands, normalise):
    """1, 2, one more than the band tile, and 16 bands: the exact steps, the smallest and the largest, odd random ones."""
    steps = (EDGE_STEPS + _odd_steps(10, 7))[:nbands] if nbands > 2 else ([0x9e3779b1, 3 << 30][:nbands])
    raw = tl.random_bytes(1, 9 * BLK + 48, 40 + nbands)
    gI, gQ, _ = _both(env, raw, steps, normalise)
    if normalise:
        assert all(abs(max(np.abs(gI[b]).max(), np.abs(gQ[b]).max()) - 0.5) <= 2.0 ** -24 for b in range(nbands))   # peak * float(0.5 / peak)


@pytest.mark.parametrize("nseg", [1, 3])
def test_segments_with_a_stride_beyond_the_used_length(env, nseg):
    """bytes_per_seg = 5 blocks + 3216 bytes that belong to no output; seven bands = two passes, the second not full."""
    raw = tl.random_bytes(nseg, 5 * BLK + 3216, 60 + nseg)
    gI, _, n = _both(env, raw, EDGE_STEPS[1:5] + _odd_steps(3, 8))
    assert (n == 5).all()
    if nseg == 3:
        assert not np.array_equal(gI[0], gI[7]) and not np.array_equal(gI[7], gI[14])


def test_clipped_bytes_equal_the_checker(env):
    raw = tl.random_bytes(2, 38 * BLK, 71, clipped=True)
    raw[1, 3 * BLK - 64:3 * BLK + 64] = 0x00                                # a run across a block edge, another of 0xff
    raw[1, 7 * BLK - 32:7 * BLK + 96] = 0xff
    raw[0, :BLK] = 0x00                                                     # a whole block at the negative rail
    _both(env, raw, [1 << 30, 0x0badf00d | 1, (1 << 32) - 1])


def test_a_band_listed_twice_gives_identical_rows(env):
    raw = tl.random_bytes(2, 6 * BLK, 81)
    steps = [0x13579bdf, 1 << 30, 0x13579bdf, 5, 7, 0x13579bdf]             # in one tile, and across two
    gI, gQ, _ = _both(env, raw, steps)
    for s in range(2):
        for b in (2, 5):
            assert np.array_equal(gI[6 * s].view(np.uint32), gI[6 * s + b].view(np.uint32))
            assert np.array_equal(gQ[6 * s].view(np.uint32), gQ[6 * s + b].view(np.uint32))


def test_one_call_equals_one_call_per_band(env):
    raw = tl.random_bytes(2, 4 * BLK, 91)
    steps = _odd_steps(6, 3)
    rc, aI, aQ = _device(env, raw, steps)
    assert rc == 0
    for b, st in enumerate(steps):
        rc, oI, oQ = _device(env, raw, [st])
        assert rc == 0
        for s in range(2):
            assert np.array_equal(aI[6 * s + b].view(np.uint32), oI[s].view(np.uint32))
            assert np.array_equal(aQ[6 * s + b].view(np.uint32), oQ[s].view(np.uint32))


def test_host_entry_point_equals_the_checker(env):
    _, w, _ = env
    raw = tl.random_bytes(1, 3 * BLK + 3208 * 2 + 6, 95)[0]                 # not a multiple of 16: any length is taken
    steps = _odd_steps(5, 4)
    for normalise in (0, 1):
        I, Q, n = w.tune_u8(raw[1:], steps, normalise)                     # and any alignment
        crc, wI, wQ, wn = tl.check_rows(raw[1:1 + ((raw.size - 1) & ~15)], steps, normalise)
        assert crc == 0 and n == 3 == wn[0]
        assert np.array_equal(I.view(np.uint32), wI[:, :45000].view(np.uint32)) and np.array_equal(Q.view(np.uint32), wQ[:, :45000].view(np.uint32))
    I, Q, n = w.tune_u8(raw[:100], steps)
    assert n == 0 and not I.any() and not Q.any()


def test_refusals_write_nothing(env, capfd):
    raw = tl.random_bytes(2, 2 * BLK, 9)
    cases = [dict(nseg=-1), dict(steps=None), dict(nbands=0), dict(nbands=17), dict(bytes_per_seg=2 * BLK - 8), dict(raw_offset=8),
             dict(i_offset=4)]
    for kw in cases:
        steps = kw.pop("steps", list(range(1, 18)) if "nbands" in kw else [1, 2])
        rc, I, Q = _device(env, raw, steps, **kw)
        assert rc == -1 and np.isnan(I).all() and np.isnan(Q).all(), kw
        assert "wspr_tune_u8_batch_device" in capfd.readouterr().err
    rc, I, Q = _device(env, raw, [1, 2], nseg=0)
    assert rc == 0 and np.isnan(I).all() and np.isnan(Q).all()
    rc, I, Q = _device(env, tl.random_bytes(2, 12784, 9), [1, 2])          # shorter than a block: rows of zeros
    assert rc == 0 and not I[:4].any() and not Q[:4].any() and np.isnan(I[4]).all()


def test_two_bands_of_one_full_length_capture_decode_end_to_end(env):
    """One 576 MB capture made on the device: message A at -600 kHz, message B at +412 345 Hz, 10 LSB of noise.  The two tuned rows
    decode to A alone and B alone; row 0's spot has the call, locator and power of the K0 -> decode path on the same bytes and
    its frequency within 0.1 Hz (K0's 6401 stretches its axis by 1.6e-4); dt and SNR are recorded, dt within 0.1 s."""
    torch, w, dev = env
    msgs = [synth.message_for(11), synth.message_for(202)]
    assert msgs[0] != msgs[1]
    step_b, realised_b = w.tune_step(412345.0)
    raw = tl.synth_two_bands_gpu(torch, dev, w, msgs, f0s=[37.5, -61.25], t0s=[2.0, 1.5], step_b=step_b, seed=5, amp_lsb=0.15)
    dI = torch.zeros(3, tl.STRIDE, device=dev)
    dQ = torch.zeros(3, tl.STRIDE, device=dev)
    w.sync_torch()
    assert w.tune_u8_batch_device(raw.data_ptr(), raw.numel(), 1, [1 << 30, step_b], dI.data_ptr(), dQ.data_ptr(), 1) == 0
    assert w.lib().wspr_decimate_u8_batch_device(raw.data_ptr(), raw.numel(), 1, dI[2].data_ptr(), dQ[2].data_ptr(), 1) == 0
    dec = w.BatchDecoder(3)
    dec.decode_ptr(dI.data_ptr(), dQ.data_ptr(), 45000, tl.STRIDE)
    texts = [[s.message.decode().strip() for s in dec.spots(r)] for r in range(3)]
    print(texts)
    assert texts[0] == [synth.expected_text(msgs[0])] and texts[1] == [synth.expected_text(msgs[1])] and texts[2] == texts[0]
    a, b, k0 = dec.spots(0)[0], dec.spots(1)[0], dec.spots(2)[0]
    assert (a.call, a.loc, a.pwr) == (k0.call, k0.loc, k0.pwr)
    df_hz = (a.freq - k0.freq) * 1e6
    tl.record("end_to_end", message_a=texts[0][0], message_b=texts[1][0], offset_b_hz=realised_b,
            row0=dict(freq_mhz=a.freq, dt=a.dt, snr=a.snr), row1=dict(freq_mhz=b.freq, dt=b.dt, snr=b.snr),
            k0=dict(freq_mhz=k0.freq, dt=k0.dt, snr=k0.snr), delta_f_hz=df_hz, delta_dt_s=a.dt - k0.dt, delta_snr_db=a.snr - k0.snr)
    assert abs(df_hz) <= 0.1
    assert abs(a.dt - k0.dt) <= 0.1
