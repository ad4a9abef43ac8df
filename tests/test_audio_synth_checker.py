"""The 12 kHz audio scene synthesiser (K17) without a GPU: the serial checker (tests/helpers/audio_synth_check.cpp) against an
independent numpy formulation, its noise, its quantiser, the level convention through K12's checker and the CPU oracle, the
refusals of the library's entry points and the WAV writer."""
import ctypes as C
import math
import subprocess
import wave

import numpy as np
import pytest

import audio_lib as al
import audio_synth_lib as asl
import oracle_lib as ol
import rtlsdr_wsprd_amd as w

MSG = al.SCENE_MESSAGES[0]
F0 = [s[1] for s in al.SIGNALS]
T0S = (-1.5, 1.4, 119.0)
DRIFTS = (0.0, 3.0, -3.0)


# ---- 1. the checker against an independent formulation ---------------------------------------------------------------------
def _compare(items):
    rc, rows, count = asl.check_batch(items, 1, al.NSAMP)
    want = asl.numpy_record(items, al.NSAMP)
    assert rc == 0 and count[0] == 0
    diff = np.abs(rows[0, :al.NSAMP].astype(np.int32) - want.astype(np.int32))
    inside = sum(max(0, min(al.NSAMP, asl.first_index(it[2]) + asl.SIGLEN) - max(0, asl.first_index(it[2]))) for it in items)
    print("%d samples of frames inside the record, %d differ, largest difference %d" % (inside, int((diff != 0).sum()), int(diff.max())))
    assert np.abs(rows[0, :al.NSAMP].astype(np.int32)).max() > 7000           # the frame is there at all
    # Conditions: no sample differs by more than 1 LSB, and at most 0.001 of the samples differ at all.  A flip needs acc
    # within about 1e-6 of a half.  OBSERVED over the twelve records of the two tests below (x86-64, 80-bit longdouble):
    # 0, 2 or 3 samples of the 1.3 M of a one-transmission record differ, 3 to 5 of the 2.6 M of a three-transmission record
    # (21 in all), each by 1 LSB; profiles/audio_synth.json carries the same counts.
    assert diff.max() <= 1
    assert (diff != 0).sum() <= 0.001 * al.NSAMP
    return int((diff != 0).sum())


@pytest.mark.parametrize("drift", DRIFTS)
@pytest.mark.parametrize("t0", T0S)
def test_one_transmission_equals_numpy(t0, drift):
    _compare([asl.item(0, MSG[0], F0[0], t0, 8000.0, drift)])


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_three_transmissions_equal_numpy(shift):
    """The three offsets of audio_lib.SIGNALS; frames hang off the front (t0 = -1.5 s) and the end (119.0 s) of the record."""
    _compare([asl.item(0, MSG[j], F0[j], T0S[(j + shift) % 3], 8000.0, DRIFTS[(j + 2 * shift) % 3]) for j in range(3)])


def test_first_index_floors_and_clamps():
    assert [asl.first_index(t) for t in (0.0, 2.0, -1.5, 1.4, 119.0)] == \
        [0, 24000, -18000, math.floor(float(np.float32(1.4)) * 12000.0), 1428000]
    assert asl.first_index(-1e-5) == -1 and asl.first_index(1e9) == 4000000 and asl.first_index(-1e9) == -4000000
    rc, rows, count = asl.check_batch([asl.item(0, MSG[0], 0.0, 1e9, 8000.0), asl.item(0, MSG[0], 0.0, -1e9, 8000.0)], 1, 4096)
    assert rc == 0 and not rows[0, :4096].any()              # both frames miss the record


# ---- 2. the noise ----------------------------------------------------------------------------------------------------------
SIGMA = 1000.0


@pytest.fixture(scope="module")
def noise_record():
    rc, rows, count = asl.check_batch([], 1, al.NSAMP, seg_index0=3, sigma=SIGMA, seed=0x1234567890ABCDEF)
    assert rc == 0 and count[0] == 0
    return rows[0, :al.NSAMP].astype(np.float64)


def test_noise_moments(noise_record):
    """N = 1 440 000 independent N(0, sigma^2) samples (rounded to integers: + 1/12 of variance, 8e-8 of sigma^2).  Standard
    errors: mean sigma/sqrt(N) = 0.833; variance sigma^2 sqrt(2/N) = 1178.5 (the fourth moment of a Gaussian is 3 sigma^4);
    autocorrelation coefficient at a lag k > 0 of white noise 1/sqrt(N) = 8.33e-4.  Each bound is 5 standard errors."""
    x, n = noise_record, float(al.NSAMP)
    mean, var = x.mean(), x.var()
    r1 = np.dot(x[:-1], x[1:]) / (n * var)
    r2 = np.dot(x[:-2], x[2:]) / (n * var)
    print("mean %+.3f (5 se %.3f)  var %.1f (sigma^2 +- %.1f)  r1 %+.2e  r2 %+.2e (5 se %.2e)"
          % (mean, 5 * SIGMA / math.sqrt(n), var, 5 * SIGMA ** 2 * math.sqrt(2 / n), r1, r2, 5 / math.sqrt(n)))
    assert abs(mean) <= 5.0 * SIGMA / math.sqrt(n)
    assert abs(var - (SIGMA ** 2 + 1.0 / 12.0)) <= 5.0 * SIGMA ** 2 * math.sqrt(2.0 / n)
    assert abs(r1) <= 5.0 / math.sqrt(n) and abs(r2) <= 5.0 / math.sqrt(n)
    # the two halves of a draw are independent as well: the correlation WITHIN the pairs alone (N/2 products: 5 sqrt(2/N))
    rp = np.dot(x[0::2], x[1::2]) / (n / 2 * var)
    assert abs(rp) <= 5.0 * math.sqrt(2.0 / n)


def test_samples_2m_and_2m_plus_1_come_from_one_draw(noise_record):
    """Against the shared header's draw, exactly; and against Philox and Box-Muller restated in numpy in float64.  The
    contract rounds the angle to float32 (half an ulp below 2 pi: 2.4e-7 rad, times a radius of at most 9.4 sigma: 2.3e-3)
    and the radius and the products to float32 (6e-8 each of at most 9 400: 1.7e-3); the quantiser adds at most 0.5."""
    for m in (0, 1, 2, 4095, 4096, 719999):
        a, b = asl.gauss(0x1234567890ABCDEF, 3, m, SIGMA)
        q, _ = asl.quantise([a, b])
        assert noise_record[2 * m] == q[0] and noise_record[2 * m + 1] == q[1], m
    m = np.arange(0, 65536)
    a, b = asl.philox_pairs(0x1234567890ABCDEF, 3, m)
    assert np.abs(noise_record[2 * m] - SIGMA * a).max() <= 0.5 + 4e-3
    assert np.abs(noise_record[2 * m + 1] - SIGMA * b).max() <= 0.5 + 4e-3
    # an odd length ends on the first half of a draw
    rc, rows, _ = asl.check_batch([], 1, 4097, seg_index0=3, sigma=SIGMA, seed=0x1234567890ABCDEF)
    assert rc == 0 and np.array_equal(rows[0, :4097], noise_record[:4097].astype(np.int16))


def test_a_records_noise_does_not_depend_on_the_split():
    n = 5003
    items = [asl.item(5, MSG[1], F0[1], -0.2, 3000.0, 1.0)]
    rc8, rows8, c8 = asl.check_batch(items, 8, n, seg_index0=0, sigma=SIGMA, seed=77)
    rc1, rows1, c1 = asl.check_batch([asl.item(0, MSG[1], F0[1], -0.2, 3000.0, 1.0)], 1, n, seg_index0=5, sigma=SIGMA, seed=77)
    assert rc8 == 0 and rc1 == 0
    assert np.array_equal(rows1[0, :n], rows8[5, :n]) and c1[0] == c8[5]
    assert not np.array_equal(rows8[4, :n], rows8[5, :n]) and rows8[4, :n].any()     # other records differ
    rc, other, _ = asl.check_batch([], 1, n, seg_index0=5, sigma=SIGMA, seed=78)
    assert rc == 0 and not np.array_equal(other[0, :n], rows8[5, :n])                # and so does another seed


# ---- 3. the quantiser --------------------------------------------------------------------------------------------------------
def test_quantiser_on_crafted_values():
    eps = 2.0 ** -37                                          # one ulp of a double at 32767
    acc = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, 2.5000000000000004, 32766.5, 32767.0, 32767.0 + eps,
           32767.4, 1e6, -32767.5, -32768.0, -32768.0 - eps, -32768.4, -1e6, 7.0, -7.0]
    want = [0, 2, 2, 0, -2, -2, 0, 3, 32766, 32767, 32767, 32767, 32767, -32768, -32768, -32768, -32768, -32768, 7, -7]
    out, clipped = asl.quantise(acc)
    assert out.tolist() == want and clipped == 6


def _one_sample(pcm, amp):
    """acc = pcm + amp * cos(0) at the single sample of a record: (sample, clipped)."""
    rc, rows, count = asl.check_batch([asl.item(0, MSG[0], 0.0, 0.0, amp)], 1, 1, flags=asl.ACCUMULATE,
                                      rows=np.array([[pcm, 11, 12, 13, 14, 15, 16, 17]], np.int16))
    assert rc == 0 and rows[0, 1:].tolist() == [11, 12, 13, 14, 15, 16, 17]      # ACCUMULATE: the padding keeps what it held
    return int(rows[0, 0]), int(count[0])


def test_quantisation_through_accumulate():
    """sigma = 0; the frame's sample 0 has phi = 0.0 and cos = 1.0 exactly, so acc = pcm[0] + amp."""
    assert _one_sample(2, 0.5) == (2, 0) and _one_sample(3, 0.5) == (4, 0)       # ties round to even
    assert _one_sample(-3, 0.5) == (-2, 0) and _one_sample(-2, -0.5) == (-2, 0) and _one_sample(0, -1.5) == (-2, 0)
    assert _one_sample(32767, 0.0) == (32767, 0)                                 # 32767.0 does not clip
    assert _one_sample(32767, -0.5) == (32766, 0)
    assert _one_sample(32767, 2.0 ** -20) == (32767, 1)                          # just above: clipped and counted
    assert _one_sample(32767, 0.25) == (32767, 1)
    assert _one_sample(-32768, 0.0) == (-32768, 0)
    assert _one_sample(-32768, -2.0 ** -20) == (-32768, 1)
    assert _one_sample(-32768, -1e6) == (-32768, 1) and _one_sample(0, 1e6) == (32767, 1)


def test_clip_count_is_exact():
    """Eleven samples at 32767 under a transmission of amplitude 0.25: every sample with cos(phi) > 0 clips.  The phases are
    multiples of about pi/4, taken here from numpy; none lies within 1e-3 of a zero of the cosine."""
    n = 11
    sym = asl.symbols(MSG[0])
    phi = np.arange(n) * (2.0 * np.pi / 12000.0) * (1500.0 + (sym[0] - 1.5) * 12000.0 / 8192.0)
    assert np.abs(np.cos(phi)).min() > 1e-3
    rc, rows, count = asl.check_batch([asl.item(0, MSG[0], 0.0, 0.0, 0.25)], 1, n, flags=asl.ACCUMULATE,
                                      rows=np.full((1, 16), 32767, np.int16))
    assert rc == 0 and count[0] == int((np.cos(phi) > 0).sum()) and 0 < count[0] < n
    assert rows[0].tolist() == [32767] * 16
    # without ACCUMULATE the prepared row is ignored and the padding up to roundup8 is zeroed
    rc, rows, count = asl.check_batch([asl.item(0, MSG[0], 0.0, 0.0, 0.25)], 1, n, rows=np.full((1, 24), 32767, np.int16))
    assert rc == 0 and count[0] == 0 and rows[0].tolist() == [0] * 16 + [32767] * 8


def test_checker_under_the_sanitizers(tmp_path):
    """The checker as a stand-alone program under AddressSanitizer and UBSan: frames hanging off both ends, an odd length."""
    r = subprocess.run([asl.sanitizer_program(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == "0", r.stderr[-2000:]


# ---- 4. the level convention -----------------------------------------------------------------------------------------------
def test_audio_amp_is_the_convention():
    for snr in al.SCENE_SNRS:
        assert w.audio_amp(snr, asl.SIGMA) == pytest.approx(asl.amp_of(snr, asl.SIGMA), rel=1e-12)
    # audio_lib.audio_scene(): amplitude sqrt(2) 10^(snr/20) over noise of variance 2.4, both times 2000
    assert w.audio_amp(-20.0, asl.SIGMA) == pytest.approx(2000.0 * math.sqrt(2.0) * 0.1, rel=1e-12)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_scenes_at_audio_amp_levels_decode_in_the_oracle(k):
    """audio_lib's three scenes built by the synthesiser with audio_amp(), through K12's checker and the CPU oracle: the
    tolerances are those tests/test_audio_checker.py states for audio_scene()'s records."""
    items = al.scene_items(k)
    pcm, clipped = asl.scene(k)
    assert clipped == 0
    found = al.find_sent(asl.scene_oracle(k), items)
    for s, (msg, snr, f0, t0) in zip(found, items):
        assert s is not None, msg
        print("%-16s snr %+.2f (sent %+.1f)  f %+.3f Hz  dt %+.3f s" % (msg, s.snr, snr, al.spot_offset_hz(s) - f0, s.dt - (t0 - 2.0)))
        assert abs(al.spot_offset_hz(s) - f0) <= 0.15
        assert abs(s.dt - (t0 - 2.0)) <= 0.1
        assert abs(s.snr - snr) <= 0.5


# ---- 5. the library's refusals and the WAV writer ------------------------------------------------------------------------------
def _tx(**kw):
    d = dict(seg=0, f0=10.0, t0=1.0, amp=100.0, drift=0.0, sym=asl.symbols(MSG[0]))
    d.update(kw)
    return (d["seg"], d["f0"], d["t0"], d["amp"], d["drift"], d["sym"])


BAD_SYMBOLS = tuple([4] + [0] * 161)
REFUSALS = [   # (name, transmissions, call arguments that differ from a good call, code)
    ("symbol above 3", [_tx(sym=BAD_SYMBOLS)], {}, -1),
    ("seg negative", [_tx(seg=-1)], {}, -1),
    ("seg outside the batch", [_tx(seg=2)], {}, -1),
    ("unsorted list", [_tx(seg=1), _tx(seg=0)], {}, -1),
    ("negative ntx", [_tx()], dict(ntx=-1), -1),
    ("negative nseg", [], dict(nseg=-1), -1),
    ("negative nsamp", [_tx()], dict(nsamp=-1), -1),
    ("f0 not finite", [_tx(f0=float("nan"))], {}, -1),
    ("t0 not finite", [_tx(t0=float("inf"))], {}, -1),
    ("amp not finite", [_tx(amp=float("-inf"))], {}, -1),
    ("drift not finite", [_tx(drift=float("nan"))], {}, -1),
    ("sigma not finite", [_tx()], dict(sigma=float("nan")), -1),
    ("sigma infinite", [_tx()], dict(sigma=float("inf")), -1),
    ("sigma negative", [_tx()], dict(sigma=-1.0), -1),
    ("sigma above 1e6", [_tx()], dict(sigma=1.5e6), -1),
    ("amp above 1e6", [_tx(amp=-1.5e6)], {}, -1),
    ("f0 above 800 Hz", [_tx(f0=800.5)], {}, -1),
    ("f0 and drift above 800 Hz", [_tx(f0=-700.0, drift=201.0)], {}, -1),
    ("flag bit 1", [_tx()], dict(flags=2), -1),
    ("flag bits 0 and 1", [_tx()], dict(flags=3), -1),
    ("flag sign bit", [_tx()], dict(flags=-2147483648), -1),
    ("record above 120 s", [_tx()], dict(nsamp=1440001, stride=1440008), -2),
]
DEVICE_REFUSALS = [
    ("misaligned by 2", [_tx()], dict(offset=2), -1),
    ("misaligned by 8", [_tx()], dict(offset=8), -1),
    ("no rows", [_tx()], dict(null=True), -1),
    ("stride no multiple of 8", [_tx()], dict(stride=4100), -1),
    ("stride below nsamp", [_tx()], dict(stride=4088), -1),
]


def _call_batch(txs, ntx=None, nseg=2, nsamp=4096, sigma=10.0, flags=0, stride=4096, offset=0, null=False, rows=None):
    """wspr_synth_audio_batch_device() on HOST memory standing in for device rows: a refused call never touches them."""
    rows = np.full((2, 4200), 0x1234, np.int16) if rows is None else rows
    count = np.full(4, -7, np.int32)
    arr = w.synth_tx_list(txs)
    rc = w.lib().wspr_synth_audio_batch_device(C.addressof(arr), len(txs) if ntx is None else ntx, nseg, 0, nsamp, sigma, 9, flags,
                                              None if null else rows.ctypes.data + offset, stride, count.ctypes.data)
    return rc, rows, count


@pytest.mark.parametrize("name,txs,kw,code", REFUSALS + DEVICE_REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS + DEVICE_REFUSALS])
def test_batch_call_refuses_and_writes_nothing(name, txs, kw, code, capfd):
    rc, rows, count = _call_batch(txs, **kw)
    assert rc == code, name
    assert (rows == 0x1234).all() and (count == -7).all()
    assert "wspr_synth_audio_batch_device" in capfd.readouterr().err


@pytest.mark.parametrize("name,txs,kw,code", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_host_call_refuses_and_writes_nothing(name, txs, kw, code, capfd):
    if "nseg" in kw or any(t[0] > 0 for t in txs):
        txs, kw, code = [_tx(seg=1)], {}, -1                   # the host call has one record: seg 1 is outside it
    pcm = np.full(4200, 0x1234, np.int16)
    count = C.c_int(-7)
    arr = w.synth_tx_list(txs)
    rc = w.lib().wspr_synth_audio(C.addressof(arr), kw.get("ntx", len(txs)), kw.get("nsamp", 4096), kw.get("sigma", 10.0), 9,
                                  kw.get("flags", 0), pcm.ctypes.data, C.addressof(count))
    assert rc == code, name
    assert (pcm == 0x1234).all() and count.value == -7
    assert "wspr_synth_audio" in capfd.readouterr().err
    if code == -2:
        with pytest.raises(RuntimeError):
            w.synth_audio(txs, nsamp=1440001)


def test_device_entry_points_fail_loudly_without_gpu():
    """No CPU fallback: a good call on a box without a HIP device returns -1 and writes nothing."""
    if w.lib().wspr_device_ready() == 1:
        pytest.skip("a GPU is present")
    rc, rows, count = _call_batch([_tx()])
    assert rc == -1 and (rows == 0x1234).all() and (count == -7).all()
    rc, rows, count = _call_batch([], nseg=0)
    assert rc == -1 and (count == -7).all()
    pcm = np.full(4096, 0x1234, np.int16)
    count = C.c_int(-7)
    arr = w.synth_tx_list([_tx()])
    assert w.lib().wspr_synth_audio(C.addressof(arr), 1, 4096, 10.0, 9, 0, pcm.ctypes.data, C.addressof(count)) == -1
    assert (pcm == 0x1234).all() and count.value == -7
    with pytest.raises(RuntimeError):
        w.synth_audio([_tx()], nsamp=4096)


@pytest.mark.parametrize("nsamp", [0, 1, 7, 4097, 120001])
def test_wav_writer_round_trip(tmp_path, nsamp):
    pcm = np.random.default_rng(nsamp).integers(-32768, 32768, nsamp).astype(np.int16)
    if nsamp > 1:
        pcm[0], pcm[1] = -32768, 32767
    path = tmp_path / "out.wav"
    w.write_wav_file(path, pcm)
    back = w.read_wav_file(path)
    assert back.dtype == np.int16 and back.tobytes() == pcm.tobytes()           # byte for byte
    with wave.open(str(path), "rb") as f:                                        # and a file other readers take as well
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 12000, nsamp)
        assert f.readframes(nsamp) == pcm.astype("<i2").tobytes()
    ref = tmp_path / "ref.wav"
    al.write_wav(ref, pcm)
    assert path.read_bytes() == ref.read_bytes()                                 # the canonical 44-byte header
    assert w.lib().wspr_write_wav_file(str(tmp_path / "no" / "such" / "dir.wav").encode(), pcm.ctypes.data, nsamp) == -1
