"""The 12 kHz audio front end (K12) on the CPU: the committed tap tables, the serial checker
(tests/helpers/audio_check.c over rtlsdr-wsprd_amd/csrc/kernels/audio_front.h) and the WAV reader.  No GPU."""
import importlib.util
import os
import struct

import numpy as np
import pytest

import audio_lib as al
import oracle_lib as ol
import rtlsdr_wsprd_amd as w

K = 255


def _gen():
    spec = importlib.util.spec_from_file_location("gen_audio_taps", os.path.join(ol.ROOT, "tools", "gen_audio_taps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ulps(a, b):
    """Distance in float32 ulps between equal-signed (or zero) values."""
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


# ---- the tables -----------------------------------------------------------------------------------------------------
def test_tables_are_the_generators_output_and_have_the_stated_symmetries():
    gi, gq = al.taps()
    ti, tq = _gen().taps()
    assert _ulps(gi, ti).max() <= 1 and _ulps(gq, tq).max() <= 1
    k = np.arange(-K, K + 1)
    assert np.array_equal(gi[::-1].view(np.uint32), gi.view(np.uint32))                 # gI[-k] == gI[k]
    assert np.array_equal(gq[::-1], -gq)                                                # gQ[-k] == -gQ[k] (as values)
    assert gq[K].view(np.uint32) == 0                                                   # gQ[0] == +0
    zi, zq = (k % 8 == 2) | (k % 8 == 6), (k % 8 == 0) | (k % 8 == 4)
    assert not gi.view(np.uint32)[zi].any() and not gq.view(np.uint32)[zq].any()        # +0.0f, bit for bit
    assert np.all(gi[~zi] != 0) and np.all(gq[~zq] != 0)


def test_library_hands_out_the_same_tables():
    gi, gq = al.taps()
    li, lq, r = w.audio_constants()
    assert r == 32 and np.array_equal(li.view(np.uint32), gi.view(np.uint32))
    assert np.array_equal(lq.view(np.uint32), gq.view(np.uint32))


def test_frequency_response_of_the_committed_taps():
    """The complex filter gI + j gQ, shifted back by 1 500 Hz, in float64 on a 0.25 Hz grid."""
    gi, gq = al.taps()
    k = np.arange(-K, K + 1, dtype=np.float64)
    g = (gi.astype(np.float64) + 1j * gq.astype(np.float64)) * np.exp(2j * np.pi * 1500.0 * k / al.RATE) / 2.0

    def db(f):      # response to audio at 1500 + f
        H = np.exp(-2j * np.pi * np.outer(f, k) / al.RATE) @ np.conj(g)
        return 20.0 * np.log10(np.maximum(np.abs(H), 1e-300))

    for sign in (1.0, -1.0):
        p = db(sign * np.arange(0.0, 110.0001, 0.25))
        assert p.max() <= 0.005 and p.min() >= -0.005, (p.max(), p.min())
        assert db(sign * np.arange(0.0, 150.0001, 0.25)).min() >= -0.5
    stop = np.concatenate((np.arange(265.0, 6000.0001, 0.25), -np.arange(265.0, 6000.0001, 0.25)))
    worst = max(db(stop[i:i + 4096]).max() for i in range(0, stop.size, 4096))
    assert worst <= -80.0, worst


# ---- the checker ----------------------------------------------------------------------------------------------------
def test_checker_against_numpy_on_a_full_scale_record():
    rng = np.random.default_rng(12)
    pcm = rng.integers(-32768, 32768, al.NSAMP).astype(np.int16)
    I, Q = al.check_rows(pcm)
    gi, gq = al.taps()
    x = pcm.astype(np.float64) / 32768.0
    for got, g in ((I[0], gi), (Q[0], gq)):
        full = np.convolve(x, g.astype(np.float64)[::-1])            # full[n + 255] = sum_k g[k] x[n + k]
        want = full[K::32][:al.NOUT]
        rms = np.sqrt(np.mean(want ** 2))
        assert np.abs(got.astype(np.float64) - want).max() <= 1e-5 * rms


@pytest.mark.parametrize("nsamp", [1000, 1440000])
def test_impulses_come_out_as_the_table(nsamp):
    pcm, ei, eq = al.impulse_rows(nsamp)
    I, Q = al.check_rows(pcm)
    assert np.array_equal(I.view(np.uint32), ei.view(np.uint32))
    assert np.array_equal(Q.view(np.uint32), eq.view(np.uint32))


def test_lengths_and_row_tail():
    pcm = np.full(100, 1000, np.int16)
    I, Q = al.check_rows(pcm, nsamp=33, out_stride=45056)
    assert I.shape == (1, 45056) and np.all(I[0, 2:] == 0) and np.all(Q[0, 2:] == 0) and I[0, 0] != 0 and I[0, 1] != 0
    short, _ = al.check_rows(pcm[:33], out_stride=45056)
    assert np.array_equal(short.view(np.uint32), I.view(np.uint32))          # what lies beyond nsamp is not read
    I0, Q0 = al.check_rows(pcm, nsamp=0)
    assert not I0.view(np.uint32).any() and not Q0.view(np.uint32).any()
    chk = al.checker()
    out = np.zeros((1, al.NOUT), np.float32)
    big = np.zeros(8, np.int16)
    assert chk.audio_check_rows(ol.ptr(big), 1440008, 1440001, 0, ol.ptr(out), ol.ptr(out), al.NOUT, 0) == -2


def test_upper_sideband_and_timing():
    """A cosine at 1500 + 37 Hz comes out as a unit phasor at +37 Hz, Q leading I's zero crossings (e^{+j 2 pi f t})."""
    n = np.arange(240000)
    pcm = np.rint(16384.0 * np.cos(2.0 * np.pi * 1537.0 * n / al.RATE)).astype(np.int16)
    I, Q = al.check_rows(pcm)
    z = (I[0, 100:7000].astype(np.float64) + 1j * Q[0, 100:7000].astype(np.float64))
    assert abs(np.abs(z).mean() - 0.5) < 1e-3
    step = np.angle(z[1:] * np.conj(z[:-1]))
    assert np.abs(step * 375.0 / (2.0 * np.pi) - 37.0).max() < 0.01
    m = np.arange(100, 7000)
    want = 0.5 * np.exp(2j * np.pi * 37.0 * m / 375.0)                  # output m is centred on input sample 32 m: no delay
    assert np.abs(z - want).max() < 2e-3


def test_a_transmission_at_two_seconds_reports_zero_dt():
    spots = al.scene_oracle(0, 1)
    s = al.find_sent(spots, al.scene_items(0))[0]
    assert al.scene_items(0)[0][3] == 2.0 and s is not None and abs(s.dt) <= 0.1


@pytest.mark.parametrize("normalise", [0, 1])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_scenes_decode_in_the_oracle(k, normalise):
    items = al.scene_items(k)
    found = al.find_sent(al.scene_oracle(k, normalise), items)
    for s, (msg, snr, f0, t0) in zip(found, items):
        assert s is not None, msg
        print("%-16s snr %+.2f (sent %+.1f)  f %+.3f Hz  dt %+.3f s" % (msg, s.snr, snr, al.spot_offset_hz(s) - f0, s.dt - (t0 - 2.0)))
        assert abs(al.spot_offset_hz(s) - f0) <= 0.15
        assert abs(s.dt - (t0 - 2.0)) <= 0.1
        assert abs(s.snr - snr) <= 0.5


# ---- the WAV reader -------------------------------------------------------------------------------------------------
def _chunk(tag, body):
    return tag + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def _fmt(tag=1, channels=1, rate=12000, bits=16):
    return struct.pack("<HHIIHH", tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)


def _riff(*chunks):
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def test_wav_round_trip(tmp_path):
    pcm = np.random.default_rng(3).integers(-32768, 32768, 5000).astype(np.int16)
    al.write_wav(tmp_path / "a.wav", pcm)
    assert np.array_equal(w.read_wav_file(tmp_path / "a.wav"), pcm)
    assert np.array_equal(w.read_wav_file(tmp_path / "a.wav", cap=1234), pcm[:1234])       # cap smaller than the file
    assert w.read_wav_file(tmp_path / "missing.wav").size == 0


def test_wav_chunks_are_walked(tmp_path):
    pcm = np.arange(-300, 300, dtype=np.int16)
    data = pcm.tobytes()
    p = tmp_path / "b.wav"
    p.write_bytes(_riff(_chunk(b"fmt ", _fmt()), _chunk(b"LIST", b"INFOISFT" + b"x" * 20), _chunk(b"odd ", b"abc"),
                        _chunk(b"data", data)))
    assert np.array_equal(w.read_wav_file(p), pcm)
    p.write_bytes(_riff(_chunk(b"fmt ", _fmt() + b"\0\0"), _chunk(b"data", data)))          # fmt with an extension
    assert np.array_equal(w.read_wav_file(p), pcm)
    # data shorter than its header claims: what the file holds
    p.write_bytes(_riff(_chunk(b"fmt ", _fmt()), b"data" + struct.pack("<I", 100000) + data))
    assert np.array_equal(w.read_wav_file(p), pcm)
    p.write_bytes(_riff(_chunk(b"fmt ", _fmt()), b"data" + struct.pack("<I", 0xFFFFFFFF) + data[:-1]))
    assert np.array_equal(w.read_wav_file(p), pcm[:-1])                                     # half a sample is dropped


def test_wav_other_formats_and_broken_files_yield_nothing(tmp_path):
    pcm = np.arange(-300, 300, dtype=np.int16)
    p = tmp_path / "c.wav"
    al.write_wav(p, (pcm & 0xFF).astype(np.uint8), width=1)
    assert w.read_wav_file(p).size == 0                       # 8 bit
    al.write_wav(p, pcm, channels=2)
    assert w.read_wav_file(p).size == 0                       # stereo
    al.write_wav(p, pcm, rate=11025)
    assert w.read_wav_file(p).size == 0                       # 11 025 Hz
    p.write_bytes(pcm.tobytes())
    assert w.read_wav_file(p).size == 0                       # no RIFF header
    data = _chunk(b"data", pcm.tobytes())
    for body in (b"", b"RIFF", _riff(), _riff(_chunk(b"fmt ", _fmt())), _riff(data, _chunk(b"fmt ", _fmt())),
                 _riff(_chunk(b"fmt ", _fmt(tag=3)), data), _riff(_chunk(b"fmt ", _fmt()[:12])),
                 _riff(_chunk(b"fmt ", _fmt()), b"LIST" + struct.pack("<I", 0xFFFFFFFF) + b"abc"),
                 _riff(_chunk(b"fmt ", _fmt()), b"LIST" + struct.pack("<I", 5000) + b"abc", data)):
        p.write_bytes(body)
        assert w.read_wav_file(p).size == 0, body[:40]
