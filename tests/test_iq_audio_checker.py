"""IQ to audio (K18) without a GPU: the serial checker (tests/helpers/iq_audio_check.c over
rtlsdr-wsprd_amd/csrc/kernels/iq_audio.h) against the committed tap tables, against a float64 numpy statement, through K12's
checker and back, through the CPU oracle, at the edges of a row and of a float; the checker under sanitizers; the .c2
writer."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import audio_lib as al
import audio_synth_lib as asl
import iq_audio_lib as iq
import oracle_lib as ol
import rtlsdr_wsprd_amd as w

LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65]


def _rc0(res):
    rc, pcm, count = res
    assert rc == 0
    return pcm, count


# ---- 1. unit impulses: index, polarity, the sign of Q ------------------------------------------------------------------------
@pytest.mark.parametrize("np_", [9, 100])
def test_unit_impulses_come_out_as_the_tables(np_):
    for m0 in (0, 1, 7, 8, np_ - 1):
        for rail in (0, 1):
            x = np.zeros((2, np_), np.float32)
            x[rail, m0] = 1.0
            pcm, count = _rc0(iq.check_rows(x[0], x[1], gain=3.0e5))            # 16 x 3e5 x 0.0625 (the centre tap): clips there
            want, clipped = iq.impulse_record(m0, np_, rail, gain=3.0e5)
            assert np.array_equal(pcm[0], want), (m0, rail)
            assert count[0] == clipped and clipped >= 1 and (np.abs(want.astype(np.int32)) < 32767).any()
    # the polarity and the sign of Q at a glance: gI[0] = 2 h[0] > 0 at n = 32 m0; gQ[+-2] = -+2 h[2] (s8[2] = 1): Q = +1
    # pulls the sample before the centre up and the one after it down
    gi, gq = al.taps()
    assert gi[iq.K] > 0 and gq[iq.K - 2] > 0 and gq[iq.K + 2] < 0
    x = np.zeros(np_, np.float32)
    x[8] = 0.5
    pi, _ = _rc0(iq.check_rows(x, 0 * x))
    pq, _ = _rc0(iq.check_rows(0 * x, x))
    assert pi[0, 256] == np.rint(8.0 * 32768.0 * float(gi[iq.K])) == 16384
    assert pq[0, 254] > 1000 and pq[0, 258] == -pq[0, 254] and pq[0, 256] == 0


# ---- 2. a second statement of the definition --------------------------------------------------------------------------------
def test_checker_equals_a_float64_numpy_statement_to_one_lsb():
    """Random rows of amplitude 0.2 at gain 32768.  A chain is at most 24 fmaf on terms below 0.0625 x 0.2: its error stays
    below 24 x 2^-24 x 6554 = 0.01 LSB of the output, so the two differ only where the float64 value lies that close to a
    half-way point, and then by one."""
    rng = np.random.default_rng(18)
    I = rng.uniform(-0.2, 0.2, (2, 4000)).astype(np.float32)
    Q = rng.uniform(-0.2, 0.2, (2, 4000)).astype(np.float32)
    pcm, count = _rc0(iq.check_rows(I, Q))
    want = iq.numpy_rows(I, Q)
    diff = np.abs(pcm.astype(np.int32) - want.astype(np.int32))
    print("%d of %d samples differ, largest difference %d, peak %d" % ((diff != 0).sum(), diff.size, diff.max(), np.abs(want.astype(np.int32)).max()))
    assert diff.max() <= 1 and (diff != 0).sum() <= 0.01 * diff.size and not count.any()
    assert np.abs(want.astype(np.int32)).max() > 4000


def test_quantiser_is_the_audio_scene_synthesisers():
    """iq_audio_quantise() and audio_synth_quantise() share their clip-and-round tail (kernels/pcm_quantise.h): the two agree
    on every value but NaN, which K17 never sees and K18 defines as 0, clipped."""
    rng = np.random.default_rng(5)
    p = np.concatenate((rng.uniform(-40000, 40000, 20000), np.arange(-8, 8) + 0.5, [32767.0, 32767.4, 32767.5, 32767.0000001,
                        -32768.0, -32768.5, -32768.0000001, 1e300, -1e300, np.inf, -np.inf, 0.0, -0.0, 1e-320]))
    a, na = iq.quantise(p)
    b, nb = asl.quantise(p)
    assert np.array_equal(a, b) and na == nb and na > 3000
    assert iq.quantise([np.nan, -np.nan, 1.5, 2.5])[0].tolist() == [0, 0, 2, 2] and iq.quantise([np.nan, 1.0])[1] == 1


# ---- 3. up, then down through K12's checker ---------------------------------------------------------------------------------
TONES = (-110.0, 0.0, 55.5, 110.0)


@pytest.fixture(scope="module")
def round_trip():
    amp, np_ = 0.4, 1200
    I, Q, z = iq.tone_rows(TONES, amp, np_)
    pcm, count = _rc0(iq.check_rows(I, Q))
    assert not count.any()
    bI, bQ = al.check_rows(pcm)
    return amp, np_, z, pcm, bI[:, :np_].astype(np.float64) + 1j * bQ[:, :np_].astype(np.float64)


def test_tones_leave_as_cosines_at_1500_plus_f(round_trip):
    amp, np_, z, pcm, back = round_trip
    n = np.arange(iq.INTERP * np_)
    for row, f in enumerate(TONES):
        want = amp * 32768.0 * np.cos(2.0 * np.pi * (1500.0 + f) * n / 12000.0)
        err = np.abs(pcm[row, 1280:-1280] - want[1280:-1280]).max()
        print("%+6.1f Hz: largest deviation from the cosine %.2f LSB of %.0f" % (f, err, amp * 32768.0))
        # rounding; the pass-band ripple of 0.0006 dB (7e-5) once; the 31 images of the 375 Hz row at f + 375 j Hz, each below
        # the stop band's -81.6 dB (8.3e-5; f = -110 Hz puts one at 265 Hz, the stop band's edge).  A delay of one sample
        # would show as 0.78 A.
        assert err <= 0.5 + (7e-5 + 31 * 8.3e-5) * amp * 32768.0


def test_round_trip_through_k12_is_the_identity_in_the_search_band(round_trip):
    """|z' - z| <= 2.5e-4 A for m in [40, np - 40): the ripple of K12's filter twice (1.39e-4 at +-110 Hz, in float64) plus
    the 16-bit rounding gave 1.56e-4 in a float64 model; the bound is that with a margin of 1.6 for the float32 chains.  At
    0 Hz the filters are flat and the rounding alone is left: 5e-5 A."""
    amp, np_, z, pcm, back = round_trip
    for row, f in enumerate(TONES):
        err = np.abs(back[row, 40:np_ - 40] - z[row, 40:np_ - 40]).max() / amp
        print("%+6.1f Hz: |z' - z| / A = %.3e" % (f, err))
        assert err <= 2.5e-4, (f, err)
        if f == 0.0:
            assert err <= 5e-5, err


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("np_", LENGTHS)
def test_lengths_gains_and_what_lies_behind_the_record(np_):
    rng = np.random.default_rng(100 + np_)
    I = rng.uniform(-0.4, 0.4, (2, np_ + 3)).astype(np.float32)
    Q = rng.uniform(-0.4, 0.4, (2, np_ + 3)).astype(np.float32)
    pcm, count = _rc0(iq.check_rows(I, Q, np_, pcm_stride=32 * np_ + 8))
    assert (pcm[:, 32 * np_:] == iq.SENTINEL).all() and not count.any()
    if np_:
        want = iq.numpy_rows(I[:, :np_], Q[:, :np_])
        assert np.abs(pcm[:, :32 * np_].astype(np.int32) - want).max() <= 1 and np.abs(want.astype(np.int32)).max() > 1000
    # what lies at or behind np_ is not read
    J, R = I.copy(), Q.copy()
    J[:, np_:], R[:, np_:] = np.nan, np.inf
    again, _ = _rc0(iq.check_rows(J, R, np_, pcm_stride=32 * np_ + 8))
    assert np.array_equal(again, pcm)
    # gain 0: zeros, none clipped; a negative gain: the negated record up to the -32768 / 32767 asymmetry
    zero, zc = _rc0(iq.check_rows(I, Q, np_, gain=0.0))
    assert not zero.any() and not zc.any()
    # (p changes sign exactly and ties go to even on both sides; 32767 < p <= 32768 clips on one side only)
    for g in (32768.0, 3.0e5):
        pos, pc = _rc0(iq.check_rows(I, Q, np_, gain=g))
        neg, nc = _rc0(iq.check_rows(I, Q, np_, gain=-g))
        inside = np.abs(pos.astype(np.int32)) < 32767
        assert np.array_equal(neg[inside], -pos[inside])
        assert (neg[pos == 32767] <= -32767).all() and (neg[pos == -32768] == 32767).all()
        if g < 1e5:
            assert not pc.any() and not nc.any()
        elif np_:
            assert pc.sum() > 0 and nc.sum() > 0 and np.abs(pc - nc).max() <= (~inside).sum()


def test_refusals_of_the_checker():
    x = np.zeros((1, 64), np.float32)
    assert iq.check_rows(x, x, -1, pcm_stride=8)[0] == -1
    assert iq.check_rows(x, x, 65)[0] == -1                                     # stride below np
    assert iq.check_rows(x, x, 64, pcm_stride=2047)[0] == -1
    assert iq.check_rows(x, x, 64, gain=float("nan"))[0] == -1 and iq.check_rows(x, x, 64, gain=float("inf"))[0] == -1
    big = np.zeros((1, 45001), np.float32)
    assert iq.check_rows(big, big, 45001, pcm_stride=8)[0] == -2
    assert iq.checker().iq_audio_check_tile() == iq.TILE


def _reach(m0, np_):
    """the outputs a value at input m0 is part of: |n - 32 m0| <= 255"""
    n = np.arange(32 * np_)
    return np.abs(n - 32 * m0) <= 255


@pytest.mark.parametrize("m0", [0, 5, 40, 79])
def test_non_finite_and_extreme_inputs_and_their_counts(m0):
    np_ = 80
    rng = np.random.default_rng(7)
    I = rng.uniform(-0.4, 0.4, np_).astype(np.float32)
    Q = rng.uniform(-0.4, 0.4, np_).astype(np.float32)
    clean, cc = _rc0(iq.check_rows(I, Q))
    assert not cc.any()
    reach = _reach(m0, np_)
    n = np.arange(32 * np_)
    takes_i, takes_q = (n % 8 != 2) & (n % 8 != 6), (n % 8 != 0) & (n % 8 != 4)
    for rail, takes in ((0, takes_i), (1, takes_q)):
        hit = reach & takes                                        # the chains this input is a step of: the skipped ones are not
        for v in (np.nan, np.inf, -np.inf, 1e30, -3e38):
            x = [I.copy(), Q.copy()]
            x[rail][m0] = np.float32(v)
            pcm, count = _rc0(iq.check_rows(x[0], x[1]))
            assert np.array_equal(pcm[0, ~hit], clean[0, ~hit]), (rail, v)  # no other sample moves -- a +0 tap times Inf would be NaN
            assert count[0] == hit.sum(), (rail, v, count[0], hit.sum())   # every tap inside the chain is non-zero: all of them clip
            if np.isnan(v):
                assert not pcm[0, hit].any()                                # NaN: 0, counted
            else:
                g = al.taps()[rail][(n - 32 * m0)[hit] + iq.K]
                # a later step may turn +Inf - Inf into NaN only with a second non-finite input: there is none
                assert np.array_equal(pcm[0, hit], np.where(np.sign(g) * np.sign(v) > 0, 32767, -32768))
        for v in (1e-42, -1e-45, -0.0):                            # denormals and -0 are finite values like any other
            x = [I.copy(), Q.copy()]
            x[rail][m0] = np.float32(v)
            y = [I.copy(), Q.copy()]
            y[rail][m0] = 0.0
            pcm, count = _rc0(iq.check_rows(x[0], x[1]))
            ref, _ = _rc0(iq.check_rows(y[0], y[1]))
            assert np.array_equal(pcm, ref) and not count.any()
    # a row of denormals alone: zeros, none clipped; with a gain of 3e38 they are seen again
    tiny = np.full(np_, 1e-38, np.float32)                      # below the smallest normal float, 1.18e-38
    pcm, count = _rc0(iq.check_rows(tiny, tiny))
    assert not pcm.any() and not count.any()
    pcm, count = _rc0(iq.check_rows(tiny, tiny, gain=3e38))
    assert pcm.any()
    # Inf at gain 0 is NaN: 0 and counted
    x = I.copy()
    x[m0] = np.inf
    pcm, count = _rc0(iq.check_rows(x, Q, gain=0.0))
    assert not pcm.any() and count[0] == (reach & takes_i).sum()


def test_odd_rows_hold_every_kind_of_value():
    I, Q = iq.odd_rows(131, 3)
    both = np.concatenate((I.ravel(), Q.ravel()))
    assert np.isnan(both).any() and np.isposinf(both).any() and np.isneginf(both).any() and (np.abs(both) > 1e29).any()
    assert ((both != 0) & (np.abs(both) < 1e-38)).any()
    pcm, count = _rc0(iq.check_rows(I, Q))
    assert (count > 0).all() and (pcm == 32767).any() and (pcm == -32768).any()


# ---- 5. scenes: up, down, and through the CPU oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_scenes_survive_the_loop_in_the_oracle(k):
    """audio_lib's three scenes as IQ rows of tests/synth.py: the checker up, K12's checker down (normalised), the CPU oracle.
    The messages are those of the rows decoded as they are, and every sent one is within the tolerances
    test_audio_checker.py states for its scenes."""
    items = al.scene_items(k)
    direct, loop = iq.scene_spots(k, False), iq.scene_spots(k, True)
    pcm, clipped = iq.scene_record(k)
    print("scene %d: %d samples clipped, peak %d" % (k, clipped, np.abs(pcm.astype(np.int32)).max()))
    assert sorted(s.message for s in loop) == sorted(s.message for s in direct)
    found, was = al.find_sent(loop, items), al.find_sent(direct, items)
    for s, d, (msg, snr, f0, t0) in zip(found, was, items):
        assert s is not None and d is not None, msg
        print("%-16s snr %+.2f (direct %+.2f, sent %+.1f)  f %+.3f Hz (direct %+.3f)  dt %+.3f s (direct %+.3f)"
              % (msg, s.snr, d.snr, snr, al.spot_offset_hz(s) - f0, al.spot_offset_hz(d) - f0, s.dt - (t0 - 2.0), d.dt - (t0 - 2.0)))
        for spot in (d, s):                                            # the rows as they are, then through the loop
            assert abs(al.spot_offset_hz(spot) - f0) <= 0.15
            assert abs(spot.dt - (t0 - 2.0)) <= 0.1
            assert abs(spot.snr - snr) <= 0.5
        assert abs(s.freq - d.freq) * 1e6 <= 0.15 and abs(s.dt - d.dt) <= 0.1 and abs(s.snr - d.snr) <= 0.5


# ---- 6. the checker under sanitizers -----------------------------------------------------------------------------------------
def test_checker_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = iq.sanitizer_program(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("iq_audio_check: ok") and not r.stderr


# ---- 7. the library without a device: the .c2 writer, the refusals ---------------------------------------------------------
def test_c2_writer_is_what_the_reader_reads(tmp_path):
    rng = np.random.default_rng(2)
    I = rng.uniform(-0.5, 0.5, 45000).astype(np.float32)
    Q = rng.uniform(-0.5, 0.5, 45000).astype(np.float32)
    I[123] = 0.5                                                   # a peak of exactly 0.5: the reader's scale is 1.0
    path = tmp_path / "150426_0918.c2"
    dial = 14095600.0
    w.write_c2_file(path, I, Q, dial)
    pairs = np.empty(90000, np.float32)
    pairs[0::2], pairs[1::2] = I, -Q
    assert path.read_bytes() == b"150426_0918.c2" + struct.pack("<id", 2, dial) + pairs.tobytes()
    rI, rQ = np.zeros(45000, np.float32), np.zeros(45000, np.float32)
    freq = C.c_double(0.0)
    L = w.lib()
    n = L.wspr_read_c2_file(os.fsencode(path), C.c_void_p(rI.ctypes.data), C.c_void_p(rQ.ctypes.data), C.byref(freq))
    assert n == 45000 and freq.value == dial
    assert np.array_equal(rI.view(np.uint32), I.view(np.uint32)) and np.array_equal(rQ, Q)
    # a short base name is padded with zeros, a long one is cut at 14 bytes; the directory is not part of it
    w.write_c2_file(tmp_path / "a.c2", I, Q, 7040100.0)
    assert (tmp_path / "a.c2").read_bytes()[:26] == b"a.c2" + b"\0" * 10 + struct.pack("<id", 2, 7040100.0)
    w.write_c2_file(tmp_path / "a_rather_long_name.c2", I[:100], Q[:100], 1.0)
    body = (tmp_path / "a_rather_long_name.c2").read_bytes()
    assert body[:14] == b"a_rather_long_" and len(body) == 26 + 8 * 45000
    assert not np.frombuffer(body[26 + 800:], np.float32).any()                # the padding: 0.0 and -0.0
    with pytest.raises(OSError):
        w.write_c2_file(tmp_path / "no" / "such" / "dir.c2", I, Q, 1.0)
    assert L.wspr_write_c2_file(os.fsencode(tmp_path / "b.c2"), None, None, 1.0) == 0


def test_entry_points_refuse_bad_arguments_before_they_look_for_a_device():
    L = w.lib()
    pcm = np.full(64, 0x1234, np.int16)
    n = C.c_int(-7)
    x = np.zeros(8, np.float32)
    for args, want in (((x.ctypes.data, x.ctypes.data, -1, 1.0), -1), ((x.ctypes.data, x.ctypes.data, 45001, 1.0), -2),
                       ((x.ctypes.data, x.ctypes.data, 2, float("nan")), -1), ((x.ctypes.data, x.ctypes.data, 2, float("inf")), -1),
                       ((None, x.ctypes.data, 2, 1.0), -1)):
        assert L.wspr_iq_to_audio(*args, pcm.ctypes.data, C.addressof(n)) == want, args
        assert (pcm == 0x1234).all() and n.value == -7
    assert L.wspr_iq_to_audio_batch_device(16, 16, -1, 8, 8, 1.0, 16, 256, None) == -1
    assert L.wspr_iq_to_audio_batch_device(16, 16, 1, 45001, 45004, 1.0, 16, 1440032, None) == -2
    assert L.wspr_iq_to_audio_batch_device(16, 24, 1, 8, 8, 1.0, 16, 256, None) == -1        # misaligned d_qdat
    assert L.wspr_iq_to_audio_batch_device(16, 16, 1, 8, 6, 1.0, 16, 256, None) == -1        # stride no multiple of 4, below samples
    assert L.wspr_iq_to_audio_batch_device(16, 16, 1, 8, 8, 1.0, 18, 256, None) == -1        # misaligned d_pcm
    assert L.wspr_iq_to_audio_batch_device(16, 16, 1, 8, 8, 1.0, 16, 252, None) == -1        # pcm_stride no multiple of 8
    assert L.wspr_iq_to_audio_batch_device(16, 16, 1, 8, 8, 1.0, 16, 248, None) == -1        # ... below 32 * samples
    assert L.wspr_iq_to_audio_batch_device(16, 16, 1, 8, 8, float("-inf"), 16, 256, None) == -1
    assert L.wspr_iq_to_audio_batch_device(None, None, 0, 8, 8, 1.0, None, 256, None) == 0  # nseg == 0 does nothing
