"""The tunable multi-band front end (K21) without a GPU: the serial checker (tests/helpers/tune_check.c over
rtlsdr-wsprd_amd/csrc/kernels/tune.h) against the committed tables' derivation, a float64 numpy statement, exact rotors, a
tone's frequency, the filter's response beside the oracle front end's, oscillator spurs, the refusals and the edge lengths.
WSPR_TUNE_FIGURES=<file> makes the measuring tests write their figures there as JSON lines (tools/tune_ab.py collects them
into profiles/tuner.json)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tune_lib as tl

BLK = tl.BLOCK_BYTES


_record = tl.record


def test_committed_tables_are_what_the_definition_states():
    import rtlsdr_wsprd_amd as w
    c, f, spo = w.tune_constants()
    wc, wf = tl.tables_from_numpy()
    assert spo == 6400 and np.array_equal(c, wc) and np.array_equal(f, wf)
    assert tuple(c[0]) == (16384, 0) and tuple(f[0]) == (16384, 0) and tuple(c[64]) == (0, 16384) and tuple(c[128]) == (-16384, 0)
    out = subprocess.run([sys.executable, os.path.join(tl.ol.ROOT, "tools", "gen_tune_tables.py")], capture_output=True, text=True, check=True).stdout
    with open(os.path.join(tl.ol.ROOT, "rtlsdr-wsprd_amd", "csrc", "kernels", "tune_tables.h")) as fh:
        assert fh.read() == out
    assert ("0x%08x" % np.float32(tl.SCALE).view(np.uint32)) in out


def test_step_rule_and_realised_offset():
    """step = floor(-offset 2^32 / fs + 0.5) mod 2^32, by exact rational arithmetic; the library's wspr_tune_step() equals the
    header's; the realised offset is the step's own and lies within half a step of the request."""
    from fractions import Fraction
    import rtlsdr_wsprd_amd as w
    rng = np.random.default_rng(3)
    offs = [0.0, 600000.0, -600000.0, 1200000.0, -1200000.0, 2400000.0, 136000.0, 474200.0, 1836600.0, -0.0003, 1e-9, 7e9, -7e9]
    offs += list(rng.uniform(-1.2e6, 1.2e6, 200))
    FS = 2400000
    for o in offs:
        x = -Fraction(o) * (1 << 32) / FS + Fraction(1, 2)
        want = (x.numerator // x.denominator) % (1 << 32)
        got, realised = tl.step_of(o)
        # the header divides in double: a request within 1e-9 of a tie between two steps may take either
        assert got == want or abs(x - round(x)) < Fraction(1, 10 ** 6), (o, got, want)
        assert (got, realised) == w.tune_step(o)
        signed = got - (1 << 32) if got >= 1 << 31 else got
        assert realised == -signed * 2.4e6 / 4294967296.0
        assert abs(((realised - o + FS / 2) % FS) - FS / 2) <= 0.5 * 2.4e6 / 4294967296.0 * 1.000001
    assert [tl.step_of(o)[0] for o in (0.0, -600000.0, 600000.0, 1200000.0)] == [0, 1 << 30, 3 << 30, 1 << 31]
    assert tl.step_of(float("nan")) == (0, 0.0) and tl.step_of(float("inf")) == (0, 0.0)


def test_exact_rotors_at_quarter_turn_steps():
    """At 0, +-fs/4 and fs/2 every rotor is 16384 (1, j, -1, -j)^m: z is 16384 times the exactly mixed vector sum and y is
    16384 times the same sum turned by (8 v step): exact multiples, no rounding anywhere."""
    raw = tl.random_bytes(1, 16 * 1000, 5, clipped=True)[0]
    s = raw.astype(np.int64).reshape(-1, 8, 2) - 128
    s = s[..., 0] + 1j * s[..., 1]
    for m in range(4):
        step = (m << 30) & 0xffffffff
        z, y = tl.check_zy(raw, step)
        want = (s * (1j ** (m * np.arange(8)))[None, :]).sum(axis=1)          # 8 v step is a whole number of turns
        assert np.array_equal(z[:, 0], 16384 * np.rint(want.real).astype(np.int64))
        assert np.array_equal(z[:, 1], 16384 * np.rint(want.imag).astype(np.int64))
        assert np.array_equal(y, z) and not (z % 16384).any()


def test_checker_equals_the_float64_statement_within_the_derived_bound():
    """Tone of A = 100 LSB at offset + 20 Hz over 3 LSB of noise, 40 blocks + a partial one, three steps.  Bound on
    max |checker - float64| / max |float64|, every error taken at its worst and added coherently:
      rotor   each table entry is off by at most sqrt(2)/2 (int16 rounding, 2^-15 of 16384 per part), the product of two and
              its rs14 give |rot - 16384 e| <= 3 (sqrt(2)/2) + 2^-15, e_rot = that / 16384 = 1.2947e-4; a sample meets two
              rotors: e_mix = 2 e_rot + e_rot^2 of |s| <= smax;
      rs14    of y: sqrt(2)/2 per vector against 16384 * 8 per LSB of a sample: sqrt(2)/2 / 131072 LSB;
      filter  the two sums and differences pass an error of constant size e with gain 4 * 800^2, the same as a signal at 0 Hz;
              the taps then at most sum |t|: in units of the 0 Hz output of one LSB, e * L1, L1 = sum |t|;
      float   one rounding of d (2^-24), one of the scale (2^-24), 33 products and 33 sums (66 * 2^-24) on values of at most
              the row's peak: 68 * 2^-24 * L1 of the peak.
    The measured distance is far below it (the rounding errors are not coherent); it is printed and recorded."""
    t = tl.taps().astype(np.float64)
    L1 = np.abs(t).sum()
    e_rot = (3 * np.sqrt(0.5) + 2.0 ** -15) / 16384
    e_mix = 2 * e_rot + e_rot ** 2
    worst = 0.0
    for k, off in enumerate((-600000.0, 412345.0, 0.7)):
        step, realised = tl.step_of(off)
        raw = tl.tone_bytes([realised + 20.0], 100.0, 40 * tl.SPO + 3208, seed=10 + k, noise=3.0)
        smax = np.abs((raw.astype(np.float64).reshape(-1, 2) - 128.0) @ np.array([1, 1j])).max()
        got, want = tl.k21_row(raw, step), tl.numpy_rows(raw, step)
        assert got.size == want.size == 40
        unit = 4 * 800.0 ** 2 * 8 * 16384 * tl.SCALE                        # output of 1 LSB at 0 Hz before the taps
        bound = ((e_mix * smax + np.sqrt(0.5) / 131072) * unit * L1 + 68 * 2.0 ** -24 * L1 * np.abs(want).max()) / np.abs(want).max()
        dist = np.abs(got - want).max() / np.abs(want).max()
        _record("float64_distance", offset_hz=off, distance=dist, bound=bound)
        assert dist <= bound and bound < 2e-3
        worst = max(worst, dist)
    assert worst > 0.0                                                       # two statements, not one


def test_a_tone_comes_out_at_its_offset_from_the_band():
    """A tone at offset + f leaves at +f within 0.001 Hz (phase slope over 400 outputs behind the filter's start-up)."""
    for off, f in ((-600000.0, 50.0), (136000.0, -73.3), (-1036600.25, 101.7), (1199000.0, 0.0)):
        step, realised = tl.step_of(off)
        raw = tl.tone_bytes([realised + f], 90.0, 440 * tl.SPO, seed=2)
        row = tl.k21_row(raw, step)[40:]
        ph = np.unwrap(np.angle(row))
        slope = np.polyfit(np.arange(ph.size), ph, 1)[0] * 375.0 / (2 * np.pi)
        assert abs(slope - f) < 0.001, (off, f, slope)


def _gain_db(front, f_hz, amp, n):
    """Output power behind the start-up over the power of a tone of `amp` LSB at f_hz, dB."""
    row = front(tl.tone_bytes([f_hz], amp, n, seed=1))
    return 10 * np.log10(np.mean(np.abs(row[40:]) ** 2) / amp ** 2)


def _sweep(front, rate_in, centre):
    """Droop over +-110 Hz and the worst rejection of tones that fold into +-110 Hz: from the first three zones of the output
    rate on either side, and from 300 kHz * k, k = 1 .. 7.  front(raw) -> complex row; the output rate is fs / rate_in.
    Amplitudes: the reference's int32 integrators wrap once an in-band tone exceeds 2^31 / (4 * 6401^2) = 13.1 LSB, so the
    in-band tones have 10 LSB; tones that fold in are attenuated and have 50 (zones) and 100 LSB (300 kHz images).  The
    dithered quantisation leaves a floor of about -63 dB - 20 log10(amp / 10) in these figures."""
    fo = tl.FS / rate_in
    n = 64 * rate_in
    fs_in = np.arange(-110.0, 111.0, 10.0)
    g = np.array([_gain_db(front, centre + f, 10.0, n) for f in fs_in])
    droop = g.max() - g.min()
    ref = g[fs_in == 0.0][0]
    zones, images = [], []
    for k in (1, 2, 3, -1, -2, -3):
        for f in (-110.0, -60.0, 0.0, 60.0, 110.0):
            zones.append(_gain_db(front, centre + k * fo + f, 50.0, n) - ref)
    for k in range(1, 8):
        for f in (-110.0, 0.0, 110.0):
            images.append(_gain_db(front, centre + 300000.0 * k + f, 100.0, n) - ref)
    return droop, max(zones), max(images), ref


def test_filter_response_is_no_worse_than_the_oracle_front_ends():
    """Same sweep through K21's checker at -600 kHz and through the oracle's decimator (its band is fs/4 below the tuner).
    Requirement: droop and worst rejection no worse than the oracle's by more than 0.1 dB.  The in-band gain is the oracle's
    within 0.01 dB: that is what the scale is for."""
    step = 1 << 30
    d21, z21, i21, g21 = _sweep(lambda raw: tl.k21_row(raw, step), 6400, -600000.0)
    d0, z0, i0, g0 = _sweep(tl.oracle_k0, 6401, -600000.0)
    _record("filter", k21=dict(droop_db=d21, zones_db=z21, images_300k_db=i21, gain_db=g21, rejection_db=max(z21, i21)),
            oracle_k0=dict(droop_db=d0, zones_db=z0, images_300k_db=i0, gain_db=g0, rejection_db=max(z0, i0)))
    assert d21 <= d0 + 0.1
    assert max(z21, i21) <= max(z0, i0) + 0.1
    assert abs(g21 - g0) < 0.01


def test_no_spur_above_what_a_4096_phase_14_bit_rotor_bounds():
    """A full-scale tone (127 LSB, dithered) at 50 offsets, 25 Hz above each band's centre.  A rotor with 4096 phases bounds
    its worst spur at -6.02 * 12 = -72.2 dBc and 14 bits of amplitude at -84 dBc; this one has 65536 phases.  Worst bin of a
    256-point spectrum under a four-term Blackman-Harris window (side lobes at -92 dB) within +-110 Hz, the tone's own lobe
    (+-5 bins) left out; the dithered 8-bit quantisation puts the floor of these spectra near -107 dBc per bin."""
    rng = np.random.default_rng(77)
    steps = [int(x) | 1 for x in rng.integers(0, 1 << 32, 47)] + [1, (1 << 32) - 1, 0x55555555]
    m = 2 * np.pi * np.arange(256) / 256
    win = 0.35875 - 0.48829 * np.cos(m) + 0.14128 * np.cos(2 * m) - 0.01168 * np.cos(3 * m)
    worst = -400.0
    for i, step in enumerate(steps):
        signed = step - (1 << 32) if step >= 1 << 31 else step
        realised = -signed * 2.4e6 / 4294967296.0
        raw = tl.tone_bytes([realised + 25.0], 127.0, (40 + 256) * tl.SPO, seed=100 + i)
        spec = np.abs(np.fft.fftshift(np.fft.fft(tl.k21_row(raw, step)[40:] * win))) ** 2
        f = (np.arange(256) - 128) * 375.0 / 256
        peak = int(np.argmax(spec))
        assert abs(f[peak] - 25.0) < 1.5
        mask = (np.abs(f) <= 110.0) & (np.abs(np.arange(256) - peak) > 5)
        worst = max(worst, 10 * np.log10(spec[mask].max() / spec[peak]))
    _record("spurs", worst_dbc=worst, bound_dbc=-72.2, offsets=len(steps))
    assert worst <= -72.2


def test_refusals_write_nothing():
    raw = tl.random_bytes(2, 2 * BLK, 9)
    for kw in (dict(nseg=-1), dict(steps=None), dict(nbands=0), dict(nbands=17), dict(bytes_per_seg=2 * BLK - 8), dict(raw_offset=8)):
        steps = kw.pop("steps", [1, 2])
        rc, I, Q, n = tl.check_rows(raw, steps, **kw)
        assert rc == -1 and np.isnan(I).all() and np.isnan(Q).all() and (n == -7).all(), kw
    rc, I, Q, n = tl.check_rows(raw, [1, 2], nseg=0)
    assert rc == 0 and np.isnan(I).all() and (n == -7).all()


@pytest.mark.parametrize("nsamp", [0, 8, 6392, 6400, 6408, 6400 * 37, 6400 * 40 + 3208])
def test_edge_lengths(nsamp):
    """n_out = floor(nsamples / 6400); the partial block is dropped (bytes behind the last whole block do not matter); every
    other column is 0.0f; a row shorter than one block is all zeros."""
    raw = tl.random_bytes(1, 2 * nsamp, 20 + nsamp % 97, clipped=True)
    rc, I, Q, n = tl.check_rows(raw, [0x12345677, 1 << 30])
    assert rc == 0 and (n == nsamp // 6400).all()
    assert not I[:, nsamp // 6400:].any() and not Q[:, nsamp // 6400:].any() and not np.isnan(I).any()
    if nsamp >= 6400:
        assert I[:, :nsamp // 6400].any() and not np.array_equal(I[0], I[1])
        other = raw.copy()
        other[0, (nsamp // 6400) * BLK:] ^= 0x5a
        assert np.array_equal(tl.check_rows(other, [0x12345677, 1 << 30])[1], I)
    rc, I1, Q1, _ = tl.check_rows(raw, [0x12345677, 1 << 30], normalise=1)
    if nsamp >= 6400:
        assert abs(max(np.abs(I1[0]).max(), np.abs(Q1[0]).max()) - 0.5) <= 2.0 ** -24                # peak * float(0.5 / peak)


def test_closed_form_of_the_block_sums_equals_the_running_sums():
    """d_b = 800 (S_{b-1} + 2 S_{b-2} + S_{b-3}) + W_b + W_{b-1} - W_{b-2} - W_{b-3} (what the kernel's second pass forms) is what
    the checker's two running sums and differences give, in Python's exact integers."""
    raw = tl.random_bytes(1, 7 * BLK, 31, clipped=True)[0]
    step = 0x9e3779b1
    _, y = tl.check_zy(raw, step)
    d = np.zeros(14, np.int64)
    tl.checker().tune_check_outputs(tl.ol.ptr(raw), 7, step, tl.ol.ptr(d))
    yb = y.reshape(7, 800, 2)
    S = [[int(v) for v in yb[b].sum(axis=0)] for b in range(7)]
    W = [[int(v) for v in ((800 - np.arange(800))[:, None] * yb[b]).sum(axis=0)] for b in range(7)]
    g = lambda A, b, r: A[b][r] if b >= 0 else 0
    for b in range(7):
        for r in range(2):
            want = 800 * (g(S, b - 1, r) + 2 * g(S, b - 2, r) + g(S, b - 3, r)) + g(W, b, r) + g(W, b - 1, r) - g(W, b - 2, r) - g(W, b - 3, r)
            assert int(d[2 * b + r]) == want


def test_checker_is_clean_under_the_sanitizers(tmp_path):
    exe = tl.sanitizer_program(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[:2] == ["0", "2"], (r.stdout, r.stderr[-2000:])
