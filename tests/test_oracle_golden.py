"""Pins the CPU oracle (oracle/*.c) to the reference's own golden answers.

  * documentation/bug-fix/REPORT.md:202  -r signals/refSignalSnr0dB.iq spot line
  * documentation/bug-fix/REPORT.md:198  -t self-test spot line (+ rtlsdr_wsprd.c:782-788)
  * SURVEY.md §8(c) per-stage anchors recorded from the reference
  * tests/golden/message_vectors.json    outputs of the real reference objects
  * reference tests/test_wsprd.c         unit-test expectations, restated
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import oracle_lib as ol


# ------------------------------------------------------------------ decode pins
def test_ref_signal_spot_line_matches_reference_report():
    I, Q, n = ol.read_iq_file(os.path.join(ol.GOLDEN, "refSignalSnr0dB.iq"))
    assert n == 45000
    spots, _, _, tr = ol.decode(I, Q, n, trace=True)
    assert len(spots) == 1
    # byte-identical to documentation/bug-fix/REPORT.md:202
    assert ol.spot_line(spots[0]) == "Spot :  -0.07   0.01 144.490550  0    K1JT   FN20 20"
    s = spots[0]
    # SURVEY §8(c) anchors (values recorded from the reference build)
    assert s.message == b"K1JT FN20 20" and s.cycles == 82 and s.jitter == 0 and s.drift == 0
    assert s.snr == pytest.approx(-0.0706653595, abs=2e-6)
    assert s.dt == pytest.approx(0.00533333328, abs=1e-9)
    assert s.freq == pytest.approx(144.490550005, abs=1e-9)
    assert tr.passes_run == 2 and tr.npk[0] == 1 and tr.npk[1] == 0
    assert tr.noise_level[0] == pytest.approx(4934.7959, rel=2e-6)
    pk = tr.cand_peaks[0][0]
    assert pk.freq == pytest.approx(49.804688, abs=1e-5) and pk.snr == pytest.approx(-0.0707, abs=1e-4)
    co = tr.cand_coarse[0][0]
    assert co.shift == 768 and co.drift == 0 and co.sync == pytest.approx(0.535337, abs=2e-6)
    assert tr.mode0_shift[0][0] == 752 and tr.mode0_sync[0][0] == pytest.approx(0.641268, abs=2e-6)
    fi = tr.cand_fine[0][0]
    assert fi.freq == pytest.approx(50.004688, abs=1e-5) and fi.sync == pytest.approx(0.919728, abs=2e-6)
    assert tr.first_rms[0][0] == pytest.approx(50.1764, abs=1e-3)
    assert list(tr.first_symbols[0][0][:8]) == [176, 178, 178, 77, 177, 77, 177, 179]
    assert tr.fano_metric[0][0] == 810 and tr.fano_cycles[0][0] == 82 and tr.fano_maxnp[0][0] == 80
    assert bytes(tr.decdata[0][0][:7]) == bytes.fromhex("f70ddd7b39d500")
    assert tr.subtracted[0][0] == 1


def _selftest_signal():
    """decoderSelfTest() generator, rtlsdr_wsprd.c:729-760, with glibc rand() (seed 1)."""
    libc = C.CDLL("libc.so.6")
    libc.srand(1)
    RAND_MAX = 2147483647
    ok, sym = ol.channel_symbols("K1JT FN20QI 20")
    assert ok
    f0, t0, amp, wgn = np.float32(50.0), np.float32(2.0), np.float32(1.0), np.float32(0.02)
    df, dt = 375.0 / 256.0, 1 / 375.0
    I = np.zeros(45000, np.float32)
    Q = np.zeros(45000, np.float32)
    state = {"phase": 0, "V2": 0.0, "S": 0.0}

    def wgn_sample():
        if state["phase"] == 0:
            while True:
                u1 = libc.rand() / float(RAND_MAX)
                u2 = libc.rand() / float(RAND_MAX)
                v1, v2 = 2 * u1 - 1, 2 * u2 - 1
                s = v1 * v1 + v2 * v2
                if not (s >= 1 or s == 0):
                    break
            state["V2"], state["S"] = v2, s
            x = v1 * math.sqrt(-2 * math.log(s) / s)
        else:
            x = state["V2"] * math.sqrt(-2 * math.log(state["S"]) / state["S"])
        state["phase"] = 1 - state["phase"]
        return np.float32(np.float32(x) * wgn)

    phi = 0.0
    for i in range(162):
        dphi = 2.0 * math.pi * dt * (float(f0) + (float(sym[i]) - 1.5) * df)
        for j in range(256):
            idx = int(float(t0) / dt + 256 * i + j)
            I[idx] = np.float32(float(amp) * math.cos(phi) + float(wgn_sample()))
            Q[idx] = np.float32(float(amp) * math.sin(phi) + float(wgn_sample()))
            phi += dphi
    return I, Q


def test_selftest_spot_line_matches_reference_report():
    I, Q = _selftest_signal()
    spots, _, _ = ol.decode(I, Q, 45000)      # the self-test does not normalise
    assert len(spots) >= 1
    s = spots[0]
    assert (s.call, s.loc, s.pwr) == (b"K1JT", b"FN20", b"20")          # rtlsdr_wsprd.c:782-788
    line = "Spot(%i) %6.2f %6.2f %10.6f %2d %7s %6s %2s" % (
        0, s.snr, s.dt, s.freq, int(s.drift), s.call.decode(), s.loc.decode(), s.pwr.decode())
    assert line == "Spot(0)  22.80   0.01 144.490550  0    K1JT   FN20 20"   # REPORT.md:198


# ------------------------------------------------------- message-layer pins
def test_survey_kats():
    L = ol.lib()
    for call, h in [("K1JT", 14767), ("VA2GKA", 12125), ("W1AW", 5970), ("PJ4/K1ABC", 19735)]:
        assert L.orc_nhash(call.encode(), len(call), 146) == h
    for call, n in [("K1JT", 259055063), ("VA2GKA", 221674590), ("W1AW", 261410543)]:
        assert L.orc_pack_call(call.encode()) == n
    ok, sym = ol.channel_symbols("K1JT FN20QI 20")
    assert ok and "".join(map(str, sym[:16])) == "3320202210203110"
    idn = (C.c_ubyte * 162)(*range(162))
    L.orc_interleave(idn)
    assert list(idn[:12]) == [0, 81, 41, 122, 21, 102, 61, 142, 11, 92, 51, 132]
    mt = (C.c_int * 256 * 2)()
    L.orc_build_mettab(mt)
    assert [mt[0][i] for i in (0, 64, 127, 128, 192, 255)] == [5, 5, -5, -5, -61, -137]
    assert [mt[1][i] for i in range(256)] == [mt[0][255 - i] for i in range(256)]


def test_golden_nhash_pack(golden_vectors):
    L = ol.lib()
    for call, h in golden_vectors["nhash"]:
        assert L.orc_nhash(call.encode(), len(call), 146) == h
    for call, n in golden_vectors["pack_call"]:
        assert L.orc_pack_call(call.encode()) == n, call
    for grid, p, m in golden_vectors["pack_grid4_power"]:
        codes = bytes(L.orc_loc_char_code(C.c_char(ch.encode())) & 0xFF for ch in grid)
        assert L.orc_pack_grid4_power(codes, C.c_int(p)) == m


def test_golden_channel_symbols(golden_vectors):
    for v in golden_vectors["channel_symbols"]:
        ok, sym = ol.channel_symbols(v["message"])
        assert ok == v["ok"], v["message"]
        if ok:
            assert "".join(map(str, sym)) == v["symbols"], v["message"]


def test_golden_interleaver(golden_vectors):
    L = ol.lib()
    a = (C.c_ubyte * 162)(*range(162)); L.orc_interleave(a)
    assert list(a) == golden_vectors["interleave_identity"]
    a = (C.c_ubyte * 162)(*range(162)); L.orc_deinterleave(a)
    assert list(a) == golden_vectors["deinterleave_identity"]
    a = (C.c_ubyte * 162)(*range(162)); L.orc_interleave(a); L.orc_deinterleave(a)
    assert list(a) == list(range(162))                  # reference tests/test_wsprd.c:137-163


def _unpk(L, fn, v):
    hashtab = C.create_string_buffer(32768 * 13); loctab = C.create_string_buffer(32768 * 5)
    for idx, txt in v["pre_hash"]:
        C.memmove(C.addressof(hashtab) + idx * 13, txt.encode(), len(txt))
    msg = (C.c_byte * 12)(*[(b - 256 if b > 127 else b) for b in v["data"]] + [0] * 5)
    clp = C.create_string_buffer(23); call = C.create_string_buffer(13); loc = C.create_string_buffer(7)
    pwr = C.create_string_buffer(3); cs = C.create_string_buffer(13)
    r = getattr(L, fn)(msg, hashtab, loctab, clp, call, loc, pwr, cs)
    return (int(r), clp.value.decode("latin1"), call.value.decode("latin1"), loc.value.decode("latin1"),
            pwr.value.decode("latin1"), cs.value.decode("latin1"))


def test_golden_unpk(golden_vectors):
    L = ol.lib()
    for v in golden_vectors["unpk"]:
        got = _unpk(L, "orc_unpk", v)
        want = (v["noprint"], v["call_loc_pow"], v["call"], v["loc"], v["pwr"], v["callsign"])
        assert got == want, v["data"]


def test_golden_fano(golden_vectors):
    L = ol.lib()
    mt = (C.c_int * 256 * 2)()
    L.orc_build_mettab(mt)
    assert [mt[0][i] for i in range(256)] == golden_vectors["mettab0"]
    for v in golden_vectors["fano"]:
        s = (C.c_ubyte * 162)(*v["symbols"])
        dec = (C.c_ubyte * 11)(); metric = C.c_uint(0); cycles = C.c_uint(0); maxnp = C.c_uint(0)
        r = L.orc_fano(C.byref(metric), C.byref(cycles), C.byref(maxnp), dec, s, C.c_uint(81), mt,
                       C.c_int(60), C.c_uint(v["maxcycles"]))
        assert (r, metric.value, cycles.value, maxnp.value) == (v["ret"], v["metric"], v["cycles"], v["maxnp"])
        if r == 0:      # on timeout the reference returns bytes of never-visited (uninitialised) nodes
            assert list(dec)[:10] == v["decdata"]


def test_reference_unit_test_expectations():
    """Restates reference tests/test_wsprd.c:58-132, 168-220, 304-384 against the oracle."""
    L = ol.lib()
    L.orc_call_char_code.restype = C.c_byte
    L.orc_loc_char_code.restype = C.c_byte
    cc = lambda ch: L.orc_call_char_code(C.c_char(ch.encode()))
    lc = lambda ch: L.orc_loc_char_code(C.c_char(ch.encode()))
    assert [cc(c) for c in "09AZ "] == [0, 9, 10, 35, 36]
    assert [lc(c) for c in "09AR "] == [0, 9, 0, 17, 36]
    for call in ("K1JT", "VA2GKA", "W1AW"):
        n = L.orc_pack_call(call.encode())
        out = C.create_string_buffer(13)
        assert L.orc_unpackcall(C.c_int32(n), out) == 1 and out.value.decode() == call
    out = C.create_string_buffer(13)
    assert L.orc_unpackcall(C.c_int32(262177560), out) == 0
    g = C.create_string_buffer(5)
    assert L.orc_unpackgrid(C.c_int32(32400 << 7), g) == 0 and g.value == b"XXXX"
    assert L.orc_pack_call(b"TOOLONG1") == 0
    # Fano round trip on hard 0/255 symbols
    n = L.orc_pack_call(b"K1JT")
    m = L.orc_pack_grid4_power(bytes(lc(c) for c in "FN20"), C.c_int(20))
    data = [(n >> 20) & 255, (n >> 12) & 255, (n >> 4) & 255, ((n & 15) << 4) + ((m >> 18) & 15),
            (m >> 10) & 255, (m >> 2) & 255, (m & 3) << 6, 0, 0, 0, 0]
    enc = (C.c_ubyte * 176)()
    L.orc_conv_encode(enc, (C.c_ubyte * 11)(*data), C.c_uint(11))
    soft = (C.c_ubyte * 162)(*[255 if enc[i] else 0 for i in range(162)])
    mt = (C.c_int * 256 * 2)(); L.orc_build_mettab(mt)
    dec = (C.c_ubyte * 11)(); a = C.c_uint(); b = C.c_uint(); c = C.c_uint()
    assert L.orc_fano(C.byref(a), C.byref(b), C.byref(c), dec, soft, C.c_uint(81), mt, C.c_int(60), C.c_uint(10000)) == 0
    assert list(dec)[:7] == data[:7]
    n1 = C.c_int32(); n2 = C.c_int32()
    L.orc_unpack50((C.c_byte * 11)(*[(x - 256 if x > 127 else x) for x in data]), C.byref(n1), C.byref(n2))
    assert (n1.value, n2.value) == (n, m)
    got = _unpk(L, "orc_unpk", {"data": data[:7], "pre_hash": []})
    assert got[0] == 0 and got[2:5] == ("K1JT", "FN20", "20")


@pytest.mark.skipif(ol.ref_lib() is None, reason="oracle/_ref not built")
def test_oracle_equals_real_reference_objects_on_random_inputs():
    """Live cross-check against the compiled reference sources (more cases than the JSON)."""
    L, R = ol.lib(), ol.ref_lib()
    rng = np.random.default_rng(7)
    mt = (C.c_int * 256 * 2)(); L.orc_build_mettab(mt)
    for t in range(60):
        soft = rng.integers(0, 256, 162).astype(np.uint8) if t % 3 == 0 else \
            np.clip(np.where(rng.integers(0, 2, 162) > 0, 180, 76) + rng.normal(0, 30, 162), 0, 255).astype(np.uint8)
        res = []
        for lib, fn in ((L, "orc_fano"), (R, "fano")):
            s = (C.c_ubyte * 162)(*soft.tolist())
            dec = (C.c_ubyte * 11)(); a = C.c_uint(); b = C.c_uint(); c = C.c_uint()
            r = getattr(lib, fn)(C.byref(a), C.byref(b), C.byref(c), dec, s, C.c_uint(81), mt, C.c_int(60), C.c_uint(300))
            res.append((r, a.value, b.value, c.value, list(dec)[:10] if r == 0 else None))
        assert res[0] == res[1]
    for t in range(2000):
        n = int(rng.integers(0, 1 << 28)); m = int(rng.integers(0, 1 << 22))
        d = [(n >> 20) & 255, (n >> 12) & 255, (n >> 4) & 255, ((n & 15) << 4) | ((m >> 18) & 15),
             (m >> 10) & 255, (m >> 2) & 255, (m & 3) << 6]
        v = {"data": d, "pre_hash": []}
        assert _unpk(L, "orc_unpk", v) == _unpk(R, "unpk_", v)


def test_oracle_reproduces_committed_scene_spots():
    """tests/golden/scene_spots.json (made by make_scene_vectors.py from this oracle): a regression pin --
    any edit of oracle/ that changes a decision or a reported float shows up here."""
    import json
    import scenes
    gold = json.load(open(os.path.join(ol.GOLDEN, "scene_spots.json")))["scenes"]
    assert [g["seed"] for g in gold] == scenes.GOLDEN_SEEDS
    for g in gold:
        I, Q = scenes.make_scene(g["seed"])
        spots, _, _ = ol.decode(I, Q, scenes.NS)
        assert [scenes.spot_record(s) for s in spots] == g["spots"], g["seed"]
    assert sum(len(g["spots"]) for g in gold) >= 25


# ------------------------------------------------------- front-end constants
def test_front_end_constants_equal_the_reference_source():
    """The decimator has no reference-held fixture (its translation unit needs librtlsdr/libcurl), so its
    CONSTANTS at least, as read out of the reference source into tests/golden/front_end_constants.json, are compared
    with what the oracle and the product use: the 33 zCoef taps (rtlsdr_wsprd.c:142-152), SAMPLING_RATE /
    SIGNAL_SAMPLE_RATE (:38-39) and the '<= DOWNSAMPLING' test that makes the ratio 6401 (:199)."""
    import json
    import rtlsdr_wsprd_amd as w
    ot = (C.c_float * 33)(); orr = C.c_int()
    ol.lib().orc_front_end_constants(ot, C.byref(orr))
    pt = (C.c_float * 33)(); pr = C.c_int()
    w.lib().wspr_front_end_constants(pt, C.byref(pr))
    assert list(ot) == list(pt) and orr.value == pr.value == 6401
    with open(os.path.join(ol.GOLDEN, "front_end_constants.json")) as f:
        ref = json.load(f)
    taps = [np.float32(float(x)) for x in ref["zCoef"]]
    assert len(taps) == 33 and [float(t) for t in taps] == [float(np.float32(x)) for x in ot]
    rate, out_rate = ref["SAMPLING_RATE"], ref["SIGNAL_SAMPLE_RATE"]
    assert ref["decimation_test"] == "<="                                   # <=, hence one more than the quotient
    assert rate // out_rate + 1 == orr.value
