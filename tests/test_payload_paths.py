"""The branches at the end of the reference's candidate loop (wsprd.c:768-822), on payloads no well-formed text packs to
(tests/payloads.py).  No GPU: the payload encoder against the oracle's, every catalogue payload against what the real
reference objects (oracle/_ref), the oracle and the product's host message layer make of it, and the oracle's decode of
scenes that carry one of them pinned to the spots the reference's loop gives by reading: a re-encode failure or an
"A000AA" locator ends the pass, a noprint decode is reported and not subtracted, an unknown hash subtracts a wrong signal.
tests/test_gpu_loop_exits.py holds the product to the same on the GPU."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import payloads as P
import synth

NS = P.NS
OPTION_SETS = [dict(), dict(subtraction=0), dict(npasses=1), dict(npasses=3), dict(quickmode=1)]
STOPPERS = ["A000AA", "K1A", "bad_call", "bad_grid", "t2_bad_prefix", "t3_ntype_m64", "t3_bad_grid", "t3_unknown_hash"]
CONTROL_TEXTS = [P.text_of(c) for c, _ in P.CONTROLS]


def expected_messages(name, opts):
    """Spot texts (strongest first) the reference's loop gives on P.stopper_scene(name), by reading wsprd.c:768-822."""
    a, b, c = CONTROL_TEXTS
    if name == "A000AA":                               # every pass meets it right after the -8 dB control and breaks
        return [a]
    if name == "K1A":                                  # breaks where it would be re-encoded (pass 0 with subtraction);
        if opts.get("npasses", 2) == 1 and opts.get("subtraction", 1):   # any later pass reports it and the rest
            return [a]
        return [a, "K1A FN20 37", b, c]
    middle = {"bad_call": "", "bad_grid": "", "t2_bad_prefix": "", "t3_ntype_m64": "<...> FN42AB 63",
              "t3_bad_grid": "<...> CKA1AB 37", "t3_unknown_hash": "<...> FN42AB 37"}[name]
    return [a, middle, b, c]


# ------------------------------------------------------------------------------------------------------ the encoder
def _type2_payload(text):
    call, pwr = text.split()
    n = C.c_int32(); m = C.c_int32(); nadd = C.c_int32()
    ol.lib().orc_pack_prefix(C.create_string_buffer(call.encode(), 16), C.byref(n), C.byref(m), C.byref(nadd))
    return n.value, 128 * m.value + int(pwr) + 1 + nadd.value + 64


def test_payload_encoder_equals_channel_symbols():
    rng = np.random.default_rng(50)
    for idx in rng.integers(0, 1 << 62, 2000):
        msg = synth.message_wide(int(idx))
        c, g, p = msg.split()
        ok, sym = ol.channel_symbols(msg)
        assert ok and np.array_equal(P.payload_symbols(*P.type1(c, g, int(p))), sym), msg
    n23 = 0
    for st in range(len(synth.STATIONS)):
        for seg in (0, 1):
            msg = synth.station_message(st, seg)
            ok, sym = ol.channel_symbols(msg)
            if msg.startswith("<"):
                call, grid6, pwr = msg.split()
                n1, n2 = P.type3(call.strip("<>"), grid6, int(pwr))
            else:
                n1, n2 = _type2_payload(msg)
            assert ok and np.array_equal(P.payload_symbols(n1, n2), sym), msg
            n23 += 1
    assert n23 == 2 * len(synth.STATIONS)
    # the 11 bytes are the layout of the reference's unit test (tests/test_message_layer.py)
    n, m = P.type1("K1JT", "FN20", 20)
    assert P.data11(n, m)[:7] == [(n >> 20) & 255, (n >> 12) & 255, (n >> 4) & 255, ((n & 15) << 4) + ((m >> 18) & 15),
                                  (m >> 10) & 255, (m >> 2) & 255, (m & 3) << 6]


def test_packers_and_hash_equal_the_oracle():
    L = ol.lib()
    for call in ["K1ABC", "W1AW", "K1A", "VA2GKA", "000AAA", "N42ABF", "KA1ABC"]:
        assert P.pack_call6(call) == L.orc_pack_call(call.encode()), call
    for s in ["K1ABC", "K1XYZ", "...", "PJ4/K1ABC", "a much longer text than twelve bytes", ""]:
        assert P.nhash(s) == L.orc_nhash(s.encode(), len(s), 146), s       # ("" : unmasked in both, nhash.c:443)


# ------------------------------------------------------------------------------------------------------ the catalogue
def _unpk(lib, fn, n1, n2, tables):
    hashtab, loctab = tables
    d = P.data11(n1, n2)
    msg = (C.c_byte * 12)(*[(b - 256 if b > 127 else b) for b in d] + [0])
    clp = C.create_string_buffer(23); call = C.create_string_buffer(13); loc = C.create_string_buffer(7)
    pwr = C.create_string_buffer(3); cs = C.create_string_buffer(13)
    r = getattr(lib, fn)(msg, hashtab, loctab, clp, call, loc, pwr, cs)
    return int(r), clp.value.decode("latin1"), call.value.decode("latin1"), loc.value.decode("latin1"), cs.value.decode("latin1")


def _encode(lib, fn, text, tables):
    sym = (C.c_ubyte * 162)()
    ok = getattr(lib, fn)(C.create_string_buffer(text.encode(), 32), tables[0], tables[1], sym)
    return int(ok), np.frombuffer(sym, np.uint8).copy()


def _tables():
    return C.create_string_buffer(32768 * 13), C.create_string_buffer(32768 * 5)


# name -> (unpk_ return, call_loc_pow, loc, callsign, re-encodes) with fresh hash tables
CATALOGUE_EXPECT = {
    "ctrl_a": (0, "W1AW FN31 30", "FN31", "W1AW", True),
    "ctrl_b": (0, "G4ABC IO91 27", "IO91", "G4ABC", True),
    "ctrl_c": (0, "JA1XYZ PM95 20", "PM95", "JA1XYZ", True),
    "ctrl_t1": (0, "K1ABC FN42 37", "FN42", "K1ABC", True),
    "A000AA": (1, "<...> A000AA 37", "A000AA", "<...>", None),
    "K1A": (0, "K1A FN20 37", "FN20", "K1A", False),
    "bad_call": (1, "", "", "......", None),
    "bad_grid": (1, "", "", "K1ABC", None),
    "t2_bad_prefix": (1, "", "", "K1ABC", None),
    "t3_ntype_m64": (1, "<...> FN42AB 63", "FN42AB", "<...>", None),
    "t3_bad_grid": (1, "<...> CKA1AB 37", "CKA1AB", "<...>", None),
    "t3_unknown_hash": (0, "<...> FN42AB 37", "FN42AB", "<...>", True),
}


def _message_layers():
    import rtlsdr_wsprd_amd as w
    layers = [(ol.lib(), "orc_unpk", "orc_channel_symbols"), (w.lib(), "unpk_", "get_wspr_channel_symbols")]
    R = ol.ref_lib()
    return ([(R, "unpk_", "get_wspr_channel_symbols")] if R is not None else []) + layers


def test_catalogue_payloads_take_their_paths():
    """Against the real reference objects where oracle/_ref is built, and always against the oracle and the product."""
    assert set(CATALOGUE_EXPECT) == set(P.CATALOGUE)
    for name, (n1, n2, _) in P.CATALOGUE.items():
        noprint, text, loc, callsign, encodes = CATALOGUE_EXPECT[name]
        for lib, unpk, chan in _message_layers():
            t = _tables()
            r, clp, call, lc, cs = _unpk(lib, unpk, n1, n2, t)
            assert (r, clp, lc, cs) == (noprint, text, loc, callsign), (name, unpk, (r, clp, lc, cs))
            if not noprint:                    # the decoder re-encodes what it prints (subtraction branch)
                ok, sym = _encode(lib, chan, clp, t)
                assert bool(ok) == encodes, (name, chan)
                if name == "t3_unknown_hash":  # "<...>" re-encodes as the hash of "...": another signal
                    assert ok and not np.array_equal(sym, P.payload_symbols(n1, n2))
                    assert np.array_equal(sym, P.payload_symbols(*P.type3("...", "FN42AB", 37)))
                elif ok:
                    assert np.array_equal(sym, P.payload_symbols(n1, n2)), name
    # the A000AA payload is a type 3 of a KNOWN call too: once K1ABC is stored its text resolves, the locator stays
    for lib, unpk, _ in _message_layers():
        t = _tables()
        _unpk(lib, unpk, *P.CATALOGUE["ctrl_t1"][:2], t)
        assert _unpk(lib, unpk, *P.CATALOGUE["A000AA"][:2], t)[:4] == (1, "<K1ABC> A000AA 37", "<K1ABC>", "A000AA")


def test_type2_power_is_never_bad():
    """wsprd_utils.c:276-285 gives a type-2 decode noprint when its power does not end in 0, 3 or 7; ntype - nadd always
    does, so that branch cannot fire (the catalogue's type-2 noprint payload is a prefix unpackpfx rejects instead)."""
    for lib, unpk, _ in _message_layers():
        for ntype in range(0, 63):
            if ntype % 10 in (0, 3, 7):
                continue
            r, clp, *_ = _unpk(lib, unpk, P.pack_call6("K1ABC"), 128 * 100 + ntype + 64, _tables())
            assert r == 0 and "/" in clp, (unpk, ntype, clp)


# ------------------------------------------------------------------------------------------------------ the oracle pin
@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "defaults")
@pytest.mark.parametrize("name", STOPPERS)
def test_oracle_loop_exits_follow_the_reference(name, opts):
    I, Q = P.stopper_scene(name, seed=1)
    spots, _, _, tr = ol.decode(I, Q, NS, ol.default_options(**opts), trace=True)
    assert [s.message.decode() for s in spots] == expected_messages(name, opts), (name, opts)
    if name in ("bad_call", "bad_grid", "t2_bad_prefix"):                    # unpk_ returned early: empty texts
        (odd,) = [s for s in spots if s.message.decode() == ""]
        assert (odd.call, odd.loc, odd.pwr) == (b"", b"", b"")
    # where the pass left the candidate loop, and why
    npasses = opts.get("npasses", 2)
    assert tr.passes_run == npasses
    subtracting = opts.get("subtraction", 1)
    for p in range(npasses):
        if name == "A000AA":
            want = 2
        elif name == "K1A" and p == 0 and subtracting:
            want = 1
        else:
            want = 0
        assert tr.stop_reason[p] == want, (p, tr.stop_reason[p])
        if want:
            j = tr.stop_cand[p]
            assert tr.n_visited[p] == j + 1 and tr.decoded[p][j] and not tr.subtracted[p][j]
            assert abs(tr.cand_fine[p][j].freq - (-35.0)) < 1.0          # the crafted signal, not a control
        else:
            assert tr.stop_cand[p] == 0
            assert tr.n_visited[p] == tr.npk[p]


NOPRINT = ["bad_call", "bad_grid", "t2_bad_prefix", "t3_ntype_m64", "t3_bad_grid"]


@pytest.mark.parametrize("name", NOPRINT + ["A000AA"])
def test_oracle_reports_noprint_without_subtracting_it(name):
    """Alone in its segment the payload decodes and (but for A000AA) is reported; the residual is the input: nothing was
    subtracted.  Next to the controls, its candidate is decoded and not subtracted while the controls are."""
    I, Q = P.scene([(name, -11.0, -35.0)], seed=2)
    spots, ri, rq, tr = ol.decode(I, Q, NS, ol.default_options(), trace=True)
    assert len(spots) == (0 if name == "A000AA" else 1)
    assert sum(tr.decoded[0][j] for j in range(tr.n_visited[0])) == 1
    assert np.array_equal(ri, I) and np.array_equal(rq, Q)
    if name == "A000AA":
        return
    I, Q = P.stopper_scene(name, seed=1)
    spots, _, _, tr = ol.decode(I, Q, NS, ol.default_options(), trace=True)
    dec = [(tr.cand_fine[0][j].freq, tr.subtracted[0][j]) for j in range(tr.n_visited[0]) if tr.decoded[0][j]]
    assert sorted(round(f) for f, _ in dec) == [-75, -35, 5, 55]
    assert [(round(f), s) for f, s in dec if s == 0] == [(-35, 0)]


def test_oracle_subtracts_a_wrong_signal_for_an_unknown_hash():
    """'<...>' re-encodes with nhash("...") (wsprsim_utils.c:212-230): the residual is the input minus THAT signal,
    not the input minus the one that was sent."""
    name = "t3_unknown_hash"
    I, Q = P.scene([(name, -11.0, -35.0)], seed=2)
    spots, ri, rq, tr = ol.decode(I, Q, NS, ol.default_options(), trace=True)
    assert [s.message.decode() for s in spots] == ["<...> FN42AB 37"]
    (j,) = [j for j in range(tr.n_visited[0]) if tr.subtracted[0][j]]
    f = tr.cand_fine[0][j]

    def subtracted(sym):
        i, q = I.copy(), Q.copy()
        ol.lib().orc_subtract(ol.ptr(i), ol.ptr(q), NS, f.freq, f.shift, f.drift, ol.ptr(np.ascontiguousarray(sym)))
        return i, q
    wi, wq = subtracted(P.payload_symbols(*P.type3("...", "FN42AB", 37)))
    assert np.array_equal(ri, wi) and np.array_equal(rq, wq)
    ei, eq = subtracted(P.symbols_of(name))
    assert not np.array_equal(ri, ei)
    # the exact subtraction leaves much less of the signal behind than the wrong one
    assert np.sum((ei - I) ** 2) > 0 and np.sum(ri.astype(np.float64) ** 2) > np.sum(ei.astype(np.float64) ** 2)
