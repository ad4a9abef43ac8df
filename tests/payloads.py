"""Channel symbols for ANY 50-bit WSPR payload, built from the bit layout alone (test helper, no product code).

get_wspr_channel_symbols() only encodes what a text packs to, so it cannot produce the payloads a decoder must cope with
although no well-formed text yields them: an invalid call, a grid past the table, a type-3 message with ntype -64, a
hash nobody stored.  Here the payload (n1: 28-bit call field, n2: 22-bit grid/power field) goes straight through the
K=32 rate-1/2 convolutional code (polynomials 0xf2d05351 / 0xe4613c47), the bit-reversal interleaver and the sync
vector.  The sync vector is read off a valid message's symbols (symbol & 1), not typed in.

CATALOGUE names one payload per path at the end of the reference's candidate loop (wsprd.c:768-822) plus ordinary
control messages; each entry says what it is meant to exercise, and tests/test_payload_paths.py checks that it does.
"""
import numpy as np

NSYM = 162
POLY = (0xF2D05351, 0xE4613C47)
NCALL_MAX = 262177560                 # unpackcall() accepts n1 < 37*36*10*27*27*27
NGRID_MAX = 32400                     # unpackgrid() accepts n2 >> 7 < 180*180
HASH_N = 32768


# ------------------------------------------------------------------------------------------------ packing by meaning
def _call_code(ch):
    if ch.isdigit():
        return ord(ch) - 48
    if ch == " ":
        return 36
    if "A" <= ch <= "Z":
        return ord(ch) - 55
    raise ValueError(ch)


def pack_call6(call):
    """28-bit call field of a type-1 call (the digit at index 2, or at index 1 with a leading space added)."""
    if len(call) > 6:
        raise ValueError(call)
    if len(call) > 2 and call[2].isdigit():
        six = call.ljust(6)
    elif len(call) > 1 and call[1].isdigit():
        six = (" " + call).ljust(6)[:6]
    else:
        raise ValueError(call)
    c = [_call_code(x) for x in six]
    n = c[0]
    n = n * 36 + c[1]
    n = n * 10 + c[2]
    for k in (3, 4, 5):
        n = n * 27 + c[k] - 10
    return n


def pack_grid4_power(grid, power):
    """22-bit field of a type-1 message: 4-character locator and power (any ntype = power, 0..63)."""
    g = [ord(x) - 65 if x.isalpha() else ord(x) - 48 for x in grid.upper()]
    m = (179 - 10 * g[0] - g[2]) * 180 + 10 * g[1] + g[3]
    return m * 128 + power + 64


def nhash(s, initval=146):
    """Bob Jenkins' lookup3 hashlittle() over the bytes of s, masked to 15 bits (what the WSPR hashed calls use)."""
    k = s.encode() if isinstance(s, str) else bytes(s)
    M = 0xFFFFFFFF
    rol = lambda x, r: ((x << r) | (x >> (32 - r))) & M
    a = b = c = (0xDEADBEEF + len(k) + initval) & M
    n = len(k)
    while n > 12:
        a = (a + int.from_bytes(k[0:4], "little")) & M
        b = (b + int.from_bytes(k[4:8], "little")) & M
        c = (c + int.from_bytes(k[8:12], "little")) & M
        a = (a - c) & M; a ^= rol(c, 4); c = (c + b) & M
        b = (b - a) & M; b ^= rol(a, 6); a = (a + c) & M
        c = (c - b) & M; c ^= rol(b, 8); b = (b + a) & M
        a = (a - c) & M; a ^= rol(c, 16); c = (c + b) & M
        b = (b - a) & M; b ^= rol(a, 19); a = (a + c) & M
        c = (c - b) & M; c ^= rol(b, 4); b = (b + a) & M
        k, n = k[12:], n - 12
    if n == 0:
        return c
    t = k.ljust(12, b"\0")
    a = (a + int.from_bytes(t[0:4], "little")) & M
    b = (b + int.from_bytes(t[4:8], "little")) & M
    c = (c + int.from_bytes(t[8:12], "little")) & M
    c ^= b; c = (c - rol(b, 14)) & M
    a ^= c; a = (a - rol(c, 11)) & M
    b ^= a; b = (b - rol(a, 25)) & M
    c ^= b; c = (c - rol(b, 16)) & M
    a ^= c; a = (a - rol(c, 4)) & M
    b ^= a; b = (b - rol(a, 14)) & M
    c ^= b; c = (c - rol(b, 24)) & M
    return c & (HASH_N - 1)


def type1(call, grid, power):
    return pack_call6(call), pack_grid4_power(grid, power)


def type3(hashed_call, grid6, power, ntype=None):
    """Hashed call + 6-character locator: n1 carries the locator rotated by one (grid6[1:] + grid6[0]), n2 the 15-bit
    hash and ntype = -(power + 1)."""
    ntype = -(power + 1) if ntype is None else ntype
    ih = nhash(hashed_call) if isinstance(hashed_call, str) else int(hashed_call)
    return pack_call6(grid6[1:] + grid6[0]), 128 * ih + ntype + 64


# ------------------------------------------------------------------------------------------------ payload -> symbols
def data11(n1, n2):
    """The 11 bytes fed to the encoder: 28 + 22 payload bits, MSB first, then zeros (wsprsim_utils.c layout)."""
    assert 0 <= n1 < (1 << 28) and 0 <= n2 < (1 << 22), (n1, n2)
    return [(n1 >> 20) & 255, (n1 >> 12) & 255, (n1 >> 4) & 255, ((n1 & 15) << 4) | ((n2 >> 18) & 15),
            (n2 >> 10) & 255, (n2 >> 2) & 255, (n2 & 3) << 6, 0, 0, 0, 0]


def _taps(poly):
    return np.array([k for k in range(32) if (poly >> k) & 1])


_TAPS = [_taps(p) for p in POLY]


def conv_encode(data):
    """162 code bits of the first 81 data bits: at bit t the encoder state holds bit t in its LSB and bit t-k at
    position k; the output pair is (parity(state & POLY[0]), parity(state & POLY[1]))."""
    bits = np.unpackbits(np.asarray(data, np.uint8))[:81].astype(np.int64)
    padded = np.concatenate([np.zeros(31, np.int64), bits])
    t = np.arange(81) + 31
    out = np.empty(NSYM, np.uint8)
    for p, taps in enumerate(_TAPS):
        out[p::2] = (padded[t[:, None] - taps[None, :]].sum(axis=1) & 1).astype(np.uint8)
    return out


def _bitrev8(i):
    return int("{:08b}".format(i)[::-1], 2)


INTERLEAVE = np.array([j for j in (_bitrev8(i) for i in range(256)) if j < NSYM])   # p-th code bit -> position


def interleave(bits):
    out = np.empty(NSYM, np.uint8)
    out[INTERLEAVE] = bits
    return out


_SYNC = None


def sync_bits():
    """The 162-bit sync vector: the low bit of every channel symbol of a valid message."""
    global _SYNC
    if _SYNC is None:
        import oracle_lib as ol
        ok, sym = ol.channel_symbols("K1ABC FN42 37")
        assert ok
        _SYNC = (sym & 1).astype(np.uint8)
    return _SYNC


def payload_symbols(n1, n2):
    return (sync_bits() + 2 * interleave(conv_encode(data11(n1, n2)))).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------ catalogue
def _t1(text):
    c, g, p = text.split()
    return type1(c, g, int(p))


# name -> (n1, n2, what it exercises).  "K1XYZ" is never sent in plain form in any test scene, so its hash is unknown.
CATALOGUE = {
    # ordinary control messages
    "ctrl_a": _t1("W1AW FN31 30") + ("type 1, decodes, re-encodes, is subtracted",),
    "ctrl_b": _t1("G4ABC IO91 27") + ("type 1",),
    "ctrl_c": _t1("JA1XYZ PM95 20") + ("type 1",),
    "ctrl_t1": _t1("K1ABC FN42 37") + ("type 1 that stores K1ABC's hash",),
    # the early exits of the candidate loop
    "A000AA": type3("K1ABC", "A000AA", 37) + ("loc == 'A000AA' (n1 == 0): breaks out of the candidate loop, wsprd.c:791-793",),
    "K1A": type1("K1A", "FN20", 37) + ("3-character call: unpacks (noprint 0) but does not re-encode: break, wsprd.c:786-788",),
    # unpk_ returns early: a spot with empty texts
    "bad_call": (NCALL_MAX + 1234, pack_grid4_power("FN20", 37), "unpackcall fails: spot with empty texts, callsign '......'"),
    "bad_grid": (pack_call6("K1ABC"), ((NGRID_MAX + 17) << 7) + 37 + 64,
                 "unpackgrid fails: spot with empty texts, de-duplicated on the callsign written before"),
    # (the power of a type-2 payload always ends in 0, 3 or 7, so its "bad power" noprint cannot happen, as
    #  tests/test_payload_paths.py shows; the type-2 payload that does give noprint is a prefix unpackpfx rejects)
    "t2_bad_prefix": (pack_call6("K1ABC"), 128 * 50 + 64 + 6,
                      "type 2 with nadd 3: the suffix code (char)(50 + 65536 - 60000) is negative, unpackpfx fails: "
                      "spot with empty texts"),
    "t3_ntype_m64": type3("K1ABC", "FN42AB", 0, ntype=-64) + ("type 3 with ntype -64: texts written, noprint",),
    "t3_bad_grid": type3("K1ABC", "CKA1AB", 37) + ("type 3 whose locator is not letter-letter-digit-digit: noprint",),
    "t3_unknown_hash": type3("K1XYZ", "FN42AB", 37) +
                       ("type 3 of an unknown hash: '<...>', re-encoded with nhash('...'): a wrong signal is subtracted",),
}


def symbols_of(name):
    n1, n2, _ = CATALOGUE[name]
    return payload_symbols(n1, n2)


# ------------------------------------------------------------------------------------------------------ scenes
NS = 45000
CONTROLS = (("ctrl_a", -8.0), ("ctrl_b", -14.0), ("ctrl_c", -20.0))


def scene(parts, seed=0, noise=True):
    """One segment: parts = [(catalogue name, snr dB, f0 Hz)], each sent at t0 = 2 s + a few ms; complex AWGN of unit
    power in 2500 Hz (tests/synth.py's model) and the receiver's normalisation."""
    import synth
    rng = np.random.default_rng(seed)
    sigma = np.sqrt((375.0 / 2500.0) / 2.0)
    I = rng.normal(0, sigma, NS) if noise else np.zeros(NS)
    Q = rng.normal(0, sigma, NS) if noise else np.zeros(NS)
    for name, snr, f0 in parts:
        si, sq = synth.tone_signal(symbols_of(name), f0, 2.0 + rng.uniform(-0.05, 0.05), 10.0 ** (snr / 20.0))
        I += si; Q += sq
    return synth.normalise(I.astype(np.float32), Q.astype(np.float32))


def stopper_scene(name, seed=0, snr=-11.0):
    """Three control messages at -8, -14 and -20 dB and the payload `name` at `snr` (between the first two: every pass
    meets it right after the strongest control)."""
    freqs = [-75.0, 5.0, 55.0]
    parts = [(c, s, f) for (c, s), f in zip(CONTROLS, freqs)] + [(name, snr, -35.0)]
    return scene(parts, seed)


def text_of(name):
    """What the decoder reports for a control message."""
    return {"ctrl_a": "W1AW FN31 30", "ctrl_b": "G4ABC IO91 27", "ctrl_c": "JA1XYZ PM95 20",
            "ctrl_t1": "K1ABC FN42 37"}[name]


def loop_exit_scenes():
    """The crafted scene set: (label, I, Q).  Every stopper next to the controls; two scenes where the stopper follows
    three strong noprint decodes (nothing subtracted before it: a speculative window of the subtraction pass has grown
    past one candidate when the stop comes); one where it directly follows two subtractions (the window is cut to one)."""
    out = [(name, *stopper_scene(name, seed=1)) for name in
           ("A000AA", "K1A", "bad_call", "bad_grid", "t2_bad_prefix", "t3_ntype_m64", "t3_bad_grid", "t3_unknown_hash")]
    noprints = [("t3_ntype_m64", -4.0, -110.0), ("t3_bad_grid", -5.5, -80.0), ("bad_call", -7.0, -50.0)]
    for stopper in ("K1A", "A000AA"):
        out.append(("window_" + stopper,
                    *scene(noprints + [(stopper, -10.0, -20.0), ("ctrl_b", -14.0, 20.0), ("ctrl_c", -20.0, 60.0)], seed=3)))
    out.append(("cut_A000AA", *scene([("ctrl_a", -6.0, -90.0), ("ctrl_b", -8.0, -40.0), ("A000AA", -10.0, 10.0),
                                      ("ctrl_c", -18.0, 60.0)], seed=4)))
    return out
