"""Ordered-statistics decoding on the device (K9, wspr_osd_batch_device / wspr_set_osd_depth; definition in
rtlsdr-wsprd_amd/csrc/kernels/osd.h): the kernel against the serial CPU checker field for field, the setter, "off is
off", the rescue stage inside the decode loop against checker + gate on the loop's own trace, and the ordering of the
"heard before" look-up in a batch with usehashtable."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as orc
import osd_lib as ol
import synth

pytestmark = pytest.mark.gpu
NS = 45000
MINSYNC2, MINRMS = 0.12, 52.0 * (50 / 64.0)          # the Fano gate of wsprd.c:758 on passes 0 and 1 (wsprd.c:423-433)


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    return mod


@pytest.fixture(scope="module")
def vectors():
    """The noise ladder of tests/test_fano_wave.py plus the degenerate vectors, 257 in all, and the checker's answer for
    every one of them at every depth (computed once)."""
    lad, _ = ol.ladder_vectors(257 - len(ol.degenerate_vectors()))
    vec = np.concatenate([ol.degenerate_vectors(), lad])
    assert vec.shape == (257, 162)
    want = {d: [ol.check(v, d) for v in vec] for d in range(4)}
    return vec, want


@pytest.fixture()
def depth_off(w):
    """Whatever a test sets, the next one starts with the stage off -- in both libraries."""
    yield
    for L in (w.lib(), w.lab()):
        w.set_osd_depth(-1, L)
        L.wspr_set_fano_device_mode(-1)


def _got(w, vec, depth):
    data, dist, nhard, order = w.osd_batch(vec, depth)
    return [(tuple(int(x) for x in data[i]), int(dist[i]), int(nhard[i]), int(order[i])) for i in range(len(vec))]


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_kernel_equals_the_checker(w, vectors, depth):
    vec, want = vectors
    for n in (1, 64, 65, 257):                           # one launch group, its edge, one over, several
        got = _got(w, vec[:n], depth)
        bad = [i for i in range(n) if got[i] != want[depth][i]]
        assert not bad, (depth, n, bad[:5], got[bad[0]], want[depth][bad[0]])
    # vectors elsewhere in the batch do not matter: the last 65 alone
    assert _got(w, vec[-65:], depth) == want[depth][-65:]


def test_entry_point_arguments(w, vectors):
    vec, _ = vectors
    L = w.lib()
    guard = np.full(16, 0xA5, np.uint8)
    d = guard.copy()
    u = [np.full(2, 0xA5A5A5A5, np.uint32) for _ in range(3)]
    args = (d.ctypes.data, u[0].ctypes.data, u[1].ctypes.data, u[2].ctypes.data)
    assert L.wspr_osd_batch_device(vec.ctypes.data, 0, 3, *args) == 0             # n == 0: nothing happens
    assert L.wspr_osd_batch_device(vec.ctypes.data, 1, 4, *args) == -1            # depth outside 0..3
    assert L.wspr_osd_batch_device(vec.ctypes.data, 1, -1, *args) == -1
    assert L.wspr_osd_batch_device(vec.ctypes.data, -1, 2, *args) == -1           # n < 0
    assert np.array_equal(d, guard) and all(np.all(x == 0xA5A5A5A5) for x in u)   # and nothing was written


def _symbols(msg):
    ok, s = orc.channel_symbols(msg)
    assert ok, msg
    return s


def _tup(x):
    return (x.message, x.call, x.loc, x.pwr, x.cycles, x.jitter, x.drift, x.sync, x.snr, x.dt, x.freq)


def _decode_writeback(w, I, Q, opt, K=16):
    """wspr_decode_batch with writeback: (spots per segment, residual I, residual Q)."""
    I, Q = I.copy(), Q.copy()
    nseg = I.shape[0]
    out = (w.decoder_results * (nseg * K))()
    nres = (C.c_int * nseg)()
    rc = w.lib().wspr_decode_batch(orc.ptr(I), orc.ptr(Q), nseg, NS, NS, opt, C.addressof(out), K, C.addressof(nres), 1)
    assert rc == 0, rc
    return [[_tup(out[s * K + i]) for i in range(nres[s])] for s in range(nseg)], I, Q


def test_off_is_off_after_the_stage_was_switched_on_and_off(w, depth_off):
    """A crowded 64-segment scene at the default, then the same scene after wspr_set_osd_depth(3) and (-1): spots and
    residual IQ byte for byte.  (Runs before any test of this file sets a depth.)"""
    segs = [synth.make_segment(7000 + s, _symbols, n_signals=3, snr_db=-12.0, snr_span=16.0, t_jitter=0.5) for s in range(64)]
    I, Q = np.stack([x[0] for x in segs]), np.stack([x[1] for x in segs])
    before = _decode_writeback(w, I, Q, w.default_options())
    assert sum(len(x) for x in before[0]) >= 64
    assert w.set_osd_depth(3) == -1 and w.set_osd_depth(-1) == 3
    after = _decode_writeback(w, I, Q, w.default_options())
    assert after[0] == before[0]
    assert after[1].tobytes() == before[1].tobytes() and after[2].tobytes() == before[2].tobytes()
    t = w.last_timings()
    assert t["osd_ms"] == 0 and t["osd_vectors"] == 0 and t["osd_spots"] == 0


def test_unknown_calls_are_never_rescued_without_the_hash_memory(w, depth_off):
    """usehashtable = 0: the hash memory is each segment's own and starts empty.  One signal per segment, every call
    different: half of them decodable (-22 dB), half far below the Fano threshold (-31 dB: candidates that pass the
    sync/rms gate, fail every Fano attempt and go through K9).  Depth 3 must report exactly what depth -1 reports."""
    rng = np.random.default_rng(99)
    sigma = np.sqrt((375.0 / 2500.0) / 2.0)
    I = np.empty((64, NS), np.float32); Q = np.empty((64, NS), np.float32)
    for s in range(64):
        m = synth.message_wide(int(rng.integers(0, 1 << 62)))
        si, sq = synth.tone_signal(_symbols(m), rng.uniform(-100, 100), 2.0 + rng.uniform(-0.5, 0.5),
                                   10.0 ** ((-22.0 if s % 2 == 0 else -31.0) / 20.0))
        I[s], Q[s] = synth.normalise((rng.normal(0, sigma, NS) + si).astype(np.float32),
                                     (rng.normal(0, sigma, NS) + sq).astype(np.float32))
    off = [[_tup(x) for x in g] for g in w.wspr_decode_batch(I, Q, w.default_options())]
    assert w.set_osd_depth(3) == -1
    on = [[_tup(x) for x in g] for g in w.wspr_decode_batch(I, Q, w.default_options())]
    t = w.last_timings()
    print("depth 3, own tables: %d vectors tried in %.2f ms, %d accepted" % (t["osd_vectors"], t["osd_ms"], t["osd_spots"]))
    assert on == off and sum(len(x) for x in off) >= 24
    assert t["osd_vectors"] > 0 and t["osd_spots"] == 0


def test_setter_returns_the_previous_value(w, depth_off):
    assert w.set_osd_depth(-1) == -1                      # the default is off
    assert w.set_osd_depth(2) == -1 and w.set_osd_depth(0) == 2 and w.set_osd_depth(3) == 0
    assert w.set_osd_depth(4) == -2 and w.set_osd_depth(-2) == -2 and w.set_osd_depth(100) == -2
    assert w.set_osd_depth(-1) == 3                       # the refused values changed nothing


def _prime(path, calls):
    """hashtable.txt as the decoder writes it (wsprd.c:842-852): the calls a receiver has heard before."""
    import rtlsdr_wsprd_amd as mod
    with open(path, "w") as f:
        for slot, call in sorted((mod.lib().nhash(c.encode(), len(c), 146), c) for c in calls):
            f.write("%5d %s %s\n" % (slot, call, "AA00"))


def _flat_table(w, calls):
    hashtab = np.zeros(32768 * 13, np.uint8)
    for c in calls:
        slot = w.lib().nhash(c.encode(), len(c), 146)
        hashtab[slot * 13:slot * 13 + len(c)] = np.frombuffer(c.encode(), np.uint8)
    return hashtab, np.zeros(32768 * 5, np.uint8)


def _text_of(w, data):
    """The text a decoded message unpacks to (unpk_ on scratch tables)."""
    h, l = C.create_string_buffer(32768 * 13), C.create_string_buffer(32768 * 5)
    msg = (C.c_byte * 12)(*[x - 256 if x > 127 else x for x in data], 0)
    out = [C.create_string_buffer(32) for _ in range(5)]
    w.lib().unpk_(msg, h, l, *out)
    return out[0].value.decode()


@pytest.mark.parametrize("fano_on_device", [0, 1])
def test_rescue_stage_against_checker_and_gate(w, tmp_path, depth_off, fano_on_device):
    """24 single-signal segments at -30 dB (tests/synth.py make_segment, seeds 5000..5023; messages of the twenty calls of
    synth.CALLS, all in the primed hashtable.txt).  The seeds were chosen on the CPU (`python tools/osd_rescue_seeds.py -30
    5000 5024` prints it): on the oracle's trace of these segments Fano decodes 6 of them and, on the rung-0 symbols of
    candidates the oracle leaves undecoded, the checker at depth 3 plus the gate recovers the transmitted message in 7
    more (seeds 5005, 5011, 5015, 5016, 5017, 5022, 5023).
    Here the product's own trace is held to the checker, once with the Fano attempts on the host pool and once with all of
    them on the device (the stage follows either path): every decode it reports with cycles == 0 is the checker's answer
    for that candidate's first_symbols and passes the gate, carries a transmitted message, and every visited, undecoded
    candidate that passed the sync/rms gate is one that checker + gate refuse.  The gate is evaluated here over the primed
    calls; that this is the memory the run saw throughout is checked on the hashtable.txt it leaves (no other call was
    stored)."""
    w.lab().wspr_set_fano_device_mode(fano_on_device)
    segs = [synth.make_segment(5000 + s, _symbols, snr_db=-30.0) for s in range(24)]
    I, Q = np.stack([x[0] for x in segs]), np.stack([x[1] for x in segs])
    sent = [synth.expected_text(x[2][0][0]) for x in segs]
    hashtab, loctab = _flat_table(w, synth.CALLS)
    gate = lambda data: ol.checker().osd_gate(np.array(data, np.uint8).ctypes.data, hashtab.ctypes.data, loctab.ctypes.data)
    opt = w.default_options()
    opt.usehashtable = 1
    assert w.set_osd_depth(3, w.lab()) == -1
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        _prime("hashtable.txt", synth.CALLS)
        spots, tr = w.wspr_decode_batch_trace(I, Q, opt, max_results=16)
        left = sorted(ln.split()[1] for ln in open("hashtable.txt"))
    finally:
        os.chdir(cwd)
    assert left == sorted(synth.CALLS)
    rescued = refused = 0
    for s in range(24):
        for x in spots[s]:
            if x.cycles == 0:
                assert x.message.decode() == sent[s] and x.jitter == 0, (s, x.message)
        for p in range(tr[s].passes_run):
            for j in range(tr[s].n_visited[p]):
                c = tr[s].cand[p][j]
                if c.decoded and c.cycles == 0:
                    want = ol.check(np.array(c.first_symbols, np.uint8), 3)
                    assert tuple(c.decdata) == want[0] and gate(want[0]) == 1, (s, p, j)
                    assert c.jitter == 0 and _text_of(w, want[0]) == sent[s], (s, p, j)
                    assert c.first_sync > MINSYNC2 and c.first_rms > MINRMS
                    rescued += 1
                elif not c.decoded and c.attempts > 0 and c.first_sync > MINSYNC2 and c.first_rms > MINRMS:
                    assert gate(ol.check(np.array(c.first_symbols, np.uint8), 3)[0]) == 0, (s, p, j)
                    refused += 1
    nspots0 = sum(x.cycles == 0 for g in spots for x in g)
    print("rescue: %d OSD decodes in the trace, %d OSD spots, %d gated candidates refused, %d Fano spots"
          % (rescued, nspots0, refused, sum(x.cycles != 0 for g in spots for x in g)))
    assert rescued >= 1 and nspots0 >= 1


def _hashed(w, I, Q, K=16):
    """wspr_decode_batch_hashed: (spots per segment, n_redecoded)."""
    L = w.lib()
    nseg = I.shape[0]
    out = (w.decoder_results * (nseg * K))()
    nres = (C.c_int * nseg)()
    n_st, n_re = C.c_int(0), C.c_int(0)
    L.wspr_decode_batch_hashed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, w.decoder_options, C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_void_p]
    opt = w.default_options()
    opt.usehashtable = 1
    rc = L.wspr_decode_batch_hashed(orc.ptr(I), orc.ptr(Q), nseg, NS, NS, opt, C.addressof(out), K, C.addressof(nres), 0,
                                    0, None, 0, 0, None, 0, C.byref(n_st), C.byref(n_re))
    assert rc == 0, rc
    return [[out[s * K + i] for i in range(nres[s])] for s in range(nseg)], n_re.value


@pytest.mark.parametrize("fano_on_device", [0, 1])
def test_the_gate_is_ordered_like_a_hash_lookup(w, tmp_path, depth_off, fano_on_device):
    """An empty hash memory, usehashtable = 1, two segments.  One carries "K1JT IN80 30" at -15 dB (Fano decodes it and
    stores the call); the other is seed 5015 of the rescue scene, the same message at -30 dB, which only K9 finds.  Strong first: the
    weak segment's first round meets an empty memory, is decoded again once the strong one's store is known, and its
    OSD spot is reported.  Weak first: the call has not been heard when its turn comes, and it stays undecoded.  The
    memory written is the same."""
    rng = np.random.default_rng(5)
    sigma = np.sqrt((375.0 / 2500.0) / 2.0)
    si, sq = synth.tone_signal(_symbols("K1JT IN80 30"), 40.0, 2.0, 10.0 ** (-15.0 / 20.0))
    strong = synth.normalise((rng.normal(0, sigma, NS) + si).astype(np.float32), (rng.normal(0, sigma, NS) + sq).astype(np.float32))
    wi, wq, truth = synth.make_segment(5015, _symbols, snr_db=-30.0)
    assert truth[0][0] == "K1JT IN80 30"
    assert w.set_osd_depth(3) == -1
    w.lib().wspr_set_fano_device_mode(fano_on_device)      # the stage follows the host-Fano and the device-Fano path
    runs = {}
    for name, order in (("strong_first", (strong, (wi, wq))), ("weak_first", ((wi, wq), strong))):
        I, Q = np.stack([order[0][0], order[1][0]]), np.stack([order[0][1], order[1][1]])
        d = tmp_path / name
        d.mkdir()
        cwd = os.getcwd()
        os.chdir(d)
        try:
            spots, n_re = _hashed(w, I, Q)
            runs[name] = (spots, n_re, open("hashtable.txt").read())
        finally:
            os.chdir(cwd)
    spots, n_re, table = runs["strong_first"]
    assert [x.message for x in spots[0]] == [b"K1JT IN80 30"] and spots[0][0].cycles >= 81
    assert [(x.message, x.cycles, x.jitter) for x in spots[1]] == [(b"K1JT IN80 30", 0, 0)] and n_re >= 1
    spots, n_re, table2 = runs["weak_first"]
    assert spots[0] == [] and [x.message for x in spots[1]] == [b"K1JT IN80 30"] and spots[1][0].cycles >= 81
    assert table2 == table and "K1JT" in table
