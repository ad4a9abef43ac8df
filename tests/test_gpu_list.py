"""List decoding against known messages on the device (K14, wspr_set_message_list / wspr_list_match_batch_device; definition
in rtlsdr-wsprd_amd/csrc/kernels/listmatch.h): the kernel against the serial CPU checker field for field, the entry points'
arguments, "off is off", the stage inside the decode loop against checker + gate on the loop's own trace, messages that
are not listed, the order against the block-detection and ordered-statistics stages, and hashed batches."""
import ctypes as C
import os

import numpy as np
import pytest

import list_lib as ll
import oracle_lib as orc
import synth

pytestmark = pytest.mark.gpu
NS = 45000
ZMIN16 = 96


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    return mod


@pytest.fixture(scope="module")
def reference():
    """The 257 vectors and the checker's answer for every list size (computed once, never modified)."""
    vec, sym = ll.match_vectors(), ll.all_symbols()
    want = {m: ll.check(sym[:m], vec) for m in (1, 2, 31, 32, 33, 64, 65, 257, 7600)}
    for a in want.values():
        a.setflags(write=False)
    return vec, want


@pytest.fixture(autouse=True)
def stages_off(w):
    """Whatever a test sets, the next one starts with every opt-in stage off -- in both libraries."""
    yield
    for L in (w.lib(), w.lab()):
        w.set_message_list(None, library=L)
        w.set_osd_depth(-1, L)
        w.set_block_detection(1, L)
        L.wspr_set_fano_device_mode(-1)


def _rows(a):
    return np.stack([a[f] for f in ll.FIELDS], axis=1).astype(np.int64)


def _symbols(msg):
    ok, s = orc.channel_symbols(msg)
    assert ok, msg
    return s


def _tup(x):
    return (x.message, x.call, x.loc, x.pwr, x.cycles, x.jitter, x.drift, x.sync, x.snr, x.dt, x.freq)


def _timings(L):
    ms = (C.c_double * 64)()
    n = L.wspr_last_timings(C.addressof(ms), 64)
    import rtlsdr_wsprd_amd as mod
    return {mod.TIMING_NAMES[i]: ms[i] for i in range(n)}


# ---- 1. the kernel equals the checker, field for field ------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 31, 32, 33, 64, 65, 257, 7600])
def test_kernel_equals_the_checker(w, reference, m):
    vec, want = reference
    assert w.set_message_list(ll.all_messages()[:m], ZMIN16) == m
    for n in (1, 63, 64, 65, 257):
        got = _rows(w.list_match(vec[:n]))
        bad = np.flatnonzero((got != want[m][:n]).any(axis=1))
        assert bad.size == 0, (m, n, bad[:5], got[bad[0]], want[m][bad[0]])
    # vectors elsewhere in the batch do not matter: the last 65 alone
    assert np.array_equal(_rows(w.list_match(vec[-65:])), want[m][-65:])
    if m == 1:
        assert np.all(want[1][:, 2] == ll.NO_SECOND)
    if m == 7600:
        # what the crafted vectors are for: both members of every tie pair are listed, the lower index wins, second == score
        t0 = 5 + 9 + 9
        for k, (a, b, _) in enumerate(ll.tie_cases()):
            r = want[m][t0 + k]
            assert r[0] == min(a, b) and r[1] == r[2], (a, b, r)
        assert tuple(want[m][5][[0, 1, 3]]) == (0, ll.S_CLEAN, ll.V_MAX)      # the clean code word of entry 0


# ---- 2. arguments -------------------------------------------------------------------------------------------------------
def test_entry_point_arguments(w, reference):
    vec, want = reference
    L = w.lib()
    guard = np.full(8, 0x5A5A5A5A, np.int32)
    assert L.wspr_list_match_batch_device(vec.ctypes.data, 1, guard.ctypes.data) == -1          # no list set
    assert L.wspr_list_match_batch_device(vec.ctypes.data, 0, guard.ctypes.data) == -1
    msgs = ll.all_messages()
    assert w.set_message_list(msgs[:33], ZMIN16) == 33
    assert L.wspr_list_match_batch_device(vec.ctypes.data, -1, guard.ctypes.data) == -1         # n < 0
    assert L.wspr_list_match_batch_device(vec.ctypes.data, 0, guard.ctypes.data) == 0           # n == 0: nothing happens
    assert np.all(guard == 0x5A5A5A5A)
    # the setter's refusals change nothing: the list of 33 is still what the kernel matches against
    assert w.set_message_list([msgs[0], "<K1JT> FN20QI 37"]) == -1 and w.set_message_list(msgs[:2], 204) == -1
    assert w.set_message_list(["HELLO"]) == -1 and L.wspr_set_message_list(guard.ctypes.data, -1, 96) == -1
    assert np.array_equal(_rows(w.list_match(vec[:65])), want[33][:65])
    L.wspr_fano_batch_device_wave.argtypes = [C.c_void_p, C.c_int, C.c_uint] + [C.c_void_p] * 6
    for k in (0, 32):
        text, dec, s = w.message_list_entry(k)
        assert text == synth.expected_text(msgs[k]) and np.array_equal(s, ll.all_symbols()[k])
        # decdata is what the device's own Fano search returns for the entry's clean code word
        ret, cyc, met, mnp = (np.zeros(1, t) for t in (np.int32, np.uint32, np.uint32, np.uint32))
        data = np.zeros(10, np.uint8)
        clean = ll.clean(s)
        assert L.wspr_fano_batch_device_wave(orc.ptr(clean), 1, C.c_uint(10000), orc.ptr(ret), orc.ptr(cyc), orc.ptr(met),
                                             orc.ptr(mnp), orc.ptr(data), None) == 0
        assert ret[0] == 0 and np.array_equal(data, dec[:10]) and dec[10] == 0
    assert w.message_list_entry(33) is None and w.message_list_entry(-1) is None
    # a new list replaces the table on the device; switching off makes the entry refuse again
    assert w.set_message_list(msgs[:2], ZMIN16) == 2
    assert np.array_equal(_rows(w.list_match(vec[:65])), want[2][:65])
    assert w.set_message_list(None) == 0
    assert L.wspr_list_match_batch_device(vec.ctypes.data, 1, guard.ctypes.data) == -1 and np.all(guard == 0x5A5A5A5A)


# ---- 3. off is off ------------------------------------------------------------------------------------------------------
def _decode_writeback(w, I, Q, opt, K=16):
    I, Q = I.copy(), Q.copy()
    nseg = I.shape[0]
    out = (w.decoder_results * (nseg * K))()
    nres = (C.c_int * nseg)()
    rc = w.lib().wspr_decode_batch(orc.ptr(I), orc.ptr(Q), nseg, NS, NS, opt, C.addressof(out), K, C.addressof(nres), 1)
    assert rc == 0, rc
    return [[_tup(out[s * K + i]) for i in range(nres[s])] for s in range(nseg)], I, Q


def test_off_is_off_after_a_list_was_set_and_cleared(w):
    """The crowded 64-segment scene of tests/test_gpu_osd.py at the default, then the same scene after a list was set and
    cleared: spots and residual IQ byte for byte, and the stage's three timing slots zero."""
    segs = [synth.make_segment(7000 + s, _symbols, n_signals=3, snr_db=-12.0, snr_span=16.0, t_jitter=0.5) for s in range(64)]
    I, Q = np.stack([x[0] for x in segs]), np.stack([x[1] for x in segs])
    before = _decode_writeback(w, I, Q, w.default_options())
    assert sum(len(x) for x in before[0]) >= 64
    assert w.set_message_list(ll.all_messages(), ZMIN16) == 7600 and w.set_message_list(None) == 0
    after = _decode_writeback(w, I, Q, w.default_options())
    assert after[0] == before[0]
    assert after[1].tobytes() == before[1].tobytes() and after[2].tobytes() == before[2].tobytes()
    t = w.last_timings()
    assert t["list_ms"] == 0 and t["list_vectors"] == 0 and t["list_spots"] == 0


# ---- 4. the stage against checker and gate on the product's own trace ---------------------------------------------------
@pytest.fixture(scope="module")
def weak_scenes():
    """24 single-signal segments at -30 dB (tests/synth.py make_segment, seeds 5000..5023)."""
    segs = [synth.make_segment(5000 + s, _symbols, snr_db=-30.0) for s in range(24)]
    I, Q = np.stack([x[0] for x in segs]), np.stack([x[1] for x in segs])
    for a in (I, Q):
        a.setflags(write=False)
    return I, Q, [synth.expected_text(x[2][0][0]) for x in segs]


def _walk(tr, nseg):
    for s in range(nseg):
        for p in range(tr[s].passes_run):
            for j in range(tr[s].n_visited[p]):
                yield s, p, j, tr[s].cand[p][j]


def _hold_trace_to_the_checker(w, spots, tr, sent, entries_sym, entry_text, entry_dec, also_decoded_ok=lambda c: False):
    """Every list decode of the trace is the checker's winner and passes the gate; every candidate left undecoded is one
    checker + gate refuse.  Returns (rescued, refused)."""
    cands = [(s, p, j, c) for s, p, j, c in _walk(tr, len(sent)) if c.attempts > 0 and (not c.decoded or c.cycles == 1)]
    if not cands:
        return 0, 0
    res = ll.check(entries_sym, np.array([np.array(c.first_symbols, np.uint8) for _, _, _, c in cands]))
    rescued = refused = 0
    for (s, p, j, c), (idx, s1, s2, v2) in zip(cands, res):
        ok = ll.gate(s1, v2, ZMIN16) == 1
        if c.decoded:
            assert ok and tuple(c.decdata) == tuple(entry_dec[idx]), (s, p, j, idx, s1, v2)
            assert c.jitter == 0 and entry_text[idx] == sent[s], (s, p, j, entry_text[idx], sent[s])
            rescued += 1
        else:
            assert not ok or also_decoded_ok(c), (s, p, j, idx, s1, v2)
            refused += 1
    for s in range(len(sent)):
        for x in spots[s]:
            if x.cycles == 1:
                assert x.message.decode() == sent[s] and x.jitter == 0, (s, x.message)
    return rescued, refused


@pytest.fixture(scope="module")
def listed(w):
    """Text and decdata of the 7 600 entries as the library holds them."""
    assert w.set_message_list(ll.all_messages(), ZMIN16) == 7600
    ent = [w.message_list_entry(k) for k in range(7600)]
    w.set_message_list(None)
    assert all(np.array_equal(e[2], ll.all_symbols()[k]) for k, e in enumerate(ent))
    return [e[0] for e in ent], [e[1] for e in ent]


@pytest.mark.parametrize("fano_on_device", [0, 1])
def test_stage_against_checker_and_gate(w, weak_scenes, listed, fano_on_device):
    """The list = all 7 600 messages of synth.CALLS x GRIDS x POWERS, zmin16 = 96.  On the CPU (`python
    tools/list_rescue_seeds.py -30 5000 5024` prints it; the oracle's trace):
        SNR -30 dB, seeds 5000..5023, zmin16 96: Fano decodes 6 / 24; of the 18 Fano-failed scenes the list rule recovers the
        sent message in 16 (14 on candidates that also pass the sync/rms gate), z 6.65 .. 7.97; accepted entries that are NOT
        the sent message: 0
    so a floor of one rescued candidate is safe.  Here the product's own trace is held to the checker, once with the Fano
    attempts on the host pool and once with all of them on the device: every decode with cycles == 1 is the checker's winner
    for that candidate's first_symbols, passes the gate, has jitter 0 and carries the sent message; every visited candidate
    that was worth a ladder and stays undecoded is one that checker + gate refuse; every spot with cycles == 1 is the sent
    text."""
    I, Q, sent = weak_scenes
    text, dec = listed
    L = w.lab()
    L.wspr_set_fano_device_mode(fano_on_device)
    assert w.set_message_list(ll.all_messages(), ZMIN16, L) == 7600
    spots, tr = w.wspr_decode_batch_trace(I, Q, w.default_options(), max_results=16)
    rescued, refused = _hold_trace_to_the_checker(w, spots, tr, sent, ll.all_symbols(), text, dec)
    t = _timings(L)
    nspots1 = sum(x.cycles == 1 for g in spots for x in g)
    print("list stage: %d list decodes in the trace, %d list spots, %d candidates refused, %d Fano spots; %d vectors in %.2f ms"
          % (rescued, nspots1, refused, sum(x.cycles != 1 for g in spots for x in g), t["list_vectors"], t["list_ms"]))
    assert rescued >= 1 and nspots1 >= 1
    assert t["list_vectors"] >= rescued + refused and t["list_spots"] >= nspots1 and t["list_ms"] > 0


# ---- 5. not in the list, not reported -----------------------------------------------------------------------------------
def test_messages_that_are_not_listed_are_not_reported(w, weak_scenes):
    """The same scenes against 7 600 messages of calls that are NOT sent (synth.message_wide): the spots are the stage-off
    spots, although the stage matched vectors."""
    I, Q, _ = weak_scenes
    others, k = [], 0
    while len(others) < 7600:
        m = synth.message_wide(1000003 * k + 17)
        k += 1
        if m.split()[0] not in synth.CALLS:
            others.append(m)
    off = [[_tup(x) for x in g] for g in w.wspr_decode_batch(I, Q, w.default_options())]
    kept = w.set_message_list(others, ZMIN16)
    assert 7000 <= kept <= 7600                              # (repeats among the drawn texts are dropped)
    on = [[_tup(x) for x in g] for g in w.wspr_decode_batch(I, Q, w.default_options())]
    t = w.last_timings()
    print("foreign list: %d vectors matched in %.2f ms, %d accepted" % (t["list_vectors"], t["list_ms"], t["list_spots"]))
    assert on == off and sum(len(g) for g in off) >= 1
    assert t["list_vectors"] > 0 and t["list_spots"] == 0


# ---- 6. order with the other stages -------------------------------------------------------------------------------------
def _prime(path, mod, calls):
    with open(path, "w") as f:
        for slot, call in sorted((mod.lib().nhash(c.encode(), len(c), 146), c) for c in calls):
            f.write("%5d %s %s\n" % (slot, call, "AA00"))


def test_list_stage_runs_before_the_ordered_statistics_stage(w, weak_scenes, listed, tmp_path):
    """wspr_set_osd_depth(3) and a primed hashtable.txt as well (every sent call "heard before": the OSD stage would take
    these candidates, tests/test_gpu_osd.py): whatever checker + gate accept is reported with cycles == 1, never 0, and OSD
    (cycles == 0) only has what the list stage left."""
    I, Q, sent = weak_scenes
    text, dec = listed
    L = w.lab()
    assert w.set_message_list(ll.all_messages(), ZMIN16, L) == 7600 and w.set_osd_depth(3, L) == -1
    opt = w.default_options()
    opt.usehashtable = 1
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        _prime("hashtable.txt", w, synth.CALLS)
        spots, tr = w.wspr_decode_batch_trace(I, Q, opt, max_results=16)
    finally:
        os.chdir(cwd)
    # a candidate the list refuses may still be an OSD decode (cycles 0); none that the list accepts may be
    rescued, _ = _hold_trace_to_the_checker(w, spots, tr, sent, ll.all_symbols(), text, dec, also_decoded_ok=lambda c: False)
    by_osd = [(s, p, j, c) for s, p, j, c in _walk(tr, 24) if c.decoded and c.cycles == 0]
    if by_osd:
        res = ll.check(ll.all_symbols(), np.array([np.array(c.first_symbols, np.uint8) for _, _, _, c in by_osd]))
        assert not any(ll.gate(s1, v2, ZMIN16) for _, s1, _, v2 in res)
    print("list before OSD: %d list decodes, %d OSD decodes" % (rescued, len(by_osd)))
    assert rescued >= 1


def test_block_stage_runs_before_the_list_stage(w, weak_scenes, listed):
    """wspr_set_block_detection(3) as well: a candidate the block stage decodes never reaches K14 -- it keeps its block size,
    Fano's cycles and the rung's jitter in the trace; a list decode is a candidate no block size decoded (block == 1)."""
    I, Q, sent = weak_scenes
    text, dec = listed
    L = w.lab()
    assert w.set_message_list(ll.all_messages(), ZMIN16, L) == 7600 and w.set_block_detection(3, L) == 1
    spots, tr = w.wspr_decode_batch_trace(I, Q, w.default_options(), max_results=16)
    rescued, _ = _hold_trace_to_the_checker(w, spots, tr, sent, ll.all_symbols(), text, dec)
    blocks = both = 0
    for s, p, j, c in _walk(tr, 24):
        if c.decoded and c.block >= 2:
            assert c.cycles >= 81, (s, p, j, c.cycles)
            blocks += 1
            idx, s1, _, v2 = ll.check(ll.all_symbols(), np.array(c.first_symbols, np.uint8)[None])[0]
            both += ll.gate(s1, v2, ZMIN16)
        if c.decoded and c.cycles == 1:
            assert c.block == 1, (s, p, j, c.block)
    t = _timings(L)
    print("block before list: %d block decodes (%d of them the list would have accepted too), %d list decodes"
          % (blocks, both, rescued))
    assert blocks >= 1 and t["block2_decodes"] + t["block3_decodes"] >= blocks


# ---- 7. hashed batches --------------------------------------------------------------------------------------------------
def test_revisit_under_another_list_is_refused(w, weak_scenes, tmp_path):
    """WSPR_HASH_REVISIT completes the calling thread's previous hashed call: under another list (even the same texts set
    again), another zmin16, or with the stage switched on or off in between it is refused, results untouched."""
    I, Q, _ = weak_scenes
    I, Q = np.ascontiguousarray(I[:8]), np.ascontiguousarray(Q[:8])
    nseg, K = 8, 16
    L = w.lib()
    L.wspr_decode_batch_hashed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, w.decoder_options, C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_void_p]
    opt = w.default_options()
    opt.usehashtable = 1
    out = (w.decoder_results * (nseg * K))()
    nres = (C.c_int * nseg)()

    def call(flags):
        st = np.zeros((64 * nseg, 32), np.uint8)
        n_st = C.c_int(0)
        rc = L.wspr_decode_batch_hashed(orc.ptr(I), orc.ptr(Q), nseg, NS, NS, opt, C.addressof(out), K, C.addressof(nres), 0,
                                        0, None, 0, flags, orc.ptr(st), len(st), C.byref(n_st), None)
        return rc, bytes(out), list(nres)

    def list_spots():
        return sum(out[s * K + i].cycles == 1 for s in range(nseg) for i in range(nres[s]))

    msgs = ll.all_messages()
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        assert w.set_message_list(msgs, ZMIN16) == 7600
        rc, first, n_first = call(1)
        assert rc == 0 and list_spots() >= 1
        assert call(1 | 2) == (0, first, n_first)                        # a legitimate revisit: nothing to decode again
        assert w.set_message_list(msgs, ZMIN16) == 7600                   # the same texts, but another list
        rc, after, n_after = call(1 | 2)
        assert rc < 0 and after == first and n_after == n_first
        assert w.set_message_list(None) == 0                              # the stage off
        rc, after, n_after = call(1 | 2)
        assert rc < 0 and after == first and n_after == n_first
        rc, plain, n_plain = call(1)                                      # a fresh call without a list ...
        assert rc == 0 and list_spots() == 0
        assert w.set_message_list(msgs[:64], 104) == 64                   # ... cannot be completed under one
        rc, after, n_after = call(1 | 2)
        assert rc < 0 and after == plain and n_after == n_plain
    finally:
        os.chdir(cwd)
