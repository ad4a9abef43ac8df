"""Decode-quality figures and provenance per spot on the device (K19, wspr_spot_quality_batch_device /
wspr_set_spot_details / wspr_last_spot_details; the definition in rtlsdr-wsprd_amd/csrc/kernels/spot_quality.h).  The
kernel against the serial checker field for field (tests/spotq_lib.py); the three identities that tie the figures to the
Fano search, the ordered-statistics stage (K9) and the list stage (K14); the stage inside the decode call -- "off is off",
records following the spots through sort and cut, provenance against the lab library's trace of the same input; every
stage that can make a spot at least once; and when the records are refused."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import block_lib as bl
import list_lib as ll
import oracle_lib as orc
import scenes
import spotq_lib as sq
import synth

pytestmark = pytest.mark.gpu
NS = 45000
ZMIN16 = 96


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    return mod


@pytest.fixture(autouse=True)
def stages_off(w):
    """Whatever a test sets, the next one starts with every opt-in stage off -- in both libraries."""
    yield
    for L in (w.lib(), w.lab()):
        w.set_spot_details(0, L)
        w.set_spread_estimate(0, L)
        w.set_message_list(None, library=L)
        w.set_osd_depth(-1, L)
        w.set_block_detection(1, L)
        L.wspr_set_fano_device_mode(-1)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the kernel over host vectors ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 257])
def test_kernel_equals_the_checker(w, n):
    """A partial workgroup, whole workgroups (four jobs each) and one job over; edge vectors, Fano's own decodes, random
    soft bytes with random payloads.  Every field is the checker's."""
    vec, dec, want = sq.kernel_jobs()
    got = sq.words(w.spot_quality_batch(vec[:n], dec[:n]))
    bad = np.flatnonzero((got != want[:n]).any(axis=1))
    assert bad.size == 0, (n, bad[:5], got[bad[0]], want[bad[0]])
    # jobs elsewhere in the batch do not matter: the last n alone
    got = sq.words(w.spot_quality_batch(vec[-n:], dec[-n:]))
    assert np.array_equal(got, want[-n:]), n


def test_entry_point_arguments(w):
    vec, dec, want = sq.kernel_jobs()
    L = w.lib()
    out = np.full(10, 0x5A5A5A5A, np.int32)
    assert L.wspr_spot_quality_batch_device(_p(vec), _p(dec), 0, _p(out)) == 0            # n == 0: nothing happens
    assert L.wspr_spot_quality_batch_device(_p(vec), _p(dec), -1, _p(out)) == -1          # n < 0
    assert L.wspr_spot_quality_batch_device(None, _p(dec), 1, _p(out)) == -1
    assert L.wspr_spot_quality_batch_device(_p(vec), None, 1, _p(out)) == -1
    assert L.wspr_spot_quality_batch_device(_p(vec), _p(dec), 1, None) == -1
    assert (out == 0x5A5A5A5A).all()                                                      # and nothing was written
    assert L.wspr_spot_quality_batch_device(_p(vec), _p(dec), 1, _p(out)) == 0
    assert out[:5].tolist() == want[0].tolist() and (out[5:] == 0x5A5A5A5A).all()
    # bits of decdata behind the fiftieth are not read, and no arithmetic mode touches the figures
    noisy = np.array(dec[:65])
    noisy[:, 6] |= 0x3F
    noisy[:, 7:] = 0xFF
    w.wspr_set_arithmetic(1)
    try:
        assert np.array_equal(sq.words(w.spot_quality_batch(vec[:65], noisy)), want[:65])
    finally:
        w.wspr_set_arithmetic(0)


# ---- the three identities -----------------------------------------------------------------------------------------------
def test_identity_b_the_ordered_statistics_winner(w):
    """K19 on K9's `data` gives K9's nhard and dist (65 vectors, depth 2)."""
    vec = sq.kernel_jobs()[0][-65:]
    data, dist, nhard, order = w.osd_batch(vec, 2)
    got = w.spot_quality_batch(vec, data)
    assert np.array_equal(got["nhard"], nhard.astype(np.int32)) and np.array_equal(got["dist"], dist.astype(np.int32))
    assert np.array_equal(sq.words(got), sq.check(vec, data))


def test_identity_c_the_list_winner(w):
    """K19 on the decdata of K14's winner gives its score (rsum - 2 dist) and v2 (65 vectors, a list of 16 messages)."""
    assert w.set_message_list(ll.all_messages()[:16], ZMIN16) == 16
    vec = np.concatenate([sq.kernel_jobs()[0][-60:], ll.clean(ll.all_symbols()[3])[None], sq.edge_vectors()[:4]])
    assert vec.shape == (65, 162)
    m = w.list_match(vec)
    dec = np.stack([w.message_list_entry(int(k))[1] for k in m["index"]])
    got = w.spot_quality_batch(vec, dec)
    assert np.array_equal(got["rsum"] - 2 * got["dist"], m["score"]) and np.array_equal(got["v2"], m["v2"])
    assert m["index"][60] == 3 and got["nhard"][60] == 0 and got["dist"][60] == 0         # an entry's own clean code word


def test_identity_a_the_fano_metric_on_the_device(w):
    """The Fano successes of the CPU test through wspr_fano_batch_device_wave(): its metric output is K19's."""
    vec, dec, metric = sq.fano_successes()
    n = len(vec)
    assert n >= 20
    ret, cyc, met, mnp = (np.zeros(n, np.int32) for _ in range(4))
    data = np.zeros((n, 10), np.uint8)
    assert w.lib().wspr_fano_batch_device_wave(_p(vec), n, C.c_uint(10000), _p(ret), _p(cyc), _p(met), _p(mnp), _p(data), None) == 0
    assert not ret.any() and np.array_equal(data, dec[:, :10])
    got = w.spot_quality_batch(vec, dec)
    assert np.array_equal(got["metric"], met) and np.array_equal(got["metric"].astype(np.int64), metric)


# ---- the stage inside the decode call -----------------------------------------------------------------------------------
def _decode(w, I, Q, options, max_results, L=None):
    """wspr_decode_batch() keeping the raw arrays: (bytes of the spot records per segment, spots per segment, n_results)."""
    nseg, samples = I.shape
    out = (w.decoder_results * (nseg * max_results))()
    nres = (C.c_int * nseg)()
    rc = (L or w.lib()).wspr_decode_batch(orc.ptr(I), orc.ptr(Q), nseg, samples, samples, options, C.addressof(out), max_results,
                                          C.addressof(nres), 0)
    assert rc == 0
    spots = [[out[s * max_results + i] for i in range(nres[s])] for s in range(nseg)]
    raw = [bytes(memoryview(out).cast("B")[(s * max_results) * 80:(s * max_results + nres[s]) * 80]) for s in range(nseg)]
    return raw, spots, list(nres)


def _text_of(w, data):
    """The text a decoded message unpacks to on empty hash tables (unpk_)."""
    h, l = C.create_string_buffer(32768 * 13), C.create_string_buffer(32768 * 5)
    msg = (C.c_byte * 12)(*[int(x) - 256 if x > 127 else int(x) for x in data], 0)
    out = [C.create_string_buffer(32) for _ in range(5)]
    w.lib().unpk_(msg, h, l, *out)
    return out[0].value.decode()


def _hold_records_to_the_trace(w, spots, det, tr, rows=None):
    """Every spot's record: valid, and its provenance is the trace's -- the candidate at cand[pass][cand] decoded, with the
    spot's jitter, the record's block size, a decdata that unpacks to the spot's message; a ladder decode at jitter 0 was made
    on the trace's first_symbols, so the five figures are the checker's on them.  rows = (I, Q) of a call WITHOUT subtraction:
    a ladder decode on another rung was made on mode 2's vector at shift + jitter, which is K10's block size 1 bit for bit.
    Returns (spots, figures checked)."""
    total = checked = 0
    other_rungs = []
    for s, seg_spots in enumerate(spots):
        for i, sp in enumerate(seg_spots):
            r = det[s, i]
            assert r["valid"] == 1 and r["pad"] == 0, (s, i, r)
            assert r["pass"] < tr[s].passes_run and 0 <= r["cand"] < tr[s].n_visited[r["pass"]], (s, i, r)
            c = tr[s].cand[r["pass"]][r["cand"]]
            assert c.decoded == 1 and c.block == r["block"] and c.jitter == sp.jitter and c.cycles == sp.cycles, (s, i, r)
            assert r["block"] == {1: 1, 2: 2, 3: 3, 4: 1, 5: 1}[int(r["stage"])], (s, i, r)
            assert (r["stage"] == w.STAGE_OSD) == (sp.cycles == 0) and (r["stage"] == w.STAGE_LIST) == (sp.cycles == 1)
            text = _text_of(w, c.decdata)
            assert text == sp.message.decode() or "<" in sp.message.decode(), (s, i, text, sp.message)
            if r["stage"] == w.STAGE_LADDER and sp.jitter == 0:
                want = sq.check(np.array(c.first_symbols, np.uint8), np.array(c.decdata, np.uint8))[0]
                assert sq.words(r).tolist() == want.tolist(), (s, i, sp.message, r, want)
                checked += 1
            elif r["stage"] == w.STAGE_LADDER and rows is not None:
                sym = w.block_demod(rows[0], rows[1], [(s, c.freq, c.shift + sp.jitter, c.drift)])[0, 0]
                want = sq.check(sym, np.array(c.decdata, np.uint8))[0]
                assert sq.words(r).tolist() == want.tolist(), (s, i, sp.message, sp.jitter, r, want)
                other_rungs.append(int(sp.jitter))
            total += 1
        assert not det[s, len(seg_spots):].view(np.uint8).any()                # entries beyond n_results[s] are zero
    if rows is not None:
        print("ladder decodes on other rungs held to the checker: jitter", other_rungs)
        return total, len(other_rungs)
    return total, checked


@functools.lru_cache(maxsize=None)
def _three_signal_batch():
    rows = [scenes.make_scene(seed) for seed in sq.THREE_SIGNAL_SEEDS]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def test_decoder_with_the_stage_on(w):
    """Four three-signal scenes of tests/scenes.py, default options (two passes, subtraction), wspr_decode_batch(): stage
    off, on, and on together with the spread stage -- the same bytes of spots; the records against the lab library's trace
    of the same input; the cut at max_results = 2; host Fano and device Fano alike."""
    I, Q = _three_signal_batch()
    opt = w.default_options()
    K = 16
    _, tr = w.wspr_decode_batch_trace(I, Q, opt, max_results=K)
    seen = []
    for mode in (0, 1):
        w.lib().wspr_set_fano_device_mode(mode)
        off_raw, _, off_n = _decode(w, I, Q, opt, K)
        assert w.last_spot_details(4, K) is None                               # the stage was off for that call
        t = w.last_timings()
        assert t["spot_detail_ms"] == 0 and t["spot_detail_jobs"] == 0
        assert w.set_spot_details(1) == 0
        on_raw, spots, nres = _decode(w, I, Q, opt, K)
        det = w.last_spot_details(4, K)
        t = w.last_timings()
        assert on_raw == off_raw and nres == off_n and sum(nres) >= 4 and det is not None
        assert w.last_spreads(4, K) is None
        total, checked = _hold_records_to_the_trace(w, spots, det, tr)
        print("device Fano %d: %d spots, %d ladder decodes at jitter 0 held to the checker, spot_detail_ms %.3f; nhard %s metric %s"
              % (mode, total, checked, t["spot_detail_ms"], det["nhard"][det["valid"] == 1].tolist(),
                 det["metric"][det["valid"] == 1].tolist()))
        assert total == sum(nres) and checked >= 1 and t["spot_detail_jobs"] == total and t["spot_detail_ms"] > 0
        assert (det["stage"][det["valid"] == 1] == w.STAGE_LADDER).all()
        assert w.lib().wspr_last_spot_details(_p(det), 4 * K - 1) == -1        # capacity too small
        # together with the spread stage: the same spots, the same records, and the spread stage's own
        assert w.set_spread_estimate(1) == 0
        both_raw, _, both_n = _decode(w, I, Q, opt, K)
        assert both_raw == off_raw and both_n == off_n
        assert w.last_spot_details(4, K).tobytes() == det.tobytes()
        spr = w.last_spreads(4, K)
        assert spr is not None and (spr["valid"][det["valid"] == 1] == 1).all()
        assert w.set_spread_estimate(0) == 1
        # max_results = 2 cuts both arrays alike; every spot was still measured
        raw2, spots2, nres2 = _decode(w, I, Q, opt, 2)
        det2 = w.last_spot_details(4, 2)
        assert nres2 == [min(n, 2) for n in nres] and all(a == b[:len(a)] for a, b in zip(raw2, on_raw))
        assert det2.tobytes() == det[:, :2].tobytes() and w.last_timings()["spot_detail_jobs"] == total
        assert w.last_spot_details(4, K) is None                               # the layout is the last call's
        assert w.set_spot_details(0) == 1
        seen.append(det.tobytes())
    assert seen[0] == seen[1]
    # the single-segment entry point: entry i, *n_results of them
    w.set_spot_details(1)
    one, _, _ = w.wspr_decode(I[0], Q[0])
    buf = np.zeros(100, w.SPOT_DETAIL_DTYPE)
    assert w.lib().wspr_last_spot_details(_p(buf), 100) == len(one) >= 1
    assert buf[:len(one)].tobytes() == np.frombuffer(seen[0], w.SPOT_DETAIL_DTYPE).reshape(4, K)[0, :len(one)].tobytes()


# ---- every stage that can make a spot -----------------------------------------------------------------------------------
def _weak_batch(seeds):
    rows = [bl.weak_scene(s) for s in seeds]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def test_ladder_decodes_on_other_rungs(w):
    """Three weak scenes (one pass, no subtraction): seeds 5000 and 5021 decode on rungs +6 and -3 of the jitter ladder, 5004
    on rung 0.  A decode on another rung is measured on that rung's vector in the ladder's 43-lag block, not on the rung-0
    vector: the figures are the checker's on mode 2's vector at shift + jitter."""
    I, Q = _weak_batch((5000, 5021, 5004))
    opt = w.default_options(npasses=1, subtraction=0)
    _, tr = w.wspr_decode_batch_trace(I, Q, opt, max_results=8)
    seen = []
    for mode in (0, 1):
        w.lib().wspr_set_fano_device_mode(mode)
        w.set_spot_details(1)
        raw, spots, nres = _decode(w, I, Q, opt, 8)
        det = w.last_spot_details(3, 8)
        w.set_spot_details(0)
        total, others = _hold_records_to_the_trace(w, spots, det, tr, (I, Q))
        assert total >= 3 and others >= 1
        seen.append(det.tobytes())
    assert seen[0] == seen[1]


def test_block_stage_spots(w):
    """The eight weak scenes of tests/test_gpu_block.py (one pass, no subtraction), block detection up to 3: at least one spot
    of stage 2 or 3, and its figures are the checker's on the (block size, rung) vector K10 forms at the trace's refined
    parameters -- the vector the stage handed on to the bookkeeping."""
    seeds = (5003, 5007, 5008, 5010, 5002, 5011, 5012, 5013)
    I, Q = _weak_batch(seeds)
    opt = w.default_options(npasses=1, subtraction=0)
    for L in (w.lib(), w.lab()):
        assert w.set_block_detection(3, L) == 1
    _, tr = w.wspr_decode_batch_trace(I, Q, opt, max_results=8)
    for mode in (0, 1):
        w.lib().wspr_set_fano_device_mode(mode)
        off_raw, _, _ = _decode(w, I, Q, opt, 8)
        w.set_spot_details(1)
        raw, spots, nres = _decode(w, I, Q, opt, 8)
        det = w.last_spot_details(8, 8)
        w.set_spot_details(0)
        assert raw == off_raw
        _hold_records_to_the_trace(w, spots, det, tr, (I, Q))
        nblock = 0
        for s in range(8):
            for i in range(nres[s]):
                r = det[s, i]
                if r["stage"] not in (w.STAGE_BLOCK2, w.STAGE_BLOCK3):
                    continue
                c = tr[s].cand[r["pass"]][r["cand"]]
                sym = w.block_demod(I, Q, [(s, c.freq, c.shift + spots[s][i].jitter, c.drift)])[0, r["block"] - 1]
                want = sq.check(sym, np.array(c.decdata, np.uint8))[0]
                assert sq.words(r).tolist() == want.tolist(), (s, i, r, want)
                nblock += 1
        print("device Fano %d: %d block spots, stages %s" % (mode, nblock, det["stage"][det["valid"] == 1].tolist()))
        assert nblock >= 1


def test_list_stage_spots(w):
    """The same weak scenes with every message of the synthetic population listed: at least one spot of stage 4, and for
    each rsum - 2 dist and v2 are what wspr_list_match_batch_device() gives on the trace's first_symbols."""
    seeds = (5003, 5007, 5008, 5010, 5002, 5011, 5012, 5013)
    I, Q = _weak_batch(seeds)
    opt = w.default_options()
    for L in (w.lib(), w.lab()):
        assert w.set_message_list(ll.all_messages(), ZMIN16, L) == 7600
    _, tr = w.wspr_decode_batch_trace(I, Q, opt, max_results=8)
    off_raw, _, _ = _decode(w, I, Q, opt, 8)
    w.set_spot_details(1)
    raw, spots, nres = _decode(w, I, Q, opt, 8)
    det = w.last_spot_details(8, 8)
    assert raw == off_raw
    _hold_records_to_the_trace(w, spots, det, tr)
    nlist = 0
    for s in range(8):
        for i in range(nres[s]):
            r = det[s, i]
            if r["stage"] != w.STAGE_LIST:
                continue
            c = tr[s].cand[r["pass"]][r["cand"]]
            m = w.list_match(np.array(c.first_symbols, np.uint8))[0]
            assert r["rsum"] - 2 * r["dist"] == m["score"] and r["v2"] == m["v2"], (s, i, r, m)
            assert tuple(w.message_list_entry(int(m["index"]))[1]) == tuple(c.decdata)
            nlist += 1
    print("%d list spots, stages %s, nhard %s" % (nlist, det["stage"][det["valid"] == 1].tolist(), det["nhard"][det["valid"] == 1].tolist()))
    assert nlist >= 1 and w.last_timings()["list_spots"] >= nlist


def _in_dir(path, fn):
    cwd = os.getcwd()
    os.makedirs(path, exist_ok=True)
    os.chdir(path)
    try:
        return fn()
    finally:
        os.chdir(cwd)


def test_ordered_statistics_stage_spots(w, tmp_path):
    """The two-segment scene of tests/test_gpu_osd.py, usehashtable = 1 on an empty memory: "K1JT IN80 30" at -15 dB, which
    Fano decodes and stores, then the same message at -30 dB (seed 5015), which only K9 finds.  The weak segment's spot has
    stage 5, and its nhard and dist are wspr_osd_batch_device()'s on the trace's first_symbols."""
    rng = np.random.default_rng(5)
    sigma = np.sqrt((375.0 / 2500.0) / 2.0)
    si, sq_ = synth.tone_signal(bl.symbols_of("K1JT IN80 30"), 40.0, 2.0, 10.0 ** (-15.0 / 20.0))
    strong = synth.normalise((rng.normal(0, sigma, NS) + si).astype(np.float32), (rng.normal(0, sigma, NS) + sq_).astype(np.float32))
    wi, wq, truth = synth.make_segment(5015, bl.symbols_of, snr_db=-30.0)
    assert truth[0][0] == "K1JT IN80 30"
    I, Q = np.stack([strong[0], wi]), np.stack([strong[1], wq])
    opt = w.default_options()
    opt.usehashtable = 1
    for L in (w.lib(), w.lab()):
        assert w.set_osd_depth(3, L) == -1
    _, tr = _in_dir(tmp_path / "trace", lambda: w.wspr_decode_batch_trace(I, Q, opt, max_results=8))
    off_raw, _, _ = _in_dir(tmp_path / "off", lambda: _decode(w, I, Q, opt, 8))
    w.set_spot_details(1)
    raw, spots, nres = _in_dir(tmp_path / "on", lambda: _decode(w, I, Q, opt, 8))
    det = w.last_spot_details(2, 8)
    assert raw == off_raw and det is not None
    assert open(tmp_path / "on" / "hashtable.txt").read() == open(tmp_path / "off" / "hashtable.txt").read()
    _hold_records_to_the_trace(w, spots, det, tr)
    nosd = 0
    for s in range(2):
        for i in range(nres[s]):
            r = det[s, i]
            if r["stage"] != w.STAGE_OSD:
                continue
            c = tr[s].cand[r["pass"]][r["cand"]]
            data, dist, nhard, order = w.osd_batch(np.array(c.first_symbols, np.uint8), 3)
            assert tuple(data[0]) == tuple(c.decdata) and r["nhard"] == nhard[0] and r["dist"] == dist[0], (s, i, r)
            nosd += 1
    print("%d OSD spots, records %s" % (nosd, det[det["valid"] == 1].tolist()))
    assert nosd >= 1 and det[1, 0]["stage"] == w.STAGE_OSD


# ---- when there are no records ------------------------------------------------------------------------------------------
def test_records_are_refused(w):
    I, Q = _three_signal_batch()
    opt = w.default_options(npasses=1, subtraction=0)
    buf = np.zeros(4 * 4, w.SPOT_DETAIL_DTYPE)
    L = w.lib()
    # the stage on, a recording call: records; the stage off again: none
    w.set_spot_details(1)
    _decode(w, I, Q, opt, 4)
    assert L.wspr_last_spot_details(_p(buf), 16) == 16 and buf["valid"].any()
    assert L.wspr_last_spot_details(_p(buf), 15) == -1                         # too small a capacity
    # a family that does not record them
    out = (w.decoder_results * 16)()
    nres = (C.c_int * 4)()
    L.wspr_decode_batch_node.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, w.decoder_options, C.c_void_p,
                                         C.c_int, C.c_void_p, C.c_int]
    assert L.wspr_decode_batch_node(orc.ptr(I), orc.ptr(Q), 4, NS, NS, opt, C.addressof(out), 4, C.addressof(nres), 0) >= 0
    assert sum(nres) >= 4 and L.wspr_last_spot_details(_p(buf), 16) == -1
    # a traced call (the lab library keeps its own setting and its own records)
    w.set_spot_details(1, w.lab())
    _decode(w, I, Q, opt, 4, w.lab())
    assert w.lab().wspr_last_spot_details(_p(buf), 16) == 16
    w.wspr_decode_batch_trace(I, Q, opt, max_results=4)
    assert w.lab().wspr_last_spot_details(_p(buf), 16) == -1
    # the stage off
    w.set_spot_details(0)
    _decode(w, I, Q, opt, 4)
    zero = np.zeros(16, w.SPOT_DETAIL_DTYPE)
    assert L.wspr_last_spot_details(_p(zero), 16) == -1 and not zero.view(np.uint8).any()
    assert w.last_spot_details(4, 4) is None
