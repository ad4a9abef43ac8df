"""The product's candidate loop on the payloads of tests/payloads.py: the two early exits (a decode that does not re-encode,
an "A000AA" locator: wsprd.c:786-793), the early returns of unpk_, noprint decodes and the unknown hash, against the oracle
segment by segment on every spot field, and against the spots the reference gives by reading
(tests/test_payload_paths.py).  The product decodes a subtraction pass in speculative windows (wspr_pipeline.hip,
build_wave / keep_books) and re-encodes through a per-thread MessageCache: a stop has to end its own segment's pass
wherever in a window it falls, leave the other segments of the wave alone, and be answered from the cache as well as
computed.  (Soak: WSPR_LOOPEXIT_SEGMENTS=1536 for the batch test.)"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as ol
import payloads as P
import trace_parity as tp
from test_gpu_parity import _spot_tuple, random_scenes
from test_payload_paths import NOPRINT, OPTION_SETS, STOPPERS, expected_messages

pytestmark = pytest.mark.gpu
NS = P.NS


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    return mod


@pytest.fixture(scope="module")
def scenes():
    labels, Is, Qs = zip(*P.loop_exit_scenes())
    return list(labels), np.stack(Is), np.stack(Qs)


def _same(got, ref, where):
    g = [_spot_tuple(x) for x in got]
    r = [_spot_tuple(x) for x in ref]
    assert g == r, (where, g, r)
    assert all(abs(a.snr - b.snr) < 1e-4 for a, b in zip(got, ref)), where


def _oracle(I, Q, opts, trace=False):
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        return list(pool.map(lambda s: ol.decode(I[s], Q[s], NS, ol.default_options(**opts), trace=trace), range(len(I))))


def _want_stop(label, opts, p):
    """Stop reason of pass p on a crafted scene, by reading wsprd.c:786-793."""
    stopper = label.split("_", 1)[1] if label.startswith(("window_", "cut_")) else label
    if stopper == "A000AA":
        return 2
    if stopper == "K1A" and p == 0 and opts.get("subtraction", 1):
        return 1
    return 0


@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "defaults")
def test_loop_exits_equal_oracle_under_option_sets(w, scenes, opts):
    labels, I, Q = scenes
    ref = _oracle(I, Q, opts, trace=True)
    got = w.wspr_decode_batch(I, Q, w.default_options(**opts), max_results=32)
    for s, lab in enumerate(labels):
        _same(got[s], ref[s][0], (lab, opts))
        if lab in STOPPERS:
            assert [x.message.decode() for x in got[s]] == expected_messages(lab, opts), (lab, opts)
    # per candidate: the production kernels and the loop's bookkeeping, with where and why each pass stopped
    _, tr = w.wspr_decode_batch_trace(I, Q, w.default_options(**opts), max_results=32)
    fired = {1: 0, 2: 0}
    for s, lab in enumerate(labels):
        ot = ref[s][3]
        tp.compare_segment(tr[s], ot, (lab, opts))
        reason, cand = tp.stops_of(tr[s])
        for p in range(tr[s].passes_run):
            want = _want_stop(lab, opts, p)
            assert reason[p] == want, (lab, opts, p)
            if want:
                fired[want] += 1
                j = cand[p]
                assert tr[s].n_visited[p] == j + 1 and tr[s].cand[p][j].decoded and not tr[s].cand[p][j].subtracted
        if lab.startswith("window_") and ot.stop_reason[0]:      # three noprint decodes, none subtracted, before the stop
            j = ot.stop_cand[0]
            assert j >= 3 and sum(ot.decoded[0][k] and not ot.subtracted[0][k] for k in range(j)) >= 3
    assert fired[2] >= 3 and (fired[1] >= 2 if opts.get("subtraction", 1) else fired[1] == 0), fired
    # the residual of the single call, bit for bit: noprint decodes leave their signal, "<...>" subtracts a wrong one
    for name in NOPRINT + ["t3_unknown_hash"]:
        s = labels.index(name)
        _, ri, rq = w.wspr_decode(I[s], Q[s], NS, w.default_options(**opts))
        _, oi, oq, _ = ref[s]
        assert np.array_equal(ri, oi) and np.array_equal(rq, oq), (name, opts)


def test_stoppers_in_a_large_batch(w):
    """>= 384 segments (the fused K1 path), every third one a crafted scene between ordinary random scenes: the same K1A
    payload in many segments, so most of its re-encode failures are answered by the message cache.  Every segment equals
    the oracle; the ordinary segments equal their own decode without the stoppers beside them."""
    nseg = max(384, int(os.environ.get("WSPR_LOOPEXIT_SEGMENTS", "384")))
    nrand = nseg - nseg // 3
    RI, RQ = random_scenes(nrand, seed=4242)
    I = np.empty((nseg, NS), np.float32); Q = np.empty((nseg, NS), np.float32)
    labels, r = [], 0
    for s in range(nseg):
        if s % 3 == 1:
            name = "A000AA" if s % 12 == 4 else "K1A"
            I[s], Q[s] = P.stopper_scene(name, seed=100 + s)
            labels.append(name)
        else:
            I[s], Q[s] = RI[r], RQ[r]
            labels.append(None)
            r += 1
    plain = [s for s in range(nseg) if labels[s] is None]
    for opts in (dict(), dict(npasses=1)):
        got = w.wspr_decode_batch(I, Q, w.default_options(**opts), max_results=32)
        tm = w.last_timings()
        assert tm["message_cache_hits"] > 0
        ref = _oracle(I, Q, opts)
        for s in range(nseg):
            _same(got[s], ref[s][0], (s, labels[s], opts))
            if labels[s]:
                assert [x.message.decode() for x in got[s]] == expected_messages(labels[s], opts), (s, opts)
        alone = w.wspr_decode_batch(I[plain], Q[plain], w.default_options(**opts), max_results=32)
        for k, s in enumerate(plain):
            assert [_spot_tuple(x) for x in alone[k]] == [_spot_tuple(x) for x in got[s]], (s, opts)
        assert sum(len(g) for g in alone) > len(plain)


def test_loop_exits_with_the_hashtable(w, scenes, tmp_path):
    """usehashtable on a batch of the crafted scenes, with a plain K1ABC message in the middle (the type-3 payloads after
    it resolve to <K1ABC>): spots and hashtable.txt equal the oracle called segment by segment in order; the K1A store
    that unpk_ makes before the re-encode fails and the loop breaks is in the file."""
    from test_gpu_hashtable import _hashed, _in_dir, _opt, _tup
    labels, I0, Q0 = scenes
    mid = P.scene([("ctrl_t1", -9.0, -60.0), ("ctrl_c", -15.0, 40.0)], seed=7)
    I = np.concatenate([I0, mid[0][None], I0]); Q = np.concatenate([Q0, mid[1][None], Q0])
    nseg = I.shape[0]

    def batch():
        return [[_tup(x) for x in g] for g in w.wspr_decode_batch(I, Q, _opt(w, 1), max_results=16)]

    def oracle():
        o = ol.default_options()
        o.usehashtable = 1
        return [[_tup(x) for x in ol.decode(I[s], Q[s], NS, o)[0]] for s in range(nseg)]

    b, bf = _in_dir(tmp_path / "batch", batch)
    r, rf = _in_dir(tmp_path / "oracle", oracle)
    strip = lambda res: [[t[:8] + t[9:] for t in seg] for seg in res]
    assert strip(b) == strip(r)
    assert all(abs(x[8] - y[8]) < 1e-4 for sb, sr in zip(b, r) for x, y in zip(sb, sr))
    assert bf == rf
    (_, _, _, _, _), hf = _in_dir(tmp_path / "hashed", lambda: _hashed(w, I, Q))
    assert hf == bf
    assert "%5d K1A FN20\n" % P.nhash("K1A") in bf
    msgs = [m.decode() for seg in b for (m, *_) in seg]
    assert "<K1ABC> FN42AB 63" in msgs and "<...> FN42AB 63" in msgs
