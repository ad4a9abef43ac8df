"""wspr_set_arithmetic(WSPR_ARITH_CONTRACTED) on the device equals the CONTRACT=1 checker (tests/helpers/contract_dsp.c)
bit for bit: the exported stages, the lab's FFT bank, candidate lists and per-candidate trace, and whole decodes through
every entry point (every spot field and the residual IQ; the SNR, whose log10f is the device's, within 1e-4 dB as in
tests/test_gpu_parity.py).  Going back to the exact mode gives what a fresh process gives, byte for byte."""
import ctypes as C
import os
import subprocess
import sys
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import contract_lib as cl
import oracle_lib as ol
from test_gpu_parity import _spot_tuple, random_scenes, symf
import synth
import trace_parity as tp

pytestmark = pytest.mark.gpu

NS = 45000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_SETS = [dict(), dict(quickmode=1), dict(subtraction=0), dict(npasses=1), dict(npasses=3)]   # test_gpu_parity.py


def _checker_all(I, Q, opts=None):
    """cl.decode(1, ...) of every row, in parallel (the checker releases the GIL)."""
    I0, Q0 = I[0], Q[0]
    cl.decode(1, I0, Q0, NS)
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        return list(ex.map(lambda k: cl.decode(1, I[k], Q[k], NS, ol.default_options(**(opts or {}))), range(I.shape[0])))


def _decode_writeback(w, I, Q, opts=None, max_results=32):
    """wspr_decode_batch with writeback: (spot lists, residual I, Q)."""
    I = np.ascontiguousarray(I, dtype=np.float32).copy()
    Q = np.ascontiguousarray(Q, dtype=np.float32).copy()
    nseg = I.shape[0]
    out = (w.decoder_results * (nseg * max_results))()
    nres = (C.c_int * nseg)()
    rc = w.lib().wspr_decode_batch(ol.ptr(I), ol.ptr(Q), nseg, NS, NS, w.default_options(**(opts or {})),
                                   C.addressof(out), max_results, C.addressof(nres), 1)
    assert rc == 0, rc
    return [[out[k * max_results + i] for i in range(nres[k])] for k in range(nseg)], I, Q


def _same_as_checker(got, ref, where):
    assert [_spot_tuple(x) for x in got] == [_spot_tuple(x) for x in ref], where
    assert all(abs(a.snr - b.snr) < 1e-4 for a, b in zip(got, ref)), where


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    cl.contract(1)
    yield mod
    mod.wspr_set_arithmetic(mod.WSPR_ARITH_EXACT)
    if mod.os.path.exists(mod.LAB_PATH):
        mod.wspr_set_arithmetic(mod.WSPR_ARITH_EXACT, mod.lab())


@pytest.fixture
def contracted(w):
    assert w.wspr_set_arithmetic(w.WSPR_ARITH_CONTRACTED) == w.WSPR_ARITH_EXACT
    yield
    assert w.wspr_set_arithmetic(w.WSPR_ARITH_EXACT) == w.WSPR_ARITH_CONTRACTED


@pytest.fixture(scope="module")
def synth_batch():
    segs = [synth.make_segment(1000 + s, symf, snr_db=-20.0) for s in range(6)]
    segs.append(synth.make_segment(77, symf, n_signals=4, snr_db=-8.0, snr_span=12.0, t_jitter=0.3))
    segs.append(synth.make_segment(78, symf, snr_db=-15.0, drift=2.0))
    return np.stack([s[0] for s in segs]), np.stack([s[1] for s in segs]), [s[2] for s in segs]


def _both_demod(w, I, Q, freq, shift, drift, mode, lagmin=0, lagmax=0, lagstep=8, ifmin=0, ifmax=0, fstep=0.0, np_=NS,
                symfac=50):
    res = []
    for which in ("gpu", "cpu"):
        Ic, Qc = I.copy(), Q.copy()
        f = C.c_float(freq); sh = C.c_int(shift); dr = C.c_float(drift); sy = C.c_float(0)
        sym = (C.c_ubyte * 162)()
        args = [ol.ptr(Ic), ol.ptr(Qc), C.c_long(np_), sym, C.addressof(f), ifmin, ifmax, C.c_float(fstep),
                C.addressof(sh), lagmin, lagmax, lagstep, C.addressof(dr), symfac, C.addressof(sy), mode]
        (w.lib().sync_and_demodulate if which == "gpu" else cl.contract(1).ctr_sync_demod)(*args)
        res.append((f.value, sh.value, sy.value, bytes(sym)))
    return res


@pytest.mark.parametrize("seg,drift", [(0, 0.0), (3, 0.0), (7, 2.0), (7, -4.0), (6, 1.0)])
def test_sync_and_demodulate_modes(w, contracted, synth_batch, seg, drift):
    I, Q, truth = synth_batch
    msg, f0, t0, snr = truth[seg][0]
    fc = float(np.float32(round(f0 / 0.732421875) * 0.732421875))
    sc = int(round(t0 * 375 / 128.0)) * 128
    g, o = _both_demod(w, I[seg], Q[seg], fc, sc, drift, 0, lagmin=sc - 128, lagmax=sc + 128, lagstep=8)
    assert g[:3] == o[:3]
    g, o = _both_demod(w, I[seg], Q[seg], fc, o[1], drift, 1, ifmin=-2, ifmax=2, fstep=0.1)
    assert g[:3] == o[:3]
    for jig in (0, -3, 3, 63, -63):
        g, o = _both_demod(w, I[seg], Q[seg], o[0], o[1] + jig, drift, 2)
        assert g[2] == o[2] and g[3] == o[3]


def test_sync_and_demodulate_edges_and_symfac(w, contracted, synth_batch):
    I, Q, truth = synth_batch
    for shift in (-1400, -300, 3700, 4100):
        g, o = _both_demod(w, I[0], Q[0], 10.0, shift, 0.0, 2)
        assert g[2:] == o[2:]
        g, o = _both_demod(w, I[0], Q[0], -37.5, shift, 1.0, 0, lagmin=shift - 128, lagmax=shift + 128, lagstep=16)
        assert g[:3] == o[:3]
    g, o = _both_demod(w, I[0], Q[0], 10.0, 700, 0.0, 2, np_=44000)
    assert g[2:] == o[2:]
    msg, f0, t0, snr = truth[1][0]
    for symfac in (50, 64, 1):
        g, o = _both_demod(w, I[1], Q[1], float(np.float32(f0)), int(round(t0 * 375)), 0.0, 2, symfac=symfac)
        assert g[2] == o[2] and g[3] == o[3]


@pytest.mark.parametrize("seg,drift,shift_off,np_", [(0, 0.0, 0, NS), (7, 2.0, 0, NS), (1, 0.0, -2500, NS),
                                                     (2, -1.0, 3900, NS), (4, 1.0, -700, 41000), (5, 0.0, -41000, NS),
                                                     (0, 0.0, 44000, NS)])
def test_subtract_signal2(w, contracted, synth_batch, seg, drift, shift_off, np_):
    I, Q, truth = synth_batch
    msg, f0, t0, snr = truth[seg][0]
    sym = symf(msg)
    shift = int(round(t0 * 375)) + shift_off
    outs = []
    for which in ("gpu", "cpu"):
        Ic, Qc = I[seg].copy(), Q[seg].copy()
        args = [ol.ptr(Ic), ol.ptr(Qc), C.c_long(np_), C.c_float(f0), C.c_int(shift), C.c_float(drift), ol.ptr(sym)]
        (w.lib().subtract_signal2 if which == "gpu" else cl.contract(1).ctr_subtract)(*args)
        outs.append((Ic, Qc))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_stage_fft_bank(w, synth_batch):
    L = w.lab()
    I, Q, _ = synth_batch
    nseg, blocks = I.shape[0], 4 * (NS // 512) - 1
    ps = np.zeros((nseg, 512, blocks), np.float32)
    assert w.wspr_set_arithmetic(w.WSPR_ARITH_CONTRACTED, L) == 0
    try:
        assert L.wspr_stage_fft_bank(ol.ptr(I), ol.ptr(Q), nseg, NS, NS, ol.ptr(ps)) == blocks
    finally:
        w.wspr_set_arithmetic(w.WSPR_ARITH_EXACT, L)
    for s in range(nseg):
        want = cl.fft_bank(1, I[s], Q[s], NS)
        assert np.array_equal(ps[s][48:465], want[48:465]), s
        assert not np.array_equal(want, cl.fft_bank(0, I[s], Q[s], NS))


def test_reference_line_and_residual(w, contracted):
    I, Q, n = ol.read_iq_file(ol.os.path.join(ol.GOLDEN, "refSignalSnr0dB.iq"))
    spots, ri, rq = w.wspr_decode(I, Q, NS, w.default_options())
    ref, oi, oq = cl.decode(1, I, Q, NS)
    assert [_spot_tuple(s) for s in spots] == [_spot_tuple(s) for s in ref] and len(ref) == 1
    assert abs(spots[0].snr - ref[0].snr) < 1e-4
    assert np.array_equal(ri, oi) and np.array_equal(rq, oq)


@pytest.mark.parametrize("opts", [dict(), dict(quickmode=1), dict(subtraction=0), dict(npasses=1), dict(npasses=3)])
def test_batch_decode(w, contracted, synth_batch, opts):
    I, Q, truth = synth_batch
    got = w.wspr_decode_batch(I, Q, w.default_options(**opts), max_results=16)
    for s in range(I.shape[0]):
        ref, _, _ = cl.decode(1, I[s], Q[s], NS, ol.default_options(**opts))
        assert [_spot_tuple(x) for x in got[s]] == [_spot_tuple(x) for x in ref], s
        assert all(abs(a.snr - b.snr) < 1e-4 for a, b in zip(got[s], ref))


@pytest.mark.parametrize("opts", OPTION_SETS)
def test_random_scenes_spots_and_residuals(w, contracted, opts):
    """The 420 random scenes under every option set of tests/test_gpu_parity.py: spots and residual IQ."""
    I, Q = random_scenes()
    got, ri, rq = _decode_writeback(w, I, Q, opts)
    ref = _checker_all(I, Q, opts)
    for k in range(I.shape[0]):
        _same_as_checker(got[k], ref[k][0], k)
        assert np.array_equal(ri[k], ref[k][1]) and np.array_equal(rq[k], ref[k][2]), k


def test_config3_segments(w, contracted):
    """1 024 segments of configs[2] (ten overlapping signals, -10..-28 dB): spots and residuals."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    torch.cuda.set_device(0)
    I, Q, _ = bench.synth_batch_gpu(1024, 9876, torch.device("cuda", 0), 10, -10.0, -28.0, 0.3)
    I, Q = I.cpu().numpy(), Q.cpu().numpy()
    got, ri, rq = _decode_writeback(w, I, Q)
    ref = _checker_all(I, Q)
    for k in range(I.shape[0]):
        _same_as_checker(got[k], ref[k][0], k)
        assert np.array_equal(ri[k], ref[k][1]) and np.array_equal(rq[k], ref[k][2]), k
    assert sum(len(r[0]) for r in ref) > 5 * 1024


def test_decode_batch_device(w, contracted, synth_batch):
    import torch
    I, Q, _ = synth_batch
    ti = torch.from_numpy(I).cuda().contiguous()
    tq = torch.from_numpy(Q).cuda().contiguous()
    dec = w.BatchDecoder(I.shape[0], max_results=16)
    w.sync_torch()
    nres = dec.decode_ptr(ti.data_ptr(), tq.data_ptr(), NS, NS)
    torch.cuda.synchronize()
    for k in range(I.shape[0]):
        ref, _, _ = cl.decode(1, I[k], Q[k], NS)
        _same_as_checker([dec.out[k * 16 + i] for i in range(nres[k])], ref, k)


def test_session_decode(w, contracted):
    """One receiver session: raw u8 IQ through the front end (exact in both modes), then the contracted decode."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    torch.cuda.set_device(0)
    L = w.lib()
    raw, exp = bench.synth_raw_gpu(1, 61, torch.device("cuda", 0), -18.0)
    host = raw[0].cpu().numpy()
    L.wspr_session_create.restype = C.c_void_p
    L.wspr_session_create.argtypes = [w.decoder_options]
    L.wspr_session_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.wspr_session_rollover.argtypes = [C.c_void_p]
    L.wspr_session_decode.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.wspr_session_samples.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.wspr_session_samples.restype = C.POINTER(C.c_float)
    L.wspr_session_destroy.argtypes = [C.c_void_p]
    s = L.wspr_session_create(w.default_options(freq=14095600))
    O = ol.lib()
    ost = O.orc_decim_new()
    oi, oq = np.zeros(NS, np.float32), np.zeros(NS, np.float32)
    ofill = 0
    for pos in range(0, host.size, 65536):
        chunk = np.ascontiguousarray(host[pos:pos + 65536])
        L.wspr_session_feed(s, ol.ptr(chunk), chunk.size)
        ofill = O.orc_decim_feed(C.c_void_p(ost), ol.ptr(chunk), chunk.size, ol.ptr(oi), ol.ptr(oq), ofill, NS)
    done = L.wspr_session_rollover(s)
    out = (w.decoder_results * 50)()
    n = C.c_int(0)
    assert L.wspr_session_decode(s, done, C.addressof(out), C.byref(n)) == 1
    O.orc_normalise(ol.ptr(oi), ol.ptr(oq), C.c_int(ofill), C.c_int(NS))
    ref, ri, rq = cl.decode(1, oi, oq, NS, ol.default_options(freq=14095600))
    _same_as_checker([out[k] for k in range(n.value)], ref, "session")
    assert n.value >= 1 and out[0].message.decode() == exp[0][0]
    gi = np.ctypeslib.as_array(L.wspr_session_samples(s, done, 0), shape=(NS,))
    gq = np.ctypeslib.as_array(L.wspr_session_samples(s, done, 1), shape=(NS,))
    assert np.array_equal(gi, ri) and np.array_equal(gq, rq)
    O.orc_decim_free(C.c_void_p(ost))
    L.wspr_session_destroy(s)


@pytest.mark.parametrize("coarse", [0, 1])
def test_stage_candidates(w, synth_batch, coarse):
    """Noise level, smoothed spectrum and candidate list (peaks; + coarse sync) on the contracted spectrogram."""
    I, Q, _ = synth_batch
    nseg = I.shape[0]
    cands = (w.cand * (200 * nseg))()
    npk = (C.c_int * nseg)()
    noise = np.zeros(nseg, np.float32)
    sm = np.zeros((nseg, 411), np.float32)
    L = w.lab()
    assert w.wspr_set_arithmetic(w.WSPR_ARITH_CONTRACTED, L) == 0
    try:
        assert L.wspr_stage_candidates(ol.ptr(I), ol.ptr(Q), nseg, NS, NS, coarse, 4, C.addressof(cands),
                                       C.addressof(npk), ol.ptr(noise), ol.ptr(sm)) == 0
    finally:
        w.wspr_set_arithmetic(w.WSPR_ARITH_EXACT, L)
    O = ol.lib()
    for k in range(nseg):
        ps = cl.fft_bank(1, I[k], Q[k], NS)
        oc = (ol.Cand * 200)()
        onoise = C.c_float()
        osm = np.zeros(411, np.float32)
        onpk = O.orc_pick_peaks(ol.ptr(ps), C.c_int(347), oc, C.byref(onoise), ol.ptr(osm), None)
        if coarse:
            O.orc_coarse_sync(ol.ptr(ps), C.c_int(347), oc, C.c_int(onpk), C.c_int(4))
        assert npk[k] == onpk and noise[k] == np.float32(onoise.value) and np.array_equal(sm[k], osm), k
        for j in range(onpk):
            g, o = cands[200 * k + j], oc[j]
            assert (g.freq, g.shift, g.drift, g.sync, g.snr) == (o.freq, o.shift, o.drift, o.sync, o.snr), (k, j)


def test_per_candidate_trace(w):
    """Every visited candidate of the parity batch and of 120 random scenes: lag scan, frequency scan, rung 0, ladder
    walk, Fano, subtraction and stop marks equal the checker's trace."""
    L = w.lab()
    checker = types.SimpleNamespace(decode=lambda *a, **k: cl.decode(1, *a, **k), default_options=ol.default_options)
    assert w.wspr_set_arithmetic(w.WSPR_ARITH_CONTRACTED, L) == 0
    try:
        I, Q = tp.parity_batch()
        total, undecoded = tp.check(I, Q, w, checker, None, "parity")
        I, Q = random_scenes(120)
        t2, u2 = tp.check(I, Q, w, checker, None, "scenes")
    finally:
        w.wspr_set_arithmetic(w.WSPR_ARITH_EXACT, L)
    assert total >= 8 and t2 > 300 and u2 > 90


def test_revisit_under_another_mode_is_refused(w, tmp_path, monkeypatch):
    from test_gpu_hashtable import _opt, _traffic
    monkeypatch.chdir(tmp_path)
    nseg, K = 24, 16
    I, Q, _ = _traffic(nseg, 0.3, 4711)
    L = w.lib()
    L.wspr_decode_batch_hashed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, w.decoder_options,
                                           C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                           C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    out = (w.decoder_results * (nseg * K))(); nres = (C.c_int * nseg)()

    def call(flags):
        st = np.zeros((64 * nseg, 32), np.uint8); n_st = C.c_int(0)
        return L.wspr_decode_batch_hashed(ol.ptr(I), ol.ptr(Q), nseg, NS, NS, _opt(w, 1), C.addressof(out), K,
                                          C.addressof(nres), 0, 0, None, 0, flags, ol.ptr(st), len(st), C.byref(n_st), None)
    assert w.wspr_set_arithmetic(w.WSPR_ARITH_CONTRACTED) == 0
    try:
        assert call(1) == 0                                       # KEEP_FILE, contracted
        assert w.wspr_set_arithmetic(w.WSPR_ARITH_EXACT) == 1
        assert call(1 | 2) < 0                                    # REVISIT under the other mode: refused
        assert w.wspr_set_arithmetic(w.WSPR_ARITH_CONTRACTED) == 0
        assert call(1 | 2) == 0                                   # the same revisit under its own mode completes it
    finally:
        w.wspr_set_arithmetic(w.WSPR_ARITH_EXACT)


_CHILD = r"""
import sys, numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import torch  # noqa: F401  (first, as tests/conftest.py does)
import rtlsdr_wsprd_amd as w
import test_gpu_contracted as t
from test_gpu_parity import random_scenes
I, Q = random_scenes(int(sys.argv[3]))
got, ri, rq = t._decode_writeback(w, I, Q)
np.savez(sys.argv[2], spots=np.frombuffer(b"".join(bytes(x) for seg in got for x in seg), np.uint8),
         counts=np.array([len(seg) for seg in got]), ri=ri, rq=rq)
"""


def test_exact_after_contracted_equals_a_fresh_process(w, tmp_path):
    """Exact, contracted, exact again in this process; the last exact decode must be byte for byte what a fresh
    process (that never switched) decodes: spot records and residuals."""
    n = 160
    I, Q = random_scenes(n)
    assert w.wspr_set_arithmetic(w.WSPR_ARITH_CONTRACTED) == 0
    try:
        contracted, _, _ = _decode_writeback(w, I, Q)
    finally:
        assert w.wspr_set_arithmetic(w.WSPR_ARITH_EXACT) == 1
    got, ri, rq = _decode_writeback(w, I, Q)
    path = str(tmp_path / "fresh.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path, str(n)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    fresh = np.load(path)
    assert list(fresh["counts"]) == [len(seg) for seg in got]
    assert fresh["spots"].tobytes() == b"".join(bytes(x) for seg in got for x in seg)
    assert np.array_equal(fresh["ri"], ri) and np.array_equal(fresh["rq"], rq)
    assert [[bytes(x) for x in seg] for seg in contracted] != [[bytes(x) for x in seg] for seg in got]
