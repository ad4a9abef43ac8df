"""GPU parity tests: every HIP stage, called through the C ABI of libwspr_mi355x.so,
against the CPU oracle on the same inputs.  Bit-exact unless stated."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
import synth

pytestmark = pytest.mark.gpu

NS = 45000


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    return mod


def symf(msg):
    ok, s = ol.channel_symbols(msg)
    assert ok
    return s


@pytest.fixture(scope="module")
def ref_iq():
    I, Q, n = ol.read_iq_file(os.path.join(ol.GOLDEN, "refSignalSnr0dB.iq"))
    return I, Q


@pytest.fixture(scope="module")
def synth_batch():
    segs = [synth.make_segment(1000 + s, symf, snr_db=-20.0) for s in range(6)]
    segs.append(synth.make_segment(77, symf, n_signals=4, snr_db=-8.0, snr_span=12.0, t_jitter=0.3))
    segs.append(synth.make_segment(78, symf, snr_db=-15.0, drift=2.0))
    I = np.stack([s[0] for s in segs])
    Q = np.stack([s[1] for s in segs])
    return I, Q, [s[2] for s in segs]


def oracle_ps(I, Q, n=NS):
    L = ol.lib()
    blocks = L.orc_blocks_for(n)
    ps = np.zeros((512, blocks), np.float32)
    L.orc_fft_bank(ol.ptr(I), ol.ptr(Q), C.c_int(n), ol.ptr(ps))
    return ps


# ------------------------------------------------------------------ K1
def test_fft_bank_bit_exact_vs_oracle_and_close_to_numpy(w, synth_batch, ref_iq):
    I = np.stack([ref_iq[0], synth_batch[0][0], synth_batch[0][6]])
    Q = np.stack([ref_iq[1], synth_batch[1][0], synth_batch[1][6]])
    blocks = 347
    out = np.zeros((3, 512, blocks), np.float32)
    rc = w.lab().wspr_stage_fft_bank(ol.ptr(I), ol.ptr(Q), 3, NS, NS, ol.ptr(out))
    assert rc == blocks
    for s in range(3):
        ps = oracle_ps(I[s], Q[s])
        assert np.array_equal(out[s, 48:465], ps[48:465])            # same butterflies -> same bits
        assert not out[s, :48].any() and not out[s, 465:].any()
    # independent check of the FFT itself (double precision numpy), SURVEY parity gate 1e-5
    win = np.sin(np.float32(1.0) * 0.006147931 * np.arange(512)).astype(np.float32)
    t = 100
    x = (I[0, 128 * t:128 * t + 512].astype(np.float64) + 1j * Q[0, 128 * t:128 * t + 512]) * win
    p = np.abs(np.fft.fftshift(np.fft.fft(x))) ** 2
    assert np.allclose(out[0, 48:465, t], p[48:465], rtol=2e-4, atol=1e-4 * p.max())


# ------------------------------------------------------------------ K2 + K3
def _oracle_cands(I, Q, coarse):
    L = ol.lib()
    ps = oracle_ps(I, Q)
    cands = (ol.Cand * 200)()
    noise = C.c_float()
    sm = np.zeros(411, np.float32)
    npk = L.orc_pick_peaks(ol.ptr(ps), C.c_int(347), cands, C.byref(noise), ol.ptr(sm), None)
    if coarse:
        L.orc_coarse_sync(ol.ptr(ps), C.c_int(347), cands, C.c_int(npk), C.c_int(4))
    return npk, cands, noise.value, sm


@pytest.mark.parametrize("coarse", [0, 1])
def test_candidates_match_oracle(w, synth_batch, ref_iq, coarse):
    I = np.concatenate([ref_iq[0][None], synth_batch[0]])
    Q = np.concatenate([ref_iq[1][None], synth_batch[1]])
    nseg = I.shape[0]
    cands = (w.cand * (200 * nseg))()
    npk = (C.c_int * nseg)()
    noise = np.zeros(nseg, np.float32)
    sm = np.zeros((nseg, 411), np.float32)
    rc = w.lab().wspr_stage_candidates(ol.ptr(I), ol.ptr(Q), nseg, NS, NS, coarse, 4, C.addressof(cands),
                                       C.addressof(npk), ol.ptr(noise), ol.ptr(sm))
    assert rc == 0
    for s in range(nseg):
        onpk, oc, onoise, osm = _oracle_cands(I[s], Q[s], coarse)
        assert npk[s] == onpk
        assert noise[s] == np.float32(onoise)
        assert np.array_equal(sm[s], osm)
        for j in range(onpk):
            g, o = cands[200 * s + j], oc[j]
            assert (g.freq, g.shift, g.drift, g.sync) == (o.freq, o.shift, o.drift, o.sync), (s, j)
            assert g.snr == o.snr                                   # ranked and reported with the host libm


def test_equal_snr_ties_keep_the_reference_order(w):
    """Candidates with EXACTLY equal snr (wsprd.c:616, 631: qsort of a list built in ascending bin order; glibc's
    qsort is a stable merge sort at this size, so ties stay in bin order).  A real-valued record (Q = 0) has a
    mirror-symmetric spectrum, bit for bit, so every peak comes with a twin of identical snr at the mirrored
    frequency: the product's host re-rank must put the twins in the oracle's order -- they are then refined,
    decoded and subtracted in that order."""
    rng = np.random.default_rng(5)
    t = np.arange(NS) / 375.0
    recs = []
    for f1, f2, f3 in ((40.3, 77.7, 12.1), (5.5, 93.0, 61.2)):
        recs.append((0.02 * rng.normal(size=NS) + 0.3 * np.cos(2 * np.pi * f1 * t) + 0.2 * np.cos(2 * np.pi * f2 * t)
                     + 0.1 * np.cos(2 * np.pi * f3 * t)).astype(np.float32))
    I = np.stack(recs)
    Q = np.zeros_like(I)
    for coarse in (0, 1):
        cands = (w.cand * (200 * 2))()
        npk = (C.c_int * 2)()
        assert w.lab().wspr_stage_candidates(ol.ptr(I), ol.ptr(Q), 2, NS, NS, coarse, 4, C.addressof(cands),
                                             C.addressof(npk), None, None) == 0
        for s in range(2):
            onpk, oc, _, _ = _oracle_cands(I[s], Q[s], coarse)
            assert npk[s] == onpk and onpk >= 6
            snrs = [oc[j].snr for j in range(onpk)]
            assert len(snrs) - len(set(snrs)) >= 3                   # the twins really tie
            for j in range(onpk):
                g, o = cands[200 * s + j], oc[j]
                assert (g.freq, g.snr, g.shift, g.drift, g.sync) == (o.freq, o.snr, o.shift, o.drift, o.sync), (s, j)
    # and through the whole decoder (nothing decodes; the residuals and the empty spot lists agree)
    got = w.wspr_decode_batch(I, Q, w.default_options(), max_results=8)
    assert [len(g) for g in got] == [len(ol.decode(I[s], Q[s], NS)[0]) for s in range(2)]


@pytest.mark.parametrize("maxdrift", [4, 0])
def test_coarse_sync_of_a_large_batch_matches_oracle(w, synth_batch, ref_iq, maxdrift):
    """Batches of 1 536 segments and more take the lane-per-(candidate, lag) coarse-sync kernel (one lane holds the
    three frequency bins of its lag; amplitudes staged in two halves of 81 symbols).  The small parity batch is
    tiled to 1 600 segments; every copy's candidates equal the oracle's: frequency, lag, drift label and sync,
    with drift search (nine hypotheses per lag) and without (maxdrift 0: pattern 1 only)."""
    I0 = np.concatenate([ref_iq[0][None], synth_batch[0]])
    Q0 = np.concatenate([ref_iq[1][None], synth_batch[1]])
    n0 = I0.shape[0]
    reps = -(-1600 // n0)
    I = np.tile(I0, (reps, 1)); Q = np.tile(Q0, (reps, 1))
    nseg = I.shape[0]
    assert nseg >= 1536
    cands = (w.cand * (200 * nseg))()
    npk = (C.c_int * nseg)()
    noise = np.zeros(nseg, np.float32)
    sm = np.zeros((nseg, 411), np.float32)
    rc = w.lab().wspr_stage_candidates(ol.ptr(I), ol.ptr(Q), nseg, NS, NS, 1, maxdrift, C.addressof(cands),
                                       C.addressof(npk), ol.ptr(noise), ol.ptr(sm))
    assert rc == 0
    L = ol.lib()
    for s0 in range(n0):
        onpk, oc, onoise, osm = _oracle_cands(I0[s0], Q0[s0], 0)
        L.orc_coarse_sync(ol.ptr(oracle_ps(I0[s0], Q0[s0])), C.c_int(347), oc, C.c_int(onpk), C.c_int(maxdrift))
        for rep in range(reps):
            s = rep * n0 + s0
            assert npk[s] == onpk
            # the time average comes from the FUSED K1 here (one workgroup per segment, pairs of FFTs per wave)
            assert noise[s] == np.float32(onoise) and np.array_equal(sm[s], osm), s
            for j in range(onpk):
                g, o = cands[200 * s + j], oc[j]
                assert (g.freq, g.shift, g.drift, g.sync, g.snr) == (o.freq, o.shift, o.drift, o.sync, o.snr), (s, j)


def band_edge_records():
    """Two records with tones on the picker's last bins inside +-110 Hz (smoothed bins 55 and 355, +-109.86 Hz): their
    candidates have if0 106 and 406, so the coarse sync stages rows 100 .. 110 and 400 .. 410 -- the first and the last
    row the fused K1 stores."""
    rng = np.random.default_rng(55355)
    t = np.arange(NS) / 375.0
    recs = []
    for a_lo, a_hi in ((0.3, 0.2), (0.1, 0.25)):
        z = 0.02 * (rng.normal(size=NS) + 1j * rng.normal(size=NS))
        z = z + a_lo * np.exp(-2j * np.pi * 150 * (375.0 / 512.0) * t) + a_hi * np.exp(2j * np.pi * 150 * (375.0 / 512.0) * t)
        recs.append(z)
    return (np.stack([z.real for z in recs]).astype(np.float32), np.stack([z.imag for z in recs]).astype(np.float32))


def test_band_edge_candidates_through_the_fused_fft_bank(w, synth_batch, ref_iq):
    """256 segments (the fused K1, which stores rows 100 .. 410 only): candidates on both edge bins read exactly up to
    the first and the last stored row.  A call on the batch scaled by 10^3 comes first, so that whatever the fused K1
    does not store holds foreign values."""
    eI, eQ = band_edge_records()
    I0 = np.concatenate([ref_iq[0][None], synth_batch[0], eI])
    Q0 = np.concatenate([ref_iq[1][None], synth_batch[1], eQ])
    n0 = I0.shape[0]
    reps = -(-256 // n0)
    I = np.tile(I0, (reps, 1))[:256].copy(); Q = np.tile(Q0, (reps, 1))[:256].copy()
    nseg = 256
    cands = (w.cand * (200 * nseg))()
    npk = (C.c_int * nseg)()
    noise = np.zeros(nseg, np.float32)
    sm = np.zeros((nseg, 411), np.float32)
    Ik, Qk = I * np.float32(1e3), Q * np.float32(1e3)
    assert w.lab().wspr_stage_candidates(ol.ptr(Ik), ol.ptr(Qk), nseg, NS, NS, 1, 4, C.addressof(cands), C.addressof(npk),
                                         None, None) == 0
    assert w.lab().wspr_stage_candidates(ol.ptr(I), ol.ptr(Q), nseg, NS, NS, 1, 4, C.addressof(cands), C.addressof(npk),
                                         ol.ptr(noise), ol.ptr(sm)) == 0
    L = ol.lib()
    if0_seen = set()
    for s0 in range(n0):
        onpk, oc, onoise, osm = _oracle_cands(I0[s0], Q0[s0], 0)
        if0_seen |= {int(oc[j].freq / (375.0 / 256.0 / 2.0) + 256.0) for j in range(onpk)}
        L.orc_coarse_sync(ol.ptr(oracle_ps(I0[s0], Q0[s0])), C.c_int(347), oc, C.c_int(onpk), C.c_int(4))
        for s in range(s0, nseg, n0):
            assert npk[s] == onpk
            assert noise[s] == np.float32(onoise) and np.array_equal(sm[s], osm), s
            for j in range(onpk):
                g, o = cands[200 * s + j], oc[j]
                assert (g.freq, g.shift, g.drift, g.sync, g.snr) == (o.freq, o.shift, o.drift, o.sync, o.snr), (s, j)
    assert {106, 406} <= if0_seen


@pytest.mark.parametrize("samples", [40000, 44992, 2048, 1024])
def test_short_records_through_the_fused_fft_bank(w, synth_batch, ref_iq, samples):
    """Records shorter than 45 000 samples in a batch large enough for the fused K1 (>= 256 segments): the last group
    of time blocks is partial (waves with three blocks, or none), windows are fetched up to the end of the row.
    Peak picker inputs (time average -> smoothed spectrum, noise) and candidates equal the oracle's on the same
    truncated record."""
    I0 = np.concatenate([ref_iq[0][None], synth_batch[0]])[:, :samples].copy()
    Q0 = np.concatenate([ref_iq[1][None], synth_batch[1]])[:, :samples].copy()
    n0 = I0.shape[0]
    reps = -(-256 // n0)
    I = np.tile(I0, (reps, 1)); Q = np.tile(Q0, (reps, 1))
    nseg = I.shape[0]
    cands = (w.cand * (200 * nseg))()
    npk = (C.c_int * nseg)()
    noise = np.zeros(nseg, np.float32)
    sm = np.zeros((nseg, 411), np.float32)
    rc = w.lab().wspr_stage_candidates(ol.ptr(I), ol.ptr(Q), nseg, samples, samples, 0, 4, C.addressof(cands),
                                       C.addressof(npk), ol.ptr(noise), ol.ptr(sm))
    assert rc == 0
    L = ol.lib()
    blocks = 4 * (samples // 512) - 1
    for s0 in range(n0):
        ps = np.zeros((512, blocks), np.float32)
        assert L.orc_blocks_for(samples) == blocks
        # the reference's last block ends at 512 floor(samples / 512) + 255, which may lie behind `samples`
        # (wsprd.c:536-542): its caller's buffers hold 45 000 samples, zeros behind the record -- the oracle
        # gets such a buffer, the product zero-fills its own rows
        Iz = np.concatenate([I0[s0], np.zeros(NS - samples, np.float32)])
        Qz = np.concatenate([Q0[s0], np.zeros(NS - samples, np.float32)])
        L.orc_fft_bank(ol.ptr(Iz), ol.ptr(Qz), C.c_int(samples), ol.ptr(ps))
        oc = (ol.Cand * 200)()
        onoise = C.c_float()
        osm = np.zeros(411, np.float32)
        onpk = L.orc_pick_peaks(ol.ptr(ps), C.c_int(blocks), oc, C.byref(onoise), ol.ptr(osm), None)
        for rep in range(reps):
            s = rep * n0 + s0
            assert npk[s] == onpk, (s, samples)
            assert noise[s] == np.float32(onoise.value) and np.array_equal(sm[s], osm), (s, samples)
            for j in range(onpk):
                assert (cands[200 * s + j].freq, cands[200 * s + j].snr) == (oc[j].freq, oc[j].snr), (s, j)
    if samples > 2048:
        return
    # and through coarse_sync_kernel<false> (symbols behind the record masked; 1 024 samples are 7 blocks: a negative
    # time index reaches two rows back)
    rc = w.lab().wspr_stage_candidates(ol.ptr(I), ol.ptr(Q), nseg, samples, samples, 1, 4, C.addressof(cands),
                                       C.addressof(npk), ol.ptr(noise), ol.ptr(sm))
    assert rc == 0
    for s0 in range(n0):
        ps = np.zeros((512, blocks), np.float32)
        Iz = np.concatenate([I0[s0], np.zeros(NS - samples, np.float32)])
        Qz = np.concatenate([Q0[s0], np.zeros(NS - samples, np.float32)])
        L.orc_fft_bank(ol.ptr(Iz), ol.ptr(Qz), C.c_int(samples), ol.ptr(ps))
        oc = (ol.Cand * 200)()
        onoise = C.c_float()
        osm = np.zeros(411, np.float32)
        onpk = L.orc_pick_peaks(ol.ptr(ps), C.c_int(blocks), oc, C.byref(onoise), ol.ptr(osm), None)
        L.orc_coarse_sync(ol.ptr(ps), C.c_int(blocks), oc, C.c_int(onpk), C.c_int(4))
        for rep in range(reps):
            s = rep * n0 + s0
            assert npk[s] == onpk, (s, samples)
            assert noise[s] == np.float32(onoise.value) and np.array_equal(sm[s], osm), (s, samples)
            for j in range(onpk):
                g, o = cands[200 * s + j], oc[j]
                assert (g.freq, g.shift, g.drift, g.sync, g.snr) == (o.freq, o.shift, o.drift, o.sync, o.snr), (s, j, samples)


# ------------------------------------------------------------------ K4 / K5
def _both_demod(w, I, Q, freq, shift, drift, mode, lagmin=0, lagmax=0, lagstep=8, ifmin=0, ifmax=0, fstep=0.0, np_=NS,
                symfac=50):
    res = []
    for which in ("gpu", "cpu"):
        Ic, Qc = I.copy(), Q.copy()
        f = C.c_float(freq); sh = C.c_int(shift); dr = C.c_float(drift); sy = C.c_float(0)
        sym = (C.c_ubyte * 162)()
        args = [ol.ptr(Ic), ol.ptr(Qc), C.c_long(np_), sym, C.addressof(f), ifmin, ifmax, C.c_float(fstep),
                C.addressof(sh), lagmin, lagmax, lagstep, C.addressof(dr), symfac, C.addressof(sy), mode]
        if which == "gpu":
            w.lib().sync_and_demodulate(*args)
        else:
            ol.lib().orc_sync_demod(*args)
        res.append((f.value, sh.value, sy.value, bytes(sym)))
    return res


@pytest.mark.parametrize("seg,drift", [(0, 0.0), (3, 0.0), (7, 2.0), (7, -4.0), (6, 1.0)])
def test_sync_and_demodulate_modes_bit_exact(w, synth_batch, seg, drift):
    I, Q, truth = synth_batch
    msg, f0, t0, snr = truth[seg][0]
    fc = float(np.float32(round(f0 / 0.732421875) * 0.732421875))
    sc = int(round(t0 * 375 / 128.0)) * 128
    g, o = _both_demod(w, I[seg], Q[seg], fc, sc, drift, 0, lagmin=sc - 128, lagmax=sc + 128, lagstep=8)
    assert g[:3] == o[:3]
    shift = o[1]
    g, o = _both_demod(w, I[seg], Q[seg], fc, shift, drift, 1, ifmin=-2, ifmax=2, fstep=0.1)
    assert g[:3] == o[:3]
    fbest = o[0]
    for jig in (0, -3, 3, 63, -63):
        g, o = _both_demod(w, I[seg], Q[seg], fbest, shift + jig, drift, 2)
        assert g[2] == o[2] and g[3] == o[3]


def test_sync_and_demodulate_edges(w, synth_batch):
    """Signal window hanging off both ends of the buffer (partial decode) and short np."""
    I, Q, _ = synth_batch
    for shift in (-1400, -300, 3700, 4100):
        g, o = _both_demod(w, I[0], Q[0], 10.0, shift, 0.0, 2)
        assert g[2:] == o[2:]
        g, o = _both_demod(w, I[0], Q[0], -37.5, shift, 1.0, 0, lagmin=shift - 128, lagmax=shift + 128, lagstep=16)
        assert g[:3] == o[:3]
    g, o = _both_demod(w, I[0], Q[0], 10.0, 700, 0.0, 2, np_=44000)
    assert g[2:] == o[2:]


@pytest.mark.parametrize("symfac", [50, 64, 20, 127, 1])
def test_sync_and_demodulate_honours_symfac(w, synth_batch, symfac):
    """wsprd.c:250: the soft symbols of mode 2 are scaled by the caller's symfac (the decoder passes 50; round 2
    ignored every other value)."""
    I, Q, truth = synth_batch
    msg, f0, t0, snr = truth[1][0]
    g, o = _both_demod(w, I[1], Q[1], float(np.float32(f0)), int(round(t0 * 375)), 0.0, 2, symfac=symfac)
    assert g[2] == o[2] and g[3] == o[3]
    if symfac != 50:
        base = _both_demod(w, I[1], Q[1], float(np.float32(f0)), int(round(t0 * 375)), 0.0, 2)[0]
        assert base[3] != g[3]


# ------------------------------------------------------------------ K7
@pytest.mark.parametrize("seg,drift,shift_off,np_", [(0, 0.0, 0, NS), (6, 0.0, 0, NS), (7, 2.0, 0, NS), (1, 0.0, -2500, NS),
                                                     (2, -1.0, 3900, NS), (3, 0.5, 0, 30000)])
def test_subtract_signal_symbolwise_bit_exact(w, synth_batch, seg, drift, shift_off, np_):
    """subtract_signal() (wsprd.h:83-89, wsprd.c:263-312): exported by the reference, not called by its decoder."""
    I, Q, truth = synth_batch
    msg, f0, t0, snr = truth[seg][0]
    sym = symf(msg)
    shift = int(round(t0 * 375)) + shift_off
    outs = []
    for which in ("gpu", "cpu"):
        Ic, Qc = I[seg].copy(), Q[seg].copy()
        args = [ol.ptr(Ic), ol.ptr(Qc), C.c_long(np_), C.c_float(f0), C.c_int(shift), C.c_float(drift), ol.ptr(sym)]
        (w.lib().subtract_signal if which == "gpu" else ol.lib().orc_subtract_simple)(*args)
        outs.append((Ic, Qc))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert not np.array_equal(outs[0][0], I[seg])
    assert np.array_equal(outs[0][0][np_:], I[seg][np_:])          # nothing beyond np is touched


@pytest.mark.parametrize("seg,drift,shift_off,np_", [(0, 0.0, 0, NS), (6, 0.0, 0, NS), (7, 2.0, 0, NS), (1, 0.0, -2500, NS),
                                                     (2, -1.0, 3900, NS), (3, 0.0, 0, 30000), (4, 1.0, -700, 41000),
                                                     (5, 0.0, -41000, NS), (0, 0.0, 44000, NS)])
def test_subtract_signal2_bit_exact(w, synth_batch, seg, drift, shift_off, np_):
    """Incl. records shorter than the frame (np < 45000), frames hanging off either end by thousands of samples and
    frames almost entirely outside the record: the fused kernel's tiles (2 048 outputs, even ones first, then the odd
    ones with the halos the even ones saved) must reproduce the reference's edge handling (wsprd.c:370-404)."""
    I, Q, truth = synth_batch
    msg, f0, t0, snr = truth[seg][0]
    sym = symf(msg)
    shift = int(round(t0 * 375)) + shift_off
    outs = []
    for which in ("gpu", "cpu"):
        Ic, Qc = I[seg].copy(), Q[seg].copy()
        args = [ol.ptr(Ic), ol.ptr(Qc), C.c_long(np_), C.c_float(f0), C.c_int(shift), C.c_float(drift), ol.ptr(sym)]
        (w.lib().subtract_signal2 if which == "gpu" else ol.lib().orc_subtract)(*args)
        outs.append((Ic, Qc))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert not np.array_equal(outs[0][0], I[seg])


# ------------------------------------------------------------------ whole path
def _spot_tuple(s):
    return (s.message, s.call, s.loc, s.pwr, s.cycles, s.jitter, s.drift, s.sync, s.dt, s.freq)


def test_reference_file_spot_line(w, ref_iq):
    spots, ri, rq = w.wspr_decode(ref_iq[0], ref_iq[1], NS, w.default_options())
    assert len(spots) == 1
    assert ol.spot_line(spots[0]) == "Spot :  -0.07   0.01 144.490550  0    K1JT   FN20 20"   # REPORT.md:202
    ref, oi, oq = ol.decode(ref_iq[0], ref_iq[1], NS)
    assert _spot_tuple(spots[0]) == _spot_tuple(ref[0])
    assert abs(spots[0].snr - ref[0].snr) < 1e-4
    assert np.array_equal(ri, oi) and np.array_equal(rq, oq)        # residual after subtraction


@pytest.mark.parametrize("opts", [dict(), dict(quickmode=1), dict(subtraction=0), dict(npasses=1), dict(npasses=3)])
def test_batch_decode_equals_oracle(w, synth_batch, opts):
    I, Q, truth = synth_batch
    got = w.wspr_decode_batch(I, Q, w.default_options(**opts), max_results=16)
    for s in range(I.shape[0]):
        ref, _, _ = ol.decode(I[s], Q[s], NS, ol.default_options(**opts))
        assert [_spot_tuple(x) for x in got[s]] == [_spot_tuple(x) for x in ref], s
        for a, b in zip(got[s], ref):
            assert abs(a.snr - b.snr) < 1e-4
    if not opts:
        for s in range(6):      # the -20 dB single-signal segments all decode
            assert [x.message.decode() for x in got[s]] == [synth.expected_text(truth[s][0][0])]


def random_scenes(count=None, seed=None):
    """The randomised scenes of test_randomised_scenes_equal_oracle (also traced per candidate in test_gpu_trace.py)."""

    rng = np.random.default_rng(int(os.environ.get("WSPR_SCENE_SEED", "20260928")) if seed is None else seed)
    sigma = np.sqrt((375.0 / 2500.0) / 2.0)
    t23 = ["PJ4/K1ABC 37", "K1ABC/7 33", "<PJ4/K1ABC> FK52UD 37"]
    Is, Qs = [], []
    for scene in range(int(os.environ.get("WSPR_SCENES", "420")) if count is None else count):      # (a longer soak: WSPR_SCENES=1200)
        I = rng.normal(0, sigma, NS); Q = rng.normal(0, sigma, NS)
        nsig = 0 if scene == 0 else int(rng.integers(1, 7))
        base = rng.uniform(-125, 125, nsig)
        if nsig >= 2 and scene % 5 == 0:
            base[1] = base[0] + rng.uniform(1.0, 4.0)               # near-collision
        for k in range(nsig):
            msg = t23[int(rng.integers(0, 3))] if rng.random() < 0.2 else synth.message_for(int(rng.integers(0, 1 << 20)))
            amp = 10.0 ** (rng.uniform(-31, 6) / 20.0)
            si, sq = synth.tone_signal(symf(msg), base[k], rng.uniform(0.2, 3.8), amp, drift=float(rng.integers(-3, 4)))
            I += si; Q += sq
        if scene % 7 == 3:                                            # unmodulated carrier
            ph = 2 * np.pi * rng.uniform(-100, 100) / 375.0 * np.arange(NS)
            I += 3.0 * np.cos(ph); Q += 3.0 * np.sin(ph)
        a, b = synth.normalise(I.astype(np.float32), Q.astype(np.float32))
        Is.append(a); Qs.append(b)
    I = np.stack(Is); Q = np.stack(Qs)
    return I, Q


def test_randomised_scenes_equal_oracle(w):
    """Forty random scenes the fixed fixtures do not cover: 0-6 signals of type 1/2/3, SNR -31..+6 dB,
    drifts -3..+3 Hz, starts 0.2..3.8 s (part of the frame may fall off either end), carriers out to
    +-125 Hz (beyond the +-110 Hz candidate window), two signals a few Hz apart, a strong CW carrier, and
    a segment of plain noise.  Every spot field must equal the oracle's (SNR within the stated 0.1 dB)."""
    I, Q = random_scenes()
    got = w.wspr_decode_batch(I, Q, w.default_options())
    total = 0
    for s in range(I.shape[0]):
        ref, _, _ = ol.decode(I[s], Q[s], NS)
        assert [_spot_tuple(x) for x in got[s]] == [_spot_tuple(x) for x in ref], s
        assert all(abs(a.snr - b.snr) < 1e-4 for a, b in zip(got[s], ref))
        total += len(ref)
    assert total > 40 and len(got[0]) == 0


def test_messages_from_the_whole_type1_space_equal_oracle(w):
    """Round 6: the benchmark's signals carry messages drawn from the whole type-1 space (synth.message_wide: four-,
    five- and six-character calls of both packing shapes, every locator field, every power) instead of twenty calls x
    twenty grids.  64 segments x 3 such signals: every field of every spot equals the oracle's, and what is decoded is
    what was sent (the unpack / re-encode path written by hand in round 6 sits under every one of these spots)."""
    rng = np.random.default_rng(606)
    sigma = np.sqrt((375.0 / 2500.0) / 2.0)
    Is, Qs, sent = [], [], []
    for s in range(64):
        I = rng.normal(0, sigma, NS); Q = rng.normal(0, sigma, NS)
        msgs = [synth.message_wide(int(rng.integers(0, 1 << 62))) for _ in range(3)]
        for k, m in enumerate(msgs):
            si, sq = synth.tone_signal(symf(m), -80.0 + 80.0 * k + rng.uniform(-3, 3), rng.uniform(1.7, 2.3), 10.0 ** ((-9.0 - 3 * k) / 20.0))
            I += si; Q += sq
        a, b = synth.normalise(I.astype(np.float32), Q.astype(np.float32))
        Is.append(a); Qs.append(b); sent.append([synth.expected_text(m) for m in msgs])
    I = np.stack(Is); Q = np.stack(Qs)
    got = w.wspr_decode_batch(I, Q, w.default_options())
    hits = 0
    for s in range(64):
        ref, _, _ = ol.decode(I[s], Q[s], NS)
        assert [_spot_tuple(x) for x in got[s]] == [_spot_tuple(x) for x in ref], s
        assert all(abs(a.snr - b.snr) < 1e-4 for a, b in zip(got[s], ref))
        texts = [x.message.decode() for x in got[s]]
        assert all(t in sent[s] for t in texts), (s, texts, sent[s])          # no false decode
        hits += len(set(texts) & set(sent[s]))
    assert hits >= 0.95 * 3 * 64
    shapes = {len(t.split()[0]) for seg in sent for t in seg}
    assert shapes >= {4, 5, 6}


def crowded_scenes(count, seed=77):
    """Bands the other generators do not produce: 12-40 signals inside +-112 Hz (many closer than one tone
    spacing), -24..+12 dB, so that a segment yields dozens of candidates, repeated decodes of one signal and
    more than sixteen spots."""
    rng = np.random.default_rng(seed)
    sigma = np.sqrt((375.0 / 2500.0) / 2.0)
    Is, Qs = [], []
    for scene in range(count):
        nsig = int(rng.integers(12, 41))
        I = rng.normal(0, sigma, NS); Q = rng.normal(0, sigma, NS)
        f = np.sort(rng.uniform(-112, 112, nsig))
        for k in range(nsig):
            msg = synth.message_for(int(rng.integers(0, 1 << 20)))
            amp = 10.0 ** (rng.uniform(-24, 12) / 20.0)
            si, sq = synth.tone_signal(symf(msg), f[k], rng.uniform(0.5, 3.5), amp, drift=float(rng.integers(-2, 3)))
            I += si; Q += sq
        a, b = synth.normalise(I.astype(np.float32), Q.astype(np.float32))
        Is.append(a); Qs.append(b)
    return np.stack(Is), np.stack(Qs)


@pytest.mark.parametrize("opts", [{}, {"npasses": 3}, {"subtraction": 0}, {"quickmode": 1}, {"npasses": 1}])
def test_crowded_band_equals_oracle(w, opts):
    """Crowded bands under every option set: spot for spot the oracle's (a longer soak: WSPR_CROWDED=200)."""
    I, Q = crowded_scenes(int(os.environ.get("WSPR_CROWDED", "12")))
    got = w.wspr_decode_batch(I, Q, w.default_options(**opts), max_results=100)
    most = 0
    for s in range(I.shape[0]):
        ref, _, _ = ol.decode(I[s], Q[s], NS, ol.default_options(**opts))
        assert [_spot_tuple(x) for x in got[s]] == [_spot_tuple(x) for x in ref], (s, opts)
        assert all(abs(a.snr - b.snr) < 1e-4 for a, b in zip(got[s], ref))
        most = max(most, len(ref))
    assert most >= 8


def test_committed_scene_spots_without_the_oracle(w):
    """The product against tests/golden/scene_spots.json alone (no oracle call in the loop): every field
    of every spot, SNR to the stated 0.1 dB."""
    import json
    import scenes
    gold = json.load(open(os.path.join(ol.GOLDEN, "scene_spots.json")))["scenes"]
    I = np.stack([scenes.make_scene(g["seed"])[0] for g in gold])
    Q = np.stack([scenes.make_scene(g["seed"])[1] for g in gold])
    got = w.wspr_decode_batch(I, Q, w.default_options())
    for g, spots in zip(gold, got):
        rec = [scenes.spot_record(s) for s in spots]
        assert [{k: v for k, v in r.items() if k != "snr"} for r in rec] == \
               [{k: v for k, v in r.items() if k != "snr"} for r in g["spots"]], g["seed"]
        assert all(abs(a["snr"] - b["snr"]) <= 0.1 for a, b in zip(rec, g["spots"]))


def test_non_finite_and_extreme_inputs_terminate(w, ref_iq):
    """NaN / Inf / overflowing / denormal / all-zero IQ: the decoder must come back (no fault, no endless
    search); where the input is finite the spots are the oracle's."""
    I, Q = ref_iq
    a = I.copy(); a[1000] = np.nan
    b = I.copy(); b[5000:5100] = np.inf
    cases = [(a, Q.copy(), False), (b, Q.copy(), False), (np.full_like(I, np.nan), np.full_like(Q, np.nan), False),
             (np.zeros_like(I), np.zeros_like(Q), True), (I * np.float32(1e30), Q * np.float32(1e30), True),
             (I * np.float32(1e-42), Q * np.float32(1e-42), True), (I * np.float32(1e-3), Q * np.float32(1e-3), True)]
    for x, y, finite in cases:
        spots, _, _ = w.wspr_decode(x, y, NS)
        if finite:
            ref, _, _ = ol.decode(x, y, NS)
            assert [_spot_tuple(s) for s in spots] == [_spot_tuple(s) for s in ref]
        else:
            assert len(spots) <= 1
    # the scaled-down copy still decodes (the decoder is scale-free apart from float range)
    assert [s.message for s in w.wspr_decode(I * np.float32(1e-3), Q * np.float32(1e-3), NS)[0]] == [b"K1JT FN20 20"]


def test_empty_and_degenerate_inputs(w):
    z = np.zeros((2, NS), np.float32)
    assert w.wspr_decode_batch(z, z) == [[], []]
    rng = np.random.default_rng(5)
    n = rng.normal(0, 0.1, (2, NS)).astype(np.float32)
    got = w.wspr_decode_batch(n, n[::-1].copy())
    for s in range(2):
        ref, _, _ = ol.decode(n[s], n[::-1][s], NS)
        assert [_spot_tuple(x) for x in got[s]] == [_spot_tuple(x) for x in ref]
    # short record (ragged input): 40000 samples
    I, Q, _ = synth.make_segment(4242, symf, snr_db=-12.0)
    spots, _, _ = w.wspr_decode(I[:40000], Q[:40000], 40000)
    ref, _, _ = ol.decode(np.concatenate([I[:40000], np.zeros(5000, np.float32)]),
                          np.concatenate([Q[:40000], np.zeros(5000, np.float32)]), 40000)
    assert [_spot_tuple(x) for x in spots] == [_spot_tuple(x) for x in ref]


def test_a_record_longer_than_45000_samples_is_refused(w):
    """The reference sizes its FFT bank from `samples` (wsprd.c:516); this library's rows hold 45 000 samples and a
    longer record is an error (-2, no spots, inputs untouched), not a silently shortened decode."""
    import ctypes as C
    n = NS + 512
    I = np.full(n, 0.25, np.float32)
    Q = np.full(n, -0.25, np.float32)
    I0, Q0 = I.copy(), Q.copy()
    out = (w.decoder_results * 100)()
    nres = C.c_int(7)
    assert w.lib().wspr_decode(ol.ptr(I), ol.ptr(Q), n, w.default_options(), C.addressof(out), C.addressof(nres)) == -2
    assert nres.value == 0 and np.array_equal(I, I0) and np.array_equal(Q, Q0)
    nb = (C.c_int * 2)(5, 5)
    outb = (w.decoder_results * 20)()
    I2, Q2 = np.stack([I, I]), np.stack([Q, Q])
    assert w.lib().wspr_decode_batch(ol.ptr(I2), ol.ptr(Q2), 2, n, n, w.default_options(), C.addressof(outb), 10,
                                     C.addressof(nb), 0) == -2
    assert list(nb) == [0, 0]
    # exactly 45 000 is the reference's own case
    spots, _, _ = w.wspr_decode(I[:NS], Q[:NS], NS)
    assert spots == []


# ------------------------------------------------------------------ K0
def test_decimator_bit_exact_vs_oracle(w):
    rng = np.random.default_rng(11)
    nsamp = 6401 * 300 + 1000
    n = np.arange(nsamp)
    ph = 2 * np.pi * (-600000.0 + 40.0) / 2.4e6 * n
    sig = 6.0 * np.exp(1j * ph)
    raw = np.empty(2 * nsamp, np.uint8)
    raw[0::2] = np.clip(np.round(127.5 + sig.real + rng.normal(0, 10, nsamp)), 0, 255).astype(np.uint8)
    raw[1::2] = np.clip(np.round(127.5 + sig.imag + rng.normal(0, 10, nsamp)), 0, 255).astype(np.uint8)
    raw[:64] = 0            # int8 -128 negation case
    raw[64:128] = 255
    nbytes = (raw.size // 8) * 8
    L = ol.lib()
    st = L.orc_decim_new()
    oi = np.zeros(NS, np.float32); oq = np.zeros(NS, np.float32)
    fill = L.orc_decim_feed(C.c_void_p(st), ol.ptr(raw), nbytes, ol.ptr(oi), ol.ptr(oq), 0, NS)
    L.orc_decim_free(C.c_void_p(st))
    gi = np.zeros(NS, np.float32); gq = np.zeros(NS, np.float32)
    nout = C.c_uint32()
    assert w.lib().wspr_decimate_u8(ol.ptr(raw), nbytes, ol.ptr(gi), ol.ptr(gq), C.byref(nout), 0) == 0
    assert nout.value == fill == 300
    assert np.array_equal(gi[:fill], oi[:fill]) and np.array_equal(gq[:fill], oq[:fill])
    assert np.abs(gi[40:fill]).max() > 1e6       # in-band tone came through the CIC
    # with normalisation
    assert w.lib().wspr_decimate_u8(ol.ptr(raw), nbytes, ol.ptr(gi), ol.ptr(gq), C.byref(nout), 1) == 0
    L.orc_normalise(ol.ptr(oi), ol.ptr(oq), C.c_int(fill), C.c_int(NS))
    assert np.array_equal(gi, oi) and np.array_equal(gq, oq)


def test_decimator_block_edges_and_clipping_equal_oracle(w):
    """The whole-segment front end gives a wave one CIC block: interior vectors take the dot-product path, the
    two vectors that straddle the block's edges a masked one, and a block that holds a raw 0x00 byte (int8 -128,
    whose negation wraps) is redone sample by sample.  Zero bytes are planted on and around block edges (6401 is
    odd, so the edges fall on every position of a 16-byte vector), inside blocks, and one stretch is driven into
    hard clipping; every output equals the oracle's."""
    rng = np.random.default_rng(12)
    nblk = 70
    nsamp = 6401 * nblk + 3000
    raw = _raw_stream(rng, nsamp, f0=-35.0, amp=8.0)
    for b in (1, 2, 3, 9, 10, 17, 33, 34, 35, 64):               # around edge b: one zero byte each, I or Q rail
        k = 6401 * b + int(rng.integers(-9, 10))
        raw[2 * k + int(rng.integers(0, 2))] = 0
    raw[2 * (6401 * 20 + 3000)] = 0                                # deep inside a block
    lo, hi = 2 * 6401 * 40, 2 * 6401 * 43                         # three blocks of hard clipping (many 0x00 and 0xff)
    n = np.arange((hi - lo) // 2)
    clip = 127.5 + 400.0 * np.cos(2 * np.pi * (-600000.0 + 20.0) / 2.4e6 * n)
    raw[lo:hi:2] = np.clip(np.round(clip), 0, 255).astype(np.uint8)
    nbytes = (raw.size // 16) * 16
    L = ol.lib()
    st = L.orc_decim_new()
    oi = np.zeros(NS, np.float32); oq = np.zeros(NS, np.float32)
    fill = L.orc_decim_feed(C.c_void_p(st), ol.ptr(raw), nbytes, ol.ptr(oi), ol.ptr(oq), 0, NS)
    L.orc_decim_free(C.c_void_p(st))
    gi = np.zeros(NS, np.float32); gq = np.zeros(NS, np.float32)
    nout = C.c_uint32()
    assert w.lib().wspr_decimate_u8(ol.ptr(raw), nbytes, ol.ptr(gi), ol.ptr(gq), C.byref(nout), 0) == 0
    assert nout.value == fill == nblk
    assert np.array_equal(gi[:fill], oi[:fill]) and np.array_equal(gq[:fill], oq[:fill])
    # the same rows without any zero byte: the dot-product and masked paths alone
    raw2 = np.maximum(raw, 1)
    st = L.orc_decim_new()
    fill = L.orc_decim_feed(C.c_void_p(st), ol.ptr(raw2), nbytes, ol.ptr(oi), ol.ptr(oq), 0, NS)
    L.orc_decim_free(C.c_void_p(st))
    assert w.lib().wspr_decimate_u8(ol.ptr(raw2), nbytes, ol.ptr(gi), ol.ptr(gq), C.byref(nout), 0) == 0
    assert nout.value == fill == nblk
    assert np.array_equal(gi[:fill], oi[:fill]) and np.array_equal(gq[:fill], oq[:fill])


def _raw_stream(rng, nsamp, f0=40.0, amp=6.0):
    n = np.arange(nsamp)
    ph = 2 * np.pi * (-600000.0 + f0) / 2.4e6 * n
    sig = amp * np.exp(1j * ph)
    raw = np.empty(2 * nsamp, np.uint8)
    raw[0::2] = np.clip(np.round(127.5 + sig.real + rng.normal(0, 10, nsamp)), 0, 255).astype(np.uint8)
    raw[1::2] = np.clip(np.round(127.5 + sig.imag + rng.normal(0, 10, nsamp)), 0, 255).astype(np.uint8)
    return raw


class _DecimState(C.Structure):
    _fields_ = [("phase", C.c_uint32), ("x1", C.c_uint32 * 2), ("x2", C.c_uint32 * 2), ("hist", (C.c_uint32 * 36) * 2)]


def test_streaming_decimator_any_chunking_equals_oracle(w):
    """The reference's decimator state is static (rtlsdr_wsprd.c:135-160): it streams across callbacks.
    Chunks of 65536 bytes (the librtlsdr callback), of 16 bytes, shorter than one decimation block,
    and random sizes must all give the oracle's streamed outputs bit for bit, including clipped bytes
    (0x00 / 0xff) and a capacity that cuts the outputs off."""
    rng = np.random.default_rng(21)
    nsamp = 6401 * 90 + 3206                                 # a multiple of 8 samples
    raw = _raw_stream(rng, nsamp)
    raw[1000:1256] = 0                                       # int8 -128 negation case
    raw[70000:70512] = 255
    nbytes = raw.size
    assert nbytes % 16 == 0
    L = ol.lib()
    GL = w.lib()
    GL.wspr_decimate_u8_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32,
                                           C.c_uint32, C.c_void_p]

    def chunkings():
        yield "callback", [65536] * (nbytes // 65536) + ([nbytes % 65536] if nbytes % 65536 else [])
        yield "one", [nbytes]
        sizes, left = [], nbytes
        while left:
            c = min(left, 16 * int(rng.integers(1, 3000)))
            sizes.append(c); left -= c
        yield "random", sizes
        yield "tiny-then-rest", [16] * 40 + [6400 * 2 - 640] + [nbytes - 640 - (6400 * 2 - 640)]

    for cap in (NS, 57):
        for name, sizes in chunkings():
            assert sum(sizes) == nbytes and all(c % 16 == 0 for c in sizes)
            # the oracle is fed the same chunks: the mixer phase restarts with every call in both
            st = L.orc_decim_new()
            oi = np.zeros(NS, np.float32); oq = np.zeros(NS, np.float32)
            gi = np.zeros(NS, np.float32); gq = np.zeros(NS, np.float32)
            gs = _DecimState()
            GL.wspr_decim_stream_reset(C.byref(gs))
            fill = 0; gfill = C.c_uint32(0); pos = 0
            for c in sizes:
                chunk = np.ascontiguousarray(raw[pos:pos + c])
                fill = L.orc_decim_feed(C.c_void_p(st), ol.ptr(chunk), c, ol.ptr(oi), ol.ptr(oq), fill, cap)
                assert GL.wspr_decimate_u8_stream(C.byref(gs), ol.ptr(chunk), c, ol.ptr(gi), ol.ptr(gq), gfill.value, cap,
                                                  C.byref(gfill)) == 0
                pos += c
                assert gfill.value == fill, (name, pos)
            L.orc_decim_free(C.c_void_p(st))
            assert fill == min(cap, 90), (name, fill)
            assert np.array_equal(gi, oi) and np.array_equal(gq, oq), name
            assert gs.phase == nsamp % 6401


# ------------------------------------------------------------------ message types 2 / 3, hash memory
def _multi_segment(msgs, seed, snr=-8.0):
    rng = np.random.default_rng(seed)
    sigma = np.sqrt((375.0 / 2500.0) / 2.0)
    I = rng.normal(0, sigma, NS); Q = rng.normal(0, sigma, NS)
    for k, m in enumerate(msgs):
        si, sq = synth.tone_signal(symf(m), -80.0 + 40.0 * k, 2.0 + 0.1 * k, 10.0 ** ((snr - 2.0 * k) / 20.0))
        I += si; Q += sq
    return synth.normalise(I.astype(np.float32), Q.astype(np.float32))


def test_type2_type3_messages_equal_oracle(w):
    """Compound callsign (type 2) and hashed callsign + 6-char grid (type 3): the type-3 spot resolves
    <...> only because the stronger type-2 decode of the same call filled the hash memory first."""
    I, Q = _multi_segment(["PJ4/K1ABC 37", "<PJ4/K1ABC> FK52UD 37", "K1ABC/7 30", "W1AW FN31 10"], 31)
    spots, _, _ = w.wspr_decode(I, Q, NS)
    ref, _, _ = ol.decode(I, Q, NS)
    assert [_spot_tuple(x) for x in spots] == [_spot_tuple(x) for x in ref]
    msgs = [x.message.decode() for x in spots]
    assert "PJ4/K1ABC 37" in msgs and "<PJ4/K1ABC> FK52UD 37" in msgs and "W1AW FN31 10" in msgs


def test_hashtable_persistence_single_segment(w, tmp_path):
    """usehashtable = 1 (reference -H): hashtable.txt written by one call resolves a later type-3."""
    cwd = os.getcwd()
    try:
        for which, d in (("gpu", tmp_path / "g"), ("cpu", tmp_path / "c")):
            d.mkdir()
            os.chdir(d)
            I1, Q1 = _multi_segment(["PJ4/K1ABC 37"], 41)
            I2, Q2 = _multi_segment(["<PJ4/K1ABC> FK52UD 37"], 42)
            outs = []
            for (I, Q) in ((I1, Q1), (I2, Q2)):
                if which == "gpu":
                    sp, _, _ = w.wspr_decode(I, Q, NS, _opt(w, 1))
                else:
                    sp, _, _ = ol.decode(I, Q, NS, _oopt(1))
                outs.append([x.message.decode() for x in sp])
            assert outs[0] == ["PJ4/K1ABC 37"] and outs[1] == ["<PJ4/K1ABC> FK52UD 37"], (which, outs)
            txt = open("hashtable.txt").read()
            assert "PJ4/K1ABC" in txt
            if which == "gpu":
                gpu_txt = txt
            else:
                assert txt == gpu_txt
    finally:
        os.chdir(cwd)


def _opt(w, use):
    o = w.default_options()
    o.usehashtable = use
    return o


def _oopt(use):
    o = ol.default_options()
    o.usehashtable = use
    return o


# ------------------------------------------------------------------ K6 device Fano
def test_wave_fano_equals_host_fano(w):
    """K6w (fano_wave.h): one wavefront per vector, 64 tree visits per step.  Return code, cycle count
    and decoded bytes equal those of the REAL reference fano() (fano.c:87-238, compiled where it lies into
    oracle/_ref/libwsprd_ref.so; the oracle's restatement where that file did not travel) with the branch metrics the
    oracle derives as wsprd.c:467-473 does -- for decodable vectors, early time-outs and full 810 000-cycle time-outs;
    metric/maxnp for decoded frames.  The product's own host routine must say the same (round 4 compared only those two:
    HIP against product)."""
    import time
    L = w.lib()
    O = ol.lib()
    R = ol.ref_lib()
    rng = np.random.default_rng(18)
    mt_prod = (C.c_int * 256 * 2)(); L.wspr_fano_metric_table(mt_prod)
    mt = (C.c_int * 256 * 2)(); O.orc_build_mettab(mt)
    assert list(np.frombuffer(mt, np.int32)) == list(np.frombuffer(mt_prod, np.int32))
    if R is not None:
        checker, deint, enc_fn, inter = R.fano, R.deinterleave, R.encode, R.interleave     # the reference's own objects
        print("wave fano: checked against oracle/_ref/libwsprd_ref.so (the reference's fano.c)")
    else:
        O.orc_fano.restype = C.c_int
        checker, deint, enc_fn, inter = O.orc_fano, O.orc_deinterleave, O.orc_conv_encode, O.orc_interleave
        print("wave fano: oracle/_ref absent, checked against oracle/liboracle.so")
    enc = (C.c_ubyte * 176)()
    vecs = []
    for t in range(360):
        data = [int(x) for x in rng.integers(0, 256, 7)] + [0, 0, 0, 0]
        data[6] &= 0xC0
        enc_fn(enc, (C.c_ubyte * 11)(*data), C.c_uint(11))
        bits = (C.c_ubyte * 162)(*list(enc)[:162])
        inter(bits)                                          # transmission order, as the demodulator emits
        sigma = [5, 25, 40, 50, 55, 60, 65, 75, 100, 150, 400, 1000][t % 12]
        vecs.append(np.clip(np.where(np.frombuffer(bits, np.uint8) > 0, 178, 78) + rng.normal(0, sigma, 162), 0, 255).astype(np.uint8))
    vecs += [np.full(162, 128, np.uint8), np.zeros(162, np.uint8), np.full(162, 255, np.uint8),
             np.tile(np.array([0, 255], np.uint8), 81)]
    sym = np.stack(vecs)
    L.wspr_fano_batch_device_wave.argtypes = [C.c_void_p, C.c_int, C.c_uint] + [C.c_void_p] * 6
    for maxcycles in (50, 200, 1500, 10000):
        n = sym.shape[0]
        ret = np.zeros(n, np.int32); cyc = np.zeros(n, np.uint32); met = np.zeros(n, np.uint32); mnp = np.zeros(n, np.uint32)
        dat = np.zeros((n, 10), np.uint8); steps = np.zeros(n, np.uint32)
        t0 = time.time()
        assert L.wspr_fano_batch_device_wave(ol.ptr(sym), n, maxcycles, ol.ptr(ret), ol.ptr(cyc), ol.ptr(met), ol.ptr(mnp),
                                             ol.ptr(dat), ol.ptr(steps)) == 0
        dt = time.time() - t0
        nto = 0
        for i in range(n):
            s = (C.c_ubyte * 162)(*sym[i].tolist())
            deint(s)
            dec = (C.c_ubyte * 11)(); a = C.c_uint(); b = C.c_uint(); c = C.c_uint()
            r = checker(C.byref(a), C.byref(b), C.byref(c), dec, s, C.c_uint(81), mt, C.c_int(60), C.c_uint(maxcycles))
            assert (ret[i], cyc[i]) == (r, b.value), (i, maxcycles, ret[i], cyc[i], r, b.value)
            if r == 0:
                assert (met[i], mnp[i]) == (a.value, c.value) and list(dat[i]) == list(dec)[:10], (i, maxcycles)
            # ... and the product's host routine (wspr_message.cpp) agrees with the same checker
            s2 = (C.c_ubyte * 162)(*sym[i].tolist())
            L.deinterleave(s2)
            dec2 = (C.c_ubyte * 11)(); a2 = C.c_uint(); b2 = C.c_uint(); c2 = C.c_uint()
            r2 = L.fano(C.byref(a2), C.byref(b2), C.byref(c2), dec2, s2, C.c_uint(81), mt_prod, C.c_int(60), C.c_uint(maxcycles))
            assert (r2, b2.value) == (r, b.value) and (r != 0 or (a2.value, c2.value, list(dec2)) == (a.value, c.value, list(dec))), (i, maxcycles)
            nto += r != 0
        print("wave fano: maxcycles %d, %d vectors, %d time-outs, %.1f ms, steps max %d mean %.0f" % (
            maxcycles, n, nto, dt * 1e3, steps.max(), steps.mean()))
        assert 20 < nto < n - 20


def test_wave_fano_with_a_small_stack_in_a_subprocess():
    """K6w with a stack of 1 024 visits (test hook WSPR_FANO_WAVE_CAP, read once per process): the same vectors and the
    same assertions as test_wave_fano_equals_host_fano, now through the narrowed steps and the LDS window's spills and
    fills at those widths.  None of these vectors overflows that stack (the largest holds 777 visits; only one reaches the
    1-wide step, at the full budget): the overflow exit and the host routine behind it are not met here but in
    tests/test_gpu_fano_wave.py, with a stack of 96."""
    import subprocess
    import sys
    env = dict(os.environ, WSPR_FANO_WAVE_CAP="1024", WSPR_USE_LAB="1")      # the switch exists in the lab build only
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "test_wave_fano_equals_host_fano"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:]


def test_wave_fano_many_time_outs_throughput(w):
    """The crowded-band tail: thousands of undecodable vectors, full budget.  All time out exactly like
    the host routine says (sampled), in tens of milliseconds instead of ~5 ms of a CPU core each."""
    import time
    L = w.lib()
    rng = np.random.default_rng(99)
    n = 6000
    sym = np.clip(rng.normal(128, 45, (n, 162)), 0, 255).astype(np.uint8)
    L.wspr_fano_batch_device_wave.argtypes = [C.c_void_p, C.c_int, C.c_uint] + [C.c_void_p] * 6
    ret = np.zeros(n, np.int32); cyc = np.zeros(n, np.uint32); met = np.zeros(n, np.uint32); mnp = np.zeros(n, np.uint32)
    dat = np.zeros((n, 10), np.uint8); steps = np.zeros(n, np.uint32)
    for rep in range(2):
        t0 = time.time()
        assert L.wspr_fano_batch_device_wave(ol.ptr(sym), n, 10000, ol.ptr(ret), ol.ptr(cyc), ol.ptr(met), ol.ptr(mnp),
                                             ol.ptr(dat), ol.ptr(steps)) == 0
        dt = time.time() - t0
    print("wave fano: %d noise vectors, full budget: %.1f ms (%d time-outs), steps mean %.0f max %d" % (
        n, dt * 1e3, int((ret == -1).sum()), steps.mean(), steps.max()))
    assert (ret != -2).all()
    mt = (C.c_int * 256 * 2)(); L.wspr_fano_metric_table(mt)
    for i in range(0, n, 500):
        s = (C.c_ubyte * 162)(*sym[i].tolist())
        L.deinterleave(s)
        dec = (C.c_ubyte * 11)(); a = C.c_uint(); b = C.c_uint(); c = C.c_uint()
        r = L.fano(C.byref(a), C.byref(b), C.byref(c), dec, s, C.c_uint(81), mt, C.c_int(60), C.c_uint(10000))
        assert (ret[i], cyc[i]) == (r, b.value)
    assert dt < 1.0


def test_short_result_array_keeps_the_strongest_spots(w):
    """A caller with room for fewer spots than the segment holds gets the strongest ones of the WHOLE ranked
    list (wsprd.c:827), including signals that only decode in the second pass after subtraction."""
    I, Q, truth = synth.make_segment(501, symf, n_signals=8, snr_db=-6.0, snr_span=18.0, t_jitter=0.3)
    ref, _, _ = ol.decode(I, Q, NS)
    assert len(ref) >= 6
    full = w.wspr_decode_batch(I[None], Q[None], w.default_options())[0]
    assert [_spot_tuple(x) for x in full] == [_spot_tuple(x) for x in ref]
    for k in (1, 3, 5):
        got = w.wspr_decode_batch(I[None], Q[None], w.default_options(), max_results=k)[0]
        assert [_spot_tuple(x) for x in got] == [_spot_tuple(x) for x in ref[:k]], k


def test_decode_after_set_device(w, ref_iq):
    L = w.lib()
    L.wspr_device_count.restype = C.c_int
    assert L.wspr_device_count() >= 1 and L.wspr_set_device(0) == 0
    spots, _, _ = w.wspr_decode(ref_iq[0], ref_iq[1], NS)
    assert [s.message for s in spots] == [b"K1JT FN20 20"]
    assert L.wspr_set_device(L.wspr_device_count()) == -1


def test_hashtable_option_on_a_batch_decodes_in_order(w, tmp_path):
    """usehashtable = 1 on a batch: segments are decoded one by one in index order, each like a reference call
    (hashtable.txt read before, written after, wsprd.c:481-494, 842-852).  Segment 0 carries the compound call
    (type 2), segments 1 and 2 only its hashed form (type 3): they resolve <...> because of segment 0.
    Same spots and same hashtable.txt as the oracle called three times, and as three single product calls."""
    segs = [_multi_segment(["PJ4/K1ABC 37"], 51), _multi_segment(["<PJ4/K1ABC> FK52UD 37", "W1AW FN31 10"], 52),
            _multi_segment(["<PJ4/K1ABC> FK52UD 37"], 53)]
    I = np.stack([s[0] for s in segs]); Q = np.stack([s[1] for s in segs])
    cwd = os.getcwd()
    res = {}
    try:
        for mode in ("batch", "singles", "oracle"):
            d = tmp_path / mode
            d.mkdir()
            os.chdir(d)
            if mode == "batch":
                got = w.wspr_decode_batch(I, Q, _opt(w, 1))
                res[mode] = [[_spot_tuple(x) for x in g] for g in got]
            elif mode == "singles":
                res[mode] = [[_spot_tuple(x) for x in w.wspr_decode(I[s], Q[s], NS, _opt(w, 1))[0]] for s in range(3)]
            else:
                res[mode] = [[_spot_tuple(x) for x in ol.decode(I[s], Q[s], NS, _oopt(1))[0]] for s in range(3)]
            res[mode + "_file"] = open("hashtable.txt").read()
    finally:
        os.chdir(cwd)
    assert res["batch"] == res["singles"] == res["oracle"]
    assert res["batch_file"] == res["singles_file"] == res["oracle_file"] and "PJ4/K1ABC" in res["batch_file"]
    assert [m[0] for m in res["batch"][2]] == [b"<PJ4/K1ABC> FK52UD 37"]
    # without the option the hashed call cannot be resolved in a fresh batch
    plain = w.wspr_decode_batch(I, Q, _opt(w, 0))
    assert [x.message for x in plain[2]] != [b"<PJ4/K1ABC> FK52UD 37"]


# ------------------------------------------------------------------ node-level call
def _node(w, I, Q, ndev, max_results=16, lab=False):
    nseg = I.shape[0]
    out = (w.decoder_results * (nseg * max_results))()
    nres = (C.c_int * nseg)()
    rc = (w.lab() if lab else w.lib()).wspr_decode_batch_node(ol.ptr(I), ol.ptr(Q), nseg, NS, NS, w.default_options(), C.addressof(out),
                                        max_results, C.addressof(nres), ndev)
    return rc, [[_spot_tuple(out[s * max_results + i]) for i in range(nres[s])] for s in range(nseg)]


def test_node_level_call_equals_one_device_batch(w, synth_batch, monkeypatch):
    """wspr_decode_batch_node(): contiguous blocks over the node's devices, one host thread each.  On this 1-GPU box:
    all devices (= 1), and -- with the test hook WSPR_NODE_VIRTUAL -- three blocks of 3/3/2 segments decoded
    concurrently on three lanes of the one device.  Same spots as one wspr_decode_batch(); asking for devices that
    do not exist is an error."""
    I, Q, _ = synth_batch
    L = w.lib()
    L.wspr_decode_batch_node.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, w.decoder_options,
                                         C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    want = [[_spot_tuple(x) for x in seg] for seg in w.wspr_decode_batch(I, Q, w.default_options(), max_results=16)]
    rc, got = _node(w, I, Q, 0)
    assert rc == 0 and got == want
    ndev = L.wspr_device_count()
    rc, got = _node(w, I, Q, ndev + 2)
    assert rc == -1 and all(len(g) == 0 for g in got)
    # the test hook lives in the lab build only: the product refuses more shards than devices whatever the environment says
    monkeypatch.setenv("WSPR_NODE_VIRTUAL", "1")
    rc, got = _node(w, I, Q, 3 * ndev)
    assert rc == -1
    L = w.lab()
    L.wspr_decode_batch_node.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, w.decoder_options,
                                         C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    rc, got = _node(w, I, Q, 3 * ndev, lab=True)
    assert rc == 0 and got == want
    lo, hi = C.c_int(), C.c_int()
    L.wspr_shard_range(8, 1, 3, C.byref(lo), C.byref(hi))
    assert (lo.value, hi.value) == (3, 6)
    # ... and the same with the IQ resident on device 0 (blocks reach the other devices by peer copies)
    import torch
    torch.cuda.set_device(0)
    dI = torch.from_numpy(I).cuda(); dQ = torch.from_numpy(Q).cuda()
    w.sync_torch()
    L.wspr_decode_batch_node_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, w.decoder_options,
                                                C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    nseg = I.shape[0]
    for nd in (1, 3 * ndev):
        out = (w.decoder_results * (nseg * 16))(); nres = (C.c_int * nseg)()
        assert L.wspr_decode_batch_node_device(dI.data_ptr(), dQ.data_ptr(), 0, nseg, NS, NS, w.default_options(),
                                               C.addressof(out), 16, C.addressof(nres), nd) == 0
        assert [[_spot_tuple(out[s * 16 + i]) for i in range(nres[s])] for s in range(nseg)] == want
    out = (w.decoder_results * (nseg * 16))(); nres = (C.c_int * nseg)()
    assert L.wspr_decode_batch_node_device(dI.data_ptr(), dQ.data_ptr(), ndev + 3, nseg, NS, NS, w.default_options(),
                                           C.addressof(out), 16, C.addressof(nres), 0) == -1
    # more devices than are visible (without the test hook's virtual devices): the documented -1, no spots
    monkeypatch.delenv("WSPR_NODE_VIRTUAL")
    nres = (C.c_int * nseg)(*([7] * nseg))
    assert L.wspr_decode_batch_node_device(dI.data_ptr(), dQ.data_ptr(), 0, nseg, NS, NS, w.default_options(),
                                           C.addressof(out), 16, C.addressof(nres), ndev + 1) == -1 and not any(nres)
    monkeypatch.setenv("WSPR_NODE_VIRTUAL", "1")
    # every peer copy reports failure (fault injection of the lab build): the blocks travel through pinned host memory
    # instead and the spots are the same
    monkeypatch.setenv("WSPR_NODE_FAIL_PEER", "1")
    out = (w.decoder_results * (nseg * 16))(); nres = (C.c_int * nseg)()
    assert L.wspr_decode_batch_node_device(dI.data_ptr(), dQ.data_ptr(), 0, nseg, NS, NS, w.default_options(),
                                           C.addressof(out), 16, C.addressof(nres), 3 * ndev) == 0
    assert [[_spot_tuple(out[s * 16 + i]) for i in range(nres[s])] for s in range(nseg)] == want
    monkeypatch.delenv("WSPR_NODE_FAIL_PEER")
    # one shard fails: the WHOLE call fails and reports no spots (include/wspr_mi355x.h), the inputs are untouched and the
    # call can be repeated
    monkeypatch.setenv("WSPR_NODE_FAIL_SHARD", "1")
    nres = (C.c_int * nseg)(*([7] * nseg))
    assert L.wspr_decode_batch_node_device(dI.data_ptr(), dQ.data_ptr(), 0, nseg, NS, NS, w.default_options(),
                                           C.addressof(out), 16, C.addressof(nres), 3 * ndev) < 0 and not any(nres)
    monkeypatch.delenv("WSPR_NODE_FAIL_SHARD")
    assert torch.equal(dI.cpu(), torch.from_numpy(I)) and torch.equal(dQ.cpu(), torch.from_numpy(Q))
    out = (w.decoder_results * (nseg * 16))(); nres = (C.c_int * nseg)()
    assert L.wspr_decode_batch_node_device(dI.data_ptr(), dQ.data_ptr(), 0, nseg, NS, NS, w.default_options(),
                                           C.addressof(out), 16, C.addressof(nres), 3 * ndev) == 0
    assert [[_spot_tuple(out[s * 16 + i]) for i in range(nres[s])] for s in range(nseg)] == want
