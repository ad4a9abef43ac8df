"""The block-detection checker (tests/helpers/block_check.c) and the stage's rule over it (tests/block_lib.py walk()),
without a GPU.

At block size 1 the definition is sync_and_demodulate() mode 2, so the checker is pinned there to the CPU oracle (exact
build), to the contracted checker (CONTRACT=1) and, where oracle/_ref is built, to the compiled reference.  Block sizes 2
and 3 have no reference: they are held to a float64 numpy statement written here from the definition
(rtlsdr-wsprd_amd/csrc/kernels/blockdemod.h).  The walk over the 24 weak scenes is pinned to what the checker gives."""
import ctypes as C

import numpy as np
import pytest

import block_lib as bl
import contract_lib as cl
import oracle_lib as ol
import synth

NS = 45000


def symf(msg):
    ok, s = ol.channel_symbols(msg)
    assert ok
    return s


def _mode(fn, I, Q, freq, shift, drift, mode, lagmin=0, lagmax=0, lagstep=8, ifmin=0, ifmax=0, fstep=0.0, np_=NS):
    """sync_and_demodulate() as fn states it: (freq, shift, sync, symbols)."""
    Ic, Qc = I.copy(), Q.copy()
    f = C.c_float(freq); sh = C.c_int(shift); dr = C.c_float(drift); sy = C.c_float(0)
    sym = (C.c_ubyte * 162)()
    fn(ol.ptr(Ic), ol.ptr(Qc), C.c_long(np_), sym, C.addressof(f), ifmin, ifmax, C.c_float(fstep), C.addressof(sh), lagmin,
       lagmax, lagstep, C.addressof(dr), 50, C.addressof(sy), mode)
    return f.value, sh.value, np.float32(sy.value), bytes(sym)


@pytest.fixture(scope="module")
def mode2_inputs():
    """The mode-2 hypotheses of tests/test_gpu_parity.py's sync_and_demodulate tests: (I, Q, np, freq, shift, drift)."""
    segs = [synth.make_segment(1000 + s, symf, snr_db=-20.0) for s in range(6)]
    segs.append(synth.make_segment(77, symf, n_signals=4, snr_db=-8.0, snr_span=12.0, t_jitter=0.3))
    segs.append(synth.make_segment(78, symf, snr_db=-15.0, drift=2.0))
    fn = ol.lib().orc_sync_demod
    out = []
    for seg, drift in [(0, 0.0), (3, 0.0), (7, 2.0), (7, -4.0), (6, 1.0)]:
        I, Q, truth = segs[seg]
        msg, f0, t0, snr = truth[0]
        fc = float(np.float32(round(f0 / 0.732421875) * 0.732421875))
        sc = int(round(t0 * 375 / 128.0)) * 128
        shift = _mode(fn, I, Q, fc, sc, drift, 0, lagmin=sc - 128, lagmax=sc + 128, lagstep=8)[1]
        fbest = _mode(fn, I, Q, fc, shift, drift, 1, ifmin=-2, ifmax=2, fstep=0.1)[0]
        out += [(I, Q, NS, fbest, shift + jig, drift) for jig in (0, -3, 3, 63, -63)]
    I, Q, _ = segs[0]
    out += [(I, Q, NS, 10.0, shift, 0.0) for shift in (-1400, -300, 3700, 4100)]       # hanging over both ends
    out.append((I, Q, 44000, 10.0, 700, 0.0))
    I, Q, truth = segs[1]
    out.append((I, Q, NS, float(np.float32(truth[0][1])), int(round(truth[0][2] * 375)), 0.0))
    return out


@pytest.mark.parametrize("flag", [0, 1])
def test_block_size_1_is_mode_2(mode2_inputs, flag):
    """The CONTRACT=0 checker's B = 1 vector and sync equal orc_sync_demod(mode 2) bit for bit, the CONTRACT=1 checker's
    the contracted checker's; where oracle/_ref exists both equal the compiled reference (gcc build, clang-fma build)."""
    states = [ol.lib().orc_sync_demod if flag == 0 else cl.contract(1).ctr_sync_demod]
    ref = ol.ref_dsp_lib() if flag == 0 else ol.ref_dsp_fma_lib()
    if ref is not None:
        states.append(ref.sync_and_demodulate)
    for I, Q, np_, freq, shift, drift in mode2_inputs:
        sym, rms, sync = bl.demod(flag, I, Q, np_, freq, shift, drift)
        for fn in states:
            _, _, want_sync, want_sym = _mode(fn, I, Q, freq, shift, drift, 2, np_=np_)
            assert bytes(sym[0]) == want_sym, (freq, shift, drift)
            assert sync.tobytes() == want_sync.tobytes(), (freq, shift, drift)
        y = sym[0].astype(np.float32) - np.float32(128)
        assert rms[0] == np.sqrt(np.float32((y * y).sum()) / np.float32(162))


def numpy_block(I, Q, np_, freq, shift, drift):
    """The definition in float64: uint8 [3, 162].  The tone sums as one complex product per (symbol, tone) with the exact
    phasors exp(-i dphi j) of the float32 phase steps, the advance exp(i 256 dphi), the combine as complex arithmetic."""
    pr3 = np.array(list((C.c_ubyte * 162).in_dll(ol.lib(), "orc_sync_vector")), np.int64)
    i = np.arange(162)
    fp = (np.float64(np.float32(freq)) + (np.float64(np.float32(drift)) / 2.0) * (i - 81.0) / 81.0).astype(np.float32)
    off = np.array([-1.5, -0.5, 0.5, 1.5]) * 375.0 / 256.0
    dphi = (2.0 * np.pi / 375.0 * (fp.astype(np.float64)[:, None] + off[None, :])).astype(np.float32).astype(np.float64)
    k = shift + 256 * i[:, None] + np.arange(256)[None, :]
    ok = (k > 0) & (k < np_)
    z = np.zeros((162, 256), np.complex128)
    z[ok] = I.astype(np.float64)[k[ok]] + 1j * Q.astype(np.float64)[k[ok]]
    j = np.arange(256)
    S = np.einsum("ij,itj->it", z, np.exp(-1j * dphi[:, :, None] * j[None, None, :]))      # is + i qs
    A = np.exp(1j * dphi * 256.0)                                                          # cf + i sf
    out = np.zeros((3, 162), np.uint8)
    for B in (1, 2, 3):
        f = np.zeros(162)
        for i0 in range(0, 162, B):
            p = np.zeros(1 << B)
            for seq in range(1 << B):
                X, M = 0j, 1 + 0j
                for ib in range(B):
                    t = pr3[i0 + ib] + 2 * ((seq >> (B - 1 - ib)) & 1)
                    X += S[i0 + ib, t] * np.conj(M)
                    M *= A[i0 + ib, t]
                p[seq] = abs(X)
            for ib in range(B):
                bit = (np.arange(1 << B) >> (B - 1 - ib)) & 1
                f[i0 + ib] = max(0.0, p[bit == 1].max()) - max(0.0, p[bit == 0].max())
        fac = np.sqrt((f * f).mean() - f.mean() ** 2)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = np.clip(50.0 * f / fac, -128.0, 127.0) + 128.0
        out[B - 1] = np.where(np.isnan(v), 0, np.trunc(np.nan_to_num(v))).astype(np.uint8)
    return out


def test_numpy_statement_on_zeros_and_sync_vector():
    z = np.zeros(NS, np.float32)
    assert not numpy_block(z, z, NS, 0.0, 0, 0.0).any()
    sym, rms, sync = bl.demod(0, z, z, NS, 0.0, 0, 0.0)
    assert not sym.any() and sync == np.float32(-1e30)


def test_checker_against_float64_numpy():
    """Every byte for B = 1, 2, 3 within one count of the float64 statement, on the candidates the oracle visits in seeds
    5000..5007 at -30 dB and in two -15 dB scenes with drift +-2 Hz.  The float32 sums are off by ~1e-5 of an amplitude,
    far below one count, so only a truncation boundary can move a byte."""
    scenes = [bl.weak_scene(seed)[:2] for seed in range(5000, 5008)]
    scenes += [synth.make_segment(78 + k, symf, snr_db=-15.0, drift=d)[:2] for k, d in enumerate((2.0, -2.0))]
    ncand = ndiff = 0
    for I, Q in scenes:
        tr = ol.decode(I, Q, NS, ol.default_options(npasses=1, subtraction=0), trace=True)[3]
        for jc in range(tr.n_visited[0]):
            cf = tr.cand_fine[0][jc]
            want = numpy_block(I, Q, NS, cf.freq, cf.shift, cf.drift).astype(np.int64)
            for flag in (0, 1):
                got = bl.demod(flag, I, Q, NS, cf.freq, cf.shift, cf.drift)[0].astype(np.int64)
                d = np.abs(got - want)
                assert d.max() <= 1, (flag, cf.freq, cf.shift, cf.drift, int(d.max()))
                ndiff += int((d != 0).sum())
            ncand += 1
    print("block checker vs float64: %d candidates, %d of %d bytes differ by one" % (ncand, ndiff, ncand * 2 * 3 * 162))
    assert ncand >= 10


# seeds of 5000..5023 (one signal at -30 dB, one pass, no subtraction): what the oracle's plain ladder decodes, and what
# walk() over the float32 checker adds on the candidates it leaves undecoded (tools/block_rescue_seeds.py -30 5000 5024)
PLAIN = {5000, 5001, 5004, 5009, 5020, 5021}
RESCUED = {5003, 5005, 5006, 5007, 5008, 5010, 5015, 5016, 5019, 5022, 5023}


def test_walk_pinned_on_the_weak_scenes():
    """walk() over the oracle's undecoded worth candidates decodes the sent message in exactly the seeds of RESCUED, and no
    other message anywhere.  A float64 statement of the detector rescued 12 of the 18 segments Fano leaves; the float32 checker
    rescues these 11 (a marginal seed differs), and the checker is what the kernel is held to."""
    plain, rescued = set(), set()
    for seed in range(5000, 5024):
        I, Q, sent = bl.weak_scene(seed)
        spots, _, _, tr = ol.decode(I, Q, NS, ol.default_options(npasses=1, subtraction=0), trace=True)
        texts = [s.message.decode() for s in spots]
        assert all(t == sent for t in texts)
        if texts:
            plain.add(seed)
        for p, jc, freq, shift, drift in bl.undecoded_worth(tr):
            hit = bl.walk(0, I, Q, NS, freq, shift, drift)
            if hit:
                assert hit[0] in (2, 3) and hit[1] in bl.LADDER and hit[3] >= 81
                assert bl.unpack(hit[2]) == sent, (seed, jc, hit)
                if seed not in plain:
                    rescued.add(seed)
    assert plain == PLAIN
    assert rescued == RESCUED


def test_walk_on_noise_decodes_nothing():
    """The same generator at -60 dB is noise: neither the oracle nor the walk reports a message (three seeds here; the 24
    of the issue's table are tools/block_rescue_seeds.py -60 7000 7024)."""
    for seed in (7000, 7001, 7002):
        I, Q, _ = bl.weak_scene(seed, -60.0)
        spots, _, _, tr = ol.decode(I, Q, NS, ol.default_options(npasses=1, subtraction=0), trace=True)
        assert not spots
        for p, jc, freq, shift, drift in bl.undecoded_worth(tr):
            assert bl.walk(0, I, Q, NS, freq, shift, drift) is None


def test_switch_exists_defaults_to_off_and_refuses_other_values():
    import rtlsdr_wsprd_amd as w
    for L in (w.lib(), w.lab()):
        assert w.set_block_detection(1, L) == 1                      # the default
        assert [w.set_block_detection(v, L) for v in (0, 4, -1)] == [-2, -2, -2]
        assert w.set_block_detection(3, L) == 1 and w.set_block_detection(2, L) == 3 and w.set_block_detection(1, L) == 2
    assert w.cand_trace.block.offset == w.cand_trace.stop.offset + 1
    assert w.TIMING_NAMES[32:36] == ("block_ms", "block_vectors", "block2_decodes", "block3_decodes")


def test_block_demod_refuses_bad_arguments_without_a_device():
    """The argument checks come before the device is touched: -1 and nothing written (n == 0: 0, nothing to do)."""
    import rtlsdr_wsprd_amd as w
    L = w.lib()
    z = np.zeros((2, 1024), np.float32)
    sym = np.full((1, 3, 162), 7, np.uint8)
    item = lambda seg=0, freq=0.0, shift=0, drift=0.0: np.array([(seg, freq, shift, drift)], w.BLOCK_ITEM_DTYPE)
    call = lambda it, n=1, nseg=2, samples=1024: L.wspr_block_demod_batch(ol.ptr(z), ol.ptr(z), nseg, samples, 1024, ol.ptr(it),
                                                                          n, ol.ptr(sym))
    assert call(item(), n=0) == 0
    assert call(item(), n=-1) == -1
    assert call(item(seg=2)) == -1 and call(item(seg=-1)) == -1
    assert call(item(freq=np.nan)) == -1 and call(item(drift=np.inf)) == -1
    assert call(item(), samples=45001) == -1
    assert (sym == 7).all()
