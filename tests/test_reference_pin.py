"""The CPU checkers against the reference's own compiled code, without a GPU.

oracle/Makefile compiles the reference's wsprd.c where it lies, twice: with gcc for x86-64 (no fused multiply-add) and
with clang -ffp-contract=on -mfma.  The one thing substituted is the FFT: the oracle's orc_fft512 behind an <fftw3.h>
stand-in.  Here the exact oracle (oracle/orc_dsp.c) is held to the first build and the contracted checker
(tests/helpers/contract_dsp.c, CONTRACT=1) to the second: every spot field with ==, snr included, and the residual I and
Q bit for bit.  No tolerance anywhere.  The decimator oracle against the compiled callback is in
tests/test_reference_pin_frontend.py.

A test skips only when its library is absent (a checkout where the reference was never mounted) or, for the fused
build, when the CPU has no FMA."""
import ctypes as C
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import contract_lib as cl
import oracle_lib as ol
import payloads
import synth
import trace_parity
from test_gpu_parity import _multi_segment, _oracle_cands, crowded_scenes, random_scenes

NS = 45000
OPTION_SETS = [dict(), dict(quickmode=1), dict(subtraction=0), dict(npasses=1), dict(npasses=3)]
OPT_IDS = ["defaults", "quickmode=1", "subtraction=0", "npasses=1", "npasses=3"]
FIELDS = ("freq", "sync", "snr", "dt", "drift", "jitter", "message", "call", "loc", "pwr", "cycles")


class Side:
    """One checker and the compiled reference that pins it."""

    def __init__(self, mode):
        self.mode = mode
        if mode == "exact":
            self.ref = ol.ref_dsp_lib()
            if self.ref is None:
                pytest.skip("oracle/_ref/libwsprd_dsp_ref.so is not built (the reference is not mounted)")
            self.demod, self.subtract2 = ol.lib().orc_sync_demod, ol.lib().orc_subtract
        else:
            if not os.path.exists(os.path.join(ol.ORACLE_DIR, "_ref", "libwsprd_dsp_ref_fma.so")):
                pytest.skip("oracle/_ref/libwsprd_dsp_ref_fma.so is not built (no reference mounted, or no clang)")
            self.ref = ol.ref_dsp_fma_lib()
            if self.ref is None:
                pytest.skip("this CPU has no FMA instructions")
            self.demod, self.subtract2 = cl.contract(1).ctr_sync_demod, cl.contract(1).ctr_subtract

    def decode(self, I, Q, n=NS, opt=None, trace=False):
        if self.mode == "exact":
            return ol.decode(I, Q, n, opt, trace=trace)
        return cl.decode(1, I, Q, n, opt, trace=trace)

    def fft_bank(self, I, Q, n=NS):
        return cl.fft_bank(0 if self.mode == "exact" else 1, I, Q, n)


@pytest.fixture(scope="module", params=["exact", "fma"])
def side(request):
    return Side(request.param)


@pytest.fixture(scope="module")
def exact():
    return Side("exact")


def fields(s):
    return tuple(getattr(s, k) for k in FIELDS)


def same(ref_out, chk_out, where):
    """(spots, residual I, residual Q) of the compiled reference and of the checker."""
    rs, ri, rq = ref_out[:3]
    cs, ci, cq = chk_out[:3]
    assert [fields(s) for s in cs] == [fields(s) for s in rs], where
    assert ci.tobytes() == ri.tobytes() and cq.tobytes() == rq.tobytes(), where


def differs(a, b):
    return [fields(s) for s in a[0]] != [fields(s) for s in b[0]] or a[1].tobytes() != b[1].tobytes() \
        or a[2].tobytes() != b[2].tobytes()


def check_all(side, I, Q, opts=None, n=NS, trace=False, where=""):
    """Every row of I/Q through both; returns the checker's outputs.  The checker runs on a thread pool, the reference
    (not re-entrant) one call at a time."""
    opts = opts or {}
    side.decode(I[0], Q[0], n, ol.default_options(**opts))       # static tables initialised before the threads start
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        chk = list(pool.map(lambda s: side.decode(I[s], Q[s], n, ol.default_options(**opts), trace=trace),
                            range(len(I))))
    for s in range(len(I)):
        same(side.ref.decode(I[s], Q[s], n, ol.default_options(**opts)), chk[s], (side.mode, where, opts, s))
    return chk


@functools.lru_cache(maxsize=None)
def parity_segments():
    """The parity batch of tests/trace_parity.py with what was sent in it."""
    symf = lambda m: ol.channel_symbols(m)[1]
    segs = [synth.make_segment(1000 + s, symf, snr_db=-20.0) for s in range(6)]
    segs.append(synth.make_segment(77, symf, n_signals=4, snr_db=-8.0, snr_span=12.0, t_jitter=0.3))
    segs.append(synth.make_segment(78, symf, snr_db=-15.0, drift=2.0))
    return np.stack([s[0] for s in segs]), np.stack([s[1] for s in segs]), [s[2] for s in segs]


@functools.lru_cache(maxsize=None)
def ref_iq():
    I, Q, n = ol.read_iq_file(os.path.join(ol.GOLDEN, "refSignalSnr0dB.iq"))
    assert n == NS
    return I, Q


# ------------------------------------------------------------------------------------------------- whole decoder
@pytest.mark.parametrize("opts", OPTION_SETS, ids=OPT_IDS)
def test_reference_file_and_parity_batch(side, opts):
    I, Q = trace_parity.parity_batch()
    I0, Q0, _ = parity_segments()
    assert np.array_equal(I, I0) and np.array_equal(Q, Q0)
    I = np.concatenate([ref_iq()[0][None], I])
    Q = np.concatenate([ref_iq()[1][None], Q])
    chk = check_all(side, I, Q, opts, where="parity")
    assert [s.message for s in chk[0][0]] == [b"K1JT FN20 20"]
    assert sum(len(c[0]) for c in chk) >= 8


def test_random_scenes(side):
    """Random scenes of tests/test_gpu_parity.py (WSPR_PIN_SCENES of them, default 60).  The fused build must also
    differ from the exact oracle on at least half of them: a build that fuses nothing would otherwise pass."""
    n = int(os.environ.get("WSPR_PIN_SCENES", "60"))
    I, Q = random_scenes(n)
    chk = check_all(side, I, Q, where="random")
    total = sum(len(c[0]) for c in chk)
    print("random scenes:", n, "spots:", total)
    assert total > 100
    if side.mode == "fma":
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            orc = list(pool.map(lambda s: ol.decode(I[s], Q[s], NS), range(n)))
        moved = sum(differs(side.ref.decode(I[s], Q[s], NS), orc[s]) for s in range(n))
        print("fused reference differs from the exact oracle on", moved, "of", n)
        assert 2 * moved >= n


@pytest.mark.parametrize("opts", OPTION_SETS, ids=OPT_IDS)
def test_crowded_scenes(side, opts):
    I, Q = crowded_scenes(3)
    chk = check_all(side, I, Q, opts, where="crowded")
    assert max(len(c[0]) for c in chk) >= 8


def _want_stop(label, p):
    """Stop reason of pass p on a crafted scene under the default options, by reading wsprd.c:786-793."""
    stopper = label.split("_", 1)[1] if label.startswith(("window_", "cut_")) else label
    if stopper == "A000AA":
        return 2
    if stopper == "K1A" and p == 0:
        return 1
    return 0


def test_loop_exit_scenes(side):
    """Re-encode fails -> break (wsprd.c:786-788) and "A000AA" -> break (:791-793): the checker's record of where each
    pass stopped (orc_wspr_decode_stops) shows that every exit fired, then the outputs equal the reference's."""
    labels, Is, Qs = zip(*payloads.loop_exit_scenes())
    chk = check_all(side, np.stack(Is), np.stack(Qs), trace=True, where="loop exits")
    fired = {1: 0, 2: 0}
    for lab, c in zip(labels, chk):
        tr = c[3]
        assert tr.passes_run >= 1
        for p in range(tr.passes_run):
            want = _want_stop(lab, p)
            assert tr.stop_reason[p] == want, (side.mode, lab, p, tr.stop_reason[p])
            if want:
                fired[want] += 1
                assert tr.n_visited[p] == tr.stop_cand[p] + 1
    assert fired[1] >= 2 and fired[2] >= 3, fired


def comb_record():
    """A record that is zero except at every fourth sample: its spectrum repeats every 128 FFT bins (93.75 Hz) bit for
    bit (the three missing phases enter the butterflies as exact zeros), so a signal at -60 Hz comes with a copy at
    +33.75 Hz of exactly equal snr, and BOTH decode.  Which of the two is refined, subtracted and listed first is the
    sort's order of equal keys."""
    rng = np.random.default_rng(9)
    ok, sym = ol.channel_symbols("K1ABC FN42 37")
    assert ok
    si, sq = synth.tone_signal(sym, -60.0, 2.0, 1.0)
    I = si + rng.normal(0, 0.05, NS)
    Q = sq + rng.normal(0, 0.05, NS)
    keep = (np.arange(NS) % 4 == 0)
    return synth.normalise((I * keep).astype(np.float32), (Q * keep).astype(np.float32))


def test_equal_snr_ties(side):
    """glibc's qsort in the compiled reference (wsprd.c:631, :828) against the checker's ordering of equal keys.  The
    two real-valued records of test_equal_snr_ties_keep_the_reference_order (mirror twins; nothing decodes, so spots
    and residuals are all the reference shows) and a comb record whose twins both decode."""
    rng = np.random.default_rng(5)
    t = np.arange(NS) / 375.0
    recs = []
    for f1, f2, f3 in ((40.3, 77.7, 12.1), (5.5, 93.0, 61.2)):
        recs.append((0.02 * rng.normal(size=NS) + 0.3 * np.cos(2 * np.pi * f1 * t) + 0.2 * np.cos(2 * np.pi * f2 * t)
                     + 0.1 * np.cos(2 * np.pi * f3 * t)).astype(np.float32))
    I = np.stack(recs + [comb_record()[0]])
    Q = np.stack([np.zeros(NS, np.float32)] * 2 + [comb_record()[1]])
    for s in range(3):
        ps = side.fft_bank(I[s], Q[s])
        cands = (ol.Cand * 200)()
        noise = C.c_float()
        npk = ol.lib().orc_pick_peaks(ol.ptr(ps), C.c_int(347), cands, C.byref(noise), None, None)
        snrs = [cands[j].snr for j in range(npk)]
        assert npk >= (6 if s < 2 else 2) and len(snrs) - len(set(snrs)) >= (3 if s < 2 else 1), (s, npk)   # they tie
    if side.mode == "exact":
        for s in range(2):
            onpk, oc, _, _ = _oracle_cands(I[s], Q[s], 1)
            snrs = [oc[j].snr for j in range(onpk)]
            assert len(snrs) - len(set(snrs)) >= 3
    chk = check_all(side, I, Q, where="ties")
    twins = chk[2][0]
    assert len(twins) == 2 and twins[0].message == twins[1].message == b"K1ABC FN42 37"
    assert twins[0].snr == twins[1].snr and abs(abs(twins[0].freq - twins[1].freq) * 1e6 - 93.75) < 0.5
    for opts in (dict(npasses=1), dict(subtraction=0)):
        check_all(side, I[2:], Q[2:], opts, where="comb")


@pytest.mark.parametrize("samples", [44992, 44544, 40000, 30000, 2048, 1024])
def test_short_records(side, samples):
    """Records shorter than the frame in zero-padded 45000 buffers (not below 512 samples: the reference's
    ps[512][blocks] then has a negative extent)."""
    I0, Q0, _ = parity_segments()
    I = np.stack([ref_iq()[0], I0[6], I0[0]]).copy()
    Q = np.stack([ref_iq()[1], Q0[6], Q0[0]]).copy()
    I[:, samples:] = 0
    Q[:, samples:] = 0
    chk = check_all(side, I, Q, n=samples, where="short")
    if samples >= 40000:
        assert len(chk[0][0]) == 1 and len(chk[1][0]) >= 2


def test_finite_extremes(exact):
    I, Q = ref_iq()
    cases = [(np.zeros_like(I), np.zeros_like(Q))] + \
            [(I * np.float32(k), Q * np.float32(k)) for k in (1e30, 1e-42, 1e-3)]
    chk = check_all(exact, np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), where="extremes")
    assert chk[0][0] == [] and [s.message for s in chk[3][0]] == [b"K1JT FN20 20"]


def test_hashtable_file(exact, tmp_path):
    """usehashtable = 1: a type-2 segment, then a type-3 segment that only the stored hash resolves; each side in a
    directory of its own.  Equal spots, byte-equal hashtable.txt."""
    segs = [_multi_segment(["PJ4/K1ABC 37"], 41), _multi_segment(["<PJ4/K1ABC> FK52UD 37"], 42)]
    opt = ol.default_options()
    opt.usehashtable = 1
    dirs = {}
    for which in ("ref", "orc"):
        dirs[which] = tmp_path / which
        dirs[which].mkdir()
    for k, (I, Q) in enumerate(segs):
        r = exact.ref.decode(I, Q, NS, opt, cwd=str(dirs["ref"]))
        with ol.working_directory(str(dirs["orc"])):
            o = ol.decode(I, Q, NS, opt)
        same(r, o, ("hashtable", k))
        assert [s.message.decode() for s in o[0]] == [["PJ4/K1ABC 37"], ["<PJ4/K1ABC> FK52UD 37"]][k]
        ref_txt = (dirs["ref"] / "hashtable.txt").read_bytes()
        assert ref_txt == (dirs["orc"] / "hashtable.txt").read_bytes() and b"PJ4/K1ABC" in ref_txt


# ------------------------------------------------------------------------------- the exported stages on their own
def _both_demod(side, I, Q, freq, shift, drift, mode, lagmin=0, lagmax=0, lagstep=8, ifmin=0, ifmax=0, fstep=0.0,
                np_=NS, symfac=50):
    res = []
    for fn in (side.ref.sync_and_demodulate, side.demod):
        Ic, Qc = I.copy(), Q.copy()
        f = C.c_float(freq); sh = C.c_int(shift); dr = C.c_float(drift); sy = C.c_float(0)
        sym = (C.c_ubyte * 162)()
        fn(ol.ptr(Ic), ol.ptr(Qc), C.c_long(np_), C.addressof(sym), C.addressof(f), ifmin, ifmax, C.c_float(fstep),
           C.addressof(sh), lagmin, lagmax, lagstep, C.addressof(dr), symfac, C.addressof(sy), mode)
        res.append((f.value, sh.value, sy.value, bytes(sym)))
    return res


@pytest.mark.parametrize("seg,drift", [(0, 0.0), (3, 0.0), (7, 2.0), (7, -4.0), (6, 1.0)])
def test_sync_and_demodulate_modes(side, seg, drift):
    I, Q, truth = parity_segments()
    msg, f0, t0, snr = truth[seg][0]
    fc = float(np.float32(round(f0 / 0.732421875) * 0.732421875))
    sc = int(round(t0 * 375 / 128.0)) * 128
    r, c = _both_demod(side, I[seg], Q[seg], fc, sc, drift, 0, lagmin=sc - 128, lagmax=sc + 128, lagstep=8)
    assert r[:3] == c[:3]
    shift = r[1]
    r, c = _both_demod(side, I[seg], Q[seg], fc, shift, drift, 1, ifmin=-2, ifmax=2, fstep=0.1)
    assert r[:3] == c[:3]
    fbest = r[0]
    for jig in (0, -3, 3, 63, -63):
        r, c = _both_demod(side, I[seg], Q[seg], fbest, shift + jig, drift, 2)
        assert r[2:] == c[2:]
    # steps that are not exact in float32 (the decoder's -2..2 x 0.1 are): f0 = *freq + ifreq * fstep (wsprd.c:151)
    # rounds once or twice; a scan of one frequency hands its f0 back
    # (from a small *freq, where the product's rounding is not lost under the sum's)
    got = [_both_demod(side, I[seg], Q[seg], 0.37, shift, drift, 1, ifmin=k, ifmax=k, fstep=0.0137) for k in range(-40, 41)]
    assert [r[:3] for r, c in got] == [c[:3] for r, c in got]
    assert len({r[0] for r, c in got}) == 81


def test_sync_and_demodulate_edges(side):
    I, Q, _ = parity_segments()
    for shift in (-1400, -300, 3700, 4100):
        r, c = _both_demod(side, I[0], Q[0], 10.0, shift, 0.0, 2)
        assert r[2:] == c[2:]
        r, c = _both_demod(side, I[0], Q[0], -37.5, shift, 1.0, 0, lagmin=shift - 128, lagmax=shift + 128, lagstep=16)
        assert r[:3] == c[:3]
    r, c = _both_demod(side, I[0], Q[0], 10.0, 700, 0.0, 2, np_=44000)
    assert r[2:] == c[2:]


@pytest.mark.parametrize("symfac", [50, 64, 20, 127, 1])
def test_sync_and_demodulate_symfac(side, symfac):
    I, Q, truth = parity_segments()
    msg, f0, t0, snr = truth[1][0]
    r, c = _both_demod(side, I[1], Q[1], float(np.float32(f0)), int(round(t0 * 375)), 0.0, 2, symfac=symfac)
    assert r[2:] == c[2:]


def _subtract_both(fns, seg, drift, shift_off, np_):
    I, Q, truth = parity_segments()
    msg, f0, t0, snr = truth[seg][0]
    sym = ol.channel_symbols(msg)[1]
    shift = int(round(t0 * 375)) + shift_off
    outs = []
    for fn in fns:
        Ic, Qc = I[seg].copy(), Q[seg].copy()
        fn(ol.ptr(Ic), ol.ptr(Qc), C.c_long(np_), C.c_float(f0), C.c_int(shift), C.c_float(drift), ol.ptr(sym))
        outs.append((Ic, Qc))
    assert not np.array_equal(outs[0][0], I[seg])
    return outs


@pytest.mark.parametrize("seg,drift,shift_off,np_", [(0, 0.0, 0, NS), (6, 0.0, 0, NS), (7, 2.0, 0, NS), (1, 0.0, -2500, NS),
                                                     (2, -1.0, 3900, NS), (3, 0.0, 0, 30000), (4, 1.0, -700, 41000),
                                                     (5, 0.0, -41000, NS), (0, 0.0, 44000, NS)])
def test_subtract_signal2(side, seg, drift, shift_off, np_):
    r, c = _subtract_both((side.ref.subtract_signal2, side.subtract2), seg, drift, shift_off, np_)
    assert r[0].tobytes() == c[0].tobytes() and r[1].tobytes() == c[1].tobytes()


@pytest.mark.parametrize("seg,drift,shift_off,np_", [(0, 0.0, 0, NS), (6, 0.0, 0, NS), (7, 2.0, 0, NS), (1, 0.0, -2500, NS),
                                                     (2, -1.0, 3900, NS), (3, 0.5, 0, 30000)])
def test_subtract_signal_symbolwise(exact, seg, drift, shift_off, np_):
    r, c = _subtract_both((exact.ref.subtract_signal, ol.lib().orc_subtract_simple), seg, drift, shift_off, np_)
    assert r[0].tobytes() == c[0].tobytes() and r[1].tobytes() == c[1].tobytes()


def test_fused_subtract_signal_is_outside_the_contracted_mode():
    """A record, not a parity claim: the product keeps subtract_signal() exact in both arithmetic modes
    (include/wspr_mi355x.h) and contract_dsp.c lists no site for wsprd.c:263-312, yet clang fuses inside that function.
    So the fused build's subtract_signal() differs from the exact one, which the gcc build gives bit for bit."""
    fused = Side("fma").ref
    exact_ref = Side("exact").ref
    f, o, e = _subtract_both((fused.subtract_signal, ol.lib().orc_subtract_simple, exact_ref.subtract_signal), 0, 0.0, 0, NS)
    assert e[0].tobytes() == o[0].tobytes() and e[1].tobytes() == o[1].tobytes()
    assert f[0].tobytes() != o[0].tobytes() and f[1].tobytes() != o[1].tobytes()
