"""What each crafted case of tests/fine_lib.py is for, proved on the CPU references (the oracle; the CONTRACT=1 checker), so that
tests/test_gpu_fine.py compares the device on inputs that really exercise what they claim to: the tie multiplicities, the
hypotheses that come out NaN, which side of each record end every edge shift puts a window on, the pair of thresholds around
a sync, and that the two arithmetic modes differ where the contracted comparison is to discriminate.  The counts are pinned."""
import numpy as np

import fine_lib as fl
from fine_lib import NS, SPAN


DIFFER_LAGS = 468         # of the 528 (item, lag) syncs of the ordinary candidates, between the two arithmetic modes


def _lags(arith, rec, npts, fc, drift, sc, step):
    return np.array([fl.lag_sync(arith, rec, npts, fc, drift, sc - 128 + step * m) for m in range(256 // step + 1)], np.float32)


def _freqs(arith, rec, npts, freq, drift, shift):
    return np.array([fl.freq_sync(arith, rec, npts, freq, drift, shift, f) for f in range(-2, 3)], np.float32)


def test_period8_carrier_ties_all_lags_of_a_drifting_item():
    """All 33 lags at step 8 and all 17 at step 16 are bit-equal for drift 2.0 and -3.5; the reference keeps the first (lag 0);
    the five frequency hypotheses differ from one another."""
    recs, fc, sc = fl.tie_case()
    for arith in (0, 1):
        for drift, want in ((2.0, np.float32(0.0072562103)), (-3.5, np.float32(-0.011552207))):
            s8, s16 = _lags(arith, recs[0], NS, fc, drift, sc, 8), _lags(arith, recs[0], NS, fc, drift, sc, 16)
            assert len({fl.bits(v) for v in s8}) == 1 and len({fl.bits(v) for v in s16}) == 1 and fl.same_bits(s8[0], s16[0])
            if arith == 0:
                assert fl.same_bits(s8[0], want), (drift, s8[0])
            for step in (8, 16):
                f, sh, sy = fl.chain_mode0(arith, recs[0], NS, fc, drift, sc, step)
                assert sh == sc - 128 and fl.same_bits(f, np.float32(fc)) and fl.same_bits(sy, s8[0])
            assert len({fl.bits(v) for v in _freqs(arith, recs[0], NS, fc, drift, sc - 128)}) == 5


def test_sparse_record_ties_the_five_frequencies_at_plus_zero():
    """162 samples 256 apart, each the first of its symbol's window, where every phasor is (1, 0): the four tone amplitudes of a
    symbol are equal under every hypothesis, every sync is +0.0, and the reference keeps hypothesis -2: 10.05 from 10.25."""
    recs, _, _ = fl.tie_case()
    for arith in (0, 1):
        for drift in (0.0, 1.5):
            s = _freqs(arith, recs[1], NS, fl.SPARSE_FC, drift, fl.SPARSE_SHIFT)
            assert all(fl.bits(v) == 0 for v in s), s
            f, sh, sy = fl.chain_mode1(arith, recs[1], NS, fl.SPARSE_FC, drift, fl.SPARSE_SHIFT)
            assert sh == fl.SPARSE_SHIFT and fl.bits(sy) == 0
            assert abs(float(f) - 10.05) < 1e-5 and f < np.float32(fl.SPARSE_FC - 0.15), f
            # one sample off the grid of 256 and the tie is gone
            assert len({fl.bits(v) for v in _freqs(arith, recs[1], NS, fl.SPARSE_FC, drift, fl.SPARSE_SHIFT - 1)}) > 1


def test_no_lag_wins_on_zero_and_nan_records():
    """Every hypothesis is 0 / 0 or NaN: all 33 + 5 come out -1e30 and the chain leaves shift 0, freq 0.0, sync -1e30 twice."""
    n = 0
    for arith in (0, 1):
        recs, runs = fl.no_lag_runs(arith)
        for it in runs[0]["items"]:
            rec, fc, sc, drift = recs[it["seg"]], it["freq_coarse"], int(it["shift_coarse"]), it["drift"]
            assert (_lags(arith, rec, NS, fc, drift, sc, 8) == fl.MINUS_1E30).all()
            f, sh, sy = fl.chain_mode0(arith, rec, NS, fc, drift, sc, 8)
            assert (fl.bits(f), sh, fl.bits(sy)) == (0, 0, fl.bits(fl.MINUS_1E30))
            assert (_freqs(arith, rec, NS, f, drift, sh) == fl.MINUS_1E30).all()
            f, sh, sy = fl.chain_mode1(arith, rec, NS, f, drift, sh)
            assert (fl.bits(f), sh, fl.bits(sy)) == (0, 0, fl.bits(fl.MINUS_1E30))
            # the state (shift 0, freq 0.0) is a grid point of the lag scan for freq_coarse 0.0 and shift_coarse 128 only
            n += int(fc == 0.0 and (0 - (sc - 128)) >= 0 and (0 - (sc - 128)) % 8 == 0)
    assert n == 2 * 4


def _perturbed(rec, k):
    r = fl.Rec(rec.I, rec.Q)
    r.I[k] = np.float32(r.I[k] + 3.0)
    return r


def test_edge_shifts_put_the_record_ends_on_each_side_of_a_window():
    """A hypothesis that starts at sample `first` reads 0 < k < np of first .. first + 41 471.  Changing sample 0 never changes
    a sync; changing sample 1 changes it exactly for first <= 1; changing sample np - 1 exactly for last >= np - 1; changing
    sample np (which exists in the row) never.  First samples -1, 0, 1 give three different syncs."""
    recs, cands = fl.scenes()
    rec, fc = recs[0], cands[0][1]
    assert [fl.window(k, NS)[2] for k in fl.HEAD] == [SPAN - 2, SPAN - 1, SPAN, SPAN]
    for drift in (0.0, fl.EDGE_DRIFT):
        base = [fl.lag_sync(0, rec, NS, fc, drift, k) for k in fl.HEAD]
        assert len({fl.bits(v) for v in base[:3]}) == 3
        r0, r1 = _perturbed(rec, 0), _perturbed(rec, 1)
        for k, b in zip(fl.HEAD, base):
            assert fl.same_bits(fl.lag_sync(0, r0, NS, fc, drift, k), b), k
            assert fl.same_bits(fl.lag_sync(0, r1, NS, fc, drift, k), b) == (k > 1), k
        for npts in (45000, 44993, 30000):
            firsts = fl.tails(npts)
            assert [fl.window(k, npts)[1] for k in firsts] == [npts - 2, npts - 1, npts, npts + 1]
            if firsts[0] > 0:                                     # (at 30 000 samples the record's start cuts these windows too)
                assert [fl.window(k, npts)[2] for k in firsts] == [SPAN, SPAN, SPAN - 1, SPAN - 2]
            ra, rb = _perturbed(rec, npts - 1), _perturbed(rec, npts)
            for k in firsts:
                b = fl.lag_sync(0, rec, npts, fc, drift, k)
                assert fl.same_bits(fl.lag_sync(0, ra, npts, fc, drift, k), b) == (k + SPAN - 1 < npts - 1), (npts, k)
                assert fl.same_bits(fl.lag_sync(0, rb, npts, fc, drift, k), b), (npts, k)


def test_edge_items_reach_every_stage_at_every_end():
    """The items of the edge runs: the first / last touched sample of the frequency scan, of the ladder's first and last rung and
    of the drifting lag scan's first and last lag take each of -1, 0, 1, 2 and np - 2 .. np + 1; the two outside items read
    no sample at all, so each of their hypotheses is NaN."""
    for npts in (45000, 44993, 30000):
        _, it = fl.edge_direct_items(npts)
        for drift in (0.0, fl.EDGE_DRIFT):
            sh = {int(s) for s, d in zip(it["shift"], it["drift"]) if d == np.float32(drift)}
            assert {s + SPAN - 1 for s in sh} >= set(range(npts - 2, npts + 2))               # the scan's last sample
            assert {s + 63 + SPAN - 1 for s in sh} >= set(range(npts - 2, npts + 2))          # the last rung's
            if npts == NS:
                assert sh >= set(fl.HEAD) and {s - 63 for s in sh} >= set(fl.HEAD)            # the scan's, the first rung's first
                # rung 21 (jitter 0) inside the record while rungs 0 .. 20 hang over its start
                assert any(s > 0 and s - 63 + 3 * 20 < 0 for s in sh)
                out = [s for s in sh if fl.window(s - 63, npts)[2] == 0 and fl.window(s + 63, npts)[2] == 0]
                assert sorted(out) == [-50000, 50000]
        _, it = fl.edge_lag_items(npts)
        sc = {int(s) for s, d in zip(it["shift_coarse"], it["drift"]) if d != 0.0}
        assert {s + 128 + SPAN - 1 for s in sc} >= set(range(npts - 2, npts + 2))
        assert npts != NS or {s - 128 for s in sc} >= set(fl.HEAD)
        assert (it["drift"] == 0.0).sum() == 1 and it["drift"][0] != 0.0 and it["drift"][-1] != 0.0
    recs, cands = fl.scenes()
    for s in (-50000, 50000):
        assert fl.freq_sync(0, recs[0], NS, cands[0][1], 0.0, s, 0) == fl.MINUS_1E30


def test_ordinary_candidates_gate_and_arithmetic_counts():
    """The 16 ordinary candidates through the chain in both modes.  Pinned: how many pass sync > 0.10 after the scan (passing and
    failing items alternate, so slots and items differ down the ladder's list), and on how many hypotheses the exact oracle and
    the CONTRACT=1 checker differ -- the contracted comparison on the device discriminates between the two."""
    recs, items = fl.ordinary_items()
    assert sorted(set(items["seg"].tolist())) == [0, 1] and (items["drift"] != 0).sum() == 8 and (items["drift"][1::2] != 0).all()
    worth, differ, total = {0: [], 1: []}, 0, 0
    for it in items:
        rec, fc, sc, drift = recs[it["seg"]], it["freq_coarse"], int(it["shift_coarse"]), it["drift"]
        l0, l1 = _lags(0, rec, NS, fc, drift, sc, 8), _lags(1, rec, NS, fc, drift, sc, 8)
        differ += sum(fl.bits(a) != fl.bits(b) for a, b in zip(l0, l1))
        total += 33
        for arith in (0, 1):
            f, sh, _ = fl.chain_mode0(arith, rec, NS, fc, drift, sc, 8)
            worth[arith].append(bool(fl.chain_mode1(arith, rec, NS, f, drift, sh)[2] > fl.MINSYNC1))
    print("gate: %s; lags on which the modes differ: %d of %d" % (worth[0], differ, total))
    assert worth[0] == worth[1] == [True] * 11 + [False, True, True, False, False]
    assert total == 528 and differ == DIFFER_LAGS


def test_gate_thresholds_straddle_a_sync():
    """minsync1 = s keeps an item with sync s out (strict >), the float below s lets it in."""
    recs, items = fl.gate_items()
    for it in items:
        rec, drift = recs[it["seg"]], it["drift"]
        f, sh, _ = fl.chain_mode0(0, rec, NS, it["freq_coarse"], drift, int(it["shift_coarse"]), 8)
        s = fl.chain_mode1(0, rec, NS, f, drift, sh)[2]
        below = np.nextafter(s, np.float32(-np.inf), dtype=np.float32)
        assert s > fl.MINSYNC1 and not (s > s) and s > below and fl.bits(below) == fl.bits(s) - 1


def test_list_shapes_cover_the_issue():
    recs, runs = fl.list_shape_runs()
    shapes = [(int((r["items"]["drift"] == 0).sum()), int((r["items"]["drift"] != 0).sum())) for r in runs]
    assert shapes == list(fl.LIST_SHAPES)
    assert {s[1] for s in shapes} >= {1, 2, 7, 0} and {s[0] for s in shapes} >= {0, 1, 9}
    nine_seven = runs[2]["items"]["drift"] != 0
    assert nine_seven[1:-1].any() and not nine_seven[0] and (np.diff(np.flatnonzero(nine_seven)) >= 2).all()


def test_restated_fold_and_rms_against_the_reference():
    """fold() and rms_of() are the test's own restatements: the fold of amplitudes that give a known sync, the rms of symbols with
    a known sum of squares."""
    pr3 = fl.la.pr3()
    rows = np.zeros((2, 162, 4), np.float32)
    rows[0, :, 1], rows[0, :, 3] = pr3, pr3                       # cmet = +2 on the sync bits: ss = sum(pr3) * 2
    rows[0, :, 0] = 1 - pr3                                        # cmet = -1 off them, subtracted: ss += 1
    rows[1] = 1.0
    got = fl.fold(rows, pr3)
    ones = int(pr3.sum())
    assert got[0] == np.float32(2 * ones + (162 - ones)) / np.float32(2 * ones + (162 - ones)) and got[1] == 0.0
    assert fl.rms_of(np.full(162, 128 + 50, np.uint8)) == np.float32(50.0) and fl.rms_of(np.full(162, 0, np.uint8)) == np.float32(128.0)
