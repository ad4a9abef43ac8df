"""The kernels a decode launches for its fine search (k4_demod.hip) -- demod_drift_kernel, demod_tile_kernel<8 | 16 | 3, shared | own>,
demod_metric_kernel, phasor_freq_kernel, freq_scalar_kernel, freq_centre_rare_kernel, freq_drift_kernel, freq_metric_kernel and the
lag pick -- held to the reference on EVERY hypothesis, not on the winners alone.  tools/fine_check.hip runs the production
launchers in the pipeline's order on a case file and dumps every buffer; tests/fine_lib.py holds the cases, the references
and check_run(), which asserts, all as bits:
 mode 0   every lag's sync == the reference's single-lag sync (a value the reference reports as -1e30 must not compare above
          -1e30; a lag the pruning did not sum holds -3e38 and the fill pattern); shift, freq, sync after the pick == the chain;
 mode 1   each of the five dumped amplitude rows, folded here in float32 in sync_metric()'s order, == the reference's single
          hypothesis; freq, shift, sync after the scan == the chain; the centre row == the lag block's winning row bytewise
          when one was handed over;
 rungs    rung 0 and rungs 0 .. 42 of the ladder: sync, all 162 symbols and the rms == the reference for every item whose sync
          passed the gate; every row of an item that did not still holds the fill pattern.
tests/test_fine_cases_cpu.py proves on the CPU what each case is for."""
import numpy as np
import pytest

import fine_lib as fl
from fine_lib import NS

pytestmark = pytest.mark.gpu


def _check(tmp_path, recs, runs):
    """One run of the tool, every run's dump checked; the totals of what was compared."""
    total = {}
    dumps = fl.run_tool(tmp_path, recs, runs)
    for g in dumps:
        for k, v in fl.check_run(g, recs).items():
            total[k] = total.get(k, 0) + v
    print("%s; reference calls so far %d" % (total, fl.calls[0]))
    return dumps, total


@pytest.mark.parametrize("arith", [0, 1])
def test_ordinary_candidates(tmp_path, arith):
    """16 candidates of two scenes, every other one drifting, through 8/33 pruned, 8/33 whole and 16/17 (quick mode's
    demod_tile_kernel<16, .>).  Items pass and fail the gate of 0.10, so the ladder writes some rows and leaves others."""
    recs, runs = fl.ordinary_runs(arith)
    dumps, st = _check(tmp_path, recs, runs)
    assert st["lags_pruned"] > 0 and st["centre_copies"] == 3 * dumps[0].n and st["ladder_rows"] == 43 * st["rung0"]
    for g in dumps:                                            # an item that is gated out sits before one that passes
        worth = (g.items_m1["sync"] > g.minsync1).tolist()
        assert worth[0] and False in worth and True in worth[worth.index(False):], worth
    # the pruned and the whole scan leave the same state
    assert fl.same_bits(dumps[0].items_m1, dumps[1].items_m1)


@pytest.mark.parametrize("npts", [45000, 44993, 30000])
@pytest.mark.parametrize("arith", [0, 1])
def test_record_ends_in_the_frequency_scan_and_the_ladder(tmp_path, arith, npts):
    """Straight into the scan at shifts that put its first and last sample, and those of the ladder's first and last rung, on
    each side of the record's ends (fine_lib.edge_direct_items): freq_scalar_kernel, freq_centre_rare_kernel (no lag block:
    every centre is summed), freq_drift_kernel, demod_tile_kernel<3, shared | own>.  minsync1 = -1: every item with a sample
    inside goes down the ladder; the two outside items (NaN) are gated out between them."""
    recs, items = fl.edge_direct_items(npts)
    _, st = _check(tmp_path, recs, [fl.run_of(items, npts=npts, arith=arith, flags=fl.LADDER, minsync1=-1.0)])
    out = 4 if npts == NS else 0
    assert st["gated_out"] == out and st["rung0"] == len(items) - out and st["centre_copies"] == 0


@pytest.mark.parametrize("npts", [45000, 44993, 30000])
@pytest.mark.parametrize("arith", [0, 1])
def test_record_ends_in_the_drifting_lag_scan(tmp_path, arith, npts):
    """demod_drift_kernel (at the full length also demod_tile_kernel<16, false>, step 16) with the first lag starting at samples
    -1 .. 2 and the last lag ending at np - 2 .. np + 1; then the whole chain from wherever the lag scan leaves them (the
    centre copied out of the lag block)."""
    recs, items = fl.edge_lag_items(npts)
    runs = [fl.run_of(items, npts=npts, arith=arith, minsync1=-1.0)]
    if npts == NS:
        runs.append(fl.run_of(items, npts=npts, arith=arith, lagstep=16, minsync1=-1.0))
    _, st = _check(tmp_path, recs, runs)
    assert st["gated_out"] == 0 and st["centre_copies"] == sum(len(r["items"]) for r in runs)


def test_list_shapes(tmp_path):
    """(n_shared, n_own) = (0, 1), (1, 2), (9, 7), (9, 0), (1, 7), (0, 2), (9, 1): runs without a drift-free and without a
    drifting item, drifting items between the others, so that pad, slot and item all differ."""
    recs, runs = fl.list_shape_runs()
    dumps, st = _check(tmp_path, recs, runs)
    assert [(g.n_shared, g.n_own) for g in dumps] == list(fl.LIST_SHAPES)
    assert st["gated_out"] > 0 and st["rung0"] > 0


@pytest.mark.parametrize("arith", [0, 1])
def test_ties_keep_the_first_hypothesis(tmp_path, arith):
    """The period-8 carrier with drift 2.0 and -3.5: 33 (17) bit-equal lags, the pick is lag 0; the sparse record: five syncs of
    +0.0, the scan returns hypothesis -2.  minsync1 = -1, so rung 0 and the ladder run on them too."""
    recs, runs = fl.tie_runs(arith)
    dumps, st = _check(tmp_path, recs, runs)
    for g in dumps[:2]:
        for it in range(g.n):
            assert len({fl.bits(v) for v in g.sync0[it]}) == 1, g.sync0[it]
            assert int(g.items_m0["shift"][it]) == int(g.items_in["shift_coarse"][it]) - 128
    g = dumps[2]
    for it in range(g.n):
        assert all(fl.bits(v) == 0 for v in fl.fold(g.pwf[it], fl.la.pr3())), it
        assert g.items_m1["freq"][it] < np.float32(fl.SPARSE_FC - 0.15) and fl.bits(g.items_m1["sync"][it]) == 0
    assert st["gated_out"] == 0


@pytest.mark.parametrize("arith", [0, 1])
def test_no_lag_wins(tmp_path, arith):
    """All-zero and all-NaN records, pruned and whole: the pick leaves shift 0, freq 0.0, sync -1e30; the frequency scan then
    sums its centre (freq_centre_rare_kernel, freq_drift_kernel) unless that state is a grid point of the lag scan
    (freq_coarse 0.0, shift_coarse 128: copied from lag 0); nothing passes the gate."""
    recs, runs = fl.no_lag_runs(arith)
    dumps, st = _check(tmp_path, recs, runs)
    assert st["centre_copies"] == 2 * 4 and st["rung0"] == 0 and st["minus1e30"] == st["lags"] and st["lags"] + st["lags_pruned"] == 2 * 12 * 33
    for g in dumps:
        assert (g.items_m1["shift"] == 0).all() and (g.items_m1["freq"].view(np.uint32) == 0).all()
        assert (g.items_m1["sync"] == fl.MINUS_1E30).all()


def test_the_gates_are_strict(tmp_path):
    """An item's sync s after the scan: with minsync1 = s neither rung 0 nor the ladder writes a byte for it, with the float
    below s both are written and equal the reference (freq_metric_kernel, demod_tile_kernel<3, .>, demod_metric_kernel)."""
    recs, items = fl.gate_items()
    first, = fl.run_tool(tmp_path, recs, [fl.run_of(items, flags=fl.WHOLE_CHAIN & ~fl.LADDER)])
    fl.check_run(first, recs)
    runs = []
    for it in (0, 1):                                       # a drift-free and a drifting item
        s = first.items_m1["sync"][it]
        runs += [fl.run_of(items, minsync1=s), fl.run_of(items, minsync1=np.nextafter(s, np.float32(-np.inf), dtype=np.float32))]
    dumps = fl.run_tool(tmp_path, recs, runs)
    for g in dumps:
        fl.check_run(g, recs)
    for it in (0, 1):
        at, below = dumps[2 * it], dumps[2 * it + 1]
        assert fl.same_bits(at.items_m1, first.items_m1) and fl.same_bits(below.items_m1, first.items_m1)
        assert fl.untouched(at.sync_r0[it]) and fl.untouched(at.sym_r0[it]) and fl.untouched(at.sync_l[it]) and fl.untouched(at.sym_l[it])
        assert fl.same_bits(below.sync_r0[it], first.sync_r0[it]) and fl.same_bits(below.sym_r0[it], first.sym_r0[it])
        assert not fl.untouched(below.sync_l[it]) and fl.same_bits(below.sync_l[it, 21], first.sync_r0[it])


@pytest.mark.parametrize("arith", [0, 1])
def test_extremes(tmp_path, arith):
    """Noise x 1e20 and x 1e-30 (squares overflow and underflow) and one +Inf inside the windows of lags >= 16 only, drift-free and
    drifting: the device equals the reference whatever that is."""
    recs, runs = fl.extreme_runs(arith)
    _check(tmp_path, recs, runs)
