"""CPU proofs for the crafted K2/K3 cases of tests/k2k3_lib.py: the all-hypotheses helper is held to orc_coarse_sync, and
every case's condition -- which hypothesis wins, how many tie, what the picker keeps -- is shown with the oracle, so
that tests/test_gpu_k2k3_ps.py cannot pass vacuously.  Nothing here touches the device."""
import numpy as np
import pytest

import k2k3_lib as kl

B = kl.BLOCKS
PATTERN_COLUMN = {0: 0, 1: 4, 2: 5}                 # a column of the helper's table (maxdrift 4) per drift pattern


def _tables(case):
    for s in range(case.ps.shape[0]):
        for j in range(case.counts[s]):
            yield s, j, kl.all_hypotheses(case.ps[s], case.blocks, case.freqs[s, j], case.maxdrift)


K3_CASES = ([(kl.planted_winners, m) for m in (4, 1, 0)] + [(kl.short_record, b) for b in kl.SHORT_BLOCKS]
            + [(kl.no_plant,), (kl.ties,), (kl.q2_only,)] + [(kl.active_list, o) for o in kl.ACTIVE_ORDERS])


@pytest.mark.parametrize("case", K3_CASES, ids=lambda c: c[0].__name__ + "".join("-%s" % (a,) for a in c[1:]))
def test_first_strict_maximum_of_the_helper_table_is_the_oracle_pick(case):
    """The helper restates orc_coarse_sync's loops and keeps every hypothesis: the first strict maximum of its table is
    (freq, shift, drift, sync) of orc_coarse_sync, bit for bit, on every K3 case."""
    c = case[0](*case[1:])
    exp = kl.expected_k3(*case)
    n = 0
    for s, j, (table, _) in _tables(c):
        assert kl.first_maximum(table, c.freqs[s, j], c.maxdrift) == exp[s][j], (c.name, s, j)
        n += 1
    assert n == int(c.counts.sum())


@pytest.mark.parametrize("maxdrift,count", [(4, 288), (1, 288), (0, 96)])
def test_every_hypothesis_wins_its_plant(maxdrift, count):
    c = kl.planted_winners(maxdrift)
    exp = kl.expected_k3(kl.planted_winners, maxdrift)
    winners = set()
    for (s, j), h in c.plants.items():
        got = kl.hypothesis_of(c.freqs[s, j], maxdrift, *exp[s][j][:3])
        assert got == h, (s, j)
        winners.add(got)
    assert len(winners) == count and c.ps.shape[0] <= 300
    if0 = {kl.if0_of(f) for s in range(c.ps.shape[0]) for f in c.freqs[s, :c.counts[s]]}
    assert min(if0) == 106 and max(if0) == 406                 # smoothed bins 55 and 355: both band edges
    lags = {h[1] for h in winners}
    assert lags == set(range(32))                              # lags -10 .. -1 among them (Q2)


# The lags a plant must still win at, per record length.  A plant can lose: the metric is a RATIO, so a few noise symbols
# of a neighbouring hypothesis may carry it past the plant's 0.74; in a record of seven blocks the flat index of lag -10
# (time index -10 and +4 are the same column, two rows apart) makes the plant collide with itself.
SHORT_LAGS = {7: range(1, 17), 15: range(0, 25), 31: range(32), 163: range(32), 343: range(32)}


@pytest.mark.parametrize("blocks", kl.SHORT_BLOCKS)
def test_short_record_plants(blocks):
    """The planted hypothesis attains the maximum (together with those the short record makes identical to it) at every
    lag that has a symbol inside, for at least 45 % of the plants; lags without a symbol inside carry the previous value."""
    c = kl.short_record(blocks)
    attained, lags, carried = 0, set(), 0
    for s, j, (table, inside) in _tables(c):
        b, lag, pat = c.plants[(s, j)]
        if table[b, lag, PATTERN_COLUMN[pat]] == table.max():
            attained += 1
            lags.add(lag)
        flat, ins = table.reshape(-1), inside.reshape(-1)
        idle = np.nonzero(ins == 0)[0]
        assert idle.size == 0 or idle[0] > 0
        assert np.array_equal(flat[idle].view(np.uint32), flat[idle - 1].view(np.uint32))       # carried over
        carried += idle.size
    assert lags == set(SHORT_LAGS[blocks]) and attained * 100 >= 45 * len(c.plants), (attained, sorted(lags))
    assert (carried > 0) == (blocks < 22 + 1)                   # 7 and 15: lags >= blocks exist


def test_ties():
    c = kl.ties()
    exp = kl.expected_k3(kl.ties)
    mult = {}
    for s, j, (table, _) in _tables(c):
        top = table.max()
        mult[(s, j)] = int((table == top).sum())
        assert mult[(s, j)] >= 2
        first = np.unravel_index(int(np.argmax(table)), table.shape)
        assert kl.hypothesis_of(c.freqs[s, j], 4, *exp[s][j][:3]) == (first[0], first[1], {0: 0, 4: 1, 5: 2}[first[2]])
        if s == 0:                                              # (a) every hypothesis is 0: the first one of all
            assert top == 0 and mult[(s, j)] == 864 and exp[s][j][1:] == (-1152, -4.0, 0.0)
            assert kl.if0_of(exp[s][j][0]) == kl.if0_of(c.freqs[s, j]) - 1
        elif s == 1:                                            # (b) the first bin is negative throughout
            assert top == 0 and table[0].max() < 0 and first == (1, 0, 4) and mult[(s, j)] == 320
        else:                                                   # (c) lags >= 0 of the winning bin and pattern agree
            assert first[1] == 10 and exp[s][j][1] == 128 and mult[(s, j)] == 22
            assert np.all(table[first[0], 10:, first[2]] == top) and top > 0
    assert len(mult) == 6 + len(kl.TIE_C)


def test_q2_only_winners_have_negative_lags():
    """The only energy lies where a negative time index reads it (the previous rows' last ten columns): every candidate's
    winner has a lag below 0, eight different ones in all, and it beats every lag >= 0."""
    c = kl.q2_only()
    exp = kl.expected_k3(kl.q2_only)
    lags = set()
    for s, j, (table, _) in _tables(c):
        got = kl.hypothesis_of(c.freqs[s, j], 4, *exp[s][j][:3])
        assert got[1] < 10 and got[0] == c.plants[(s, j)][0] and table[:, 10:, :].max() < table.max()
        lags.add(got[1])
    assert lags == set(range(8))


def test_no_plant_and_active_lists():
    c = kl.no_plant()
    assert tuple(c.counts) == kl.NO_PLANT_COUNTS
    assert tuple(kl.ACTIVE_ORDERS[0]) == (5, 0, 3) and kl.active_list(kl.ACTIVE_ORDERS[0]).ps.shape[0] == 7
    assert tuple(kl.ACTIVE_ORDERS[1]) == tuple(range(6, -1, -1))


# ------------------------------------------------------------------------------------------------------------------ K2
def _maxima(nrm):
    return [j for j in range(1, 410) if nrm[j] > nrm[j - 1] and nrm[j] > nrm[j + 1]]


def _kept_bins(cands):
    return [int(round(c[0] / kl.HALF_DF)) + 205 for c in cands]


@pytest.mark.parametrize("blocks", kl.TIME_AVERAGE_BLOCKS)
def test_time_average_rows_depend_on_the_order_of_the_sum(blocks):
    c = kl.time_average(blocks)
    rows = c.ps[:, 48:465, :]
    assert blocks == 1 or np.all(rows.max(axis=2) / rows.min(axis=2) > 2.0 ** 23)
    if blocks > 2:
        serial = np.zeros(rows.shape[:2], np.float32)
        back = np.zeros(rows.shape[:2], np.float32)
        for t in range(blocks):
            serial += rows[:, :, t]
            back += rows[:, :, blocks - 1 - t]
        assert (serial != back).mean() > 0.3                    # another order of the same terms: other bits


def test_percentile_ties_and_infinities():
    exp = kl.expected_k2(kl.percentile)
    for s, (npk, cands, noise, sm, nrm) in enumerate(exp):
        srt = np.sort(sm)
        ranks = np.nonzero(srt == noise)[0]
        assert not np.isnan(sm).any() and ranks.size >= 50 and ranks[0] < 122 < ranks[-1], s
    assert np.isinf(exp[2][3]).sum() == 14 and exp[2][0] == 1 and [e[0] for e in exp[:2]] == [0, 0]


def test_floor_and_plateaus():
    (npk, cands, noise, sm, nrm), = kl.expected_k2(kl.floor_and_plateaus)
    assert noise == kl.FLOOR_C and sm[80] == kl.FLOOR_BELOW and sm[120] == kl.FLOOR_ABOVE
    below = np.float32(np.float64(sm[80] / noise) - 1.0)
    assert below < kl.MIN_SNR < nrm[120] and sm[120] == np.nextafter(sm[80], np.float32(np.inf))      # adjacent values
    assert sm[160] == sm[161] > sm[159] and sm[160] > sm[162]                  # plateau of two
    assert sm[200] == sm[201] == sm[202] > sm[199] and sm[202] > sm[203]       # plateau of three
    assert sorted(_kept_bins(cands)) == [120, 240] and npk == 2


def test_densest_list():
    (npk, cands, noise, sm, nrm), = kl.expected_k2(kl.densest)
    mx = _maxima(nrm)
    assert npk == 151 and len(mx) == 205 and mx[199] == 399                     # the cap of 200 fires ...
    assert all(abs((j - 205) * kl.HALF_DF) > 110 for j in mx[200:])            # ... on maxima the window drops anyway
    assert sorted({kl.if0_of(c[0]) for c in cands})[0] >= 105                  # (after the coarse sync: if0 - 1 .. if0 + 1)


def test_ulp_pairs():
    exp = kl.expected_k2(kl.ulp_pairs)
    pairs = swapped = 0
    peaks = []
    for npk, cands, noise, sm, nrm in exp:
        order = _kept_bins(cands)
        assert npk == 8
        for p in range(4):
            lo, hi = 62 + 56 * p, 62 + 56 * p + 28
            assert sm[hi] == np.nextafter(sm[lo], np.float32(np.inf))
            pairs += 1
            swapped += order.index(hi) < order.index(lo)
            peaks.append(nrm[lo])
    assert pairs == 64 and swapped >= 1 and min(peaks) < 0.2 and max(peaks) > 1e6 and min(peaks) >= kl.MIN_SNR


def test_edge_bins_and_short_lists():
    inside, outside = kl.expected_k2(kl.edge_bins)
    assert _maxima(inside[4]) == [55, 355] and _maxima(outside[4]) == [54, 356]
    assert inside[0] == 2 and outside[0] == 0
    assert sorted(kl.if0_of(c[0]) for c in kl.oracle_peaks(kl.edge_bins().ps[0], B)[1]) == [106, 406]     # before K3
    zero, one = kl.expected_k2(kl.zero_and_one)
    assert zero[0] == 0 and one[0] == 1
