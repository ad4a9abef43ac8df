"""What each vector set of tests/fano_lib.py is for, established on the CPU: the emulation of the device Fano search
(tests/helpers/fano_wave_check.cpp: the kernel's step rule, store and ledgers) against the serial decoders.  The GPU tests
(tests/test_gpu_fano_wave.py) then compare the kernel with this emulation step count for step count; the counts pinned
here say that those vectors do reach the budget's edge, the 8-wide and 1-wide steps, the window's moves and the overflow
exit.  Every comparison is ==."""
import numpy as np

import fano_lib as fl

RET, METRIC, CYCLES, MAXNP, STEPS, MAXSIZE = 0, 1, 2, 3, 14, 15


def test_budget_edge_triples_agree_everywhere():
    """fano.c:149-153, 231-237: a frame found at look i under B = 81 * maxcycles gives (0, i + 1) for i < B, (-1, B + 1) for
    i == B and (-1, B + 2) for i > B.  Every vector of the golden file has i = 81 * m and is recorded at m - 1, m, m + 1:
    the golden file (the reference's own results), the live reference where present, the oracle's orc_fano, the product's
    fano() and the emulation at every shape say the same, and the three regimes do appear."""
    edges = fl.budget_edges()
    cyc = sorted(cases[2][2] for _, cases in edges)
    assert len(edges) >= 9 and cyc[0] == 82 and cyc[1] < 500 and cyc[-1] > 10000, cyc
    decoders = fl.serial_decoders()
    assert {"oracle", "product"} <= set(decoders)
    for sym, cases in edges:
        m = cases[1][0]
        assert [c[0] for c in cases] == [m - 1, m, m + 1]
        c = 81 * m + 1
        assert [(c_[1], c_[2]) for c_ in cases] == [(-1, 81 * (m - 1) + 2), (-1, 81 * m + 1), (0, c)], (m, cases)
        for maxcycles, ret, cycles, metric, decdata in cases:
            want = [ret, metric, cycles, 80 if ret == 0 else 0] + list(decdata)
            for name in decoders:
                assert fl.serial(sym, maxcycles, name)[0].tolist() == want, (name, m, maxcycles)
            for width, cap in fl.SHAPES:
                assert fl.defined(fl.wave(sym, maxcycles, width, cap))[0].tolist() == want, (width, cap, m, maxcycles)


def test_alternating_family_fills_the_store():
    """Alternating saturated symbols with 5 % erasures never decode and grow bushy trees.  The first 16 at the full budget:
    15 pass 2 048 pending visits of 4 096 (where the 8-wide step begins), 14 reach 768 of 1 024 (room <= 256: the 1-wide
    step; 5 already at a budget of 1 500), and a store of 96 overflows for every one from a budget of 1 500 on, after at
    most 67 682 steps."""
    sym = fl.alternating_vectors(16)
    for cap, budget in ((4096, 10000), (1024, 10000), (1024, 1500)):
        r = fl.wave_of("alternating", budget, 64, cap)
        assert (fl.defined(r) == fl.serial_of("alternating", budget)).all()
        assert (r[:, RET] == -1).all() and (r[:, CYCLES] == 81 * budget + 2).all()
    big = fl.wave_of("alternating", 10000, 64, 4096)[:, MAXSIZE]
    assert int((big > 2048).sum()) == 15 and (big.min(), big.max()) == (1852, 2146), big
    assert int((fl.wave_of("alternating", 10000, 64, 1024)[:, MAXSIZE] >= 768).sum()) == 14
    assert int((fl.wave_of("alternating", 1500, 64, 1024)[:, MAXSIZE] >= 768).sum()) == 5
    over = {}
    for budget in fl.BUDGETS:
        r = fl.wave(sym, budget, 64, 96)
        over[budget] = (int((r[:, RET] == -2).sum()), int(r[:, STEPS].max()))
        assert (r[r[:, RET] != -2][:, [RET, CYCLES]] == [-1, 81 * budget + 2]).all()
    # (a budget of 50 or 200 runs out before the store does for most of them)
    assert over == {50: (1, 2331), 200: (7, 9343), 1500: (16, 67682), 10000: (16, 67682)}


def test_a_store_of_96_overflows_for_some_and_is_exact_for_the_rest():
    """The 364 ladder vectors through a store of 96 visits (the lab's WSPR_FANO_WAVE_CAP=96): decoded / timed out / -2 are
    123 / 230 / 11 at 200 cycles per bit and 136 / 112 / 116 at 1 500, and every vector that does not return -2 equals
    the serial decoder in everything."""
    for budget, counts in ((200, (123, 230, 11)), (1500, (136, 112, 116))):
        r = fl.wave_of("ladder", budget, 64, 96)
        s = fl.serial_of("ladder", budget)
        over = r[:, RET] == -2
        assert (int((r[:, RET] == 0).sum()), int((r[:, RET] == -1).sum()), int(over.sum())) == counts
        assert over.sum() >= 5 and (~over).sum() >= 100
        assert (fl.defined(r[~over]) == s[~over]).all()
        assert (r[over][:, 1:14] == 0).all()                   # a -2 reports nothing


def test_the_ladder_vectors_cover_the_window_and_the_kernel_shapes_are_exact():
    """At the production store of 4 096 and the full budget, 76 of the 364 vectors stay within the LDS window of 512 visits
    (it never moves), 173 peak at 513 .. 768 and 115 above (17 of them above 1 024, one above 2 048): each class of the
    window's moves is met at least 50 times.  No vector overflows 4 096 or 1 024 at any budget, and both shapes equal the
    serial decoder in everything."""
    m = fl.wave_of("ladder", 10000, 64, 4096)[:, MAXSIZE]
    classes = (int((m <= 512).sum()), int(((m > 512) & (m <= 768)).sum()), int((m > 768).sum()))
    assert classes == (76, 173, 115) and min(classes) >= 50
    assert (int((m > 1024).sum()), int((m > 2048).sum())) == (17, 1)
    for cap, budgets in ((4096, fl.BUDGETS), (1024, (200, 10000))):
        for budget in budgets:
            r = fl.wave_of("main", budget, 64, cap)
            assert (fl.defined(r) == fl.serial_of("main", budget)).all(), (cap, budget)
    # at 1 024 exactly one ladder vector reaches the 1-wide step (room <= 256), and only at the full budget
    assert int((fl.wave_of("main", 10000, 64, 1024)[:364, MAXSIZE] >= 768).sum()) == 1
    assert int((fl.wave_of("main", 200, 64, 1024)[:364, MAXSIZE] >= 768).sum()) == 0


def test_the_serial_decoders_agree_on_every_set():
    """The reference's fano() where present, orc_fano and the product's fano(): equal on the ladder and alternating vectors."""
    names = list(fl.serial_decoders())
    for budget in (50, 200, 1500):
        base = fl.serial_of("main", budget, names[0])
        for other in names[1:]:
            assert (fl.serial_of("main", budget, other) == base).all(), (other, budget)
