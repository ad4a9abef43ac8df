"""The cases of tests/test_gpu_k7_table.py on the CPU, before anything reaches a GPU: for every phase case the host's run
table in the device layout (phase_runs_table, tests/helpers/phase_runs_check.cpp), evaluated with the selection
sub_fir_fused_kernel makes (phase_table_eval), equals the reference's serial float walk bit for bit; the chained builder --
the scalar form of sub_runs_wave_kernel -- terminates and gives the same table; and the run count is the one written into
the case list (tests/subtract_lib.py).  Also the geometry of the frame-edge cases."""
import numpy as np
import pytest

import subtract_lib as sl

CASES = sl.phase_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_table_equals_the_serial_walk(case):
    name, f0, drift, sym, nr = case
    d = sl.dphi(f0, drift, sym)
    walk, nr_walk, bad = sl.serial_walk(d)
    assert bad == 0 and nr_walk == nr, (name, nr_walk, bad)
    tb = sl.host_table(d)
    assert tb.nr == nr
    phi, skipped = sl.table_eval(tb)
    assert skipped == 0
    assert sl.same_floats(phi, walk)
    for width in (64, 5):
        assert sl.chained_diff(d, width) == 0, (name, width)
    # the layout: what the builder does not write keeps the caller's bytes
    sent = np.uint16(sl.SENTINEL * 0x101)
    assert tb.first_run[sl.NSYM + 1] == sent
    if nr >= 0:
        assert tb.first_run[0] == 0 and tb.first_run[sl.NSYM] == nr and np.all(np.diff(tb.first_run[:sl.NSYM + 1].astype(int)) >= 1)
        assert np.all(tb.runs[nr:].view(np.uint8) == sl.SENTINEL) and np.all(tb.runs["start"][:nr] < sl.NSIG)
        assert np.all(np.diff(tb.runs["start"][:nr]) > 0)
    else:
        assert tb.first_run[0] == 0xFFFF
    if name in sl.NR_WIDE:
        assert sl.serial_walk(d, 4096)[1] == sl.NR_WIDE[name]


def test_the_cases_reach_the_paths_they_are_named_for():
    raw = np.int32(-2 ** 31)                                      # kPhaseRawBits: a zero, subnormal or non-finite phase
    by = {c[0]: c for c in CASES}

    def table(name):
        _, f0, drift, sym, _ = by[name]
        return sl.host_table(sl.dphi(f0, drift, sym))
    # the phase crosses zero repeatedly: tens of raw steps, and exact zeros among them
    for name in ("zero_rand", "tiny_rand"):
        tb = table(name)
        r = tb.runs[:tb.nr]
        assert (r["e"] == raw).sum() >= 20 and np.any((r["e"] == raw) & (r["m0"] == 0))
    # the non-finite walk: Inf from about sample 200 on, no NaN
    _, f0, drift, sym, _ = by["f1e38"]
    walk = sl.serial_walk(sl.dphi(f0, drift, sym))[0]
    assert np.isposinf(walk[-1]) and not np.isnan(walk).any() and 100 < np.isfinite(walk).sum() < 400
    # symbols above 3 take part in the increment as their value
    _, f0, drift, sym, _ = by["sym255"]
    assert sym.max() > 200 and float(sl.dphi(f0, drift, sym).max()) > 3.0
    # K = 40: the table fills inside the constant-tone chain (one run per symbol at its end), K = 38 fits with 11 to spare
    wide = sl.serial_walk(sl.dphi(0.0, 0.0, by["k40_tail3"][3]), 4096)[1]
    assert wide - sl.MAXRUNS < sl.NSYM - 40
    assert by["exact_fit"][4] == sl.MAXRUNS
    assert [by[n][4] for n in sl.MIXED] == [178, -1, 180, -1, 501]


def test_edge_cases_touch_what_they_say():
    seen = set()
    for name, np_, shift, touches in sl.edge_cases():
        n = np.arange(sl.NSIG)
        k = shift + n
        hit = n[(k > 0) & (k < np_)]
        assert (hit.size > 0) == touches, name
        assert 1 <= np_ <= sl.NS
        if name.startswith("first_"):
            assert k[hit[0]] == 1
            seen.add(("first", int(hit[0]) // sl.TILE, int(hit[0]) % sl.TILE))
        if name.startswith("last_"):
            assert k[hit[-1]] == np_ - 1 and hit[0] == 0
            seen.add(("last", int(hit[-1]) // sl.TILE, int(hit[-1]) % sl.TILE))
        if name in ("np2", "last_sample", "one_in_last_tile"):
            assert hit.size == 1
    # both sides of a tile boundary and of the 180-sample halo, in an even and an odd tile
    for which in ("first", "last"):
        for t in (1, 2):
            assert {(which, t - 1, sl.TILE - 181), (which, t - 1, sl.TILE - 180), (which, t - 1, sl.TILE - 1), (which, t, 0),
                    (which, t, 1), (which, t, 179), (which, t, 180)} <= seen
    assert -41470 + (sl.NSIG - 1) == 1 and (sl.NSIG - 1) // sl.TILE == sl.NTILES - 1 and sl.NSIG - (sl.NTILES - 1) * sl.TILE == 512
