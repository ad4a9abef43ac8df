"""K2 (time average, peak picker) and K3 (coarse sync, both kernels) on the crafted spectrograms of tests/k2k3_lib.py,
through wspr_stage_candidates_ps() of the lab library: every figure equals the oracle's bit for bit, in both arithmetic
modes (K2/K3 hold no contraction site).  The hook fills what the device layout leaves undefined with NaN, so a kernel
that reads a pitch column, or a column behind a short record, cannot agree.  What each case is FOR -- which hypothesis
wins, which values tie, what the picker keeps -- is proved on the CPU in tests/test_k2k3_cases_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import k2k3_lib as kl
import oracle_lib as ol

pytestmark = pytest.mark.gpu

CAND = np.dtype([("freq", "<f4"), ("snr", "<f4"), ("shift", "<i4"), ("drift", "<f4"), ("sync", "<f4")])
assert CAND.itemsize == 20


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    assert C.sizeof(mod.cand) == CAND.itemsize
    yield mod
    mod.wspr_set_arithmetic(mod.WSPR_ARITH_EXACT, mod.lab())


def stage(w, ps, coarse, maxdrift, active=None, freqs=None, counts=None, kernel=0, arith=0):
    """One call of the hook: (npk [nseg], cands [nseg][200], noise [nseg], smspec [nseg][411])."""
    L = w.lab()
    nseg, _, blocks = ps.shape
    assert ps.dtype == np.float32 and ps.flags.c_contiguous
    cands = np.zeros((nseg, 200), CAND)
    npk = np.zeros(nseg, np.int32)
    noise = np.zeros(nseg, np.float32)
    sm = np.zeros((nseg, 411), np.float32)
    act = None if active is None else np.ascontiguousarray(active, np.int32)
    assert w.wspr_set_arithmetic(arith, L) == 0
    try:
        rc = L.wspr_stage_candidates_ps(ol.ptr(ps), nseg, blocks, coarse, maxdrift, None if act is None else ol.ptr(act),
                                        0 if act is None else act.size, None if freqs is None else ol.ptr(freqs),
                                        None if counts is None else ol.ptr(counts), kernel, ol.ptr(cands), ol.ptr(npk),
                                        ol.ptr(noise), ol.ptr(sm))
    finally:
        w.wspr_set_arithmetic(0, L)
    assert rc == 0
    return npk, cands, noise, sm


def both_modes(w, *args, **kw):
    """The call in the exact and in the contracted arithmetic: identical words; the exact one's result."""
    a = stage(w, *args, arith=0, **kw)
    b = stage(w, *args, arith=1, **kw)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    return a


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def check_k3(case, exp, got, segments=None):
    """Candidates of the listed segments (default: all) against the oracle; any other segment as the hook set it."""
    npk, cands, noise, sm = got
    nseg = case.ps.shape[0]
    done = set(range(nseg) if segments is None else segments)
    assert np.array_equal(npk, case.counts)
    assert np.isnan(noise).all() and np.isnan(sm).all()          # the picker did not run
    for s in range(nseg):
        n = case.counts[s]
        g = cands[s, :n]
        if s in done:
            e = np.array([(f, 0, sh, dr, sy) for f, sh, dr, sy in exp[s]], CAND) if n else np.zeros(0, CAND)
        else:
            e = np.zeros(n, CAND)
            e["freq"] = case.freqs[s, :n]
        for field in ("freq", "drift", "sync"):
            assert np.array_equal(bits(g[field]), bits(e[field])), (case.name, s, field, g[field], e[field])
        assert np.array_equal(g["shift"], e["shift"]), (case.name, s)
        assert not cands[s, n:].view(np.uint32).any()


def run_k3(w, case_fn, *args, kernels=(1, 2)):
    case = case_fn(*args)
    exp = kl.expected_k3(case_fn, *args)
    for kernel in kernels:
        got = both_modes(w, case.ps, 1, case.maxdrift, active=case.active, freqs=case.freqs, counts=case.counts, kernel=kernel)
        check_k3(case, exp, got, case.active)


# ------------------------------------------------------------------------------------------------------------------ K3
@pytest.mark.parametrize("maxdrift", [4, 1, 0])
def test_every_planted_hypothesis_wins_on_both_kernels(w, maxdrift):
    """288 / 288 / 96 plants, one per (bin, lag, drift pattern): every running sum of both kernels is the winner once,
    lags -10 .. -1 (the previous bin's row) and candidates on both band edges (rows 100 and 410) included."""
    run_k3(w, kl.planted_winners, maxdrift)


@pytest.mark.parametrize("blocks", kl.SHORT_BLOCKS)
def test_short_records_with_plants(w, blocks):
    """coarse_sync_kernel<false>: symbols behind the record masked, lags without any symbol never win; the lane selector
    falls back to it.  Records of fewer than ten blocks reach more than one row back with a negative time index."""
    run_k3(w, kl.short_record, blocks, kernels=(0, 1, 2))


def test_list_lengths_without_a_plant(w):
    """0, 1, 2, 3 (the last pair's second half idles), 31 .. 34 (the pair loop's second round starts at 33) and 199, 200."""
    run_k3(w, kl.no_plant)


def test_ties_keep_the_first_hypothesis(w):
    run_k3(w, kl.ties)


def test_energy_only_behind_a_negative_time_index(w):
    run_k3(w, kl.q2_only)


@pytest.mark.parametrize("order", kl.ACTIVE_ORDERS)
def test_active_segment_lists(w, order):
    """A device segment list, as every pass after the first passes one: the listed segments in the list's order, the
    others untouched."""
    run_k3(w, kl.active_list, order)


def test_large_batch_takes_the_product_choice(w):
    """1 540 segments (the no-plant segments tiled) with selector 0: the product's own choice, the lane kernel."""
    case = kl.no_plant()
    exp = kl.expected_k3(kl.no_plant)
    n0 = case.ps.shape[0]
    reps = -(-1536 // n0)
    ps = np.tile(case.ps, (reps, 1, 1))
    freqs = np.tile(case.freqs, (reps, 1))
    counts = np.tile(case.counts, reps)
    assert ps.shape[0] >= 1536
    npk, cands, noise, sm = stage(w, ps, 1, 4, freqs=freqs, counts=counts, kernel=0)
    assert np.array_equal(npk, counts)
    first = cands[:n0]
    assert all(cands[r * n0:(r + 1) * n0].tobytes() == first.tobytes() for r in range(1, reps))
    check_k3(case, exp, (npk[:n0], first, noise[:n0], sm[:n0]))


# ------------------------------------------------------------------------------------------------------------------ K2
def check_k2(case, exp, got, segments=None):
    npk, cands, noise, sm = got
    nseg = case.ps.shape[0]
    done = set(range(nseg) if segments is None else segments)
    for s in range(nseg):
        if s not in done:
            assert npk[s] == 0 and np.isnan(noise[s]) and np.isnan(sm[s]).all() and not cands[s].view(np.uint32).any()
            continue
        onpk, oc, onoise, osm, _ = exp[s]
        assert npk[s] == onpk, (case.name, s, npk[s], onpk)
        assert bits(noise[s]) == bits(onoise), (case.name, s)
        assert np.array_equal(bits(sm[s]), bits(osm)), (case.name, s)
        e = np.array(oc, CAND) if onpk else np.zeros(0, CAND)
        g = cands[s, :onpk]
        for field in ("freq", "snr", "drift", "sync"):
            assert np.array_equal(bits(g[field]), bits(e[field])), (case.name, s, field, g[field], e[field])
        assert np.array_equal(g["shift"], e["shift"]), (case.name, s)
        assert not cands[s, onpk:].view(np.uint32).any()


@pytest.mark.parametrize("case_fn", kl.K2_CASES, ids=lambda c: c[0].__name__ + "".join("-%s" % (a,) for a in c[1:]))
def test_picker_cases(w, case_fn):
    """Time average (serial sums of rows spanning 2^24), percentile with ties and infinities, the floor at min_snr and
    plateaus, the densest list (151 kept, the cap of 200 fires), peaks one ulp apart (host re-rank), the band's edge
    bins, empty and single lists -- and, where the case asks for it, the coarse sync on the picker's own list."""
    case = case_fn[0](*case_fn[1:])
    exp = kl.expected_k2(*case_fn)
    kernels = (0, 1, 2) if case.coarse else (0,)
    for kernel in kernels:
        check_k2(case, exp, both_modes(w, case.ps, case.coarse, 4, kernel=kernel))
    nseg = case.ps.shape[0]
    if nseg > 1:                                                  # the same through a segment list, last segment left out
        order = list(range(nseg - 2, -1, -1))
        check_k2(case, exp, both_modes(w, case.ps, case.coarse, 4, active=order), order)


def test_arguments_out_of_range_are_refused(w, capfd):
    case = kl.active_list(kl.ACTIVE_ORDERS[0])
    L = w.lab()
    out = (np.zeros((7, 200), CAND), np.zeros(7, np.int32))
    args = lambda **k: [k.get("ps", ol.ptr(case.ps)), 7, k.get("blocks", 347), 1, 4, k.get("active"), k.get("nactive", 0),
                        ol.ptr(k.get("freqs", case.freqs)), ol.ptr(k.get("counts", case.counts)), k.get("kernel", 0),
                        ol.ptr(out[0]), ol.ptr(out[1]), None, None]
    low = case.freqs.copy(); low[0, 0] = kl.freq_of(105)
    high = case.freqs.copy(); high[6, 2] = kl.freq_of(407)
    many = case.counts.copy(); many[3] = 201
    far = np.array([7], np.int32)
    for bad in (dict(blocks=0), dict(blocks=348), dict(kernel=3), dict(freqs=low), dict(freqs=high), dict(counts=many),
                dict(active=ol.ptr(far), nactive=1)):
        assert L.wspr_stage_candidates_ps(*args(**bad)) == -1, bad
    capfd.readouterr()
    assert L.wspr_stage_candidates_ps(*args()) == 0
