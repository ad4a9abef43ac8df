"""Crafted spectrograms for K2 (time average, peak picker) and K3 (coarse sync), shared by tests/test_k2k3_cases_cpu.py
(which proves every case's condition with the oracle) and tests/test_gpu_k2k3_ps.py (which sends the cases through
wspr_stage_candidates_ps()).  A case is a spectrogram in the oracle's layout [nseg][512][blocks], with candidate lists
where the picker is skipped; every case is deterministic from its seed.  Also here: the all-hypotheses restatement of
the coarse sync (tests/helpers/k3_all_check.c) behind ctypes.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os
import subprocess
import tempfile
import types

import numpy as np

import oracle_lib as ol

BLOCKS = 347
NSYM = 162
HALF_DF = 375.0 / 256.0 / 2.0
IF0_LO, IF0_HI = 106, 406                  # smoothed bins 55 .. 355: what the picker's +-110 Hz window keeps
PLANT = 36.0                               # added to exponential noise of mean 1
MIN_SNR = np.float32(10.0 ** -0.8)


def freq_of(if0):
    return np.float32((if0 - 256) * HALF_DF)


def if0_of(freq):
    return int(float(np.float32(freq)) / HALF_DF + 256.0)


assert all(if0_of(freq_of(i)) == i for i in range(IF0_LO - 1, IF0_HI + 2))


def sync_vector():
    return np.frombuffer((C.c_ubyte * NSYM).in_dll(ol.lib(), "orc_sync_vector"), dtype=np.uint8).astype(np.int64)


# ------------------------------------------------------------------------------------------- the all-hypotheses helper
@functools.lru_cache(maxsize=None)
def helper():
    ol.lib()
    out = os.path.join(tempfile.mkdtemp(prefix="wspr_k3all_"), "libk3all.so")
    subprocess.run(["gcc", "-O2", "-std=gnu17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", ol.ORACLE_DIR,
                    "-shared", "-o", out, os.path.join(ol.ROOT, "tests", "helpers", "k3_all_check.c"), "-L", ol.ORACLE_DIR,
                    "-loracle", "-Wl,-rpath," + ol.ORACLE_DIR, "-lm"], check=True)
    X = C.CDLL(out)
    X.k3_all.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    X.k3_all.restype = C.c_int
    return X


def all_hypotheses(ps_seg, blocks, freq, maxdrift):
    """(table, inside) [3 bins][32 lags][2 maxdrift + 1] of one candidate: the sync the reference compares with `best` at
    every hypothesis, and how many symbols lay inside the record."""
    nd = 2 * maxdrift + 1
    table = np.zeros((3, 32, nd), np.float32)
    inside = np.zeros((3, 32, nd), np.int32)
    assert ps_seg.dtype == np.float32 and ps_seg.flags.c_contiguous and ps_seg.shape == (512, blocks)
    helper().k3_all(ol.ptr(ps_seg), blocks, float(freq), maxdrift, ol.ptr(table), ol.ptr(inside))
    return table, inside


def first_maximum(table, freq, maxdrift):
    """The first strict maximum of a table in loop order, as (freq, shift, drift, sync): what `sync > best` keeps."""
    assert not np.isnan(table).any() and table.max() > -1e30
    f, lag, d = np.unravel_index(int(np.argmax(table)), table.shape)          # argmax: the first of equal maxima
    return (float(freq_of(if0_of(freq) - 1 + f)), 128 * (int(lag) - 10 + 1), float(int(d) - maxdrift), float(table[f, lag, d]))


def hypothesis_of(freq0, maxdrift, freq, shift, drift):
    """(bin 0..2, lag 0..31, pattern) of a coarse-sync result for the candidate that started at freq0; pattern 0 = the
    drifts < 0 (all alike: the reference labels them -maxdrift), 1 = no drift, 2 = the drifts > 0 (labelled 1)."""
    b = if0_of(freq) - if0_of(freq0) + 1
    pat = 1 if drift == 0 else (0 if drift < 0 else 2)
    if drift != 0:
        assert drift == (-maxdrift if drift < 0 else 1)
    return b, shift // 128 - 1 + 10, pat


# --------------------------------------------------------------------------------------------------------- the oracle
def oracle_coarse(ps_seg, blocks, freqs, maxdrift):
    """orc_coarse_sync on a list of picker-fresh candidates: [(freq, shift, drift, sync)]."""
    n = len(freqs)
    cands = (ol.Cand * 200)()
    for j in range(n):
        cands[j].freq = float(freqs[j])
    ol.lib().orc_coarse_sync(ol.ptr(ps_seg), C.c_int(blocks), cands, C.c_int(n), C.c_int(maxdrift))
    return [(cands[j].freq, cands[j].shift, cands[j].drift, cands[j].sync) for j in range(n)]


def oracle_peaks(ps_seg, blocks, coarse=0, maxdrift=4):
    """orc_pick_peaks (+ orc_coarse_sync): npk, [(freq, snr, shift, drift, sync)], noise, smspec, normalised smspec."""
    cands = (ol.Cand * 200)()
    noise = C.c_float()
    sm = np.zeros(411, np.float32)
    nrm = np.zeros(411, np.float32)
    L = ol.lib()
    npk = L.orc_pick_peaks(ol.ptr(ps_seg), C.c_int(blocks), cands, C.byref(noise), ol.ptr(sm), ol.ptr(nrm))
    if coarse:
        L.orc_coarse_sync(ol.ptr(ps_seg), C.c_int(blocks), cands, C.c_int(npk), C.c_int(maxdrift))
    return npk, [(c.freq, c.snr, c.shift, c.drift, c.sync) for c in cands[:npk]], np.float32(noise.value), sm, nrm


# ---------------------------------------------------------------------------------------------------------- K3 cases
def k3_case(name, ps, maxdrift, freqs, plants=None, active=None):
    """freqs: per segment, the candidates' frequencies.  plants: {(segment, candidate): (bin, lag, pattern)}."""
    nseg, _, blocks = ps.shape
    fr = np.zeros((nseg, 200), np.float32)
    cnt = np.zeros(nseg, np.int32)
    for s, f in enumerate(freqs):
        cnt[s] = len(f)
        fr[s, :len(f)] = f
    return types.SimpleNamespace(name=name, ps=np.ascontiguousarray(ps, np.float32), blocks=blocks, maxdrift=maxdrift,
                                 freqs=fr, counts=cnt, plants=plants or {}, active=active)


@functools.lru_cache(maxsize=None)
def _expected_k3(case_fn, *args):
    case = case_fn(*args)
    return [oracle_coarse(case.ps[s], case.blocks, case.freqs[s, :case.counts[s]], case.maxdrift)
            for s in range(case.ps.shape[0])]


def expected_k3(case_fn, *args):
    """The oracle's result for every candidate of a case (computed once per process)."""
    return _expected_k3(case_fn, *args)


def noise(rng, nseg, blocks=BLOCKS):
    return rng.exponential(1.0, (nseg, 512, blocks)).astype(np.float32)


def plant(ps_seg, if0, b, lag, pat, amount=PLANT):
    """Add `amount` to the two tone rows the sync vector favours at every symbol of hypothesis (bin b, lag, pattern) of a
    candidate at if0, with the reference's addressing: the drifting patterns read one bin lower after (pattern 0) or
    before (pattern 2) symbol 81, and a negative time index lies in the previous row of the flat array."""
    blocks = ps_seg.shape[1]
    pr3 = sync_vector()
    k = np.arange(NSYM)
    ifr = if0 - 1 + b
    ifd = {0: np.where(k > 81, ifr - 1, ifr), 1: np.full(NSYM, ifr), 2: np.where(k < 81, ifr - 1, ifr)}[pat]
    kidx = lag - 10 + 2 * k
    m = kidx < blocks
    flat = ps_seg.reshape(-1)
    for row in (np.where(pr3 == 1, ifd - 1, ifd - 3), np.where(pr3 == 1, ifd + 3, ifd + 1)):
        flat[(row * blocks + kidx)[m]] += np.float32(amount)
    return int(m.sum())


SLOT_IF0 = list(range(IF0_LO, IF0_HI + 1, 12))          # 26 candidates a segment: their eleven rows never meet
assert SLOT_IF0[-1] == IF0_HI


def _planted(name, hyps, maxdrift, blocks, seed):
    rng = np.random.default_rng(seed)
    hyps = [hyps[i] for i in rng.permutation(len(hyps))]
    nseg = -(-len(hyps) // len(SLOT_IF0))
    ps = noise(rng, nseg, blocks)
    freqs = [[] for _ in range(nseg)]
    plants = {}
    for i, h in enumerate(hyps):
        s, j = divmod(i, len(SLOT_IF0))
        plant(ps[s], SLOT_IF0[j], *h)
        freqs[s].append(freq_of(SLOT_IF0[j]))
        plants[(s, j)] = h
    return k3_case(name, ps, maxdrift, freqs, plants)


@functools.lru_cache(maxsize=None)
def planted_winners(maxdrift):
    """One plant per (bin, lag, pattern): 288 with a drift search, 96 without, on candidates from bin 55 to bin 355."""
    pats = (0, 1, 2) if maxdrift else (1,)
    hyps = [(b, lag, p) for b in range(3) for lag in range(32) for p in pats]
    return _planted("planted/maxdrift%d" % maxdrift, hyps, maxdrift, BLOCKS, 100 + maxdrift)


SHORT_BLOCKS = (7, 15, 31, 163, 343)


@functools.lru_cache(maxsize=None)
def short_record(blocks):
    """A short record: plants at every lag that still has a symbol inside (lag index - 10 < blocks), all three bins and
    patterns, maxdrift 4."""
    hyps = [(b, lag, p) for b in range(3) for lag in range(32) if lag - 10 < blocks for p in (0, 1, 2)]
    return _planted("short/blocks%d" % blocks, hyps, 4, blocks, 200 + blocks)


NO_PLANT_COUNTS = (0, 1, 2, 3, 31, 32, 33, 34, 199, 200)


@functools.lru_cache(maxsize=None)
def no_plant():
    rng = np.random.default_rng(31)
    ps = noise(rng, len(NO_PLANT_COUNTS))
    freqs = [[freq_of(i) for i in rng.integers(IF0_LO, IF0_HI + 1, n)] for n in NO_PLANT_COUNTS]
    return k3_case("no plant", ps, 4, freqs)


@functools.lru_cache(maxsize=None)
def active_list(order):
    """Seven noise segments of three candidates; `order`: the active list."""
    rng = np.random.default_rng(32)
    ps = noise(rng, 7)
    freqs = [[freq_of(i) for i in rng.integers(IF0_LO, IF0_HI + 1, 3)] for _ in range(7)]
    return k3_case("active %s" % (order,), ps, 4, freqs, active=list(order))


ACTIVE_ORDERS = ((5, 0, 3), (6, 5, 4, 3, 2, 1, 0))


def _tie_b_segment(ps_seg, if0):
    """Uniform 1 except row if0 - 4, lowered to 1/4 (amplitude 1/2) in the columns no negative time index reaches
    (0 .. 336).  Only bin if0 - 1 (all patterns) and the drifting patterns of bin if0 read that row, as tone 0: their
    sums are half the sum of the sync signs over the symbols that read it, and the sync vector holds more zeros than ones
    in every such stretch, so they are all negative; every other hypothesis stays 0."""
    ps_seg[if0 - 4, :337] = 0.25


@functools.lru_cache(maxsize=None)
def ties():
    """Segment 0: uniform (every hypothesis 0).  Segment 1: uniform except for rows that make the first bin's hypotheses
    negative.  Segments 2..: rows constant in time with random levels, at candidates whose oracle winner has lag 0 (all
    lags >= 0 of a bin and pattern are then bit-equal)."""
    ps = np.ones((2 + len(TIE_C), 512, BLOCKS), np.float32)
    freqs = [[freq_of(i) for i in (IF0_LO, 256, IF0_HI)], [freq_of(i) for i in (IF0_LO, 250, IF0_HI)]]
    for i in (IF0_LO, 250, IF0_HI):
        _tie_b_segment(ps[1], i)
    for n, (seed, if0s) in enumerate(TIE_C):
        ps[2 + n] = tie_c_segment(seed)
        freqs.append([freq_of(i) for i in if0s])
    return k3_case("ties", ps, 4, freqs)


def tie_c_segment(seed):
    rng = np.random.default_rng(seed)
    return np.repeat(rng.exponential(1.0, (512, 1)).astype(np.float32), BLOCKS, axis=1)


# (seed, the slots of SLOT_IF0 whose oracle winner has lag 0): the first four that tie_c_search(range(60)) finds on the
# CPU (31 of the 60 seeds have such a slot, 41 of their 1 560 candidates)
TIE_C = ((0, (346,)), (1, (286,)), (7, (286,)), (8, (190,)))


def tie_c_search(seeds):
    out = []
    for seed in seeds:
        seg = tie_c_segment(seed)
        keep = [i for i in SLOT_IF0 if oracle_coarse(seg, BLOCKS, [freq_of(i)], 4)[0][1] == 128]
        if keep:
            out.append((seed, tuple(keep)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def q2_only():
    """Uniform 1 except for a plant at the symbols with a negative time index (the previous rows' last ten columns) of one
    hypothesis per candidate: lags -10 .. -1, bins in turn, no drift."""
    ps = np.ones((1, 512, BLOCKS), np.float32)
    pr3 = sync_vector()
    freqs = []
    plants = {}
    for j in range(10):
        if0, b, lag = SLOT_IF0[2 * j], j % 3, j
        ifr = if0 - 1 + b
        flat = ps[0].reshape(-1)
        for k in range(NSYM):
            kidx = lag - 10 + 2 * k
            if kidx < 0:
                for row in ((ifr - 1, ifr + 3) if pr3[k] else (ifr - 3, ifr + 1)):
                    flat[row * BLOCKS + kidx] += np.float32(PLANT)
        freqs.append(freq_of(if0))
        plants[(0, j)] = (b, lag, 1)
    return k3_case("q2 only", ps, 4, [freqs], plants)


# ---------------------------------------------------------------------------------------------------------- K2 cases
def k2_case(name, ps, coarse=0):
    return types.SimpleNamespace(name=name, ps=np.ascontiguousarray(ps, np.float32), blocks=ps.shape[2], coarse=coarse)


@functools.lru_cache(maxsize=None)
def _expected_k2(case_fn, *args):
    case = case_fn(*args)
    return [oracle_peaks(case.ps[s], case.blocks, case.coarse) for s in range(case.ps.shape[0])]


def expected_k2(case_fn, *args):
    return _expected_k2(case_fn, *args)


TIME_AVERAGE_BLOCKS = (1, 31, 32, 33, 64, 347)


@functools.lru_cache(maxsize=None)
def time_average(blocks):
    """Two segments whose rows span 2^24 in magnitude: the serial sum of a row is not the sum in any other order."""
    rng = np.random.default_rng(300 + blocks)
    e = rng.integers(0, 25, (2, 512, blocks))
    if blocks > 1:                                   # every row holds both ends of the range
        at = rng.integers(0, blocks - 1, (2, 512, 1))
        np.put_along_axis(e, at, 0, axis=2)
        np.put_along_axis(e, at + 1, 24, axis=2)
    ps = (rng.uniform(1.0, 2.0, (2, 512, blocks)) * np.exp2(e)).astype(np.float32)
    return k2_case("time average/blocks%d" % blocks, ps)


def from_average(avg_rows):
    """Spectrograms (blocks 347) whose time averages are the given rows [nseg][512], exactly: the row's value sits in one
    column (the segment's own), zeros in all others."""
    avg_rows = np.asarray(avg_rows, np.float32)
    ps = np.zeros((avg_rows.shape[0], 512, BLOCKS), np.float32)
    for s in range(avg_rows.shape[0]):
        ps[s, :, (37 * s + 5) % BLOCKS] = avg_rows[s]
    return ps


def chain(levels=None, c=1.0):
    """A time average that is zero except at every seventh bin: every 7-bin window holds exactly one of them, so the
    smoothed spectrum is that bin's value, exactly.  levels (411, optional): the value wanted per smoothed bin (constant
    over each window run of seven); default c everywhere."""
    avg = np.zeros(512, np.float64)
    for n in range(48, 465, 7):                 # bin n lies in windows n - 54 .. n - 48
        avg[n] = c if levels is None else levels[min(max(n - 51, 0), 410)]
    return avg


def bump(avg, i0, left, right, width=1):
    """Two more bins, 7 - width apart: `width` windows hold both (a strict maximum at smoothed bin i0 for width 1, a
    plateau i0 .. i0 + width - 1 otherwise), six hold only one.  With whole numbers below 2^24 every sum is exact."""
    avg[48 + i0 + width - 1] += left
    avg[54 + i0] += right


def _avg_case(name, rows, coarse=0):
    rows = np.asarray(rows, np.float64)
    assert np.array_equal(rows.astype(np.float32).astype(np.float64), rows)
    return k2_case(name, from_average(rows), coarse)


@functools.lru_cache(maxsize=None)
def percentile():
    """Segment 0: 97 smoothed bins at 1/2, then equal values from rank 97 up across rank 122.  Segment 1: three levels,
    63 equal values around rank 122.  Segment 2: as 1 with +Inf in two places (14 windows) and a peak."""
    rows = []
    lv = np.full(411, 8.0); lv[300:397] = 4.0
    rows.append(chain(lv))
    lv = np.full(411, 16.0); lv[20:118] = 4.0; lv[200:263] = 8.0
    rows.append(chain(lv))
    a = chain(lv); a[60] = np.inf; a[440] = np.inf; bump(a, 150, 24.0, 24.0)
    rows.append(a)
    return k2_case("percentile", from_average(np.asarray(rows, np.float32)))


FLOOR_C = float(2 ** 23)
FLOOR_BELOW, FLOOR_ABOVE = 9718112.0, 9718113.0       # adjacent floats: / 2^23 - 1 = 0.15848923, 0.15848935; min_snr 0.15848932


@functools.lru_cache(maxsize=None)
def floor_and_plateaus():
    """Noise 2^23.  Peaks at bins 80 (just below min_snr: floored away), 120 (just above: kept), plateaus of two bins at
    160 and of three at 200 (no strict maximum), and one ordinary peak at 240."""
    a = chain(c=FLOOR_C)
    for i0, top in ((80, FLOOR_BELOW), (120, FLOOR_ABOVE)):
        h = float(int((top - FLOOR_C) // 2))
        bump(a, i0, h, top - FLOOR_C - h)
    bump(a, 160, FLOOR_C / 2, FLOOR_C / 2, width=2)
    bump(a, 200, FLOOR_C / 2, FLOOR_C / 2, width=3)
    bump(a, 240, FLOOR_C / 2, FLOOR_C / 2)
    return _avg_case("floor and plateaus", [a])


@functools.lru_cache(maxsize=None)
def densest():
    """avg[i + 7] = avg[i] +- 8 by the parity of i: the smoothed spectrum alternates between two levels, every other bin
    is a strict maximum.  Through the coarse sync as well: 151 candidates, 76 pairs, five rounds of the pair loop."""
    a = np.zeros(512, np.float64)
    for n in range(41, 512):
        a[n] = 4.0 if n < 48 else a[n - 7] + (8.0 if (n - 7) % 2 == 0 else -8.0)
    a[:41] = 4.0
    return _avg_case("densest", [a], coarse=1)


ULP_K = tuple(4 + (19 * i + 7) // 15 for i in range(16))          # noise 2^k, k = 4 .. 23
assert ULP_K[0] == 4 and ULP_K[-1] == 23


@functools.lru_cache(maxsize=None)
def ulp_pairs():
    """64 pairs of peaks whose smoothed values are adjacent floats (T and T + 1 in [2^23, 2^24)), the lower one at the
    lower bin, four pairs a segment; the segment's noise 2^k sets the scale: normalised peaks from min_snr to 10^6."""
    rng = np.random.default_rng(64)
    rows = []
    for k in ULP_K:
        c = float(2 ** k)
        a = chain(c=c)
        lo = FLOOR_ABOVE + 1 if k == 23 else float(2 ** 23)        # k = 23: stay above min_snr
        for p in range(4):
            top = float(rng.integers(int(lo), 2 ** 24 - 2))
            h = float(int((top - c) // 2))
            bump(a, 62 + 56 * p, h, top - c - h)
            bump(a, 62 + 56 * p + 28, h, top + 1.0 - c - h)
        rows.append(a)
    return _avg_case("ulp pairs", rows)


@functools.lru_cache(maxsize=None)
def edge_bins():
    """Segment 0: peaks at smoothed bins 55 and 355 (the window's last bins inside).  Segment 1: at 54 and 356 (outside)."""
    rows = []
    for bins in ((55, 355), (54, 356)):
        a = chain(c=8.0)
        for i0 in bins:
            bump(a, i0, 16.0, 16.0)
        rows.append(a)
    return _avg_case("edge bins", rows, coarse=1)


@functools.lru_cache(maxsize=None)
def zero_and_one():
    a = chain(c=8.0)
    bump(a, 205, 16.0, 16.0)
    return _avg_case("zero and one peak", [chain(c=8.0), a], coarse=1)


K2_CASES = [(time_average, b) for b in TIME_AVERAGE_BLOCKS] + [(percentile,), (floor_and_plateaus,), (densest,),
                                                               (ulp_pairs,), (edge_bins,), (zero_and_one,)]
