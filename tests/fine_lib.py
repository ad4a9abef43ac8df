"""CPU side of tests/test_gpu_fine.py and tests/test_fine_cases_cpu.py: the crafted cases of the production fine search
(k4_demod.hip: mode 0 with and without drift, mode 1 with the first rung, the 43 lags of the jitter ladder), the case / output
files of tools/fine_check.hip, and the three exact references every dumped value is held to as bits:
 (a) ONE hypothesis at a time (lagmin == lagmax, ifmin == ifmax) through the oracle's orc_sync_demod (exact mode) or the
     CONTRACT=1 checker's ctr_sync_demod (contracted mode);
 (b) the chain: the same entries over the full ranges in the reference's order (mode 0 over the lag grid, mode 1 over -2 .. 2
     at 0.1, mode 2 at shift - 63 + 3 r);
 (c) the rms of a soft-symbol vector, restated from the caller's code in orc_dsp.c.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os
import subprocess
import types

import numpy as np

import lag_audit_lib as la
import oracle_lib as ol
from lag_audit_lib import FINE, KIQ, SENTINEL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = 45000
NSYM = 162
SPAN = 256 * NSYM                  # samples one hypothesis' windows cover: k = lag .. lag + SPAN - 1
NRUNG = 43                         # the ladder's lags shift - 63 + 3 r
MINSYNC1 = np.float32(0.10)        # the product's (wspr_pipeline.hip; wsprd.c:733)
MINUS_1E30 = np.float32(-1e30)
MINUS_3E38 = np.float32(-3.0e38)   # what the pruned scan leaves in the sync of a lag it did not sum
RUN_MODE0, PRUNE, HAND, LADDER = 1, 2, 4, 8
WHOLE_CHAIN = RUN_MODE0 | PRUNE | HAND | LADDER


def same_bits(a, b):
    return np.ascontiguousarray(a).view(np.uint8).tobytes() == np.ascontiguousarray(b).view(np.uint8).tobytes()


def bits(x):
    return int(np.asarray(x, np.float32).reshape(1).view(np.uint32)[0])


class Rec:
    """One record: I, Q as rows of kIqStride floats (the samples from np on exist in memory and are never read)."""
    _next = 0

    def __init__(self, I, Q):
        self.I, self.Q = np.zeros(KIQ, np.float32), np.zeros(KIQ, np.float32)
        self.I[:len(I)], self.Q[:len(Q)] = I, Q
        self.uid = Rec._next
        Rec._next += 1


# ---- the references ----------------------------------------------------------------------------------------------------------
def _entry(arith):
    if arith:
        import contract_lib
        return contract_lib.contract(1).ctr_sync_demod
    return ol.lib().orc_sync_demod


def _call(arith, rec, npts, freq, drift, shift, ifmin, ifmax, lagmin, lagmax, lagstep, mode):
    f, sh, dr, sy = C.c_float(freq), C.c_int(shift), C.c_float(drift), C.c_float(0.0)
    sym = (C.c_ubyte * NSYM)()
    _entry(arith)(ol.ptr(rec.I), ol.ptr(rec.Q), C.c_long(npts), sym, C.addressof(f), ifmin, ifmax, C.c_float(0.1),
                  C.addressof(sh), lagmin, lagmax, lagstep, C.addressof(dr), 50, C.addressof(sy), mode)
    return np.float32(f.value), int(sh.value), np.float32(sy.value), np.frombuffer(sym, np.uint8).copy()


_memo = {}
calls = [0]                        # reference calls made (the tests print it)


def _memoised(key, make):
    if key not in _memo:
        calls[0] += 1
        _memo[key] = make()
    return _memo[key]


def lag_sync(arith, rec, npts, freq, drift, lag):
    """(a), mode 0: the sync of the single lag, as the entry returns it (its maximum from -1e30 under a strict >)."""
    return _memoised((0, arith, rec.uid, npts, bits(freq), bits(drift), lag),
                     lambda: _call(arith, rec, npts, freq, drift, 0, 0, 0, lag, lag, 8, 0)[2])


def freq_sync(arith, rec, npts, freq, drift, shift, ifreq):
    """(a), mode 1: the sync of the single hypothesis freq + ifreq * 0.1 at shift."""
    return _memoised((1, arith, rec.uid, npts, bits(freq), bits(drift), shift, ifreq),
                     lambda: _call(arith, rec, npts, freq, drift, shift, ifreq, ifreq, 0, 0, 8, 1)[2])


def rms_of(sym):
    """(c): orc_dsp.c's caller -- sq += y * y over y = (float)symbols[i] - 128.0, then sqrtf(sq / 162) -- in float32."""
    sq = np.float32(0.0)
    for v in sym:
        y = np.float32(np.float64(np.float32(v)) - 128.0)
        sq = np.float32(sq + np.float32(y * y))
    return np.sqrt(np.float32(sq / np.float32(NSYM)), dtype=np.float32)


def rung(arith, rec, npts, freq, drift, lag):
    """(a) + (c), mode 2 at (freq, lag): (sync, symbols[162], rms)."""
    def make():
        _, _, sy, sym = _call(arith, rec, npts, freq, drift, lag, -2, 2, 0, 0, 8, 2)
        return sy, sym, rms_of(sym)
    return _memoised((2, arith, rec.uid, npts, bits(freq), bits(drift), lag), make)


def chain_mode0(arith, rec, npts, fc, drift, sc, lagstep):
    """(b), mode 0 over sc - 128 .. sc + 128: (freq, shift, sync) as the reference leaves them."""
    return _memoised((10, arith, rec.uid, npts, bits(fc), bits(drift), sc, lagstep),
                     lambda: _call(arith, rec, npts, fc, drift, sc, 0, 0, sc - 128, sc + 128, lagstep, 0)[:3])


def chain_mode1(arith, rec, npts, freq, drift, shift):
    """(b), mode 1 over -2 .. 2 at 0.1 from the state mode 0 left: (freq, shift, sync)."""
    return _memoised((11, arith, rec.uid, npts, bits(freq), bits(drift), shift),
                     lambda: _call(arith, rec, npts, freq, drift, shift, -2, 2, 0, 0, 8, 1)[:3])


def through_max(v):
    """What the reference's entry returns for a single hypothesis whose ss / totp is v: its maximum from -1e30 under a strict >
    (wsprd.c:227-232) -- v itself, or -1e30 where v is NaN or not above it."""
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        return np.where(v > MINUS_1E30, v, MINUS_1E30).astype(np.float32)


def fold(rows, pr3):
    """sync_metric() of demod_math.h in float32 over amplitude rows [n][162][4]: totp = totp + p0 + p1 + p2 + p3,
    cmet = (p1 + p3) - (p0 + p2), ss +- cmet by the sync bit, ss / totp.  No contraction site."""
    rows = np.asarray(rows, np.float32)
    ss, totp = np.zeros(rows.shape[0], np.float32), np.zeros(rows.shape[0], np.float32)
    with np.errstate(all="ignore"):
        for k in range(NSYM):
            p0, p1, p2, p3 = (rows[:, k, t] for t in range(4))
            totp = (((totp + p0) + p1) + p2) + p3
            cmet = (p1 + p3) - (p0 + p2)
            ss = ss + cmet if pr3[k] == 1 else ss - cmet
        return (ss / totp).astype(np.float32)


# ---- tools/fine_check.hip: case file in, dump out ---------------------------------------------------------------------------------
def tool():
    exe = os.path.join(ROOT, "tools", "fine_check.bin")
    src = os.path.join(ROOT, "tools", "fine_check.hip")
    kern = os.path.join(ROOT, "rtlsdr-wsprd_amd", "csrc", "kernels")
    newest = max(os.path.getmtime(p) for p in (src, os.path.join(kern, "k4_demod.hip"), os.path.join(kern, "k4_lag_prune.h"),
                                               os.path.join(kern, "wspr_device.h"), os.path.join(kern, "demod_math.h")))
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-fno-fast-math", "-I", kern, src, "-o", exe], check=True, capture_output=True)
    return exe


def items_of(cands):
    """FineState records of (seg, fc, sc, drift) tuples: the state a wave starts from."""
    it = np.zeros(len(cands), FINE)
    for i, (seg, fc, sc, drift) in enumerate(cands):
        it[i] = (seg, fc, drift, sc, 0.0, sc, fc, 0)
    return it


def run_of(items, npts=NS, arith=0, lagstep=8, flags=WHOLE_CHAIN, minsync1=MINSYNC1):
    return dict(np=npts, arith=arith, lagstep=lagstep, nlag=256 // lagstep + 1, flags=flags, minsync1=np.float32(minsync1),
                items=items)


def write_case(path, recs, runs):
    with open(path, "wb") as fh:
        fh.write(np.array([0x31434E46, len(recs), len(runs)], "<i4").tobytes())
        fh.write(la.pr3().tobytes() + b"\0\0")
        fh.write(np.stack([r.I for r in recs]).tobytes() + np.stack([r.Q for r in recs]).tobytes())
        for r in runs:
            assert r["items"]["seg"].max() < len(recs) and len(r["items"]) <= 64
            fh.write(np.array([r["np"], r["arith"], r["lagstep"], r["nlag"], r["flags"], len(r["items"])], "<i4").tobytes())
            fh.write(np.float32(r["minsync1"]).tobytes() + r["items"].tobytes())


def run_tool(tmpdir, recs, runs):
    """One run of the tool over `runs` (run_of() dicts) on the records `recs`; one namespace per run with the dumped buffers.
    A non-zero exit fails here, and nothing more is run."""
    case, out = os.path.join(str(tmpdir), "case.bin"), os.path.join(str(tmpdir), "out.bin")
    write_case(case, recs, runs)
    p = subprocess.run([tool(), case, out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-1000:], p.stderr[-2000:])
    buf = open(out, "rb").read()
    res, o = [], 0

    def take(dtype, count, shape=None):
        nonlocal o
        a = np.frombuffer(buf, dtype, count, o).copy()
        o += a.nbytes
        return a.reshape(shape) if shape else a
    for r in runs:
        n, ns, no, nlag = (int(v) for v in take("<i4", 4))
        assert (n, nlag) == (len(r["items"]), r["nlag"])
        g = types.SimpleNamespace(n=n, n_shared=ns, n_own=no, nlag=nlag, **{k: r[k] for k in ("np", "arith", "lagstep", "flags", "minsync1")})
        g.list_shared, g.list_own = take("<i4", ns).tolist(), take("<i4", no).tolist()
        g.items_in, g.items_m0, g.items_m1, g.items_ladder = (take(FINE, n) for _ in range(4))
        g.sync0 = take("<f4", n * nlag, (n, nlag))
        g.mask = take("<u8", n)
        g.pw0 = take("<f4", n * nlag * NSYM * 4, (n, nlag, NSYM, 4))
        g.pwf = take("<f4", n * 5 * NSYM * 4, (n, 5, NSYM, 4))
        g.sync_r0, g.rms_r0, g.sym_r0 = take("<f4", n), take("<f4", n), take(np.uint8, n * NSYM, (n, NSYM))
        g.sync_l, g.rms_l = take("<f4", n * NRUNG, (n, NRUNG)), take("<f4", n * NRUNG, (n, NRUNG))
        g.sym_l = take(np.uint8, n * NRUNG * NSYM, (n, NRUNG, NSYM))
        res.append(g)
    assert o == len(buf)
    os.remove(case)
    os.remove(out)
    return res


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENTINEL).all())


# ---- the assertions: one dumped run against the references -------------------------------------------------------------------------
def check_run(g, recs):
    """Holds every value of one run's dump to (a), (b) and (c) as bits.  Returns counts of what was compared."""
    pr3 = la.pr3()
    a, npts, step = g.arith, g.np, g.lagstep
    # the launch plan: pad a dense table index over the drift-free items, lists in item order
    free = [i for i in range(g.n) if g.items_in["drift"][i] == 0.0]
    own = [i for i in range(g.n) if g.items_in["drift"][i] != 0.0]
    assert g.list_shared == free and g.list_own == own, (g.list_shared, g.list_own)
    slot_of = {it: s for s, it in enumerate(free + own)}
    for stage in (g.items_in, g.items_m0, g.items_m1, g.items_ladder):
        for i in range(g.n):
            assert stage["pad"][i] == sum(1 for j in free if j < i), (i, stage["pad"])
        for field in ("seg", "drift", "shift_coarse", "freq_coarse"):
            assert same_bits(stage[field], g.items_in[field]), field
    assert same_bits(g.items_ladder, g.items_m1)
    st = dict(lags=0, lags_pruned=0, minus1e30=0, freqs=0, centre_copies=0, rung0=0, gated_out=0, ladder_rows=0)
    for it in range(g.n):
        rec = recs[int(g.items_in["seg"][it])]
        fc, sc, drift = g.items_in["freq_coarse"][it], int(g.items_in["shift_coarse"][it]), g.items_in["drift"][it]
        at = "item %d (fc %r, sc %d, drift %r, np %d, arith %d, step %d)" % (it, float(fc), sc, float(drift), npts, a, step)
        # ---- mode 0: every lag against (a), the pick against (b)
        m0 = g.items_m0[it]
        if g.flags & RUN_MODE0:
            masked = bool(g.flags & PRUNE) and step == 8 and len(free) > 0
            mask = int(g.mask[it]) if masked else (1 << g.nlag) - 1
            assert masked or untouched(g.mask)
            if it in own or not masked:
                assert mask & ((1 << g.nlag) - 1) == (1 << g.nlag) - 1, (at, hex(mask))
            want = np.array([lag_sync(a, rec, npts, fc, drift, sc - 128 + step * m) for m in range(g.nlag)], np.float32)
            for m in range(g.nlag):
                if (mask >> m) & 1:
                    assert same_bits(through_max(g.sync0[it, m]), want[m]), (at, m, g.sync0[it], want)
                    st["lags"] += 1
                    st["minus1e30"] += int(want[m] == MINUS_1E30)
                else:
                    assert g.sync0[it, m] == MINUS_3E38 and untouched(g.pw0[it, m]), (at, m)
                    st["lags_pruned"] += 1
            f_b, sh_b, sy_b = chain_mode0(a, rec, npts, fc, drift, sc, step)
            assert same_bits(m0["freq"], f_b) and int(m0["shift"]) == sh_b and same_bits(m0["sync"], sy_b), (at, m0, f_b, sh_b, sy_b)
        else:
            assert same_bits(m0, g.items_in[it]) and untouched(g.sync0[it]) and untouched(g.pw0[it]), at
        # ---- mode 1: the five amplitude rows, folded here, against (a); the state against (b); the centre row
        slot = slot_of[it]
        got = fold(g.pwf[slot], pr3)
        want = np.array([freq_sync(a, rec, npts, m0["freq"], drift, int(m0["shift"]), f) for f in range(-2, 3)], np.float32)
        assert same_bits(through_max(got), want), (at, got, want)
        st["freqs"] += 5
        f_b, sh_b, sy_b = chain_mode1(a, rec, npts, m0["freq"], drift, int(m0["shift"]))
        m1 = g.items_m1[it]
        assert same_bits(m1["freq"], f_b) and int(m1["shift"]) == sh_b and same_bits(m1["sync"], sy_b), (at, m1, f_b, sh_b, sy_b)
        if g.flags & HAND:
            d = int(m0["shift"]) - (sc - 128)
            if same_bits(m0["freq"], fc) and d >= 0 and d % step == 0 and d // step < g.nlag:      # the state is a grid point
                assert same_bits(g.pwf[slot, 2], g.pw0[it, d // step]), at
                st["centre_copies"] += 1
        # ---- rung 0 and the ladder: items the gate lets through against (a) and (c); the others untouched
        with np.errstate(all="ignore"):
            worth = bool(m1["sync"] > g.minsync1)
        if worth:
            sy, sym, rms = rung(a, rec, npts, m1["freq"], drift, int(m1["shift"]))
            assert same_bits(g.sync_r0[it], sy) and same_bits(g.sym_r0[it], sym) and same_bits(g.rms_r0[it], rms), \
                (at, g.sync_r0[it], sy, g.rms_r0[it], rms)
            st["rung0"] += 1
        else:
            assert untouched(g.sync_r0[it]) and untouched(g.sym_r0[it]) and untouched(g.rms_r0[it]), at
            st["gated_out"] += 1
        if worth and (g.flags & LADDER):
            for r in range(NRUNG):
                sy, sym, rms = rung(a, rec, npts, m1["freq"], drift, int(m1["shift"]) - 63 + 3 * r)
                assert same_bits(g.sync_l[it, r], sy) and same_bits(g.sym_l[it, r], sym) and same_bits(g.rms_l[it, r], rms), \
                    (at, r, g.sync_l[it, r], sy, g.rms_l[it, r], rms)
                st["ladder_rows"] += 1
        else:
            assert untouched(g.sync_l[it]) and untouched(g.sym_l[it]) and untouched(g.rms_l[it]), at
    # slots past the lists were never written
    assert untouched(g.pwf[len(free) + len(own):])
    return st


# ---- the cases ------------------------------------------------------------------------------------------------------------------
DRIFTS = (0.5, -0.5, 1.0, -1.0, 2.5, -4.0, 0.5, -1.0)
GRID_F = 0.732421875


@functools.lru_cache(maxsize=None)
def scenes():
    """The first two scenes of test_lag_bound_cpu._candidates() (ten signals each, -10 .. -28 dB): (records, candidates
    (seg, fc, sc) -- seven signals of each at their coarse grid point and one point 7 Hz off a signal, where there is none)."""
    import synth
    symf = lambda msg: ol.channel_symbols(msg)[1]
    recs, cands = [], []
    for seg in range(2):
        I, Q, truth = synth.make_segment(4321 + seg, symf, n_signals=10, snr_db=-10.0, snr_span=18.0, t_jitter=0.3)
        recs.append(Rec(I, Q))
        for i, (_, f0, t0, _) in enumerate(truth[:8]):
            fc = float(np.float32(round((f0 + (7.0 if i == 7 else 0.0)) / GRID_F) * GRID_F))
            cands.append((seg, fc, int(round(t0 * 375 / 128.0)) * 128))
    return recs, cands


def ordinary_items():
    """The 16 candidates, every other one drifting (the two records' candidates alternate, so both kinds sit in both)."""
    recs, cands = scenes()
    order = [cands[(i % 2) * 8 + i // 2] for i in range(16)]
    return recs, items_of([(seg, fc, sc, DRIFTS[i // 2] if i % 2 else 0.0) for i, (seg, fc, sc) in enumerate(order)])


ARITH1_SUBSET = (0, 1, 14, 11, 2, 3, 15, 10)         # half of them, the three that fail the gate included


def ordinary_runs(arith):
    """Mode 0 at 8/33 pruned, 8/33 whole and 16/17 (quick mode).  The contracted checker takes four times the oracle's time per
    hypothesis, so the contracted mode runs eight of the sixteen items."""
    recs, items = ordinary_items()
    if arith:
        items = items[list(ARITH1_SUBSET)].copy()
    return recs, [run_of(items, arith=arith), run_of(items, arith=arith, flags=WHOLE_CHAIN & ~PRUNE),
                  run_of(items, arith=arith, lagstep=16)]


HEAD = (-1, 0, 1, 2)                                 # first touched sample k
EDGE_DRIFT = 1.5


def tails(npts):
    """First samples of the hypotheses whose last sample is np - 2 .. np + 1."""
    return tuple(npts - 2 + d - (SPAN - 1) for d in range(4))


def edge_direct_items(npts):
    """Straight into the frequency scan (no mode 0, null lag block: freq_scalar_kernel sums four hypotheses,
    freq_centre_rare_kernel the centre, freq_drift_kernel all five) and on to the ladder, at shifts that put the first touched
    sample of the scan (k = shift) and of the ladder's first rung (k = shift - 63) at -1, 0, 1, 2, the last touched sample of
    the scan (shift + 41 471) and of the ladder's last rung (shift + 63 + 41 471) at np - 2 .. np + 1; at the full length
    also two items whose every window lies outside the record.  Each shift drift-free and drifting, interleaved."""
    recs, cands = scenes()
    fc = cands[0][1]
    shifts = list(tails(npts)) + [s - 63 for s in tails(npts)]
    if npts == NS:
        shifts = list(HEAD) + [s + 63 for s in HEAD] + shifts + [-50000, 50000]
    it = items_of([(0, fc, s, d) for s in shifts for d in (0.0, EDGE_DRIFT)])
    return recs[:1], it


def edge_lag_items(npts):
    """Mode 0 of DRIFTING items (demod_drift_kernel; demod_tile_kernel<16, false> at step 16) whose first lag starts at sample
    -1, 0, 1, 2 (full length only) and whose last lag ends at np - 2 .. np + 1; a drift-free item between them."""
    recs, cands = scenes()
    fc = cands[0][1]
    scs = [s + 128 for s in (HEAD if npts == NS else ())] + [s - 128 for s in tails(npts)]
    c = [(0, fc, s, EDGE_DRIFT) for s in scs]
    c.insert(len(c) // 2, (0, fc, scs[-1] + 1, 0.0))
    return recs[:1], items_of(c)


def window(first, npts):
    """(first, last) sample a hypothesis starting at `first` touches, and how many of its samples the reference reads."""
    k = first + np.arange(SPAN)
    return first, first + SPAN - 1, int(((k > 0) & (k < npts)).sum())


LIST_SHAPES = ((0, 1), (1, 2), (9, 7), (9, 0), (1, 7), (0, 2), (9, 1))      # (n_shared, n_own)


def list_shape_runs():
    """The ordinary candidates re-dealt: the first n_shared + n_own of them, drifting ones spread between the others."""
    recs, cands = scenes()
    order = [cands[(i % 2) * 8 + i // 2] for i in range(16)]
    runs = []
    for ns, no in LIST_SHAPES:
        n = ns + no
        drifting = {((2 * j + 1) * n) // (2 * no) for j in range(no)}       # evenly spread, all of them when ns == 0
        assert len(drifting) == no
        runs.append(run_of(items_of([(seg, fc, sc, DRIFTS[i % 8] if i in drifting else 0.0)
                                     for i, (seg, fc, sc) in enumerate(order[:n])])))
    return recs, runs


def tie_case():
    """Records: the period-8 carrier of lag_audit_lib.fallback_cases() and a record that is zero but at 162 samples 256 apart."""
    p8 = next(c for c in la.fallback_cases() if c[0] == "period8")
    rng = np.random.default_rng(20)
    I, Q = np.zeros(NS, np.float32), np.zeros(NS, np.float32)
    at = SPARSE_SHIFT + 256 * np.arange(NSYM)
    I[at], Q[at] = rng.normal(0, 1, NSYM).astype(np.float32), rng.normal(0, 1, NSYM).astype(np.float32)
    return [Rec(p8[1], p8[2]), Rec(I, Q)], float(p8[3]), int(p8[4])


SPARSE_SHIFT, SPARSE_FC = 300, 10.25


def tie_runs(arith):
    recs, fc, sc = tie_case()
    lag_items = items_of([(0, fc, sc, 2.0), (0, fc, sc, -3.5)])
    freq_items = items_of([(1, SPARSE_FC, SPARSE_SHIFT, 0.0), (1, SPARSE_FC, SPARSE_SHIFT, 1.5)])
    return recs, [run_of(lag_items, arith=arith, minsync1=-1.0), run_of(lag_items, arith=arith, lagstep=16, minsync1=-1.0),
                  run_of(freq_items, arith=arith, flags=LADDER, minsync1=-1.0)]


def no_lag_runs(arith):
    """An all-zero and an all-NaN record: no lag wins, the pick leaves shift 0, freq 0.0, sync -1e30; that state is a grid point
    of the lag scan (centre copied from lag 0) for freq_coarse 0.0, shift_coarse 128 only."""
    recs = [Rec(np.zeros(NS, np.float32), np.zeros(NS, np.float32)), Rec(np.full(NS, np.nan, np.float32), np.full(NS, np.nan, np.float32))]
    items = items_of([(seg, fc, sc, d) for seg in (0, 1) for fc, sc in ((10.25, 128), (0.0, 128), (0.0, 132)) for d in (0.0, 1.0)])
    return recs, [run_of(items, arith=arith), run_of(items, arith=arith, flags=WHOLE_CHAIN & ~PRUNE)]


def extreme_runs(arith):
    """Noise x 1e20 (squares overflow), x 1e-30 (squares underflow), one +Inf inside the windows of lags >= 16 only."""
    cases = [c for c in la.fallback_cases() if c[0] in ("noise_1e+20", "noise_1e-30", "inf_late_lags")]
    assert len(cases) == 3
    recs = [Rec(c[1], c[2]) for c in cases]
    items = items_of([(i, c[3], c[4], d) for i, c in enumerate(cases) for d in (0.0, 1.0)])
    return recs, [run_of(items, arith=arith, minsync1=-1.0)]


def gate_items():
    """Four ordinary candidates: drift-free and drifting, both records."""
    recs, items = ordinary_items()
    return recs, items[[0, 1, 6, 7]].copy()
