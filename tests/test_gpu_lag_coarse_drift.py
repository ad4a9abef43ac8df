"""lag_coarse_drift_kernel and its fold kernel (k4_lag_prune.h) held to the quantities the proof of DESIGN.md section 4 talks about:
tests/test_gpu_lag_coarse.py's seven assertions, transposed to the DRIFTING items of a list.  tools/lagprune_check.hip with its
"drift" option runs the production launchers with LagPrune::drift on -- A: the pruned scan with the audit output, B: the whole
scan (demod_drift_kernel) -- and dumps every buffer.  Per drifting item and lag, check_run() asserts:
 1. soundness on the kernel's own numbers: not flagged bad => |sync_B - sy| <= ep; in the ordinary case sync_B equals the oracle's
    (contracted: the CONTRACT=1 checker's) single-lag sync bit for bit;
 2. accuracy (ordinary case): |sy - sync_id| <= eps_c against a float64 ideal, and R_k <= 4 R_np of the numpy restatement;
 3. tm (1 + 256u) >= T; dtab equals the float recurrence's largest distance from float64 phasors (numpy runs the same recurrence);
    ep == the DESIGN formula from the audit's own totp, ss, tm, dtab; the bad flag == the formula's preconditions;
 4. the contender rule bit for bit from (sy, ep, bad); fallback <=> bad, 0 or more than 4 contenders; fallback mask all ones;
 5. the first strict maximum of sync_B is a mask bit; shift, freq, sync after A == after B as bytes;
 6. rows: mask lags equal demod_drift_kernel's bytewise, the others hold -3e38 in sync_A and the fill pattern in pw_A; fallback
    items equal B on all 33 lags;
 7. bookkeeping: the drifting candidates' three counts and two lists, list tails untouched, and the drift-free items of the run
    served as before (their counts add up, their rows equal B on their mask lags).
Measured figures go to profiles/lag_coarse_drift_audit.json."""
import json
import os

import numpy as np
import pytest

import lag_audit_lib as la
import lag_drift_lib as ld
from lag_audit_lib import NLAG, NS

pytestmark = pytest.mark.gpu
MINUS_3E38 = np.float32(-3.0e38)
PROFILE = os.path.join(la.ROOT, "profiles", "lag_coarse_drift_audit.json")


def same_bits(a, b):
    return np.ascontiguousarray(a).view(np.uint8).tobytes() == np.ascontiguousarray(b).view(np.uint8).tobytes()


def record(key, value):
    data = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            data = json.load(fh)
    data[key] = value
    with open(PROFILE, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)
        fh.write("\n")


def exact_sync(I, Q, fc, drift, sc, npts, arith):
    fn = None
    if arith:
        import contract_lib
        fn = contract_lib.contract(1).ctr_sync_demod
    return np.array([ld.oracle_sync(I, Q, fc, drift, sc, m, npts, fn) for m in range(NLAG)], np.float32)


def check_run(g, src, ordinary=False):
    """g: one run's dump.  src[item] = (I, Q, fc, drift, sc) of the record the item reads."""
    own, shared = list(g.list_own), list(g.list_shared)
    assert g.counts_d[1] + g.counts_d[2] == g.n_own, g.counts_d                                               # 7
    fallbacks, pruned, hist, worst_k, worst_sound = [], [], {}, 0.0, 0.0
    for it in own:
        I, Q, fc, drift, sc = src[it]
        at = "item %d (fc %g, drift %g, sc %d, np %d, arith %d)" % (it, fc, drift, sc, g.np, g.arith)
        sy, ep, totp, ss, tm, dtab, badf = (g.audit[it, :, i] for i in range(la.AUDIT))
        assert set(badf.tolist()) <= {0.0, 1.0}, at
        bad = badf == 1.0
        sync_b = g.sync_b[it]
        with np.errstate(all="ignore"):
            diff = np.abs(sync_b.astype(np.float64) - sy.astype(np.float64))                               # 1
            assert (diff[~bad] <= ep[~bad].astype(np.float64)).all(), (at, diff, ep)
            if (~bad).any():
                worst_sound = max(worst_sound, float((diff[~bad] / ep[~bad]).max()))
        idl = ld.ideal(I, Q, fc, drift, sc, g.np, la.pr3())
        if ordinary:
            ref = exact_sync(I, Q, fc, drift, sc, g.np, g.arith)
            with np.errstate(all="ignore"):
                through_max = np.where(sync_b > np.float32(-1e30), sync_b, np.float32(-1e30)).astype(np.float32)
            assert same_bits(ref, through_max), (at, ref, sync_b)
            ec, valid = la.eps_c(idl)                                                                         # 2
            assert valid.all(), at
            ratio = np.abs(sy.astype(np.float64) - idl.sync) / ec
            assert (ratio <= 1.0).all(), (at, ratio)
            worst_k = max(worst_k, float(ratio.max()))
        with np.errstate(all="ignore"):
            fin = np.isfinite(idl.T)                                                                          # 3
            assert (tm[fin].astype(np.float64) * la.T_INFLATE >= idl.T[fin]).all(), (at, tm, idl.T)
            theta = np.concatenate([ld.tone_dphi(fc, drift, np.arange(162), t) for t in range(4)])
            d64 = float(ld.measured_delta(theta, bool(g.arith)).max())
            # exact: numpy runs the very recurrence; contracted: its fma is emulated through float64 (a table entry may differ by an ulp)
            tol = 2.0 ** -22 if g.arith else 3e-6 * d64 + float(np.spacing(np.float32(d64)))
            assert (dtab == dtab[0]).all() and abs(float(dtab[0]) - d64) <= tol, (at, d64, dtab[0])
            want_ep, want_ok = la.eps_from_audit(totp, ss, tm, dtab)
            f = np.isfinite(want_ep)
            assert np.isclose(ep[f].astype(np.float64), want_ep[f], rtol=3e-6, atol=2e-9).all(), (at, ep, want_ep)
            assert (bad == ~want_ok).all() and bad[~f].all(), (at, bad, want_ok)
        mask, fallback, n = la.contender_rule(sy, ep, bad)                                                   # 4
        assert int(g.mask[it]) == mask, (at, hex(int(g.mask[it])), hex(mask))
        (fallbacks if fallback else pruned).append(it)
        if not fallback:
            hist[n] = hist.get(n, 0) + 1
        win = la.first_strict_maximum(sync_b)                                                                 # 5
        assert win < 0 or (mask >> win) & 1, (at, win, hex(mask))
        for m in range(NLAG):                                                                                 # 6
            if (mask >> m) & 1:
                assert same_bits(g.sync_a[it, m], sync_b[m]) and same_bits(g.pw_a[it, m], g.pw_b[it, m]), (at, m)
            else:
                assert g.sync_a[it, m] == MINUS_3E38 and (g.pw_a[it, m].view(np.uint8) == la.SENTINEL).all(), (at, m)
    for it in shared + own:                                                                                   # 5
        for field in ("shift", "freq", "sync"):
            assert same_bits(g.items_a[field][it], g.items_b[field][it]), (it, field, g.items_a[it], g.items_b[it])
    # 7: bookkeeping
    pairs = sorted(it * 64 + m for it in pruned for m in range(NLAG) if (int(g.mask[it]) >> m) & 1)
    cd = g.counts_d
    assert cd[0] == len(pairs) and cd[1] == len(fallbacks) and cd[2] == len(pruned), (cd, len(pairs), fallbacks, pruned)
    assert sorted(g.exact_list_d[:cd[0]].tolist()) == pairs
    assert sorted(g.fb_list_d[:cd[1]].tolist()) == sorted(fallbacks)
    assert (g.exact_list_d[cd[0]:].view(np.uint8) == la.SENTINEL).all() and (g.fb_list_d[cd[1]:].view(np.uint8) == la.SENTINEL).all()
    assert g.counts[1] + g.counts[2] == g.n_shared
    for it in shared:
        for m in range(NLAG):
            if (int(g.mask[it]) >> m) & 1:
                assert same_bits(g.sync_a[it, m], g.sync_b[it, m]) and same_bits(g.pw_a[it, m], g.pw_b[it, m]), (it, m)
    for it in range(g.n):
        if it not in shared and it not in own:
            assert int(g.mask[it]) == 2 ** 64 - 1 and (g.audit[it].view(np.uint8) == la.SENTINEL).all(), it
    return {"n_own": g.n_own, "pruned": len(pruned), "fallbacks": len(fallbacks), "exact_evaluations": int(cd[0]),
            "contenders": {str(k): hist[k] for k in sorted(hist)}, "max_sy_minus_ideal_over_eps_c": round(worst_k, 5),
            "max_sync_B_minus_sy_over_ep": round(worst_sound, 5), "fallback_items": fallbacks, "pruned_items": pruned}


def _two_scenes():
    """16 drifting items from two scenes (the first eight candidates of the first two records of test_lag_bound_cpu._candidates(),
    drifts +-0.5, +-1, 2.5, -4 in turn) and the same candidates drift-free in between: (records, [(seg, fc, sc, drift)])."""
    cands = ld.soundness_cases()
    rows, seg_of, out = [], {}, []
    for I, Q, fc, drift, sc in cands:
        if id(I) not in seg_of:
            if len(rows) == 2:
                continue
            seg_of[id(I)] = len(rows)
            rows.append((I, Q))
        if sum(1 for c in out if c[0] == seg_of[id(I)] and c[3] != 0.0) < 8:
            out.append((seg_of[id(I)], fc, sc, drift))
            out.append((seg_of[id(I)], fc, sc, 0.0))
    return rows, out


@pytest.mark.parametrize("arith", [0, 1])
def test_ordinary_drifting_candidates_and_list_lengths(tmp_path, arith):
    """16 drifting items of two scenes with drift-free items in between; then lists of 1, 7, 8, 9 and 13 drifting items of them.
    R_k, the kernel's worst |sy - sync_id| / eps_c, must stay within 4 x the numpy restatement's R_np on the same candidates."""
    rows, cands = _two_scenes()
    I, Q = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    items = la.items_of(cands, len(rows))
    own = [i for i, c in enumerate(cands) if c[3] != 0.0]
    shared = [i for i, c in enumerate(cands) if c[3] == 0.0]
    assert len(own) == 16
    runs = [dict(np=NS, arith=arith, items=items, list_shared=shared, list_own=own)]
    for n in (1, 7, 8, 9, 13):
        runs.append(dict(np=NS, arith=arith, items=items, list_shared=shared[:max(1, n // 2)], list_own=own[16 - n:]))
    res = ld.run_tool(tmp_path, I, Q, runs)
    src = {i: (rows[c[0]][0], rows[c[0]][1], c[1], c[3], c[2]) for i, c in enumerate(cands)}
    st = check_run(res[0], src, ordinary=True)
    r_np = 0.0
    for it in own:
        Ii, Qi, fc, drift, sc = src[it]
        sync, _, _ = ld.coarse_pass(Ii, Qi, fc, drift, sc, la.pr3(), contracted=bool(arith))
        idl = ld.ideal(Ii, Qi, fc, drift, sc, NS, la.pr3())
        r_np = max(r_np, float((np.abs(sync.astype(np.float64) - idl.sync) / la.eps_c(idl)[0]).max()))
    r_k = st["max_sy_minus_ideal_over_eps_c"]
    st.update(R_np=round(r_np, 5))
    print("arith %d: %s" % (arith, st))
    record("ordinary_arith%d" % arith, st)
    assert r_k <= 4 * r_np, (r_k, r_np)
    assert st["pruned"] >= 8                                     # "always falls back" cannot pass
    for g in res[1:]:
        s2 = check_run(g, src)
        assert set(s2["pruned_items"]) == set(st["pruned_items"]) & set(g.list_own), (g.n_own, s2)


@pytest.mark.parametrize("arith", [0, 1])
def test_shifts_hanging_over_both_ends(tmp_path, arith):
    """Shifts of every residue mod 4 that hang over the start and over the end of records of 45 000, 44 993 and 30 000 samples."""
    rows, cands0 = _two_scenes()
    I, Q = np.stack([rows[0][0]]), np.stack([rows[0][1]])
    fc = cands0[0][1]
    runs, srcs = [], []
    for npts in (NS, 44993, 30000):
        late = npts - 41472
        cands = [(0, fc, sc, dr) for sc, dr in [(1, 1.0), (2, -0.5), (3, 2.5), (4, -4.0), (-61, 0.5), (late + 1, -1.0), (late + 2, 1.0),
                                                (late + 3, 0.5), (late + 4, -4.0), (late + 250, 2.5)]] + [(0, fc, 512, 0.0)]
        runs.append(dict(np=npts, arith=arith, items=la.items_of(cands, 1), list_shared=[10], list_own=list(range(10))))
        srcs.append({i: (I[0], Q[0], c[1], c[3], c[2]) for i, c in enumerate(cands)})
    for g, src in zip(ld.run_tool(tmp_path, I, Q, runs), srcs):
        st = check_run(g, src)
        print("np %d arith %d: %s" % (g.np, arith, st))
        record("edges_np%d_arith%d" % (g.np, arith), st)


@pytest.mark.parametrize("arith", [0, 1])
def test_inputs_that_must_fall_back_and_a_drift_of_1e_30(tmp_path, arith):
    """Zero, the period-8 carrier (drift 2.0 and -3.5: every lag ties), noise x 1e20 and x 1e-30, a NaN and an Inf inside the late
    lags' windows fall back; a NaN beyond every window does not.  A drift of 1e-30 is drifting by its list and numerically
    drift-free: its pick equals the drift-free path's on the same candidate."""
    cases = la.fallback_cases()
    I, Q = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
    cands, want = [], {}
    for seg, (name, _, _, fc, sc, expect) in enumerate(cases):
        for drift in ((2.0, -3.5) if name == "period8" else (1.0,)):
            want[len(cands)] = (name, expect)
            cands.append((seg, fc, sc, drift))
    tiny, twin = len(cands), len(cands) + 1
    seg = [c[0] for c in cases].index("nan_beyond")
    cands += [(seg, cases[seg][3], cases[seg][4], 1e-30), (seg, cases[seg][3], cases[seg][4], 0.0)]
    own = [i for i, c in enumerate(cands) if c[3] != 0.0]
    g, = ld.run_tool(tmp_path, I, Q, [dict(np=NS, arith=arith, items=la.items_of(cands, len(cases)), list_shared=[twin],
                                           list_own=own)])
    src = {i: (I[c[0]], Q[c[0]], c[1], c[3], c[2]) for i, c in enumerate(cands)}
    st = check_run(g, src)
    print("arith %d: %s" % (arith, st))
    for i, (name, expect) in want.items():
        assert (i in st["fallback_items"]) == (expect == "fallback"), (name, cands[i], st)
    assert tiny in st["pruned_items"]
    for field in ("shift", "freq", "sync"):
        assert same_bits(g.items_a[field][tiny], g.items_a[field][twin]), (field, g.items_a[tiny], g.items_a[twin])
    record("fallback_inputs_arith%d" % arith, {k: st[k] for k in ("pruned", "fallbacks", "exact_evaluations")})
