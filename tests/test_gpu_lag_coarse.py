"""lag_coarse_kernel (k4_lag_prune.h) held to the quantities the proof of DESIGN.md section 4 "The bound of the lag pruning" talks
about.  tools/lagprune_check.hip runs the production launchers on a case file -- A: the pruned scan with the kernel's audit
output (per item and lag: sy, ep, totp, ss, tm, dtab, bad), B: the whole scan -- and dumps every buffer; the references are
float64 numpy (tests/lag_audit_lib.py), the oracle's single-lag sync in the exact mode and the CONTRACT=1 checker's
(contract_lib.ctr_sync_demod) in the contracted mode.  Per drift-free item of the list and lag, check_run() asserts:
 1. soundness on the kernel's own numbers: not flagged bad => |sync_B - sy| <= ep; sync_B equals the reference bit for bit;
 2. accuracy: |sy - sync_id| <= eps_c, term (c) of the derivation alone (the ordinary case also: R_k <= 4 R_np);
 3. the bound's ingredients: tm (1 + 256u) >= T, dtab in [d64, d64 (1 + 3e-6) + ulp], ep == the DESIGN formula from the
    audit's own totp, ss, tm, dtab to 3e-6 relative + 2e-9, and the bad flag == the formula's preconditions;
 4. the contender rule bit for bit from (sy, ep, bad); fallback <=> bad, 0 or more than 4 contenders; fallback mask all ones;
 5. the first strict maximum of sync_B is a mask bit; shift, freq, sync after A == after B as bytes;
 6. rows: mask lags equal B bytewise, the others hold -3e38 in sync_A and the fill pattern in pw_A; fallback and drifting
    items equal B on all 33 lags;
 7. bookkeeping: the three counts, exact_list == the masks' (item, lag) pairs, fb_list == the fallback items, and nothing
    written for items outside list_shared.
Measured figures go to profiles/lag_coarse_audit.json."""
import numpy as np
import pytest

import lag_audit_lib as la
from lag_audit_lib import NLAG, NS

pytestmark = pytest.mark.gpu
MINUS_3E38 = np.float32(-3.0e38)


def same_bits(a, b):
    return np.ascontiguousarray(a).view(np.uint8).tobytes() == np.ascontiguousarray(b).view(np.uint8).tobytes()


def check_run(g, src, exact):
    """g: one run's dump.  src[item] = (I, Q, fc, sc) of the record the item reads.  exact(item) -> the reference's 33 syncs.
    Returns the run's statistics."""
    ns = la.NLAG
    shared, own = list(g.list_shared), list(g.list_own)
    assert g.counts[1] + g.counts[2] == g.n_shared, g.counts                                                # 7
    fallbacks, pruned, hist, worst_k, worst_sound = [], [], {}, 0.0, 0.0
    for it in shared:
        I, Q, fc, sc = src[it]
        at = "item %d (fc %g, sc %d, np %d, arith %d)" % (it, fc, sc, g.np, g.arith)
        sy, ep, totp, ss, tm, dtab, badf = (g.audit[it, :, i] for i in range(la.AUDIT))
        assert set(badf.tolist()) <= {0.0, 1.0}, at
        bad = badf == 1.0
        sync_b = g.sync_b[it]
        # 1: B is the reference, and the kernel's own bound holds against it
        # (the reference's entry returns the maximum from -1e30 under strict >, wsprd.c:227-232: a single lag's sync as it is,
        # or -1e30 where that is NaN or not above it)
        ref = exact(it)
        with np.errstate(all="ignore"):
            through_max = np.where(sync_b > np.float32(-1e30), sync_b, np.float32(-1e30)).astype(np.float32)
        assert same_bits(ref, through_max), (at, ref, sync_b)
        with np.errstate(all="ignore"):
            diff = np.abs(sync_b.astype(np.float64) - sy.astype(np.float64))
            assert (diff[~bad] <= ep[~bad].astype(np.float64)).all(), (at, diff, ep)
            if (~bad).any():
                worst_sound = max(worst_sound, float((diff[~bad] / ep[~bad]).max()))
        # 2: sy against float64 at the derived tolerance
        idl = la.ideal(I, Q, fc, sc, g.np)
        ec, valid = la.eps_c(idl)
        with np.errstate(all="ignore"):
            ratio = np.abs(sy.astype(np.float64) - idl.sync) / ec
            assert not np.isnan(ratio[valid]).any() and (ratio[valid] <= 1.0).all(), (at, ratio)
            if valid.any():
                worst_k = max(worst_k, float(ratio[valid].max()))
            # 3: T~, delta_tab, eps and the bad flag
            fin = np.isfinite(idl.T)
            assert (tm[fin].astype(np.float64) * la.T_INFLATE >= idl.T[fin]).all(), (at, tm, idl.T)
            d64 = la.table_distance(g.tabs[it], fc)
            assert (dtab == dtab[0]).all() and d64 <= float(dtab[0]) <= d64 * (1 + 3e-6) + float(np.spacing(np.float32(d64))), (at, d64, dtab[0])
            want_ep, want_ok = la.eps_from_audit(totp, ss, tm, dtab)
            f = np.isfinite(want_ep)
            assert np.isclose(ep[f].astype(np.float64), want_ep[f], rtol=3e-6, atol=2e-9).all(), (at, ep, want_ep)
            assert (bad == ~want_ok).all() and bad[~f].all(), (at, bad, want_ok)
        # 4: the contender rule
        mask, fallback, n = la.contender_rule(sy, ep, bad)
        assert int(g.mask[it]) == mask, (at, hex(int(g.mask[it])), hex(mask))
        (fallbacks if fallback else pruned).append(it)
        lags = [m for m in range(ns) if (mask >> m) & 1]
        if not fallback:
            hist[n] = hist.get(n, 0) + 1
        # 5: the winner is kept
        win = la.first_strict_maximum(sync_b)
        assert win < 0 or (mask >> win) & 1, (at, win, hex(mask))
        # 6: rows
        for m in range(ns):
            if (mask >> m) & 1:
                assert same_bits(g.sync_a[it, m], sync_b[m]) and same_bits(g.pw_a[it, m], g.pw_b[it, m]), (at, m)
            else:
                assert g.sync_a[it, m] == MINUS_3E38 and (g.pw_a[it, m].view(np.uint8) == la.SENTINEL).all(), (at, m)
        assert len(lags) == (ns if fallback else n)
    for it in shared + own:                                                                                  # 5
        for field in ("shift", "freq", "sync"):
            assert same_bits(g.items_a[field][it], g.items_b[field][it]), (it, field, g.items_a[it], g.items_b[it])
    for it in own:                                                                                           # 6
        assert same_bits(g.sync_a[it], g.sync_b[it]) and same_bits(g.pw_a[it], g.pw_b[it]), it
    # 7: bookkeeping
    pairs = sorted(it * 64 + m for it in pruned for m in range(ns) if (int(g.mask[it]) >> m) & 1)
    assert g.counts[0] == len(pairs) and g.counts[1] == len(fallbacks) and g.counts[2] == len(pruned), (g.counts, len(pairs))
    assert sorted(g.exact_list[:g.counts[0]].tolist()) == pairs
    assert sorted(g.fb_list[:g.counts[1]].tolist()) == sorted(fallbacks)
    assert (g.exact_list[g.counts[0]:].view(np.uint8) == la.SENTINEL).all() and (g.fb_list[g.counts[1]:].view(np.uint8) == la.SENTINEL).all()
    for it in range(g.n):
        if it not in shared:
            assert int(g.mask[it]) == 2 ** 64 - 1 and (g.audit[it].view(np.uint8) == la.SENTINEL).all(), it
    return {"n_shared": g.n_shared, "pruned": len(pruned), "fallbacks": len(fallbacks), "exact_evaluations": int(g.counts[0]),
            "contenders": {str(k): hist[k] for k in sorted(hist)}, "max_sy_minus_ideal_over_eps_c": round(worst_k, 5),
            "max_sync_B_minus_sy_over_ep": round(worst_sound, 5), "pruned_items": pruned, "r_k": worst_k}


def _ordinary_case():
    """The 68 candidates as items over their five records."""
    cands = la.ordinary()
    rows, seg_of = [], {}
    for c in cands:
        if id(c.I) not in seg_of:
            seg_of[id(c.I)] = len(rows)
            rows.append((c.I, c.Q))
    I, Q = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    items = la.items_of([(seg_of[id(c.I)], c.fc, c.sc, 0.0) for c in cands], len(rows))
    return cands, I, Q, items


@pytest.mark.parametrize("arith", [0, 1])
def test_ordinary_candidates(tmp_path, arith):
    """The 68 candidates of test_lag_bound_cpu._candidates().  R_k, the kernel's worst |sy - sync_id| / eps_c, must stay within
    4 x the numpy restatement's R_np on the same candidates (the kernel sums a window as 25 shared + 7 own terms with fused
    multiply-adds, numpy adds 32 terms in order).  No fallback, candidates with 1, with 2 and with >= 3 contenders, mean <= 3."""
    cands, I, Q, items = _ordinary_case()
    g, = la.run_tool(tmp_path, I, Q, [dict(np=NS, arith=arith, items=items, list_shared=list(range(len(cands))), list_own=[])])
    src = {i: (c.I, c.Q, c.fc, c.sc) for i, c in enumerate(cands)}
    st = check_run(g, src, lambda it: la.exact_sync(*src[it], NS, arith))
    r_np, r_k = la.r_np(), st.pop("r_k")
    del st["pruned_items"]
    st.update(R_k=round(r_k, 5), R_np=round(r_np, 5))
    print("arith %d: %s" % (arith, st))
    la.record_profile("ordinary_arith%d" % arith, st)
    assert r_k <= 4 * r_np, (r_k, r_np)
    h = {int(k): v for k, v in st["contenders"].items()}
    assert st["fallbacks"] == 0 and h.get(1, 0) >= 1 and h.get(2, 0) >= 1 and sum(v for k, v in h.items() if k >= 3) >= 1
    assert sum(k * v for k, v in h.items()) <= 3.0 * len(cands)


def test_list_shapes(tmp_path):
    """n_shared in {1, 7, 8, 9, 13} (the XCD-aware pos mapping: lists that are and are not a multiple of 8), list_shared a
    non-monotone subset of items[] with gaps, drifting items in between and in list_own, two items in neither list."""
    cands, I, Q, _ = _ordinary_case()
    cands = cands[:30]                                        # the records of the first two segments
    drifting = {2: 1.0, 5: -2.5, 11: 0.5, 12: 3.0, 20: -1.0, 27: 2.0}
    items = la.items_of([(0 if c.I is cands[0].I else 1, c.fc, c.sc, drifting.get(i, 0.0)) for i, c in enumerate(cands)], 2)
    free = [i for i in range(len(cands)) if i not in drifting and i not in (7, 19)]         # 7 and 19: in neither list
    order = [free[(5 * j + 3) % len(free)] for j in range(len(free))]                       # 5 and 22 are coprime: a permutation
    assert sorted(order) == free and order != free
    runs = [dict(np=NS, arith=0, items=items, list_shared=order[:ns], list_own=[27, 2, 12, 5, 20, 11][:1 + ns % 6])
            for ns in (1, 7, 8, 9, 13)]
    src = {i: (c.I, c.Q, c.fc, c.sc) for i, c in enumerate(cands)}
    exact = {}

    def ex(it):
        if it not in exact:
            exact[it] = la.exact_sync(*src[it], NS, 0)
        return exact[it]
    stats = {}
    for g in la.run_tool(tmp_path, I[:2], Q[:2], runs):
        st = check_run(g, src, ex)
        del st["pruned_items"], st["r_k"]
        stats["n_shared_%d" % g.n_shared] = st
        assert st["pruned"] >= 1
    print(stats)
    la.record_profile("list_shapes", stats)


EDGE_SHIFTS = (-700, -127, 5, 128, 129, 130, 131, 349, 2816, 3300, 3656)


@pytest.mark.parametrize("arith", [0, 1])
def test_record_edges_and_alignment(tmp_path, arith):
    """shift_coarse over every residue of k0 mod 4 (the 4-byte-aligned 16-byte loads), windows that start at or before sample
    0 (k <= 0 is skipped, index 0 included) and windows past the end, with records of 45 000, 44 993 (the last block cut) and
    30 000 samples.  Which items fall back is the bound's business; at 45 000 samples at least half of those with
    shift_coarse >= 5 are pruned."""
    cands, I, Q, _ = _ordinary_case()
    c0 = [c for c in cands if c.I is cands[0].I]
    pick = [c0[(3 * j) % len(c0)] for j in range(len(EDGE_SHIFTS))]             # the record's signals' frequencies in turn
    items = la.items_of([(0, c.fc, sc, 0.0) for c, sc in zip(pick, EDGE_SHIFTS)], 1)
    nps = (45000, 44993, 30000)
    runs = [dict(np=n, arith=arith, items=items, list_shared=list(range(len(items))), list_own=[]) for n in nps]
    src = {i: (c0[0].I, c0[0].Q, c.fc, sc) for i, (c, sc) in enumerate(zip(pick, EDGE_SHIFTS))}
    stats = {}
    for g in la.run_tool(tmp_path, I[:1], Q[:1], runs):
        st = check_run(g, src, lambda it: la.exact_sync(*src[it], g.np, arith))
        pruned = st.pop("pruned_items")
        del st["r_k"]
        stats["np_%d" % g.np] = st
        if g.np == 45000:
            late = [i for i, sc in enumerate(EDGE_SHIFTS) if sc >= 5]
            assert 2 * len([i for i in late if i in pruned]) >= len(late), (pruned, late)
    print(stats)
    la.record_profile("record_edges_arith%d" % arith, stats)


@pytest.mark.parametrize("arith", [0, 1])
def test_inputs_that_must_fall_back_and_equal_the_whole_scan(tmp_path, arith):
    """An all-zero record, the period-8 carrier (33 contenders), noise x 1e20 (T above its ceiling, squares overflow), noise x
    1e-30 (S below its floor), a NaN and a +Inf inside the windows of lags >= 16 only: all take the whole scan and equal it; the
    same NaN beyond every window of the candidate must not force the fallback."""
    cases = la.fallback_cases()
    I, Q = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
    items = la.items_of([(i, c[3], c[4], 0.0) for i, c in enumerate(cases)], len(cases))
    g, = la.run_tool(tmp_path, I, Q, [dict(np=NS, arith=arith, items=items, list_shared=list(range(len(cases))), list_own=[])])
    src = {i: (c[1], c[2], c[3], c[4]) for i, c in enumerate(cases)}
    st = check_run(g, src, lambda it: la.exact_sync(*src[it], NS, arith))
    pruned = st.pop("pruned_items")
    del st["r_k"]
    for i, c in enumerate(cases):
        assert (i in pruned) == (c[5] == "pruned"), (c[0], pruned)
        if c[0] in ("nan_late_lags", "inf_late_lags"):
            assert (g.audit[i, :, 6] == 1.0).tolist() == [m >= 16 for m in range(NLAG)], (c[0], g.audit[i, :, 6])
        if c[0] == "period8":
            assert la.contender_rule(g.audit[i, :, 0], g.audit[i, :, 1], g.audit[i, :, 6] == 1.0)[2] == NLAG
    print(st)
    la.record_profile("must_fall_back_arith%d" % arith, st)
