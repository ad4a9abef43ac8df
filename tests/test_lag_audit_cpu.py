"""The yardsticks of the coarse-kernel audit (tests/test_gpu_lag_coarse.py) on the CPU: the numpy restatement of the coarse
pass (test_lag_bound_cpu.coarse_pass) held against the float64 ideal at the tolerance term (c) of DESIGN.md section 4
derives for the coarse pass' rounding alone, and the inputs the GPU test uses to reach the fallback."""
import numpy as np

import lag_audit_lib as la


def test_numpy_restatement_meets_term_c_and_term_c_is_part_of_eps():
    """R_np = max |sync_np - sync_id| / eps_c <= 1 over the 68 candidates x 33 lags (measured 0.0013), and eps_c < eps on every
    lag (measured eps_c / eps = 0.12 .. 0.20: term (c) is one of several terms of eps)."""
    cands = la.ordinary()
    r = la.r_np()
    ratio = [float((c.eps_c / c.np_eps).max()) for c in cands]
    print("candidates %d, R_np %.5f, eps_c / eps %.3f .. %.3f"
          % (len(cands), r, min(float((c.eps_c / c.np_eps).min()) for c in cands), max(ratio)))
    assert len(cands) == 68 and r <= 1.0
    assert max(ratio) < 1.0


def test_contender_histogram_of_the_numpy_restatement():
    """41 / 14 / 11 / 2 candidates with 1 / 2 / 3 / 4 contenders, none over the cap: what the GPU test's conditions (no
    fallback, candidates with 1, 2 and >= 3 contenders, mean <= 3) rest on."""
    hist = {}
    for c in la.ordinary():
        mask, fallback, _ = la.contender_rule(c.np_sync, c.np_eps.astype(np.float32) + np.float32(1e-9), np.zeros(la.NLAG))
        assert not fallback
        n = bin(mask).count("1")
        hist[n] = hist.get(n, 0) + 1
    assert hist == {1: 41, 2: 14, 3: 11, 4: 2}, hist


def test_fallback_inputs_reach_the_fallback():
    """Zero, noise x 1e20 and noise x 1e-30 leave the bound's range; the period-8 carrier makes every lag a contender; a NaN or
    an Inf inside the windows of the late lags leaves it, one beyond every window does not."""
    seen = {}
    for name, I, Q, fc, sc, want in la.fallback_cases():
        with np.errstate(all="ignore"):
            got = la.coarse_pass(I, Q, fc, sc, la.pr3())
        if got is None:
            seen[name] = "fallback"
        else:
            _, fallback, n = la.contender_rule(got[0], got[1].astype(np.float32), np.zeros(la.NLAG))
            seen[name] = "fallback" if fallback else "pruned"
            assert (n == la.NLAG) == (name == "period8"), (name, n)
        assert seen[name] == want, (name, seen[name])
    assert sorted(seen) == ["inf_late_lags", "nan_beyond", "nan_late_lags", "noise_1e+20", "noise_1e-30", "period8", "zero"]
