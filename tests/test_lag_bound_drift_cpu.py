"""The bound of the lag pruning of DRIFTING candidates (k4_lag_prune.h: lag_coarse_drift_kernel; DESIGN.md section 4 "The bound for
drifting candidates"), restated in numpy (tests/lag_drift_lib.py) and held against the oracle's own sync of every single lag:
(a) soundness -- |exact - coarse| <= eps on every lag, the reference's pick among the contenders, and the a priori bound on the
float phasor recurrence above what the recurrence does over the whole range of frequencies and drifts; (b) the caps -- on the
drifting candidates the reference refines in configs[2]-shaped segments at most a tenth fall back and a pruned one takes at most
3 exact evaluations.  The constants are the derivation's; the figures go to profiles/lag_prune_drift_bound.json."""
import json
import os

import numpy as np

import lag_audit_lib as la
import lag_drift_lib as ld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "lag_prune_drift_bound.json")


def _record(key, value):
    data = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            data = json.load(fh)
    data[key] = value
    with open(PROFILE, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)
        fh.write("\n")


def _run(cases, pr3, method="measured"):
    """(worst |exact - coarse| / eps, contender counts of the pruned candidates, fallbacks, largest delta) over the cases."""
    worst, cont, fallbacks, dmax = 0.0, [], 0, 0.0
    for I, Q, fc, drift, sc in cases:
        got = ld.coarse_pass(I, Q, fc, drift, sc, pr3, method=method)
        if got is None:
            fallbacks += 1
            continue
        sync, eps, dtab = got
        exact = np.array([ld.oracle_sync(I, Q, fc, drift, sc, m) for m in range(ld.NLAG)], np.float32)
        diff = np.abs(exact.astype(np.float64) - sync.astype(np.float64))
        assert (diff <= eps).all(), (fc, drift, sc, float((diff / eps).max()))
        worst, dmax = max(worst, float((diff / eps).max())), max(dmax, dtab)
        c = ld.contenders(sync, eps)
        assert c[ld.first_strict_maximum(exact)], (fc, drift, sc)
        if c.sum() > ld.CAP:
            fallbacks += 1
        else:
            cont.append(int(c.sum()))
    return worst, cont, fallbacks, dmax


def test_the_recurrence_stays_inside_its_a_priori_bound():
    """(a) measured delta <= bound for f0 in [-110, 110] Hz, drift in [-4, 4], the four tones, symbols 0, 81 and 161, under both
    arithmetic policies (largest measured / bound 0.19 exact, 0.20 contracted; the bound itself <= 5.7e-5).  The kernel does not use
    this bound (it measures delta, method (ii)); the sweep says what the measurement is expected to find and that (i) is sound."""
    rng = np.random.default_rng(11)
    f0 = np.concatenate([np.linspace(-110, 110, 41), rng.uniform(-110, 110, 80)])
    dr = np.concatenate([np.linspace(-4, 4, 41), rng.uniform(-4, 4, 80)])
    theta = np.concatenate([ld.tone_dphi(f, d, np.array([0, 81, 161]), t) for f, d in zip(f0, dr) for t in range(4)])
    bound = ld.delta_bound(theta)
    assert np.isfinite(bound).all() and bound.max() < 1e-4
    out = {"thetas": int(theta.size), "largest_bound": float(bound.max())}
    for name, contracted in (("exact", False), ("contracted", True)):
        got = ld.measured_delta(theta, contracted)
        ratio = float((got / bound).max())
        print("%s: %d thetas, largest measured delta %.3e, largest measured / bound %.3f" % (name, theta.size, got.max(), ratio))
        assert (got <= bound).all()
        out[name] = {"largest_measured": float(got.max()), "largest_ratio": round(ratio, 4)}
    _record("delta_sweep", out)


def test_coarse_sync_of_drifting_candidates_is_within_its_bound_of_the_oracle():
    """(a) the drift-free candidates of test_lag_bound_cpu given drifts of +-0.5, +-1, 2.5, -4: max |exact - coarse| / eps <= 1 and
    the reference's pick is a contender."""
    cases = ld.soundness_cases()
    worst, cont, fallbacks, dmax = _run(cases, la.pr3())
    print("candidates %d, max |exact - coarse| / eps %.5f, mean contenders %.2f, fallbacks %d, largest delta %.3e"
          % (len(cases), worst, float(np.mean(cont)), fallbacks, dmax))
    assert len(cases) >= 60 and worst <= 1.0
    _record("soundness", {"candidates": len(cases), "max_ratio_diff_over_eps": round(worst, 5),
                          "mean_contenders": round(float(np.mean(cont)), 2), "fallbacks": fallbacks, "largest_delta": dmax})


def test_the_caps_hold_on_the_drifting_candidates_of_config3_segments():
    """(b) the drifting candidates the reference refines in 16 configs[2]-shaped segments: sound as above, fallbacks <= 10 % and
    exact evaluations <= 3.0 per pruned candidate -- the conditions tests/test_gpu_lag_prune.py sets for drift-free ones -- with
    delta measured on the recurrence (method (ii): 3 of 30 fall back, 1.52 evaluations per pruned candidate).  With the a priori
    bound (method (i)) 4 of 30 fall back, which is over the cap: recorded, and the reason the kernel measures."""
    cases, visited = ld.config3_drifting()
    _, cont_i, fallbacks_i, dmax_i = _run(cases, la.pr3(), "a priori")
    _record("config3_a_priori", {"drifting": len(cases), "fallback_share": round(fallbacks_i / max(1, len(cases)), 4),
                                 "evaluations_per_pruned": round(float(np.mean(cont_i)), 3), "largest_delta": dmax_i})
    worst, cont, fallbacks, dmax = _run(cases, la.pr3())
    hist = {str(n): cont.count(n) for n in sorted(set(cont))}
    print("visited %d, drifting %d, max ratio %.5f, contender histogram %s, fallbacks %d, evaluations per pruned %.2f"
          % (visited, len(cases), worst, hist, fallbacks, float(np.mean(cont))))
    _record("config3", {"candidates_visited": visited, "drifting": len(cases), "max_ratio_diff_over_eps": round(worst, 5),
                        "contender_histogram": hist, "fallback_share": round(fallbacks / max(1, len(cases)), 4),
                        "evaluations_per_pruned": round(float(np.mean(cont)), 3), "largest_delta": dmax, "delta_method": "measured"})
    assert len(cases) >= 16 and worst <= 1.0
    assert fallbacks <= 0.10 * len(cases)
    assert sum(cont) <= 3.0 * len(cont)
