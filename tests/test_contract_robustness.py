"""What the contracted arithmetic changes in the spots (tools/contract_robustness.py, profiles/contracted_robustness.json),
on CPU: the committed result covers configs[1] and the 3 000 scenes (configs[2], `--workloads c2`, is not in it yet), and a
fixed sample of the study's own segments, decoded again here, stays within what that result reports; a sample of configs[2]
is held to the same absolute limits."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
RESULT = os.path.join(ROOT, "profiles", "contracted_robustness.json")


def test_committed_study_covers_the_three_workloads():
    r = json.load(open(RESULT))
    wl = r["workloads"]
    assert (wl["c1"]["segments"], wl["scenes"]["segments"]) == (1024, 3000)
    for name, b in wl.items():
        assert b["spots_text_changed"] == 0, name                 # no call/loc/pwr ever changes under one message text
        assert b["spots_beyond_tolerance_fraction"] <= 0.001, name
        assert b["max_dsnr_db"] < 0.1 and b["max_dfreq_hz"] <= 0.1, name
        assert b["spots_variant"] >= 0.999 * b["spots_base"], name


@pytest.mark.parametrize("wl,n", [("c1", 24), ("scenes", 24), ("c2", 6)])
def test_a_sample_stays_within_the_committed_result(wl, n):
    import contract_robustness as cr
    import fft_robustness as fr
    a = type("A", (), {"n_c1": n, "n_c2": n, "n_scenes": n, "threads": min(8, os.cpu_count() or 1)})()
    segs = cr.segments(wl, a)
    got = cr.study(segs, a.threads)
    assert got["segments"] == n and got["spots_base"] > 0
    assert got["spots_text_changed"] == 0 and got["max_dsnr_db"] < 0.1 and got["max_dfreq_hz"] <= 0.1
    assert fr.TOL == json.load(open(RESULT))["tolerances"]
    if wl not in json.load(open(RESULT))["workloads"]:
        return
    full = json.load(open(RESULT))["workloads"][wl]
    for k in ("spots_text_changed", "segments_spot_set_differs", "spots_beyond_tolerance", "spots_lost", "spots_gained",
              "spots_drift_changed", "spots_jitter_changed", "spots_cycles_changed", "segments_coarse_candidates_differ"):
        assert got[k] <= full[k], (wl, k, got[k], full[k])
    for k in ("max_dsnr_db", "max_ddt_s", "max_dfreq_hz"):
        assert got[k] <= full[k], (wl, k)
