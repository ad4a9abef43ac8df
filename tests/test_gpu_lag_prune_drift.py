"""The lag pruning of DRIFTING candidates in the decode pipeline (k4_lag_prune.h: lag_coarse_drift_kernel names the lags that can
still win, lag_exact_kernel<., true> sums those, demod_drift_kernel<., true>, the whole scan over the fallback list, is the fallback) must leave every candidate's mode-0 result --
and with it everything downstream -- what the oracle computes: through wspr_decode_batch_trace() and trace_parity.check, as
tests/test_gpu_lag_prune.py does for the drift-free candidates.  The counts come from the LAB library's wspr_last_timings():
[41] drifting candidates pruned, [42] their exact single-lag evaluations, [43] their fallbacks; [29]..[31] keep counting the
drift-free candidates and must not move."""
import json
import os
import subprocess
import sys
import types

import pytest

import oracle_lib as ol
import trace_parity as tp
from test_gpu_lag_prune import ROOT, _config3, lag_counts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    return mod


def drift_counts(w):
    """(pruned, exact evaluations, fallbacks) among the drifting candidates of the lab library's most recent batch call."""
    import ctypes as C
    ms = (C.c_double * len(w.TIMING_NAMES))()
    n = w.lab().wspr_last_timings(C.addressof(ms), len(w.TIMING_NAMES))
    t = {w.TIMING_NAMES[i]: ms[i] for i in range(n)}
    return int(t["lag_drift_pruned"]), int(t["lag_drift_exact_evals"]), int(t["lag_drift_fallbacks"])


def _check_config3(w, checker, name):
    I, Q = _config3(16)
    total, undecoded = tp.check(I, Q, w, checker, None, name)
    free, (pruned, evals, fallbacks) = lag_counts(w), drift_counts(w)
    print("%s: candidates %d; drifting: pruned %d, exact evaluations %d (%.2f each), fallbacks %d (%.1f %%); drift-free %s"
          % (name, total, pruned, evals, evals / max(1, pruned), fallbacks, 100.0 * fallbacks / max(1, pruned + fallbacks), free))
    assert total >= 9 * 16 and undecoded >= 16
    # the caps of tests/test_lag_bound_drift_cpu.py, so that "always falls back" cannot pass
    assert pruned > 0 and evals > 0
    assert fallbacks <= 0.10 * (pruned + fallbacks)
    assert evals <= 3.0 * pruned
    return free, (pruned, evals, fallbacks)


def test_config3_segments_prune_drifting_candidates_and_equal_the_oracle(w):
    """16 segments of configs[2]: the trace equals the oracle's; the drifting candidates' counts are nonzero and inside the caps;
    the drift-free counts equal what WSPR_K4_LAG=nodrift gives on the same call (a subprocess: the switch is read once)."""
    free, drifting = _check_config3(w, ol, "config3 drift")
    e = dict(os.environ, WSPR_K4_LAG="nodrift")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "counts"], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["drift_free"] == list(free) and got["drifting"] == [0, 0, 0], (got, free, drifting)


def test_config3_segments_under_the_contracted_policy(w):
    """The same under wspr_set_arithmetic(WSPR_ARITH_CONTRACTED) against the contracted checker."""
    import contract_lib as cl
    checker = types.SimpleNamespace(decode=lambda *a, **k: cl.decode(1, *a, **k), default_options=ol.default_options)
    L = w.lab()
    assert w.wspr_set_arithmetic(w.WSPR_ARITH_CONTRACTED, L) == 0
    try:
        _check_config3(w, checker, "config3 drift contracted")
    finally:
        w.wspr_set_arithmetic(w.WSPR_ARITH_EXACT, L)


def test_trace_parity_with_the_default():
    """Trace parity of the parity batch, 20 scenes and the loop-exit cases with drifting candidates pruned (the default)."""
    e = dict(os.environ, WSPR_TRACE_SCENES="20")
    e.pop("WSPR_K4_LAG", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "trace_parity.py"), "parity", "scenes", "loopexits"],
                       env=e, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "TRACE PARITY OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


if __name__ == "__main__" and sys.argv[1:] == ["counts"]:
    sys.path.insert(0, ROOT)
    import rtlsdr_wsprd_amd as mod
    I, Q = _config3(16)
    tp.check(I, Q, mod, ol, None, "config3 nodrift")
    print(json.dumps({"drift_free": list(lag_counts(mod)), "drifting": list(drift_counts(mod))}))
