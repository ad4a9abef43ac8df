"""The lag pruning of the fine search's mode-0 scan (k4_lag_prune.h: lag_coarse_kernel picks the lags that can still win,
lag_exact_kernel sums those, the whole strided scan is the fallback) must leave every candidate's mode-0 result -- and
with it everything downstream -- what the oracle computes: all of it through wspr_decode_batch_trace() and
trace_parity.check, on inputs made to reach the corners of the new path.  The counts come from the LAB library's
wspr_last_timings() ([29] pruned, [30] exact single-lag evaluations, [31] fallbacks)."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import oracle_lib as ol
import synth
import trace_parity as tp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = 45000
symf = lambda msg: ol.channel_symbols(msg)[1]


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    return mod


def lag_counts(w):
    """(pruned, exact evaluations, fallbacks) of the lab library's most recent batch call."""
    ms = (C.c_double * len(w.TIMING_NAMES))()
    n = w.lab().wspr_last_timings(C.addressof(ms), len(w.TIMING_NAMES))
    t = {w.TIMING_NAMES[i]: ms[i] for i in range(n)}
    return int(t["lag_pruned"]), int(t["lag_exact_evals"]), int(t["lag_fallbacks"])


def test_exact_ties_and_an_all_zero_segment(w):
    """(i) IQ with a period of 8 samples (a carrier at 375 / 8 Hz): one lag step shifts the record by exactly one period,
    so the interior lags tie bit for bit and the first of them must win -- every lag is a contender, which is more than
    the cap, so these candidates take the whole scan.  And an all-zero segment (totp == 0: the metric is 0 / 0)."""
    n = np.arange(NS)
    pat_i = (0.5 * np.cos(2 * np.pi * np.arange(8) / 8)).astype(np.float32)
    pat_q = (0.5 * np.sin(2 * np.pi * np.arange(8) / 8)).astype(np.float32)
    I = np.stack([pat_i[n % 8], np.zeros(NS, np.float32)])
    Q = np.stack([pat_q[n % 8], np.zeros(NS, np.float32)])
    total, _ = tp.check(I, Q, w, ol, None, "ties")
    pruned, evals, fallbacks = lag_counts(w)
    print("ties: candidates %d, pruned %d, exact evaluations %d, fallbacks %d" % (total, pruned, evals, fallbacks))
    assert total >= 1 and fallbacks >= 1


def test_signals_hanging_over_both_ends_of_the_record(w):
    """(ii) A signal that starts 0.3 s before the record (k <= 0 is skipped, index 0 included: wsprd.c:199), one at the
    latest start that still fits (45 000 - 162 x 256 samples in), and one at the late end of the coarse search's range."""
    segs = []
    for seed, t0 in ((1, -0.3), (2, (NS - 162 * 256) / 375.0), (3, 7.4)):
        rng = np.random.default_rng(seed)
        sigma = np.sqrt((375.0 / 2500.0) / 2.0)
        I, Q = rng.normal(0, sigma, NS), rng.normal(0, sigma, NS)
        si, sq = synth.tone_signal(symf(synth.message_for(seed)), 20.0 * seed - 35.0, t0, 10.0 ** (-12.0 / 20.0))
        segs.append(synth.normalise((I + si).astype(np.float32), (Q + sq).astype(np.float32)))
    I, Q = np.stack([s[0] for s in segs]), np.stack([s[1] for s in segs])
    total, _ = tp.check(I, Q, w, ol, None, "edges")
    pruned, evals, fallbacks = lag_counts(w)
    print("edges: candidates %d, pruned %d, exact evaluations %d, fallbacks %d" % (total, pruned, evals, fallbacks))
    assert total >= 3 and pruned >= 1


def test_one_sample_at_full_scale_the_rest_60_db_down(w):
    """(iii) One sample at full scale (0.5), everything else 60 dB below it: a carrier of amplitude 5e-4 at 10 Hz (with
    ordinary noise and signals scaled 60 dB below the spike the decoder finds no candidate at all: the spike's flat
    spectrum buries every peak).  The carrier's candidate has the spike inside one window of every lag, at full scale
    against amplitudes near 0.13.  What sends it to the whole scan is not the size of the T-bound (the spike adds 0.5 to
    a sum of T of 26 and 2 to a totp of 21: eps stays near 2e-4) but the carrier: the lags that keep the spike in the same
    symbol differ by rounding only, so ten of them are contenders, more than the cap."""
    n = np.arange(NS)
    ph = 2 * np.pi * 10.0 / 375.0 * n
    I, Q = (5e-4 * np.cos(ph)).astype(np.float32), (5e-4 * np.sin(ph)).astype(np.float32)
    I[20000] = 0.5
    total, _ = tp.check(I[None, :], Q[None, :], w, ol, None, "spike")
    pruned, evals, fallbacks = lag_counts(w)
    print("spike: candidates %d, pruned %d, exact evaluations %d, fallbacks %d" % (total, pruned, evals, fallbacks))
    assert total >= 1 and fallbacks >= 1


def _config3(n):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    torch.cuda.set_device(0)
    I, Q, _ = bench.synth_batch_gpu(n, 4321, torch.device("cuda", 0), 10, -10.0, -28.0, 0.3)
    return I.cpu().numpy(), Q.cpu().numpy()


def _check_config3(w, checker, name):
    I, Q = _config3(16)
    total, undecoded = tp.check(I, Q, w, checker, None, name)
    pruned, evals, fallbacks = lag_counts(w)
    print("%s: candidates %d, pruned %d, exact evaluations %d (%.2f each), fallbacks %d (%.1f %%)"
          % (name, total, pruned, evals, evals / max(1, pruned), fallbacks, 100.0 * fallbacks / max(1, pruned + fallbacks)))
    assert total >= 9 * 16 and undecoded >= 16
    # conditions, so that "always falls back" cannot pass
    assert pruned > 0 and fallbacks <= 0.10 * (pruned + fallbacks)
    assert evals <= 3.0 * pruned


def test_config3_segments_prune_and_equal_the_oracle(w):
    """(iv) 16 segments of configs[2] (ten overlapping signals, -10 .. -28 dB): the trace equals the oracle's, at most a
    tenth of the drift-free candidates fall back and a pruned candidate takes at most 3 exact evaluations on average."""
    _check_config3(w, ol, "config3")


def test_config3_segments_under_the_contracted_policy(w):
    """The same under wspr_set_arithmetic(WSPR_ARITH_CONTRACTED) against the contracted checker."""
    import contract_lib as cl
    checker = types.SimpleNamespace(decode=lambda *a, **k: cl.decode(1, *a, **k), default_options=ol.default_options)
    L = w.lab()
    assert w.wspr_set_arithmetic(w.WSPR_ARITH_CONTRACTED, L) == 0
    try:
        _check_config3(w, checker, "config3 contracted")
    finally:
        w.wspr_set_arithmetic(w.WSPR_ARITH_EXACT, L)


def test_the_whole_scan_stays_selectable():
    """(v) WSPR_K4_LAG=full: every drift-free candidate through the strided scan, as before the pruning (the switch is
    read once per process: a subprocess, as tests/test_gpu_trace.py does for the other kept alternatives)."""
    e = dict(os.environ, WSPR_K4_LAG="full", WSPR_TRACE_SCENES="20")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "trace_parity.py"), "parity", "scenes", "loopexits"],
                       env=e, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "TRACE PARITY OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
