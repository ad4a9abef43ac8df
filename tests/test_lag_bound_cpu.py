"""The bound of the lag pruning (k4_lag_prune.h: lag_coarse_kernel; DESIGN.md section 4 "The bound of the lag pruning"), restated in
numpy and held against the oracle's own sync of every single lag: for a drift-free candidate the sync of lag m formed
from sliding block sums of ONE mixed-down stream per tone differs from the reference's by at most eps(m), and the lag
the reference picks is therefore among the contenders.  The constants are the derivation's, not tuned to this data;
the largest observed |exact - coarse| / eps goes to profiles/lag_prune_bound.json (a ratio anywhere near 1 would mean
that a term is missing)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as ol
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = 45000
_libm = C.CDLL("libm.so.6")
for _f in (_libm.sinf, _libm.cosf):
    _f.argtypes, _f.restype = [C.c_float], C.c_float

# ---- the derivation's constants (kLp* of k4_lag_prune.h) ----
U = 2.0 ** -24
GAMMA_REF = 514 * U / (1 - 514 * U)              # (a) the reference's serial sum: 514 roundings per term
COARSE = 64 * U                                  # (c) the coarse pass' own rounding
T_INFLATE = 1 + 256 * U                          # T~ is itself a rounded sum
GAMMA_FOLD = 648 * U / (1 - 648 * U) + 700 * U / (1 - 700 * U)     # (d) the two folds of totp and ss
ABS = 1e-15
TOTP_FLOOR, T_CEIL = 1e-9, 1e18
CAP = 4


def tone_dphi(f0, tone):
    """tone_dphi() of k4_demod.hip (wsprd.c:158-177) without drift: a float."""
    off = (-1.5, -0.5, 0.5, 1.5)[tone] * (375.0 / 256.0)
    return np.float32((2.0 * 3.14159265358979323846 * 1.0 / 375.0) * (float(np.float32(f0)) + off))


def reference_table(dphi):
    """The float recurrence of wsprd.c:174-188 from libm's sinf/cosf: (c[256], s[256])."""
    cd, sd = np.float32(_libm.cosf(float(dphi))), np.float32(_libm.sinf(float(dphi)))
    c, s = np.empty(256, np.float32), np.empty(256, np.float32)
    c[0], s[0] = 1.0, 0.0
    for j in range(1, 256):
        c[j] = np.float32(c[j - 1] * cd) - np.float32(s[j - 1] * sd)
        s[j] = np.float32(c[j - 1] * sd) + np.float32(s[j - 1] * cd)
    return c, s


def coarse_pass(I, Q, fc, sc, pr3, npts=NS):
    """sync~(m), eps(m) for the 33 lags, or None where the kernel would send the candidate to the whole scan."""
    k0 = sc - 128
    n = np.arange(8 * 5216)
    k = k0 + n
    ok = (k > 0) & (k < npts)
    x = np.zeros(n.size, np.complex64)
    x[ok] = I[k[ok]] + 1j * Q[k[ok]]
    tb = (np.abs(x.real) + np.abs(x.imag)).astype(np.float32).reshape(5216, 8).sum(axis=1, dtype=np.float32)
    P = np.empty((5185, 4), np.float32)
    dtab = 0.0
    for t in range(4):
        theta = float(tone_dphi(fc, t))
        c, s = reference_table(np.float32(theta))
        j = np.arange(256)
        dtab = max(dtab, float(np.hypot(c - np.cos(theta * j), s - np.sin(theta * j)).max()) * (1 + 1e-6))
        e3 = np.exp(-1j * theta * np.arange(8)).astype(np.complex64)
        blk = (x.reshape(5216, 8) * e3[None, :]).sum(axis=1, dtype=np.complex64)
        blk = blk * np.exp(-1j * theta * 8.0 * np.arange(5216)).astype(np.complex64)
        w = blk[0:5185].copy()
        for i in range(1, 32):                           # the direct sum of 32 block sums, no prefix differences
            w = w + blk[i:i + 5185]
        P[:, t] = np.abs(w)
    sync, eps = np.empty(33, np.float32), np.empty(33)
    sign = np.where(np.asarray(pr3) == 1, 1.0, -1.0).astype(np.float32)
    for m in range(33):
        p = P[32 * np.arange(162) + m]
        totp = p.sum(dtype=np.float32)
        ss = (sign * ((p[:, 1] + p[:, 3]) - (p[:, 0] + p[:, 2]))).sum(dtype=np.float32)
        T = float(tb[m:m + 5184].sum(dtype=np.float64)) * T_INFLATE
        S, dt = float(totp), dtab + 1e-12
        kappa = dt + (GAMMA_REF + 3 * U * (1 + GAMMA_REF)) * (1 + dt) + COARSE
        E = 4 * kappa * T + GAMMA_FOLD * (S + 4 * kappa * T) + ABS
        if not (S >= TOTP_FLOOR and S > 4 * E and T < T_CEIL):
            return None
        r = abs(float(ss)) / S
        sync[m] = ss / totp
        eps[m] = (E * (1 + r) / (S - E) + 4 * U * (1 + r)) * (1 + 1e-6)
    return sync, eps


def oracle_sync(I, Q, fc, sc, m, npts=NS, sync_demod=None):
    """The reference's sync of the single lag m of a record of npts samples; sync_demod: another checker's entry of the
    same signature (contract_lib's ctr_sync_demod) instead of the oracle's."""
    f, sh, dr, sy = C.c_float(fc), C.c_int(sc), C.c_float(0.0), C.c_float(0.0)
    sym = (C.c_ubyte * 162)()
    lag = sc - 128 + 8 * m
    (sync_demod or ol.lib().orc_sync_demod)(ol.ptr(I), ol.ptr(Q), C.c_long(npts), sym, C.addressof(f), 0, 0, C.c_float(0.0),
                                            C.addressof(sh), lag, lag, 8, C.addressof(dr), 50, C.addressof(sy), 0)
    return np.float32(sy.value)


def _candidates():
    """~60 candidates of 4 configs[2]-shaped segments (ten signals, -10 .. -28 dB): every signal at its coarse grid point,
    every other one also a grid step off in time or frequency; plus 8 candidates of a noise-only segment."""
    symf = lambda msg: ol.channel_symbols(msg)[1]
    out = []
    for seg in range(4):
        I, Q, truth = synth.make_segment(4321 + seg, symf, n_signals=10, snr_db=-10.0, snr_span=18.0, t_jitter=0.3)
        for i, (_, f0, t0, _) in enumerate(truth):
            fc = float(np.float32(round(f0 / 0.732421875) * 0.732421875))
            sc = int(round(t0 * 375 / 128.0)) * 128
            out.append((I, Q, fc, sc))
            if i % 2 == 0:
                out.append((I, Q, float(np.float32(fc + (0.732421875 if i % 4 else 0.0))), sc + (128 if i % 4 == 0 else -128)))
    I, Q, _ = synth.make_segment(99, symf, n_signals=1, snr_db=-90.0)
    rng = np.random.default_rng(5)
    for _ in range(8):
        out.append((I, Q, float(np.float32(round(rng.uniform(-100, 100) / 0.732421875) * 0.732421875)),
                    int(rng.integers(2, 9)) * 128))
    return out


def test_coarse_sync_is_within_its_bound_of_the_oracle_and_keeps_the_winner():
    pr3 = np.frombuffer((C.c_ubyte * 162).in_dll(ol.lib(), "orc_sync_vector"), np.uint8).copy()
    worst, contenders, fallbacks, n = 0.0, [], 0, 0
    for I, Q, fc, sc in _candidates():
        got = coarse_pass(I, Q, fc, sc, pr3)
        assert got is not None, (fc, sc)             # ordinary data never needs the fallback for the bound's sake
        sync, eps = got
        exact = np.array([oracle_sync(I, Q, fc, sc, m) for m in range(33)], np.float32)
        diff = np.abs(exact.astype(np.float64) - sync.astype(np.float64))
        assert (diff <= eps).all(), (fc, sc, float((diff / eps).max()))
        worst = max(worst, float((diff / eps).max()))
        best, win = np.float32(-1e30), -1              # wsprd.c:227-232: strict >, first maximum in lag order
        for m in range(33):
            if exact[m] > best:
                best, win = exact[m], m
        lo = (sync - eps).max()
        cont = sync + eps >= lo
        assert cont[win], (fc, sc, win)
        contenders.append(int(cont.sum()))
        fallbacks += int(cont.sum() > CAP)
        n += 1
    print("candidates %d, max |exact - coarse| / eps %.5f, mean contenders %.2f, over the cap %d"
          % (n, worst, float(np.mean(contenders)), fallbacks))
    assert n >= 60 and worst < 1.0
    with open(os.path.join(ROOT, "profiles", "lag_prune_bound.json"), "w") as fh:
        json.dump({"candidates": n, "max_ratio_diff_over_eps": round(worst, 5),
                   "mean_contenders": round(float(np.mean(contenders)), 2), "over_cap_%d" % CAP: fallbacks}, fh, indent=1)
        fh.write("\n")
