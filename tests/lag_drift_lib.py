"""CPU side of the lag pruning of DRIFTING candidates (k4_lag_prune.h: lag_coarse_drift_kernel and its fold kernel; DESIGN.md
section 4 "The bound for drifting candidates"): the coarse pass at one frequency per symbol restated in numpy, the a priori bound
delta_{s,t} on the reference's float phasor recurrence, the oracle's single-lag sync of a drifting candidate, and the case sets of
tests/test_lag_bound_drift_cpu.py and the GPU tests.  The constants are those of tests/test_lag_bound_cpu.py.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os
import subprocess
import types

import numpy as np

import oracle_lib as ol
import synth
from test_lag_bound_cpu import (ABS, CAP, GAMMA_FOLD, GAMMA_REF, COARSE, NS, T_CEIL, T_INFLATE, TOTP_FLOOR, U, _candidates,
                                _libm)

NLAG = 33
REC_STEP = 3 * U                    # the a priori bound's rounding of one step of the float recurrence, either policy
ROTOR_MAX = 1e-7                    # ... and the largest |w - e^{i theta}| it is derived for (the kernel measures delta instead)
DRIFTS = (0.5, -0.5, 1.0, -1.0, 2.5, -4.0)
TWOPIDT = 2.0 * 3.14159265358979323846 * 1.0 / 375.0
OFFS = (-1.5 * 375.0 / 256.0, -0.5 * 375.0 / 256.0, 0.5 * 375.0 / 256.0, 1.5 * 375.0 / 256.0)


def tone_dphi(f0, drift, sym, tone):
    """tone_dphi() of demod_math.h (wsprd.c:158-177): the symbol's frequency on the drift line as a float, the tone's offset in
    double, the product rounded to float.  sym may be an array."""
    sym = np.asarray(sym)
    fp = (float(np.float32(f0)) + (float(np.float32(drift)) / 2.0) * (sym.astype(np.float32) - np.float32(81.0)).astype(np.float64)
          / 81.0).astype(np.float32)
    return (TWOPIDT * (fp.astype(np.float64) + OFFS[tone])).astype(np.float32)


def rotor(theta):
    """(cd, sd) = libm's (cosf, sinf) of float32 thetas, as float32 arrays."""
    th = np.atleast_1d(np.asarray(theta, np.float32))
    return (np.array([_libm.cosf(float(v)) for v in th], np.float32), np.array([_libm.sinf(float(v)) for v in th], np.float32))


def delta_bound(theta):
    """The a priori bound on max_j |tab[j] - e^{i theta j}| of the float recurrence from (1, 0) with the rotor libm gives:
    255 (rho + 3u)(1 + 1e-4), rho = |w - e^{i theta}| (+ 1e-15); NaN where rho exceeds 1e-7 (the kernel then falls back)."""
    th = np.atleast_1d(np.asarray(theta, np.float32)).astype(np.float64)
    cd, sd = rotor(theta)
    rho = np.hypot(cd.astype(np.float64) - np.cos(th), sd.astype(np.float64) - np.sin(th)) + 1e-15
    d = 255.0 * (rho + REC_STEP) * (1 + 1e-4)
    return np.where(rho <= ROTOR_MAX, d, np.nan)


def recurrence_tables(theta, contracted=False):
    """The reference's tables (wsprd.c:174-188) of many thetas at once: complex128 [len(theta)][256] of float32 values.
    contracted: c' = fma(c, cd, -(s sd)), s' = fma(c, sd, s cd) (Arith<true>::mms / mma)."""
    cd, sd = rotor(theta)
    c, s = np.ones(cd.size, np.float32), np.zeros(cd.size, np.float32)
    out = np.empty((cd.size, 256), np.complex128)
    out[:, 0] = 1.0
    for j in range(1, 256):
        if contracted:
            cn = (c.astype(np.float64) * cd - (s * sd).astype(np.float64)).astype(np.float32)
            sn = (c.astype(np.float64) * sd + (s * cd).astype(np.float64)).astype(np.float32)
        else:
            cn = (c * cd) - (s * sd)
            sn = (c * sd) + (s * cd)
        c, s = cn, sn
        out[:, j] = c.astype(np.float64) + 1j * s.astype(np.float64)
    return out


def measured_delta(theta, contracted=False):
    th = np.atleast_1d(np.asarray(theta, np.float32)).astype(np.float64)
    tab = recurrence_tables(theta, contracted)
    return np.abs(tab - np.exp(1j * th[:, None] * np.arange(256)[None, :])).max(axis=1)


def coarse_pass(I, Q, fc, drift, sc, pr3, npts=NS, method="measured", contracted=False):
    """sync~(m), eps(m) of the 33 lags of a drifting candidate as lag_coarse_drift_kernel forms them, or None where the
    kernel would send it to the whole scan; also the largest delta_{s,t}."""
    k0 = sc - 128
    k = k0 + np.arange(163 * 256)
    ok = (k > 0) & (k < npts)
    x = np.zeros(k.size, np.complex64)
    x[ok] = I[k[ok]] + 1j * Q[k[ok]]
    tb = (np.abs(x.real) + np.abs(x.imag)).astype(np.float32)[:8 * 5216].reshape(5216, 8).sum(axis=1, dtype=np.float32)
    X = np.lib.stride_tricks.sliding_window_view(x, 512)[::256][:162]            # [162][512]: the samples from 256 s on
    sym = np.arange(162)
    P = np.empty((162, NLAG, 4), np.float32)
    dtab = 0.0
    for t in range(4):
        theta = tone_dphi(fc, drift, sym, t)
        if method == "measured":                                # what the kernel does
            d = measured_delta(theta, contracted)
        else:
            d = delta_bound(theta)
            if np.isnan(d).any():
                return None
        dtab = max(dtab, float(d.max()))
        th = theta.astype(np.float64)
        e3 = np.exp(-1j * th[:, None] * np.arange(8)[None, :]).astype(np.complex64)
        anchor = np.exp(-1j * th[:, None] * 8.0 * np.arange(64)[None, :]).astype(np.complex64)
        blk = (X.reshape(162, 64, 8) * e3[:, None, :]).sum(axis=2, dtype=np.complex64) * anchor
        w = blk[:, 0:NLAG].copy()
        for i in range(1, 32):
            w = w + blk[:, i:i + NLAG]
        P[:, :, t] = np.abs(w)
    sync, eps = np.empty(NLAG, np.float32), np.empty(NLAG)
    sign = np.where(np.asarray(pr3) == 1, 1.0, -1.0).astype(np.float32)
    for m in range(NLAG):
        p = P[:, m, :]
        totp = p.sum(dtype=np.float32)
        ss = (sign * ((p[:, 1] + p[:, 3]) - (p[:, 0] + p[:, 2]))).sum(dtype=np.float32)
        T = float(tb[m:m + 5184].sum(dtype=np.float64)) * T_INFLATE
        S, dt = float(totp), dtab * (1 + 1e-6) + 1e-12
        kappa = dt + (GAMMA_REF + 3 * U * (1 + GAMMA_REF)) * (1 + dt) + COARSE
        E = 4 * kappa * T + GAMMA_FOLD * (S + 4 * kappa * T) + ABS
        if not (S >= TOTP_FLOOR and S > 4 * E and T < T_CEIL):
            return None
        r = abs(float(ss)) / S
        sync[m] = ss / totp
        eps[m] = (E * (1 + r) / (S - E) + 4 * U * (1 + r)) * (1 + 1e-6)
    return sync, eps, dtab


def oracle_sync(I, Q, fc, drift, sc, m, npts=NS, sync_demod=None):
    """The reference's mode-0 sync of the single lag m of a drifting candidate."""
    f, sh, dr, sy = C.c_float(fc), C.c_int(sc), C.c_float(drift), C.c_float(0.0)
    sym = (C.c_ubyte * 162)()
    lag = sc - 128 + 8 * m
    (sync_demod or ol.lib().orc_sync_demod)(ol.ptr(I), ol.ptr(Q), C.c_long(npts), sym, C.addressof(f), 0, 0, C.c_float(0.0),
                                            C.addressof(sh), lag, lag, 8, C.addressof(dr), 50, C.addressof(sy), 0)
    return np.float32(sy.value)


def contenders(sync, eps):
    """The contender rule on float64 eps as tests/test_lag_bound_cpu.py applies it: boolean [33]."""
    return sync + eps >= (sync - eps).max()


def first_strict_maximum(sync):
    best, win = np.float32(-1e30), -1                           # wsprd.c:227-232
    for m in range(NLAG):
        if sync[m] > best:
            best, win = sync[m], m
    return win


def soundness_cases():
    """The drift-free candidates of tests/test_lag_bound_cpu.py given drifts of +-0.5, +-1, 2.5, -4 in turn: (I, Q, fc, drift, sc)."""
    return [(I, Q, fc, DRIFTS[i % len(DRIFTS)], sc) for i, (I, Q, fc, sc) in enumerate(_candidates())]


@functools.lru_cache(maxsize=None)
def config3_drifting(nseg=16):
    """The drifting candidates the reference refines in 16 configs[2]-shaped segments (ten signals, -10 .. -28 dB, the CPU
    generator's twins of tests/test_gpu_lag_prune.py::_config3): the oracle's own coarse candidates of every pass it ran, from
    its trace.  Returns (list of (I, Q, fc, drift, sc), number of candidates visited)."""
    symf = lambda msg: ol.channel_symbols(msg)[1]
    out, visited = [], 0
    for seg in range(nseg):
        I, Q, _ = synth.make_segment(4321 + seg, symf, n_signals=10, snr_db=-10.0, snr_span=18.0, t_jitter=0.3)
        tr = ol.decode(I, Q, trace=True)[3]
        for p in range(tr.passes_run):
            for i in range(tr.n_visited[p]):
                c = tr.cand_coarse[p][i]
                visited += 1
                if c.drift != 0.0:
                    out.append((I, Q, float(c.freq), float(c.drift), int(c.shift)))
    return out, visited


def ideal(I, Q, fc, drift, sc, npts=NS, pr3=None):
    """The quantities the proof talks about, in float64, for the 33 lags of a drifting candidate: sync_id = ss_id / S_id from the
    magnitudes of the 256-sample windows mixed with each symbol's own float theta, widened; samples outside 0 < k < npts skipped
    as the reference does; T = sum of |x_I| + |x_Q| over the lag's 41 472 samples."""
    k = sc - 128 + np.arange(163 * 256)
    ok = (k > 0) & (k < npts)
    xi, xq = np.zeros(k.size), np.zeros(k.size)
    xi[ok], xq[ok] = I[k[ok]], Q[k[ok]]
    with np.errstate(all="ignore"):
        x = xi + 1j * xq
        tb = (np.abs(xi) + np.abs(xq))[:8 * 5216].reshape(5216, 8).sum(axis=1)
        X = np.lib.stride_tricks.sliding_window_view(x, 512)[::256][:162]
        P = np.empty((162, NLAG, 4))
        for t in range(4):
            th = tone_dphi(fc, drift, np.arange(162), t).astype(np.float64)
            blk = (X * np.exp(-1j * th[:, None] * np.arange(512)[None, :])).reshape(162, 64, 8).sum(axis=2)
            w = blk[:, 0:NLAG].copy()
            for i in range(1, 32):
                w = w + blk[:, i:i + NLAG]
            P[:, :, t] = np.abs(w)
        sign = np.where(np.asarray(pr3) == 1, 1.0, -1.0)
        S = P.sum(axis=(0, 2))
        ss = (sign[:, None] * ((P[:, :, 1] + P[:, :, 3]) - (P[:, :, 0] + P[:, :, 2]))).sum(axis=0)
        T = np.array([tb[m:m + 5184].sum() for m in range(NLAG)])
        return types.SimpleNamespace(sync=ss / S, S=S, ss=ss, T=T)


# ---- tools/lagprune_check.hip with its "drift" option: case file in, dump out (tests/lag_audit_lib.py: run_tool, plus the
# drifting candidates' lists and counts) ----
CD_WAVES, CD_PART = 11, 68          # kCdWaves, kCdPart


def run_tool(tmpdir, I, Q, runs):
    """As lag_audit_lib.run_tool(), with LagPrune::drift on.  Every run's namespace also has exact_list_d, fb_list_d (the drifting
    candidates' lists) and counts_d (exact evaluations, fallbacks, pruned)."""
    import lag_audit_lib as la
    I, Q = np.asarray(I, np.float32), np.asarray(Q, np.float32)
    nseg = I.shape[0]
    rows = np.zeros((2, nseg, la.KIQ), np.float32)
    rows[0, :, :I.shape[1]], rows[1, :, :Q.shape[1]] = I, Q
    case, out = os.path.join(str(tmpdir), "case.bin"), os.path.join(str(tmpdir), "out.bin")
    with open(case, "wb") as fh:
        fh.write(np.array([0x3143504C, nseg, len(runs)], "<i4").tobytes())
        fh.write(la.pr3().tobytes() + b"\0\0")
        fh.write(rows.tobytes())
        for r in runs:
            ls, lo = np.asarray(r["list_shared"], "<i4"), np.asarray(r["list_own"], "<i4")
            fh.write(np.array([r["np"], r["arith"], len(r["items"]), ls.size, lo.size], "<i4").tobytes())
            fh.write(r["items"].tobytes() + ls.tobytes() + lo.tobytes())
    # WSPR_LAGPRUNE_TOOL: another build of the tool (a mutated kernel file: DESIGN.md section 4, "Mutations")
    p = subprocess.run([os.environ.get("WSPR_LAGPRUNE_TOOL") or la.tool(), case, out, "drift"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-1000:], p.stderr[-2000:])
    buf = open(out, "rb").read()
    res, o = [], 0

    def take(dtype, count, shape=None):
        nonlocal o
        a = np.frombuffer(buf, dtype, count, o).copy()
        o += a.nbytes
        return a.reshape(shape) if shape else a
    for r in runs:
        n, ns, no, sb = (int(v) for v in take("<i4", 4))
        assert (n, ns, no) == (len(r["items"]), len(r["list_shared"]), len(r["list_own"]))
        g = types.SimpleNamespace(n=n, n_shared=ns, n_own=no, np=r["np"], arith=r["arith"], items=r["items"],
                                  list_shared=list(r["list_shared"]), list_own=list(r["list_own"]))
        g.tabs = take("<f4", n * 2048, (n, 256, 8))
        g.items_a, g.items_b = take(la.FINE, n), take(la.FINE, n)
        g.sync_a, g.sync_b = take("<f4", n * NLAG, (n, NLAG)), take("<f4", n * NLAG, (n, NLAG))
        g.pw_a, g.pw_b = take("<f4", n * NLAG * 648, (n, NLAG, 648)), take("<f4", n * NLAG * 648, (n, NLAG, 648))
        scratch = take(np.uint8, sb)
        g.mask = scratch[:8 * n].view("<u8")
        g.exact_list = scratch[8 * n:8 * n + 16 * ns].view("<i4")
        g.fb_list = scratch[8 * n + 16 * ns:8 * n + 20 * ns].view("<i4")
        d0 = (28 * n + 15) & ~15                                # lag_prune_scratch_bytes(): the drifting candidates' part
        g.exact_list_d = scratch[d0:d0 + 16 * n].view("<i4")
        g.fb_list_d = scratch[d0 + 16 * n:d0 + 20 * n].view("<i4")
        assert sb == d0 + ((n * (5 + CD_WAVES * CD_PART) * 4 + 15) & ~15)
        g.counts = take("<i4", 4)[:3]
        g.audit = take("<f4", n * NLAG * la.AUDIT, (n, NLAG, la.AUDIT))
        g.counts_d = take("<i4", 4)[:3]
        res.append(g)
    assert o == len(buf)
    os.remove(case)
    os.remove(out)
    return res
