"""CPU side of the coarse-kernel audit (tests/test_gpu_lag_coarse.py, tests/test_lag_audit_cpu.py): the float64 references
of what lag_coarse_kernel computes (k4_lag_prune.h; DESIGN.md section 4 "The bound of the lag pruning"), the bound restated
from the kernel's own audit numbers, the contender rule in float32, and the case / output files of tools/lagprune_check.hip.
The kernel's pass in numpy (coarse_pass), the oracle's single-lag sync and the candidates are those of
tests/test_lag_bound_cpu.py.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import json
import os
import subprocess
import types

import numpy as np

import oracle_lib as ol
from test_lag_bound_cpu import (ABS, CAP, GAMMA_FOLD, GAMMA_REF, COARSE, NS, T_CEIL, T_INFLATE, TOTP_FLOOR, U, _candidates,
                                coarse_pass, oracle_sync, tone_dphi)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIQ = 45056                        # kIqStride
NLAG = 33
AUDIT = 7                          # kLpAuditStride: sy, ep, totp, ss, tm, dtab, bad (1.0 / 0.0)
SENTINEL = 0xA5                    # what tools/lagprune_check.hip fills every output buffer with
GAMMA_700 = 700 * U / (1 - 700 * U)
KAPPA_C = 64 * U * (1 + 256 * U)
FINE = np.dtype([("seg", "<i4"), ("freq", "<f4"), ("drift", "<f4"), ("shift", "<i4"), ("sync", "<f4"),
                 ("shift_coarse", "<i4"), ("freq_coarse", "<f4"), ("pad", "<i4")])
PROFILE = os.path.join(ROOT, "profiles", "lag_coarse_audit.json")


def pr3():
    return np.frombuffer((C.c_ubyte * 162).in_dll(ol.lib(), "orc_sync_vector"), np.uint8).copy()


# ---- float64 references -------------------------------------------------------------------------------------------------
def ideal(I, Q, fc, sc, npts=NS):
    """The quantities the proof talks about, in float64, for the 33 lags: sync_id = ss_id / S_id from the magnitudes
    |W_t(u)| of the mixed-down stream's 256-sample windows (theta = the float tone_dphi, widened; samples outside
    0 < k < npts skipped as the reference does), and T = sum of |x_I| + |x_Q| over the lag's 41 472 samples."""
    k = sc - 128 + np.arange(8 * 5216)
    ok = (k > 0) & (k < npts)
    xi, xq = np.zeros(k.size), np.zeros(k.size)
    xi[ok], xq[ok] = I[k[ok]], Q[k[ok]]
    with np.errstate(all="ignore"):
        x = xi + 1j * xq
        tb = (np.abs(xi) + np.abs(xq)).reshape(5216, 8).sum(axis=1)
        P = np.empty((5185, 4))
        n = np.arange(k.size, dtype=np.float64)
        for t in range(4):
            blk = (x * np.exp(-1j * float(tone_dphi(fc, t)) * n)).reshape(5216, 8).sum(axis=1)
            w = blk[0:5185].copy()
            for i in range(1, 32):
                w = w + blk[i:i + 5185]
            P[:, t] = np.abs(w)
        sign = np.where(pr3() == 1, 1.0, -1.0)
        S, ss, T = np.empty(NLAG), np.empty(NLAG), np.empty(NLAG)
        for m in range(NLAG):
            p = P[32 * np.arange(162) + m]
            S[m] = p.sum()
            ss[m] = (sign * ((p[:, 1] + p[:, 3]) - (p[:, 0] + p[:, 2]))).sum()
            T[m] = tb[m:m + 5184].sum()
        return types.SimpleNamespace(sync=ss / S, S=S, ss=ss, T=T)


def eps_c(idl):
    """Term (c) of the derivation alone -- the coarse pass' own rounding against exact arithmetic on the same phasors:
    E_c (1 + r) / (S - E_c) + 4u (1 + r), E_c = 4 kappa_c T + gamma_700 (S + 4 kappa_c T) + 1e-15, kappa_c = 64u (1 + 256u).
    Returns (eps_c, valid): valid where the derivation's preconditions hold for the float64 quantities."""
    with np.errstate(all="ignore"):
        E = 4 * KAPPA_C * idl.T + GAMMA_700 * (idl.S + 4 * KAPPA_C * idl.T) + ABS
        r = np.abs(idl.ss) / idl.S
        e = E * (1 + r) / (idl.S - E) + 4 * U * (1 + r)
        valid = np.isfinite(e) & np.isfinite(idl.sync) & (idl.S >= TOTP_FLOOR) & (idl.S > 4 * E) & (idl.T < T_CEIL)
    return e, valid


def eps_from_audit(totp, ss, tm, dtab):
    """DESIGN's eps(m) in float64 from the kernel's own float sums, paddings included; and the kernel's `ok`."""
    with np.errstate(all="ignore"):
        T, S, dt = tm.astype(np.float64) * T_INFLATE, totp.astype(np.float64), dtab.astype(np.float64) + 1e-12
        kappa = dt + (GAMMA_REF + 3 * U * (1 + GAMMA_REF)) * (1 + dt) + COARSE
        E = 4 * kappa * T + GAMMA_FOLD * (S + 4 * kappa * T) + ABS
        r = np.abs(ss.astype(np.float64)) / S
        eps = (E * (1 + r) / (S - E) + 4 * U * (1 + r)) * (1 + 1e-6)
        sy = ss / totp                                          # float32
        ok = ((S >= TOTP_FLOOR) & (S > 4 * E) & (T < T_CEIL) & (eps == eps) & (eps < 1.0) & (sy == sy) &
              (np.abs(sy) <= np.float32(2.0)))
        return eps * (1 + 1e-6) + 1e-9, ok


def table_distance(tab, fc):
    """d64: the largest distance of a dumped table [256][8] (cos of the four tones, sin of the four tones) from float64 phasors."""
    j = np.arange(256, dtype=np.float64)
    d = 0.0
    for t in range(4):
        th = float(tone_dphi(fc, t))
        d = max(d, float(np.hypot(tab[:, t].astype(np.float64) - np.cos(th * j), tab[:, 4 + t].astype(np.float64) - np.sin(th * j)).max()))
    return d


def contender_rule(sy, ep, bad):
    """The kernel's rule in float32, in its operation order: (mask, fallback, contenders before the cap)."""
    f = np.float32
    with np.errstate(all="ignore"):
        lo = f(-3.0e38)
        for m in range(NLAG):
            l = f(f(sy[m] - ep[m]) - f(1e-6))
            lo = l if l > lo else lo
        mask, n = 0, 0
        for m in range(NLAG):
            if f(f(sy[m] + ep[m]) + f(1e-6)) >= lo:
                mask |= 1 << m
                n += 1
    fallback = bool(np.any(bad)) or n > CAP or n == 0
    return ((1 << NLAG) - 1 if fallback else mask), fallback, n


def first_strict_maximum(sync):
    best, win = np.float32(-1e30), -1                           # wsprd.c:227-232
    for m in range(NLAG):
        if sync[m] > best:
            best, win = sync[m], m
    return win


# ---- the exact reference and the numpy restatement, once per candidate -----------------------------------------------------
def exact_sync(I, Q, fc, sc, npts, arith):
    """The reference's sync of the 33 single lags: the oracle (exact mode) or the CONTRACT=1 checker (contracted mode)."""
    fn = None
    if arith:
        import contract_lib
        fn = contract_lib.contract(1).ctr_sync_demod
    return np.array([oracle_sync(I, Q, fc, sc, m, npts, fn) for m in range(NLAG)], np.float32)


@functools.lru_cache(maxsize=None)
def ordinary():
    """The 68 candidates of test_lag_bound_cpu._candidates() with everything the tests hold against them; computed once
    per process and not modified: list of namespaces (I, Q, fc, sc, idl, eps_c, np_sync, np_eps)."""
    out = []
    for I, Q, fc, sc in _candidates():
        idl = ideal(I, Q, fc, sc)
        ec, valid = eps_c(idl)
        assert valid.all(), (fc, sc)
        sync, eps = coarse_pass(I, Q, fc, sc, pr3())
        out.append(types.SimpleNamespace(I=I, Q=Q, fc=fc, sc=sc, idl=idl, eps_c=ec, np_sync=sync, np_eps=eps))
    return out


def r_np():
    """The yardstick: the numpy restatement's worst |sync_np - sync_id| / eps_c over the ordinary candidates."""
    return max(float((np.abs(c.np_sync.astype(np.float64) - c.idl.sync) / c.eps_c).max()) for c in ordinary())


@functools.lru_cache(maxsize=None)
def fallback_cases():
    """Inputs that must take the whole scan, and one that must not: (name, I, Q, fc, sc, "fallback" | "pruned")."""
    import synth
    symf = lambda msg: ol.channel_symbols(msg)[1]
    n = np.arange(NS)
    rng = np.random.default_rng(77)
    noise = lambda: (rng.normal(0, 0.27, NS).astype(np.float32), rng.normal(0, 0.27, NS).astype(np.float32))
    out = [("zero", np.zeros(NS, np.float32), np.zeros(NS, np.float32), 10.25390625, 256, "fallback")]
    # the carrier of test_gpu_lag_prune.test_exact_ties...: 375 / 8 Hz = 64 grid steps; every window inside the record
    pat_i = (0.5 * np.cos(2 * np.pi * np.arange(8) / 8)).astype(np.float32)
    pat_q = (0.5 * np.sin(2 * np.pi * np.arange(8) / 8)).astype(np.float32)
    out.append(("period8", pat_i[n % 8], pat_q[n % 8], 46.875, 512, "fallback"))
    for scale in (1e20, 1e-30):
        I, Q = noise()
        out.append(("noise_%g" % scale, I * np.float32(scale), Q * np.float32(scale), -21.97265625, 384, "fallback"))
    # one strong signal at its grid point; sample k0 + 41592 lies in the windows of lags 16 .. 32 only, k0 + 41731 in none
    I, Q, truth = synth.make_segment(2024, symf, n_signals=1, snr_db=-8.0, t_jitter=0.3)
    _, f0, t0, _ = truth[0]
    fc, sc = float(np.float32(round(f0 / 0.732421875) * 0.732421875)), int(round(t0 * 375 / 128.0)) * 128
    k0 = sc - 128
    assert k0 > 0 and k0 + 41731 < NS
    for name, k, v, want in (("nan_late_lags", k0 + 41592, np.nan, "fallback"), ("inf_late_lags", k0 + 41592, np.inf, "fallback"),
                             ("nan_beyond", k0 + 41731, np.nan, "pruned")):
        Iv = I.copy()
        Iv[k] = v
        out.append((name, Iv, Q.copy(), fc, sc, want))
    return out


# ---- tools/lagprune_check.hip: case file in, dump out ------------------------------------------------------------------------
def tool():
    exe = os.path.join(ROOT, "tools", "lagprune_check.bin")
    src = os.path.join(ROOT, "tools", "lagprune_check.hip")
    kern = os.path.join(ROOT, "rtlsdr-wsprd_amd", "csrc", "kernels")
    newest = max(os.path.getmtime(os.path.join(kern, f)) for f in ("k4_demod.hip", "k4_lag_prune.h", "wspr_device.h"))
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(newest, os.path.getmtime(src)):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-fno-fast-math", "-I", kern, src, "-o", exe], check=True, capture_output=True)
    return exe


def items_of(cands, segs):
    """FineState records of (seg, fc, sc, drift) tuples."""
    it = np.zeros(len(cands), FINE)
    for i, (seg, fc, sc, drift) in enumerate(cands):
        it[i] = (seg, fc, drift, sc, 0.0, sc, fc, 0)
    assert it["seg"].max() < segs
    return it


def run_tool(tmpdir, I, Q, runs):
    """I, Q: [nseg][NS] float32.  runs: dicts with np, arith, items (FINE), list_shared, list_own.  Returns one namespace per
    run with the dumped buffers."""
    I, Q = np.asarray(I, np.float32), np.asarray(Q, np.float32)
    nseg = I.shape[0]
    rows = np.zeros((2, nseg, KIQ), np.float32)
    rows[0, :, :I.shape[1]], rows[1, :, :Q.shape[1]] = I, Q
    case, out = os.path.join(str(tmpdir), "case.bin"), os.path.join(str(tmpdir), "out.bin")
    with open(case, "wb") as fh:
        fh.write(np.array([0x3143504C, nseg, len(runs)], "<i4").tobytes())
        fh.write(pr3().tobytes() + b"\0\0")
        fh.write(rows.tobytes())
        for r in runs:
            ls, lo = np.asarray(r["list_shared"], "<i4"), np.asarray(r["list_own"], "<i4")
            fh.write(np.array([r["np"], r["arith"], len(r["items"]), ls.size, lo.size], "<i4").tobytes())
            fh.write(r["items"].tobytes() + ls.tobytes() + lo.tobytes())
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
        n, ns, no, sb = (int(v) for v in take("<i4", 4))
        assert (n, ns, no) == (len(r["items"]), len(r["list_shared"]), len(r["list_own"]))
        g = types.SimpleNamespace(n=n, n_shared=ns, n_own=no, np=r["np"], arith=r["arith"], items=r["items"],
                                  list_shared=list(r["list_shared"]), list_own=list(r["list_own"]))
        g.tabs = take("<f4", n * 2048, (n, 256, 8))
        g.items_a, g.items_b = take(FINE, n), take(FINE, n)
        g.sync_a, g.sync_b = take("<f4", n * NLAG, (n, NLAG)), take("<f4", n * NLAG, (n, NLAG))
        g.pw_a, g.pw_b = take("<f4", n * NLAG * 648, (n, NLAG, 648)), take("<f4", n * NLAG * 648, (n, NLAG, 648))
        scratch = take(np.uint8, sb)
        g.mask = scratch[:8 * n].view("<u8")
        g.exact_list = scratch[8 * n:8 * n + 16 * ns].view("<i4")
        g.fb_list = scratch[8 * n + 16 * ns:8 * n + 20 * ns].view("<i4")
        g.counts = take("<i4", 4)[:3]
        g.audit = take("<f4", n * NLAG * AUDIT, (n, NLAG, AUDIT))
        res.append(g)
    assert o == len(buf)
    os.remove(case)
    os.remove(out)
    return res


def record_profile(key, value):
    """profiles/lag_coarse_audit.json, one key per case (read, update, write: the tests run in one process)."""
    data = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            data = json.load(fh)
    data[key] = value
    with open(PROFILE, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)
        fh.write("\n")
