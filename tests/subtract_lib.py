"""CPU side of the K7 table tests (tests/test_phase_table_cpu.py, tests/test_gpu_k7_table.py): the phase cases and the
frame-edge cases, the host's run table in the device layout (tests/helpers/phase_runs_check.cpp), the references of the
residual (the oracle, the CONTRACT=1 checker) and the case / output files of tools/subtract_check.hip.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os
import subprocess
import tempfile
import types

import numpy as np

import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "rtlsdr-wsprd_amd", "csrc", "kernels")
NS = 45000                         # kMaxSamples
KIQ = 45056                        # kIqStride
NSYM, SPS, NSIG = 162, 256, 162 * 256
MAXRUNS = 512                      # kPhaseMaxRuns
TILE, HALO, NTILES = 2048, 180, 21  # kFir8Out, kHalo, kFirWgs
SENTINEL = 0xA5                    # what tools/subtract_check.hip fills the scratch with
TAIL = np.float32(7.0)             # what the case rows hold behind sample 45 000: nothing may read or change it
TWOPIDT = 2.0 * np.pi / 375.0

SUBJOB = np.dtype([("seg", "<i4"), ("f0", "<f4"), ("shift", "<i4"), ("drift", "<f4"), ("sym", "u1", (NSYM,)), ("pad", "u1", (2,))])
RUN = np.dtype([("start", "<i4"), ("m0", "<i4"), ("q", "<i4"), ("e", "<i4")])
TABLE = np.dtype([("runs", RUN, (MAXRUNS,)), ("sym_phi", "<f4", (NSYM,)), ("dphi", "<f4", (NSYM,)), ("first_run", "<u2", (NSYM + 2,))])
assert SUBJOB.itemsize == 180 and TABLE.itemsize == 9816


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_floats(a, b):
    """Equal as bits, except that a NaN is only required to be a NaN at the same samples."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def dphi(f0, drift, sym):
    """test_phase_runs._wspr_dphi for symbols 0..255: wsprd.c:343 in double, rounded to float once."""
    cs = np.asarray(sym, np.uint8).astype(np.float64)
    i = np.arange(NSYM, dtype=np.float64)
    with np.errstate(over="ignore"):
        arg = np.float64(np.float32(f0)) + (np.float64(np.float32(drift)) / 2.0) * (i - 81.0) / 81.0 + (cs - 1.5) * 375.0 / 256.0
        return (TWOPIDT * arg).astype(np.float32)


# ---- the host's tables: tests/helpers/phase_runs_check.cpp ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def helper(src=None):
    """phase_runs_check.cpp compiled for the host (src: another copy of it)."""
    out = os.path.join(tempfile.mkdtemp(prefix="wspr_phase_runs_"), "phase_runs_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", out,
                    src or os.path.join(ROOT, "tests", "helpers", "phase_runs_check.cpp")], check=True)
    L = C.CDLL(out)
    L.phase_runs_check.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.phase_runs_chained_diff.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    L.phase_runs_chained_diff.restype = C.c_long
    L.phase_runs_table.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.phase_table_eval.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p]
    L.phase_table_eval.restype = C.c_long
    return L


def serial_walk(d, max_runs=0):
    """(the reference's float walk of the 41 472 phases, the serial builder's run count at max_runs (0: 512), mismatches of
    the table -- or of the per-symbol fallback, when it overflows -- against the walk)."""
    d = np.ascontiguousarray(d, np.float32)
    phi, bad = np.zeros(NSIG, np.float32), C.c_long(-1)
    nr = helper().phase_runs_check(ol.ptr(d), NSYM, 8, C.addressof(bad), ol.ptr(phi), max_runs)
    return phi, nr, bad.value


def chained_diff(d, width):
    d = np.ascontiguousarray(d, np.float32)
    return helper().phase_runs_chained_diff(ol.ptr(d), NSYM, 8, 0, width)


def host_table(d):
    """The serial builder's table in the device layout, every byte it does not write 0xa5; .nr = the run count or -1."""
    d = np.ascontiguousarray(d, np.float32)
    tb = np.frombuffer(bytes([SENTINEL]) * TABLE.itemsize, TABLE, 1).copy()
    runs, sym_phi, first = (np.ascontiguousarray(tb[0][k]) for k in ("runs", "sym_phi", "first_run"))
    nr = helper().phase_runs_table(ol.ptr(d), NSYM, 8, ol.ptr(runs), ol.ptr(sym_phi), ol.ptr(first))
    return types.SimpleNamespace(nr=nr, runs=runs, sym_phi=sym_phi, first_run=first, dphi=d)


def table_eval(tb):
    """Every sample's phase from a table (host_table() or a dumped one), selected as sub_fir_fused_kernel selects; samples of
    symbols whose run range no builder may leave keep the 0xa5 fill and are counted in the second value."""
    runs, sym_phi, d, first = (np.ascontiguousarray(x) for x in (tb.runs, tb.sym_phi, tb.dphi, tb.first_run))
    assert runs.dtype == RUN and runs.size == MAXRUNS and first.dtype == np.uint16 and first.size == NSYM + 2
    phi = np.frombuffer(bytes([SENTINEL]) * (4 * NSIG), np.float32).copy()
    skipped = helper().phase_table_eval(ol.ptr(runs), ol.ptr(sym_phi), ol.ptr(d), ol.ptr(first), NSYM, 8, ol.ptr(phi))
    return phi, skipped


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _alt(a, b, k=NSYM, tail=0):
    s = np.full(NSYM, tail, np.uint8)
    s[0:k:2], s[1:k:2] = a, b
    return s


def _rand(seed, hi=4):
    return np.random.default_rng(seed).integers(0, hi, NSYM).astype(np.uint8)


# Found by a CPU search over K leading symbols alternating 1,2, a constant tail tone and changed single symbols (23 328
# candidates with one changed symbol reach 511 runs at most; a second changed symbol on top of the 510-run ones gives 512):
# a walk of exactly 512 runs, the largest table that is not an overflow.
def exact_fit_symbols():
    s = _alt(1, 2, 45, 3)
    s[36], s[101] = 0, 0
    return s


# (name, f0, drift, symbols, nr): nr = runs of the serial builder with the product's table of 512, -1 = overflow (the dense
# path of sub_fir_fused_kernel); tests/test_phase_table_cpu.py recomputes every one.
def phase_cases():
    return [
        ("alt12", 0.0, 0.0, _alt(1, 2), -1),                       # overflows during walks
        ("alt03", 0.0, 0.0, _alt(0, 3), -1),
        ("alt12_f0.01", 0.01, 0.0, _alt(1, 2), -1),
        ("k38_tail3", 0.0, 0.0, _alt(1, 2, 38, 3), 501),
        ("k38_tail0", 0.0, 0.0, _alt(1, 2, 38, 0), 501),
        ("k40_tail3", 0.0, 0.0, _alt(1, 2, 40, 3), -1),            # the 512th run falls inside the constant-tone chain
        ("k40_tail0", 0.0, 0.0, _alt(1, 2, 40, 0), -1),
        ("zero_rand", 0.0, 0.0, _rand(11), 320),
        ("tiny_rand", 1e-30, 0.0, _rand(12), 304),
        ("f1e6", 1e6, 0.0, _rand(13), 179),
        ("f-1e9_d4", -1e9, 4.0, _rand(14), 179),
        ("f10_d1e4", 10.0, 1e4, _rand(15), 183),
        ("sym255", 0.0, 0.0, _rand(16, 256), 179),
        ("f1e38", 1e38, 0.0, _rand(17), -1),                       # the phases reach +Inf
        ("ord_110", 110.0, -4.0, _rand(18), 178),
        ("ord_-110", -110.0, 4.0, _rand(19), 180),
        ("ord_2.2", 2.2, -4.0, _rand(20), 178),
        ("exact_fit", 0.0, 0.0, exact_fit_symbols(), 512),
    ]


# runs of the overflowing walks with a table of 4 096 (f1e38 overflows that one too: one run per sample once the phase is Inf)
NR_WIDE = {"alt12": 1539, "alt03": 1539, "alt12_f0.01": 1456, "k40_tail3": 518, "k40_tail0": 518}
MIXED = ("ord_110", "alt12", "ord_-110", "k40_tail3", "k38_tail3")      # the one launch with dense and run-table jobs side by side


def case_named(name):
    return next(c for c in phase_cases() if c[0] == name)


def job(seg, f0, shift, drift, sym):
    j = np.zeros(1, SUBJOB)
    j["seg"], j["f0"], j["shift"], j["drift"], j["sym"] = seg, f0, shift, drift, np.asarray(sym, np.uint8)
    return j


def rows(nseg, seed=5):
    """Synthetic working rows [nseg][kIqStride]: noise and a carrier each, so that every low-pass output is far from zero;
    the stride's tail behind sample 45 000 holds TAIL."""
    rng = np.random.default_rng(seed)
    n = np.arange(NS)
    I, Q = np.full((nseg, KIQ), TAIL, np.float32), np.full((nseg, KIQ), TAIL, np.float32)
    for s in range(nseg):
        ph = 2 * np.pi * (3.0 + 1.7 * s) * n / 375.0
        I[s, :NS] = (0.2 * rng.normal(size=NS) + 0.3 * np.cos(ph)).astype(np.float32)
        Q[s, :NS] = (0.2 * rng.normal(size=NS) + 0.3 * np.sin(ph)).astype(np.float32)
    return I, Q


def edge_cases():
    """(name, np, shift, touches): one ordinary signal against the tiles of 2 048 outputs (even tiles first, odd tiles fed
    from saved 180-sample halos, the k > 0 rule, the last tile of 512 outputs).  The first touched sample n (k == 1) and the
    last touched one (k == np - 1) are put at 2048 t + d; touches = whether any sample may change."""
    out = []
    for t in (1, 2):
        for d in (-181, -180, -1, 0, 1, 179, 180):
            n = TILE * t + d
            out.append(("first_t%d_d%d" % (t, d), NS, 1 - n, True))
            out.append(("last_t%d_d%d" % (t, d), 500 + n + 1, 500, True))      # k == np - 1 at sample n
    out += [("np2", 2, 0, True), ("last_sample", NS, NS - 1, True), ("one_in_last_tile", NS, -41470, True),
            ("k0_only", NS, -41471, False), ("np1", 1, 5, False)]
    return out


EDGE_SIGNAL = ("ord_2.2",)          # the signal of the edge cases


def reference(arith, I, Q, np_, f0, shift, drift, sym):
    """The residual of one row (copies): the oracle's subtract_signal2 (arith 0) or the CONTRACT=1 checker's (arith 1)."""
    if arith:
        import contract_lib
        fn = contract_lib.contract(1).ctr_subtract
    else:
        fn = ol.lib().orc_subtract
    Ic, Qc = np.array(I, np.float32, copy=True), np.array(Q, np.float32, copy=True)
    sym = np.ascontiguousarray(sym, np.uint8)
    with np.errstate(all="ignore"):
        fn(ol.ptr(Ic), ol.ptr(Qc), C.c_long(np_), C.c_float(f0), C.c_int(shift), C.c_float(drift), ol.ptr(sym))
    return Ic, Qc


# ---- tools/subtract_check.hip: case file in, dump out -------------------------------------------------------------------------------
def tool():
    exe = os.path.join(ROOT, "tools", "subtract_check.bin")
    src = os.path.join(ROOT, "tools", "subtract_check.hip")
    deps = [src] + [os.path.join(KERNELS, f) for f in ("k7_subtract.hip", "phase_runs.h", "wspr_device.h", "arith.h", "glibc_sincosf.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-value", "-I", KERNELS, src, "-o", exe],
                       check=True, capture_output=True)
    return exe


def run_tool(tmpdir, I, Q, runs, exe=None):
    """I, Q: [nseg][KIQ] float32.  runs: dicts with np, arith, jobs (SUBJOB array).  Returns one namespace per run: tables
    (TABLE per job), halo [njobs][21][360][2], I, Q after the launch."""
    I, Q = np.ascontiguousarray(I, np.float32), np.ascontiguousarray(Q, np.float32)
    nseg = I.shape[0]
    assert I.shape == Q.shape == (nseg, KIQ)
    case, out = os.path.join(str(tmpdir), "k7case.bin"), os.path.join(str(tmpdir), "k7out.bin")
    with open(case, "wb") as fh:
        fh.write(np.array([0x31374B53, nseg, len(runs)], "<i4").tobytes() + I.tobytes() + Q.tobytes())
        for r in runs:
            jobs = np.ascontiguousarray(r["jobs"], SUBJOB)
            fh.write(np.array([r["np"], r["arith"], jobs.size], "<i4").tobytes() + jobs.tobytes())
    p = subprocess.run([exe or tool(), case, out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-1000:], p.stderr[-2000:])
    with open(out, "rb") as fh:
        buf = fh.read()
    res, o = [], 0

    def take(dtype, count, shape=None):
        nonlocal o
        a = np.frombuffer(buf, dtype, count, o).copy()
        o += a.nbytes
        return a.reshape(shape) if shape else a
    for r in runs:
        nj, ns, sf, tf = (int(v) for v in take("<i4", 4))
        assert (nj, ns, tf * 4) == (len(r["jobs"]), nseg, TABLE.itemsize) and sf == nj * (tf + NTILES * 2 * HALO * 2)
        g = types.SimpleNamespace(np=r["np"], arith=r["arith"], jobs=r["jobs"])
        g.tables = take(TABLE, nj)
        g.halo = take("<f4", nj * NTILES * 2 * HALO * 2, (nj, NTILES, 2 * HALO, 2))
        g.I, g.Q = take("<f4", nseg * KIQ, (nseg, KIQ)), take("<f4", nseg * KIQ, (nseg, KIQ))
        res.append(g)
    assert o == len(buf)
    os.remove(case)
    os.remove(out)
    return res


def dumped_table(rec):
    """One record of a run's .tables as the namespace host_table() returns (no .nr)."""
    return types.SimpleNamespace(runs=rec["runs"].copy(), sym_phi=rec["sym_phi"].copy(), dphi=rec["dphi"].copy(),
                                 first_run=rec["first_run"].copy())
