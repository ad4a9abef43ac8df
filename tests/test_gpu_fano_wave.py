"""K6w (k6_fano_wave.hip), the device Fano search, against the host emulation of its step structure
(tests/helpers/fano_wave_check.cpp through tests/fano_lib.py) and the serial reference: steps, return code, cycle count,
metric, maxnp and decoded bytes of EVERY vector, ==.  tests/test_fano_cases_cpu.py says what the vector sets reach (the
budget's edge, the 8-wide and 1-wide steps, the window's moves, the overflow exit).

The device hides its own failures: a vector for which the kernel returns -2 is decoded again by the host, so a kernel that
corrupts its store is slower, not wrong.  Here the step count (which the host never touches) and the lab library's counter
of such hand-overs make that visible: with the production store of 4 096 visits and with 1 024 the counter must not move;
with 96 it must move by exactly the number of overflows the emulation predicts, on both of its branches.

The stores of 1 024 and 96 visits are lab switches read once per process (WSPR_FANO_WAVE_CAP): this file, run as a
script with the capacity as its argument, is their child process."""
import ctypes as C
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":                               # the child process: what tests/conftest.py does for a test run
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        import torch  # noqa: F401
    except ImportError:
        pass

import fano_lib as fl
import oracle_lib as ol

# One wave per workgroup, a persistent grid of kWaveGrid = 256 CUs x WSPR_K6W_PER_CU (13, by LDS) = 3 328 workgroups
# (k6_fano_wave.hip): up to 3 328 vectors every wave has one vector of its own, from 3 329 on a wave that has finished
# takes another from the work counter and meets its own stale tables, window and stack slice.
WAVE_GRID = 256 * 13
RET, METRIC, CYCLES, MAXNP, STEPS = 0, 1, 2, 3, 14


def _bind(L):
    L.wspr_fano_batch_device_wave.argtypes = [C.c_void_p, C.c_int, C.c_uint] + [C.c_void_p] * 6
    L.wspr_fano_batch_device_wave.restype = C.c_int
    return L


def _handovers(L):
    """(on the pool, one by one) of the lab library; None for the product, which must not export the counter."""
    if not hasattr(L, "wspr_fano_host_handovers"):
        return None
    a, b = C.c_ulonglong(), C.c_ulonglong()
    L.wspr_fano_host_handovers(C.byref(a), C.byref(b))
    return a.value, b.value


def _run(L, sym, maxcycles, with_steps=True, fill=0):
    """The device search on a stack of vectors: int64 [n, 15] = ret, metric, cycles, maxnp, data[10], steps."""
    sym = np.ascontiguousarray(sym, np.uint8)
    n = len(sym)
    ret = np.full(n, fill, np.int32); cyc = np.full(n, fill, np.uint32); met = np.full(n, fill, np.uint32)
    mnp = np.full(n, fill, np.uint32); dat = np.full((n, 10), fill, np.uint8); steps = np.full(n, fill, np.uint32)
    assert L.wspr_fano_batch_device_wave(ol.ptr(sym), n, maxcycles, ol.ptr(ret), ol.ptr(cyc), ol.ptr(met), ol.ptr(mnp),
                                         ol.ptr(dat), ol.ptr(steps) if with_steps else None) == 0
    return np.column_stack([ret, met, cyc, mnp, dat, steps]).astype(np.int64)


def _compare(L, cap, sym, maxcycles, emu, ser, tag):
    """One call against the emulation at this capacity (rows of fl.wave) and the serial reference (rows of fl.serial).
    Where the emulation predicts -2 the host has answered: everything equals the reference and `steps` is still the
    kernel's count at the -2 exit.  Returns the number of such vectors; the counter's pool branch moves by it."""
    before = _handovers(L)
    got = _run(L, sym, maxcycles)
    after = _handovers(L)
    over = emu[:, RET] == -2
    bad = np.flatnonzero((got[:, STEPS] != emu[:, STEPS]) | (~over & (got[:, :14] != emu[:, :14]).any(axis=1))
                         | (fl.defined(got) != ser).any(axis=1))
    assert bad.size == 0, (tag, maxcycles, bad[:8].tolist(), got[bad[:3]].tolist(), emu[bad[:3]].tolist(), ser[bad[:3]].tolist())
    if cap != 96:
        assert not over.any()
    if before is not None:
        assert (after[0] - before[0], after[1] - before[1]) == (int(over.sum()), 0), (tag, maxcycles, before, after)
    return int(over.sum())


def step_for_step(L, cap):
    """The 364 ladder vectors and the first 16 alternating ones at every budget (up to 1 500 for the store of 96, where
    most of them overflow), and the budget-edge triples at their own budgets."""
    n_over = n_vec = 0
    for budget in (b for b in fl.BUDGETS if cap != 96 or b <= 1500):
        n_over += _compare(L, cap, fl.main_set(), budget, fl.wave_of("main", budget, 64, cap), fl.serial_of("main", budget), "main")
        n_vec += len(fl.main_set())
    regimes = set()
    for k, (sym, cases) in enumerate(fl.budget_edges()):
        for maxcycles, ret, cycles, metric, decdata in cases:
            ser = fl.serial(sym, maxcycles)
            assert ser[0].tolist() == [ret, metric, cycles, 80 if ret == 0 else 0] + list(decdata)       # the golden file
            n_over += _compare(L, cap, sym[None], maxcycles, fl.wave(sym, maxcycles, 64, cap), ser, "edge %d" % k)
            n_vec += 1
            regimes.add((ret, cycles - 81 * maxcycles if ret else 0))
    assert regimes == {(-1, 2), (-1, 1), (0, 0)}
    return n_vec, n_over


def queue(L, cap, sizes):
    """Calls of more vectors than the grid has waves, the ladder vectors in a seeded shuffle (deep stacks and instant
    decodes alternate on a wave), each call made twice: every vector against the emulation and the reference."""
    emu, ser = fl.wave_of("ladder", 200, 64, cap), fl.serial_of("ladder", 200)
    n_over = 0
    for n in sizes:
        idx = fl.queue_order(n)
        sym = fl.ladder_vectors()[idx]
        for again in range(2):
            n_over += _compare(L, cap, sym, 200, emu[idx], ser[idx], "queue %d call %d" % (n, again))
    return n_over


def decode_loop_fallback(w, L):
    """The other branch of the fallback (no host copy of the vectors: each is fetched from the device), which only the
    decode loop takes: a few crowded scenes with every Fano attempt on the device and a store of 96 visits.  Spots and
    residuals are the oracle's, and the one-by-one counter has moved.  (-2 is a designed return code of the kernel.)"""
    import scenes
    seeds = [s for s in scenes.GOLDEN_SEEDS if s % 6][:4]
    segs = [scenes.make_scene(s) for s in seeds]
    I, Q = np.stack([x[0] for x in segs]), np.stack([x[1] for x in segs])
    refs = [ol.decode(I[k], Q[k], scenes.NS) for k in range(len(seeds))]
    gi, gq = I.copy(), Q.copy()
    nseg, samples = gi.shape
    out = (w.decoder_results * (nseg * 16))()
    nres = (C.c_int * nseg)()
    before = _handovers(L)
    old = L.wspr_set_fano_device_mode(1)
    try:
        assert L.wspr_decode_batch(ol.ptr(gi), ol.ptr(gq), nseg, samples, samples, w.default_options(), C.addressof(out), 16,
                                   C.addressof(nres), 1) == 0
    finally:
        L.wspr_set_fano_device_mode(old)
    after = _handovers(L)

    def fields(s):
        return (s.message, s.call, s.loc, s.pwr, s.cycles, s.jitter, s.drift, s.sync, s.snr, s.dt, s.freq)
    nspots = 0
    for k, (ref, oi, oq) in enumerate(refs):
        got = [fields(out[k * 16 + i]) for i in range(nres[k])]
        want = [fields(s) for s in ref]
        print("scene %d: %d spots (oracle %d)" % (seeds[k], len(got), len(want)))
        assert got == want, (seeds[k], got, want)
        assert np.array_equal(gi[k].view(np.uint32), oi.view(np.uint32)) and np.array_equal(gq[k].view(np.uint32), oq.view(np.uint32)), seeds[k]
        nspots += len(got)
    assert nspots >= 4
    assert after[0] == before[0] and after[1] > before[1], (before, after)
    return after[1] - before[1]


# ------------------------------------------------------------------------------------------------ the child process
def main(cap):
    """Run by test_small_stores with WSPR_USE_LAB=1 and WSPR_FANO_WAVE_CAP=<cap>: the lab library with that store."""
    faulthandler.dump_traceback_later(420, exit=True)
    assert os.environ.get("WSPR_USE_LAB") == "1" and os.environ.get("WSPR_FANO_WAVE_CAP") == str(cap)
    import rtlsdr_wsprd_amd as w
    L = _bind(w.lib())
    assert L.wspr_device_ready() == 1 and _handovers(L) == (0, 0)
    n_vec, n_over = step_for_step(L, cap)
    n_over += queue(L, cap, (WAVE_GRID + 1,))
    assert _handovers(L) == (n_over, 0)
    summary = {"cap": cap, "vectors": n_vec, "overflows": n_over, "pool": _handovers(L)[0], "one_by_one": 0}
    if cap == 96:
        summary["one_by_one"] = decode_loop_fallback(w, L)
    print("K6W_CHILD " + json.dumps(summary))


if __name__ == "__main__":
    main(int(sys.argv[1]))


# ------------------------------------------------------------------------------------------------ the tests
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    return mod


@pytest.fixture()
def limit():
    """A time limit of the test's own: a search that never ends takes the process down instead of the machine's time."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _library(w, which):
    return _bind(w.lib() if which == "product" else w.lab())


@pytest.mark.parametrize("which", ["product", "lab"])
def test_step_for_step(w, limit, which):
    L = _library(w, which)
    assert (_handovers(L) is None) == (which == "product" and os.environ.get("WSPR_USE_LAB") != "1")
    n_vec, n_over = step_for_step(L, 4096)
    assert n_over == 0 and n_vec == 4 * 380 + 3 * len(fl.budget_edges())
    assert _handovers(L) in (None, (0, 0))


@pytest.mark.parametrize("which", ["product", "lab"])
def test_queue(w, limit, which):
    queue(_library(w, which), 4096, (WAVE_GRID - 1, WAVE_GRID, WAVE_GRID + 1, 4000))


@pytest.mark.parametrize("which", ["product", "lab"])
def test_arguments(w, limit, which):
    L = _library(w, which)
    sym = fl.main_set()
    full = _run(L, sym, 200)
    assert (_run(L, sym, 200, with_steps=False, fill=0xA5)[:, :14] == full[:, :14]).all()          # steps == NULL
    # n == 0: returns 0 and writes nothing
    outs = [np.full(64, 0xA5, np.uint8) for _ in range(6)]
    assert L.wspr_fano_batch_device_wave(ol.ptr(np.ascontiguousarray(sym[:1])), 0, 200, *[ol.ptr(o) for o in outs]) == 0
    assert all((o == 0xA5).all() for o in outs)
    # maxcycles == 0: the budget is spent before the first look (fano.c:149-153, 231-237)
    zero = _run(L, sym, 0)
    assert (zero[:, [RET, CYCLES]] == [-1, 2]).all() and (fl.defined(zero) == fl.serial_of("main", 0)).all()
    assert (zero == fl.wave_of("main", 0, 64, 4096)[:, :15]).all()


@pytest.mark.parametrize("cap", [1024, 96])
def test_small_stores(cap):
    """The step-for-step body and a call of 3 329 vectors with a store of 1 024 visits (narrow steps, window moves at those
    widths; the counter stays 0) and of 96 (overflows, as many as the emulation predicts, each finished by the host on the
    pool; then the decode loop with every attempt on the device, whose overflows the host fetches one by one)."""
    env = dict(os.environ, WSPR_FANO_WAVE_CAP=str(cap), WSPR_USE_LAB="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(cap)], env=env, capture_output=True, text=True, timeout=480)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("K6W_CHILD ")]
    assert len(line) == 1, r.stdout[-2000:]
    s = json.loads(line[0][len("K6W_CHILD "):])
    print(s)
    assert s["cap"] == cap and s["vectors"] > 1000
    if cap == 1024:
        assert (s["overflows"], s["pool"], s["one_by_one"]) == (0, 0, 0)
    else:
        assert s["overflows"] > 100 and s["pool"] == s["overflows"] and s["one_by_one"] > 0
