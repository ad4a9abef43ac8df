"""Noncoherent block detection on the device (K10, wspr_block_demod_batch / wspr_set_block_detection; definition in
rtlsdr-wsprd_amd/csrc/kernels/blockdemod.h): the kernel against the serial CPU checker byte for byte in both arithmetic
modes, block size 1 against the product's own mode 2, the entry point's refusals, "off is off", and the stage inside the
decode loop against the checker's walk (tests/block_lib.py) on the loop's own trace."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import block_lib as bl
import oracle_lib as orc
import synth

pytestmark = pytest.mark.gpu
NS = 45000
# of tools/block_rescue_seeds.py -30 5000 5024: four seeds the walk rescues (block 2 at jitter 6 and 0, block 3 at
# jitter 0 and -3) and four that neither the plain ladder nor the walk decodes
RESCUED, LOST = (5003, 5007, 5008, 5010), (5002, 5011, 5012, 5013)


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    return mod


@pytest.fixture()
def stage_off(w):
    """Whatever a test sets, the next one starts with the stage off, exact arithmetic -- in both libraries."""
    yield
    for L in (w.lib(), w.lab()):
        w.set_block_detection(1, L)
        w.set_osd_depth(-1, L)
        w.wspr_set_arithmetic(0, L)
        L.wspr_set_fano_device_mode(-1)


def _record(seed, n):
    """One -10 dB signal in a record of n samples: rows (the record, zeros, noise nobody asks about), true f0, shift."""
    I, Q, truth = synth.make_segment(seed, bl.symbols_of, snr_db=-10.0)
    rng = np.random.default_rng(seed + 1)
    rows_i = np.stack([I[:n], np.zeros(n, np.float32), rng.normal(0, 0.1, n).astype(np.float32)])
    rows_q = np.stack([Q[:n], np.zeros(n, np.float32), rng.normal(0, 0.1, n).astype(np.float32)])
    return rows_i, rows_q, np.float32(truth[0][1]), int(round(truth[0][2] * 375))


def _items(w, f0, s0, n, count, seed):
    """`count` hypotheses on a record of n samples: the placements of the issue first, random ones after them.  Segment 1
    is the all-zero record, segment 2 gets none."""
    it = [(0, f0, s0, 0.0)]
    it += [(0, f0, s0 + d, 0.0) for d in range(-6, 7) if d]                    # every residue mod 4 and mod 3
    it += [(0, f0, 0, 0.0), (0, f0, -300, 0.0), (0, f0, -41500, 0.0)]          # k = 0 excluded; off the front
    it += [(0, f0, n - 41472 + 500, 0.0), (0, f0, n - 20000, 1.37), (0, f0, n - 100, 0.0), (0, f0, n + 5, 0.0)]   # off the end
    it += [(0, f0, s0, d) for d in (1.37, -1.37, 4.0, -4.0)]
    it += [(0, 150.0, s0, 0.0), (0, -150.0, s0, -4.0)]
    it += [(1, f0, s0, 0.0), (1, 0.0, 0, 2.0), (1, -150.0, -300, 0.0)]         # all-zero record: the NaN bytes
    rng = np.random.default_rng(seed)
    while len(it) < count:
        it.append((int(rng.random() < 0.1), rng.uniform(-110, 110), int(rng.integers(-600, 4600)),
                   float(rng.choice([0.0, 0.0, 1.37, -4.0, rng.uniform(-4, 4)]))))
    return np.array(it[:count], w.BLOCK_ITEM_DTYPE)


@functools.lru_cache(maxsize=None)
def _scene(n, count):
    import rtlsdr_wsprd_amd as mod
    I, Q, f0, s0 = _record(4242 + n, n)
    items = _items(mod, f0, s0, n, count, n)
    want = {flag: np.stack([bl.demod(flag, I[x["seg"]], Q[x["seg"]], n, x["freq"], x["shift"], x["drift"])[0] for x in items])
            for flag in (0, 1)}
    return I, Q, items, want


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("n,counts", [(45000, (1, 63, 64, 65, 200)), (44993, (40,)), (30000, (40,))])
def test_kernel_equals_the_checker(w, stage_off, arith, n, counts):
    """All three vectors of every hypothesis, byte for byte, through wspr_block_demod_batch()."""
    I, Q, items, want = _scene(n, max(counts))
    assert set(items["seg"]) == {0, 1} and (want[arith][items["seg"] == 0] != 0).any()
    assert not want[arith][items["seg"] == 1].any()                       # the all-zero record: NaN -> 0 everywhere
    assert w.wspr_set_arithmetic(arith) == 0
    for cnt in counts:
        got = w.block_demod(I, Q, items[:cnt])
        bad = np.argwhere((got != want[arith][:cnt]).any(axis=2))
        assert bad.size == 0, (arith, n, cnt, bad[:5].tolist(), items[bad[0][0]])
    # hypotheses elsewhere in the batch do not matter: the last ones alone
    assert np.array_equal(w.block_demod(I, Q, items[-7:]), want[arith][-7:])


@pytest.mark.parametrize("arith", [0, 1])
def test_block_size_1_is_the_products_mode_2(w, stage_off, arith):
    I, Q, items, _ = _scene(45000, 200)
    assert w.wspr_set_arithmetic(arith) == 0
    pick = [k for k in range(26) if items[k]["seg"] == 0] + [40, 41, 42]
    got = w.block_demod(I, Q, items[pick])
    for g, x in zip(got, items[pick]):
        Ic, Qc = I[x["seg"]].copy(), Q[x["seg"]].copy()
        f = C.c_float(x["freq"]); sh = C.c_int(int(x["shift"])); dr = C.c_float(x["drift"]); sy = C.c_float(0)
        sym = (C.c_ubyte * 162)()
        w.lib().sync_and_demodulate(orc.ptr(Ic), orc.ptr(Qc), C.c_long(NS), sym, C.addressof(f), 0, 0, C.c_float(0.0),
                                    C.addressof(sh), 0, 0, 8, C.addressof(dr), 50, C.addressof(sy), 2)
        assert bytes(g[0]) == bytes(sym), tuple(x)


def test_entry_point_arguments(w):
    L = w.lib()
    I, Q, items, want = _scene(45000, 200)
    sym = np.full((2, 3, 162), 0xA5, np.uint8)
    one = lambda **kw: np.array([tuple(kw.get(k, v) for k, v in (("seg", 0), ("freq", 1.0), ("shift", 5), ("drift", 0.0)))],
                                w.BLOCK_ITEM_DTYPE)
    call = lambda it, n=1, nseg=3, samples=NS: L.wspr_block_demod_batch(orc.ptr(I), orc.ptr(Q), nseg, samples, NS, orc.ptr(it),
                                                                        n, orc.ptr(sym))
    assert call(one(), n=0) == 0                                               # n == 0: nothing happens
    assert call(one(), n=-1) == -1
    assert call(one(seg=3)) == -1 and call(one(seg=-1)) == -1 and call(one(seg=1), nseg=1) == -1
    assert call(one(freq=np.nan)) == -1 and call(one(freq=np.inf)) == -1
    assert call(one(drift=np.nan)) == -1 and call(one(drift=-np.inf)) == -1
    assert call(one(), samples=45001) == -1
    two = np.concatenate([one(), one(seg=7)])                                  # one bad item refuses the whole call
    assert call(two, n=2) == -1
    assert (sym == 0xA5).all()                                                 # and nothing was written
    assert call(items[:1].copy()) == 0 and np.array_equal(sym[0], want[0][0]) and (sym[1] == 0xA5).all()


def _tup(x):
    return (x.message, x.call, x.loc, x.pwr, x.cycles, x.jitter, x.drift, x.sync, x.snr, x.dt, x.freq)


def _decode_writeback(w, I, Q, opt, K=16):
    """wspr_decode_batch with writeback: (spots per segment, residual I, residual Q)."""
    I, Q = I.copy(), Q.copy()
    nseg = I.shape[0]
    out = (w.decoder_results * (nseg * K))()
    nres = (C.c_int * nseg)()
    rc = w.lib().wspr_decode_batch(orc.ptr(I), orc.ptr(Q), nseg, NS, NS, opt, C.addressof(out), K, C.addressof(nres), 1)
    assert rc == 0, rc
    return [[_tup(out[s * K + i]) for i in range(nres[s])] for s in range(nseg)], I, Q


def _timings(w, L):
    ms = (C.c_double * len(w.TIMING_NAMES))()
    n = L.wspr_last_timings(C.addressof(ms), len(w.TIMING_NAMES))
    return {w.TIMING_NAMES[i]: ms[i] for i in range(n)}


def test_off_is_off_after_the_stage_was_switched_on_and_off(w, stage_off):
    """A crowded 64-segment scene at the default, then the same scene after wspr_set_block_detection(3) and (1): spots and
    written-back residual byte for byte, and the stage's timings zero."""
    segs = [synth.make_segment(7000 + s, bl.symbols_of, n_signals=3, snr_db=-12.0, snr_span=16.0, t_jitter=0.5) for s in range(64)]
    I, Q = np.stack([x[0] for x in segs]), np.stack([x[1] for x in segs])
    before = _decode_writeback(w, I, Q, w.default_options())
    assert sum(len(x) for x in before[0]) >= 64
    assert w.set_block_detection(1) == 1                                        # the default is off
    assert [w.set_block_detection(v) for v in (0, 4, -1)] == [-2, -2, -2]       # refused, nothing changed
    assert w.set_block_detection(3) == 1 and w.set_block_detection(2) == 3 and w.set_block_detection(1) == 2
    after = _decode_writeback(w, I, Q, w.default_options())
    assert after[0] == before[0]
    assert after[1].tobytes() == before[1].tobytes() and after[2].tobytes() == before[2].tobytes()
    t = w.last_timings()
    assert t["block_ms"] == 0 and t["block_vectors"] == 0 and t["block2_decodes"] == 0 and t["block3_decodes"] == 0


@functools.lru_cache(maxsize=None)
def _walk(seed, freq, shift, drift, quick):
    I, Q, _ = bl.weak_scene(seed)
    return bl.walk(0, I, Q, NS, freq, shift, drift, quickmode=quick, maxblock=3)


def _stage_against_walk(w, quick, fano_on_device):
    """The eight segments through the lab library's traced decode with the stage on; every visited candidate the plain
    ladder left undecoded must be what walk() says of the original record at the trace's (freq, shift, drift).  Returns the
    number of trace entries decoded by the stage."""
    seeds = RESCUED + LOST
    L = w.lab()
    L.wspr_set_fano_device_mode(fano_on_device)
    assert w.set_block_detection(3, L) == 1
    I = np.stack([bl.weak_scene(s)[0] for s in seeds])
    Q = np.stack([bl.weak_scene(s)[1] for s in seeds])
    opt = w.default_options(npasses=1, subtraction=0, quickmode=quick)
    spots, tr = w.wspr_decode_batch_trace(I, Q, opt, max_results=16)
    t = _timings(w, L)
    nblock = 0
    for s, seed in enumerate(seeds):
        sent = bl.weak_scene(seed)[2]
        assert all(x.message.decode() == sent for x in spots[s]), (seed, [x.message for x in spots[s]])
        assert tr[s].passes_run == 1
        for j in range(tr[s].n_visited[0]):
            c = tr[s].cand[0][j]
            assert c.block in (0, 1, 2, 3) and (c.block != 0) == bool(c.decoded)
            if c.block == 1:
                continue                                                   # the plain ladder's: test_gpu_parity.py's ground
            want = _walk(seed, c.freq, c.shift, c.drift, quick) if np.float32(c.sync) > bl.MINSYNC1 else None
            got = (c.block, c.jitter, tuple(c.decdata), c.cycles) if c.decoded else None
            assert got == want, (seed, j, got, want)
            nblock += c.block >= 2
    assert t["block2_decodes"] + t["block3_decodes"] == nblock
    assert t["block_vectors"] >= nblock and t["block_ms"] > 0
    print("stage (quick %d, device Fano %d): %d block decodes (%d at 2, %d at 3), %d vectors to Fano, %.1f ms"
          % (quick, fano_on_device, nblock, t["block2_decodes"], t["block3_decodes"], t["block_vectors"], t["block_ms"]))
    return nblock


@pytest.mark.parametrize("fano_on_device", [0, 1])
def test_stage_against_the_walk(w, stage_off, fano_on_device):
    assert _stage_against_walk(w, 0, fano_on_device) >= 1


@pytest.mark.parametrize("fano_on_device", [0, 1])
def test_stage_in_quick_mode_walks_rung_0_only(w, stage_off, fano_on_device):
    _stage_against_walk(w, 1, fano_on_device)


def test_default_options_on_the_weak_scenes(w, stage_off):
    """Two passes with subtraction on seeds 5000..5023, maxblock 3: every spot's message was sent, every segment the
    default decoder decodes is still decoded, and a segment only the stage decodes had its signal subtracted."""
    scenes = [bl.weak_scene(s) for s in range(5000, 5024)]
    I, Q = np.stack([x[0] for x in scenes]), np.stack([x[1] for x in scenes])
    off, _, _ = _decode_writeback(w, I, Q, w.default_options())
    assert w.set_block_detection(3) == 1
    on, ri, rq = _decode_writeback(w, I, Q, w.default_options())
    t = w.last_timings()
    for s in range(24):
        assert all(x[0].decode() == scenes[s][2] for x in on[s] + off[s]), (s, on[s], off[s])
        assert on[s] or not off[s], s
    dec_off, dec_on = [s for s in range(24) if off[s]], [s for s in range(24) if on[s]]
    print("default options, 24 segments at -30 dB: %d decoded with the stage off, %d with maxblock 3 (%d at 2, %d at 3); "
          "%d vectors to Fano, %.1f ms" % (len(dec_off), len(dec_on), t["block2_decodes"], t["block3_decodes"],
                                           t["block_vectors"], t["block_ms"]))
    gained = sorted(set(dec_on) - set(dec_off))
    assert gained and t["block2_decodes"] + t["block3_decodes"] >= len(gained)
    for s in gained:
        assert ri[s].tobytes() != I[s].tobytes() and rq[s].tobytes() != Q[s].tobytes(), s


def _prime(w, path, calls):
    """hashtable.txt as the decoder writes it (wsprd.c:842-852): the calls a receiver has heard before."""
    with open(path, "w") as f:
        for slot, call in sorted((w.lib().nhash(c.encode(), len(c), 146), c) for c in calls):
            f.write("%5d %s %s\n" % (slot, call, "AA00"))


def _in_dir(path, fn):
    cwd = os.getcwd()
    os.makedirs(path, exist_ok=True)
    os.chdir(path)
    try:
        return fn()
    finally:
        os.chdir(cwd)


def test_with_the_ordered_statistics_stage_on_as_well(w, tmp_path, stage_off):
    """Depth 3, primed hashtable.txt, usehashtable = 1: the block stage runs first, so every message it decodes with OSD
    off is still reported with OSD on, and as a Fano decode (cycles != 0)."""
    seeds = RESCUED + LOST
    I = np.stack([bl.weak_scene(s)[0] for s in seeds])
    Q = np.stack([bl.weak_scene(s)[1] for s in seeds])
    opt = w.default_options()
    opt.usehashtable = 1
    assert w.set_block_detection(3) == 1

    def run():
        _prime(w, "hashtable.txt", synth.CALLS)
        return [[(x.message, x.cycles) for x in g] for g in w.wspr_decode_batch(I, Q, opt)]
    block_only = _in_dir(tmp_path / "a", run)
    assert w.set_osd_depth(3) == -1
    both = _in_dir(tmp_path / "b", run)
    assert sum(len(g) for g in block_only) >= 1
    for s in range(len(seeds)):
        assert all(c != 0 for _, c in block_only[s])
        for m, _ in block_only[s]:
            assert [c for mm, c in both[s] if mm == m and c != 0], (seeds[s], m, both[s])


def test_hash_memory_on_a_batch_equals_single_calls_in_order(w, tmp_path, stage_off):
    """usehashtable = 1 on four segments with the stage on: spots and hashtable.txt are those of four single calls."""
    seeds = (5000, 5007, 5002, 5008)
    I = np.stack([bl.weak_scene(s)[0] for s in seeds])
    Q = np.stack([bl.weak_scene(s)[1] for s in seeds])
    opt = w.default_options()
    opt.usehashtable = 1
    assert w.set_block_detection(3) == 1

    def batch():
        spots = [[_tup(x) for x in g] for g in w.wspr_decode_batch(I, Q, opt)]
        return spots, open("hashtable.txt").read()

    def singles():
        spots = [[_tup(x) for x in w.wspr_decode_batch(I[s:s + 1], Q[s:s + 1], opt)[0]] for s in range(len(seeds))]
        return spots, open("hashtable.txt").read()
    got, want = _in_dir(tmp_path / "batch", batch), _in_dir(tmp_path / "single", singles)
    assert got[0] == want[0] and got[1] == want[1]
    assert sum(len(g) for g in got[0]) >= 3 and len(got[1].splitlines()) >= 3
