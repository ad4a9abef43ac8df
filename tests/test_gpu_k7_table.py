"""K7 on the device, table by table: tools/subtract_check.hip runs the production launch_subtract() and dumps every job's
PhaseTable as sub_runs_wave_kernel left it, the halos and the rows.  The table is held against the host's serial builder
(byte for byte) and against the reference's serial float walk (every sample's phase, as bits), the residual against the
oracle (exact mode) and the CONTRACT=1 checker (contracted mode), bit for bit, and the same jobs go through the C ABI's
subtract_signal2().  The cases (tests/subtract_lib.py; tests/test_phase_table_cpu.py proves them on the CPU first) reach what
real code words never do: the dense fallback of sub_fir_fused_kernel, an overflow in the middle of a chain and during a
walk, a table of exactly 512 runs, walks through zero, subnormal and infinite phases, symbols above 3; one launch mixes
dense and run-table jobs; and a frame edge is put on either side of every tile and halo boundary."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as ol
import subtract_lib as sl

pytestmark = pytest.mark.gpu

CASES = sl.phase_cases()
NAMES = [c[0] for c in CASES]
EDGES = sl.edge_cases()
SENT32 = np.uint32(0xA5A5A5A5)


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    yield mod
    mod.wspr_set_arithmetic(mod.WSPR_ARITH_EXACT)


@pytest.fixture(scope="module")
def rows8():
    return sl.rows(8)


def _shift(i):
    return 900 + 37 * i


@functools.lru_cache(maxsize=None)
def _ref(arith, seg, np_, name, shift):
    """The reference's residual of rows(8)[seg] for the named phase case; computed once and not modified."""
    I, Q = sl.rows(8)
    _, f0, drift, sym, _ = sl.case_named(name)
    return sl.reference(arith, I[seg], Q[seg], np_, f0, shift, drift, sym)


def _phase_runs(arith):
    """The phase cases eight to a launch (case i on row i % 8), then the mixed launch."""
    runs, where = [], {}
    for r0 in range(0, len(CASES), 8):
        jobs = []
        for i in range(r0, min(r0 + 8, len(CASES))):
            name, f0, drift, sym, _ = CASES[i]
            jobs.append(sl.job(i % 8, f0, _shift(i), drift, sym))
            where[name] = (len(runs), i - r0, i % 8, _shift(i))
        runs.append(dict(np=sl.NS, arith=arith, jobs=np.concatenate(jobs)))
    mixed = []
    for j, name in enumerate(sl.MIXED):
        _, f0, drift, sym, _ = sl.case_named(name)
        mixed.append(sl.job(7 - j, f0, -2000 + 1111 * j, drift, sym))       # rows and shifts of their own
    runs.append(dict(np=sl.NS, arith=arith, jobs=np.concatenate(mixed)))
    return runs, where


@pytest.fixture(scope="module", params=[0, 1], ids=["exact", "contracted"])
def phase_dump(request, rows8, tmp_path_factory):
    runs, where = _phase_runs(request.param)
    res = sl.run_tool(tmp_path_factory.mktemp("k7"), rows8[0], rows8[1], runs)
    return request.param, res, where


@pytest.fixture(scope="module", params=[0, 1], ids=["exact", "contracted"])
def edge_dump(request, rows8, tmp_path_factory):
    """Two tool runs: the cases with np = 45 000 eight to a launch, the others (an np of their own) one launch each on row 0."""
    _, f0, drift, sym, _ = sl.case_named(sl.EDGE_SIGNAL[0])
    full = [e for e in EDGES if e[1] == sl.NS]
    short = [e for e in EDGES if e[1] != sl.NS]
    runs_a, where = [], {}
    for r0 in range(0, len(full), 8):
        chunk = full[r0:r0 + 8]
        for j, e in enumerate(chunk):
            where[e[0]] = ("a", len(runs_a), j)
        runs_a.append(dict(np=sl.NS, arith=request.param, jobs=np.concatenate([sl.job(j, f0, e[2], drift, sym) for j, e in enumerate(chunk)])))
    runs_b = []
    for e in short:
        where[e[0]] = ("b", len(runs_b), 0)
        runs_b.append(dict(np=e[1], arith=request.param, jobs=sl.job(0, f0, e[2], drift, sym)))
    tmp = tmp_path_factory.mktemp("k7e")
    res = {"a": sl.run_tool(tmp, rows8[0], rows8[1], runs_a), "b": sl.run_tool(tmp, rows8[0][:1], rows8[1][:1], runs_b)}
    return request.param, res, where


# ---- the assertions ------------------------------------------------------------------------------------------------------------------
def _check_table(rec, case):
    """One dumped PhaseTable against the numpy increments, the host's serial builder and the serial walk."""
    name, f0, drift, sym, nr = case
    d = sl.dphi(f0, drift, sym)
    host = sl.host_table(d)
    assert host.nr == nr
    assert np.array_equal(sl.bits(rec["dphi"]), sl.bits(d)), name
    assert sl.same_floats(rec["sym_phi"], host.sym_phi), name
    first = rec["first_run"]
    assert first[sl.NSYM + 1] == 0xA5A5                                     # the padding entry is nobody's
    if nr >= 0:
        assert np.array_equal(first[:sl.NSYM + 1], host.first_run[:sl.NSYM + 1]), name
        assert rec["runs"][:nr].tobytes() == host.runs[:nr].tobytes(), name
        assert np.all(rec["runs"][nr:].view(np.uint8) == sl.SENTINEL), name
    else:
        assert first[0] == 0xFFFF, name
    phi, skipped = sl.table_eval(sl.dumped_table(rec))
    assert skipped == 0, name
    assert sl.same_floats(phi, sl.serial_walk(d)[0]), name


def _check_halo(halo, shift, np_):
    """What the even tiles saved for the odd ones: their first and last 180 products, zero outside 0 < k < np; nothing else."""
    h = halo.view(np.uint32)
    for t in range(sl.NTILES):
        if t % 2:
            assert np.all(h[t] == SENT32), t
            continue
        for half, base in ((0, sl.TILE * t), (1, sl.TILE * t + sl.TILE - sl.HALO)):
            n = base + np.arange(sl.HALO)
            part = h[t, half * sl.HALO:(half + 1) * sl.HALO]
            k = shift + n
            inside = n < sl.NSIG
            assert np.all(part[~inside] == SENT32), (t, half)
            assert not np.any(part[inside] == SENT32), (t, half)
            assert np.all(part[inside & ~((k > 0) & (k < np_))] == 0), (t, half)


def _check_rows(g, rows, used):
    """Rows no job of the launch names, and every row's stride tail, are as they went in."""
    for s in range(g.I.shape[0]):
        assert np.all(g.I[s, sl.NS:] == sl.TAIL) and np.all(g.Q[s, sl.NS:] == sl.TAIL), s
        if s not in used:
            assert np.array_equal(sl.bits(g.I[s]), sl.bits(rows[0][s])) and np.array_equal(sl.bits(g.Q[s]), sl.bits(rows[1][s])), s


@pytest.mark.parametrize("name", NAMES)
def test_table_equals_host_builder_and_serial_walk(phase_dump, name):
    arith, res, where = phase_dump
    run, j, seg, shift = where[name]
    _check_table(res[run].tables[j], sl.case_named(name))
    _check_halo(res[run].halo[j], shift, sl.NS)


@pytest.mark.parametrize("name", NAMES)
def test_residual_equals_reference(phase_dump, rows8, name):
    arith, res, where = phase_dump
    run, j, seg, shift = where[name]
    g = res[run]
    ri, rq = _ref(arith, seg, sl.NS, name, shift)
    assert sl.same_floats(g.I[seg, :sl.NS], ri[:sl.NS]) and sl.same_floats(g.Q[seg, :sl.NS], rq[:sl.NS])
    assert not np.array_equal(sl.bits(g.I[seg]), sl.bits(rows8[0][seg])) and not np.array_equal(sl.bits(g.Q[seg]), sl.bits(rows8[1][seg]))
    if name != "f1e38":
        assert np.isfinite(g.I[seg]).all() and np.isfinite(g.Q[seg]).all()
    else:
        assert np.isnan(g.I[seg]).any()                                     # sincos of an infinite phase
    _check_rows(g, rows8, set(int(s) for s in g.jobs["seg"]))


def test_mixed_launch_dense_and_run_table_jobs_side_by_side(phase_dump, rows8):
    arith, res, _ = phase_dump
    g = res[-1]
    assert [int(t["first_run"][0] == 0xFFFF) for t in g.tables] == [0, 1, 0, 1, 0]
    for j, name in enumerate(sl.MIXED):
        jb = g.jobs[j]
        seg, shift = int(jb["seg"]), int(jb["shift"])
        _check_table(g.tables[j], sl.case_named(name))
        _check_halo(g.halo[j], shift, sl.NS)
        ri, rq = _ref(arith, seg, sl.NS, name, shift)
        assert np.array_equal(sl.bits(g.I[seg, :sl.NS]), sl.bits(ri[:sl.NS])), name
        assert np.array_equal(sl.bits(g.Q[seg, :sl.NS]), sl.bits(rq[:sl.NS])), name
        assert not np.array_equal(sl.bits(g.I[seg]), sl.bits(rows8[0][seg]))
    _check_rows(g, rows8, set(int(s) for s in g.jobs["seg"]))


@pytest.mark.parametrize("edge", EDGES, ids=[e[0] for e in EDGES])
def test_frame_edges_against_the_tiles(edge_dump, rows8, edge):
    arith, res, where = edge_dump
    name, np_, shift, touches = edge
    which, run, j = where[name]
    g = res[which][run]
    seg = int(g.jobs[j]["seg"])
    assert (g.np, int(g.jobs[j]["shift"])) == (np_, shift)
    ri, rq = _ref(arith, seg, np_, sl.EDGE_SIGNAL[0], shift)
    assert np.array_equal(sl.bits(g.I[seg, :sl.NS]), sl.bits(ri[:sl.NS])) and np.array_equal(sl.bits(g.Q[seg, :sl.NS]), sl.bits(rq[:sl.NS]))
    changed = not (np.array_equal(sl.bits(g.I[seg]), sl.bits(rows8[0][seg])) and np.array_equal(sl.bits(g.Q[seg]), sl.bits(rows8[1][seg])))
    assert changed == touches
    if touches:                                                   # and only inside 0 < k < np of the frame
        k = np.arange(sl.NS)
        may = (k > 0) & (k < np_) & (k >= shift) & (k < shift + sl.NSIG)
        assert np.array_equal(sl.bits(g.I[seg, :sl.NS])[~may], sl.bits(rows8[0][seg, :sl.NS])[~may])
        assert np.any(g.I[seg, :sl.NS][may] != rows8[0][seg, :sl.NS][may])
    _check_halo(g.halo[j], shift, np_)
    _check_table(g.tables[j], sl.case_named(sl.EDGE_SIGNAL[0]))
    _check_rows(g, rows8, set(int(s) for s in g.jobs["seg"]))


# ---- the same jobs through the C ABI ----------------------------------------------------------------------------------------------------
def _abi_subtract(w, I, Q, np_, f0, shift, drift, sym):
    Ic, Qc = np.array(I, np.float32, copy=True), np.array(Q, np.float32, copy=True)
    sym = np.ascontiguousarray(sym, np.uint8)
    w.lib().subtract_signal2(ol.ptr(Ic), ol.ptr(Qc), C.c_long(np_), C.c_float(f0), C.c_int(shift), C.c_float(drift), ol.ptr(sym))
    return Ic, Qc


@pytest.fixture(params=[0, 1], ids=["exact", "contracted"])
def abi_arith(request, w):
    modes = (w.WSPR_ARITH_EXACT, w.WSPR_ARITH_CONTRACTED)
    w.wspr_set_arithmetic(modes[request.param])
    yield request.param
    assert w.wspr_set_arithmetic(w.WSPR_ARITH_EXACT) == modes[request.param]


def test_subtract_signal2_abi_phase_cases(w, abi_arith, rows8):
    for i, (name, f0, drift, sym, _) in enumerate(CASES):
        seg, shift = i % 8, _shift(i)
        gi, gq = _abi_subtract(w, rows8[0][seg, :sl.NS], rows8[1][seg, :sl.NS], sl.NS, f0, shift, drift, sym)
        ri, rq = _ref(abi_arith, seg, sl.NS, name, shift)
        assert sl.same_floats(gi, ri[:sl.NS]) and sl.same_floats(gq, rq[:sl.NS]), name
        assert not np.array_equal(sl.bits(gi), sl.bits(rows8[0][seg, :sl.NS])), name


def test_subtract_signal2_abi_frame_edges(w, abi_arith, rows8):
    _, f0, drift, sym, _ = sl.case_named(sl.EDGE_SIGNAL[0])
    for name, np_, shift, touches in EDGES:
        seg = 0 if np_ != sl.NS else [e[0] for e in EDGES if e[1] == sl.NS].index(name) % 8
        gi, gq = _abi_subtract(w, rows8[0][seg, :sl.NS], rows8[1][seg, :sl.NS], np_, f0, shift, drift, sym)
        ri, rq = _ref(abi_arith, seg, np_, sl.EDGE_SIGNAL[0], shift)
        assert np.array_equal(sl.bits(gi), sl.bits(ri[:sl.NS])) and np.array_equal(sl.bits(gq), sl.bits(rq[:sl.NS])), name
        assert (not np.array_equal(sl.bits(gi), sl.bits(rows8[0][seg, :sl.NS]))) == touches, name


def test_np_above_the_record_is_45000(w, abi_arith, rows8):
    """np = 50 000 with caller buffers of 50 000 floats and a frame that hangs over sample 45 000 (shift 3 900: k reaches
    45 371): the first 45 000 samples are the reference's with np = 45 000, the caller's samples behind them are untouched,
    and sync_and_demodulate() reads none of them either."""
    _, f0, drift, sym, _ = sl.case_named(sl.EDGE_SIGNAL[0])
    big = 50000
    I, Q = np.full(big, 5.0, np.float32), np.full(big, -5.0, np.float32)
    I[:sl.NS], Q[:sl.NS] = rows8[0][3, :sl.NS], rows8[1][3, :sl.NS]
    gi, gq = _abi_subtract(w, I, Q, big, f0, 3900, drift, sym)
    ri, rq = _ref(abi_arith, 3, sl.NS, sl.EDGE_SIGNAL[0], 3900)
    assert np.array_equal(sl.bits(gi[:sl.NS]), sl.bits(ri[:sl.NS])) and np.array_equal(sl.bits(gq[:sl.NS]), sl.bits(rq[:sl.NS]))
    assert not np.array_equal(sl.bits(gi[:sl.NS]), sl.bits(I[:sl.NS]))
    assert np.all(gi[sl.NS:] == 5.0) and np.all(gq[sl.NS:] == -5.0)
    # mode 2 of sync_and_demodulate at the same shift
    demod = ol.lib().orc_sync_demod
    if abi_arith:
        import contract_lib
        demod = contract_lib.contract(1).ctr_sync_demod
    out = []
    for fn, np_ in ((w.lib().sync_and_demodulate, big), (demod, sl.NS)):
        Ic, Qc = I.copy(), Q.copy()
        f, sh, dr, sy = C.c_float(2.25), C.c_int(3900), C.c_float(0.0), C.c_float(0)
        symbols = (C.c_ubyte * 162)()
        fn(ol.ptr(Ic), ol.ptr(Qc), C.c_long(np_), symbols, C.addressof(f), 0, 0, C.c_float(0.0), C.addressof(sh), 0, 0, 8,
           C.addressof(dr), 50, C.addressof(sy), 2)
        out.append((sy.value, bytes(symbols)))
        assert np.array_equal(Ic, I) and np.array_equal(Qc, Q)
    assert out[0] == out[1] and out[0][0] == out[0][0]
