"""The decode loop's one Fano walk (csrc/host/wspr_fano_walk.h) where its callers meet: the two placements of the Fano
attempts (host pool, device search) with every opt-in stage on at once, and the block stage's chunk edge -- more than 256
candidates of one wave left to it, against the same segments in two halves that stay below the edge."""
import ctypes as C
import os

import numpy as np
import pytest

import block_lib as bl
import synth

pytestmark = pytest.mark.gpu
RESCUED, LOST = (5003, 5007, 5008, 5010), (5002, 5011, 5012, 5013)      # tests/test_gpu_block.py
COUNTERS = ("fano_calls", "fano_timeouts", "fano_cycles", "block_vectors", "osd_vectors", "list_vectors")


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    return mod


@pytest.fixture()
def stages_off(w):
    yield
    for L in (w.lib(), w.lab()):
        w.set_block_detection(1, L)
        w.set_message_list(None, library=L)
        w.set_osd_depth(-1, L)
        L.wspr_set_fano_device_mode(-1)


def _spot(x):
    return (x.message, x.call, x.loc, x.pwr, x.cycles, x.jitter, x.drift, x.sync, x.snr, x.dt, x.freq)


def _records(tr, nseg):
    """Per segment: passes run, peaks and visits per pass, and the whole record of every visited candidate, as bytes."""
    return [(tr[s].passes_run, list(tr[s].npk), list(tr[s].n_visited),
             [[bytes(tr[s].cand[p][j]) for j in range(tr[s].n_visited[p])] for p in range(tr[s].passes_run)])
            for s in range(nseg)]


def _first_difference(a, b):
    for s, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return s, x[:3], y[:3]
    return None


def _timings(w, L):
    ms = (C.c_double * len(w.TIMING_NAMES))()
    n = L.wspr_last_timings(C.addressof(ms), len(w.TIMING_NAMES))
    return {w.TIMING_NAMES[i]: ms[i] for i in range(n)}


def test_placements_agree_with_every_stage_on(w, stages_off, tmp_path):
    """The eight weak scenes of test_gpu_block.py and four crowded three-signal segments; block detection 3, a list of two
    of the sent messages, ordered statistics at depth 2 with every sender in the primed hash memory.  Both placements are
    exact, so spots and the whole trace record of every visited candidate are equal."""
    L = w.lab()
    weak = [synth.make_segment(s, bl.symbols_of, snr_db=-30.0) for s in RESCUED + LOST]
    crowd = [synth.make_segment(7000 + s, bl.symbols_of, n_signals=3, snr_db=-12.0, snr_span=16.0, t_jitter=0.5) for s in range(4)]
    I, Q = np.stack([x[0] for x in weak + crowd]), np.stack([x[1] for x in weak + crowd])
    assert w.set_block_detection(3, L) == 1
    assert w.set_message_list([weak[4][2][0][0], weak[5][2][0][0]], 96, L) == 2
    assert w.set_osd_depth(2, L) == -1
    opt = w.default_options()
    opt.usehashtable = 1
    senders = sorted({t[0].split()[0] for x in weak + crowd for t in x[2]} | set(synth.CALLS))
    runs = {}
    cwd = os.getcwd()
    for mode in (0, 1):
        os.makedirs(tmp_path / str(mode))
        os.chdir(tmp_path / str(mode))
        try:
            with open("hashtable.txt", "w") as f:
                for slot, call in sorted((w.lib().nhash(c.encode(), len(c), 146), c) for c in senders):
                    f.write("%5d %s %s\n" % (slot, call, "AA00"))
            L.wspr_set_fano_device_mode(mode)
            spots, tr = w.wspr_decode_batch_trace(I, Q, opt, max_results=16)
        finally:
            os.chdir(cwd)
        t = _timings(w, L)
        runs[mode] = ([[_spot(x) for x in g] for g in spots], _records(tr, len(I)))
        stages = [sum(tr[s].cand[p][j].decoded and pick(tr[s].cand[p][j]) for s in range(len(I)) for p in range(tr[s].passes_run)
                      for j in range(tr[s].n_visited[p]))
                  for pick in (lambda c: c.block >= 2, lambda c: c.cycles == 1, lambda c: c.cycles == 0)]
        print("placement %d: %d spots; decodes by block / list / OSD stage: %s; %s"
              % (mode, sum(len(g) for g in spots), stages, ", ".join("%s %d" % (k, t[k]) for k in COUNTERS)))
    assert sum(len(g) for g in runs[0][0]) >= 8
    assert runs[0][0] == runs[1][0]
    assert runs[0][1] == runs[1][1], _first_difference(runs[0][1], runs[1][1])


NSEG_EDGE = 160


@pytest.fixture(scope="module")
def edge_batch():
    segs = [synth.make_segment(8000 + s, bl.symbols_of, n_signals=3, snr_db=-31.0, snr_span=2.0) for s in range(NSEG_EDGE)]
    I, Q = np.stack([x[0] for x in segs]), np.stack([x[1] for x in segs])
    for a in (I, Q):
        a.setflags(write=False)
    return I, Q


@pytest.mark.parametrize("fano_on_device,quick", [(1, 0), (1, 1), (0, 1)])
def test_block_stage_chunk_edge(w, stages_off, edge_batch, fano_on_device, quick):
    """160 segments of three signals at -31 .. -33 dB, one pass without subtraction: one wave.  More than 256 of its
    candidates are worth a ladder and left undecoded by it (1.9 per segment where the batch was chosen), so the block stage
    takes them in two launches; the same segments in two halves stay within one launch each.  Spots and trace are equal
    segment for segment.  On the device the full ladder; on the host pool in quick mode, where the stage walks two vectors
    per candidate through the same chunks: the full walk there is 128 Fano time-outs per candidate, 33 ms each on sixteen
    threads where the batch was chosen, nine seconds per decode of this batch."""
    I, Q = edge_batch
    L = w.lab()
    assert w.set_block_detection(3, L) == 1
    opt = w.default_options(npasses=1, subtraction=0, quickmode=quick)
    half = NSEG_EDGE // 2

    def left_to_the_stage(tr, nseg):
        return sum(bool(np.float32(c.sync) > bl.MINSYNC1 and not (c.decoded and c.block == 1))
                   for s in range(nseg) for c in (tr[s].cand[0][j] for j in range(tr[s].n_visited[0])))
    L.wspr_set_fano_device_mode(fano_on_device)
    L.wspr_set_thread_slots(1)                   # one pipeline: the batch is not split, its pass is ONE wave
    try:
        spots, tr = w.wspr_decode_batch_trace(I, Q, opt, max_results=16)
    finally:
        L.wspr_set_thread_slots(0)               # the default again
    assert _timings(w, L)["gpu_waves"] == 1
    whole = ([[_spot(x) for x in g] for g in spots], _records(tr, NSEG_EDGE))
    n_whole = left_to_the_stage(tr, NSEG_EDGE)
    n_block = sum(tr[s].cand[0][j].block >= 2 for s in range(NSEG_EDGE) for j in range(tr[s].n_visited[0]))
    parts, n_parts = ([], []), []
    for lo in (0, half):
        sp, tp = w.wspr_decode_batch_trace(I[lo:lo + half], Q[lo:lo + half], opt, max_results=16)
        parts[0].extend([_spot(x) for x in g] for g in sp)
        parts[1].extend(_records(tp, half))
        n_parts.append(left_to_the_stage(tp, half))
    print("device Fano %d, quick %d: %d candidates left to the block stage (halves: %s), %d block decodes"
          % (fano_on_device, quick, n_whole, n_parts, n_block))
    assert n_whole > 256 and max(n_parts) < 256 and sum(n_parts) == n_whole, (n_whole, n_parts)
    assert n_block >= 1
    assert whole[0] == parts[0]
    assert whole[1] == parts[1], _first_difference(whole[1], parts[1])
