"""The product against the reference's own compiled code, with no checker in between.

oracle/_ref/libwsprd_dsp_ref.so is the reference's wsprd.c as gcc builds it for x86-64, libwsprd_dsp_ref_fma.so the same
file as clang builds it with -ffp-contract=on -mfma, librtlsdr_front_ref.so its receiver with the decimator callback
(oracle/Makefile; the one thing substituted is the FFT, the oracle's orc_fft512 behind an <fftw3.h> stand-in).  The
exact mode is held to the first, wspr_set_arithmetic(WSPR_ARITH_CONTRACTED) to the second, the streaming decimator to
the third: every spot field with ==, snr included, residuals and decimator outputs bit for bit.  Only the prebuilt
libraries are read.  Kept small: the reference decodes one segment at a time on the host."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
import trace_parity
from test_gpu_parity import _DecimState, _raw_stream, random_scenes
from test_reference_pin import FIELDS, parity_segments, ref_iq

pytestmark = pytest.mark.gpu

NS = 45000


@pytest.fixture(scope="module")
def w():
    import rtlsdr_wsprd_amd as mod
    assert mod.lib().wspr_device_ready() == 1
    return mod


@pytest.fixture(params=["exact", "contracted"])
def pinned(request, w):
    """(compiled reference, mode name) with the product switched to the matching arithmetic."""
    if request.param == "exact":
        R = ol.ref_dsp_lib()
        if R is None:
            pytest.skip("oracle/_ref/libwsprd_dsp_ref.so is not built")
        yield R, request.param
        return
    if not os.path.exists(os.path.join(ol.ORACLE_DIR, "_ref", "libwsprd_dsp_ref_fma.so")):
        pytest.skip("oracle/_ref/libwsprd_dsp_ref_fma.so is not built")
    R = ol.ref_dsp_fma_lib()
    if R is None:
        pytest.skip("this CPU has no FMA instructions")
    assert w.wspr_set_arithmetic(w.WSPR_ARITH_CONTRACTED) == w.WSPR_ARITH_EXACT
    try:
        yield R, request.param
    finally:
        w.wspr_set_arithmetic(w.WSPR_ARITH_EXACT)


def fields(s):
    return tuple(getattr(s, k) for k in FIELDS)


def test_wspr_decode_on_the_reference_file(w, pinned):
    R, mode = pinned
    I, Q = ref_iq()
    spots, ri, rq = w.wspr_decode(I, Q, NS, w.default_options())
    ref, oi, oq = R.decode(I, Q, NS)
    print(mode, [fields(s) for s in spots], [fields(s) for s in ref])
    assert [fields(s) for s in spots] == [fields(s) for s in ref] and len(ref) == 1
    assert ri.tobytes() == oi.tobytes() and rq.tobytes() == oq.tobytes()


def test_wspr_decode_batch_on_the_parity_batch_and_random_scenes(w, pinned):
    R, mode = pinned
    I, Q = trace_parity.parity_batch()
    Ir, Qr = random_scenes(24)
    I = np.ascontiguousarray(np.concatenate([I, Ir])); Q = np.ascontiguousarray(np.concatenate([Q, Qr]))
    gi, gq = I.copy(), Q.copy()
    nseg, max_results = I.shape[0], 32
    out = (w.decoder_results * (nseg * max_results))()
    nres = (C.c_int * nseg)()
    assert w.lib().wspr_decode_batch(ol.ptr(gi), ol.ptr(gq), nseg, NS, NS, w.default_options(), C.addressof(out),
                                     max_results, C.addressof(nres), 1) == 0
    total = 0
    for s in range(nseg):
        ref, oi, oq = R.decode(I[s], Q[s], NS)
        got = [out[s * max_results + i] for i in range(nres[s])]
        if [fields(x) for x in got] != [fields(x) for x in ref]:
            print(mode, s, [fields(x) for x in got], [fields(x) for x in ref])
        assert [fields(x) for x in got] == [fields(x) for x in ref], (mode, s)
        assert gi[s].tobytes() == oi.tobytes() and gq[s].tobytes() == oq.tobytes(), (mode, s)
        total += len(ref)
    assert total > 40


def test_exported_stages_on_the_first_parity_signal(w, pinned):
    """sync_and_demodulate in its three modes and both subtractions, the product's exports against the reference's of
    the same names.  subtract_signal() is compared in the exact mode only: the product keeps it exact in both modes
    (include/wspr_mi355x.h), while the fused build fuses inside it."""
    R, mode = pinned
    I, Q, truth = parity_segments()
    msg, f0, t0, snr = truth[0][0]
    fc = float(np.float32(round(f0 / 0.732421875) * 0.732421875))
    sc = int(round(t0 * 375 / 128.0)) * 128

    def demod(fn, freq, shift, m, **kw):
        Ic, Qc = I[0].copy(), Q[0].copy()
        f = C.c_float(freq); sh = C.c_int(shift); dr = C.c_float(0.0); sy = C.c_float(0)
        sym = (C.c_ubyte * 162)()
        fn(ol.ptr(Ic), ol.ptr(Qc), C.c_long(NS), C.addressof(sym), C.addressof(f), kw.get("ifmin", 0), kw.get("ifmax", 0),
           C.c_float(kw.get("fstep", 0.0)), C.addressof(sh), kw.get("lagmin", 0), kw.get("lagmax", 0), 8, C.addressof(dr),
           50, C.addressof(sy), m)
        return f.value, sh.value, sy.value, bytes(sym)

    G = w.lib()
    r = demod(R.sync_and_demodulate, fc, sc, 0, lagmin=sc - 128, lagmax=sc + 128)
    assert demod(G.sync_and_demodulate, fc, sc, 0, lagmin=sc - 128, lagmax=sc + 128)[:3] == r[:3]
    shift = r[1]
    r = demod(R.sync_and_demodulate, fc, shift, 1, ifmin=-2, ifmax=2, fstep=0.1)
    assert demod(G.sync_and_demodulate, fc, shift, 1, ifmin=-2, ifmax=2, fstep=0.1)[:3] == r[:3]
    fbest = r[0]
    for jig in (0, -3, 63):
        r = demod(R.sync_and_demodulate, fbest, shift + jig, 2)
        assert demod(G.sync_and_demodulate, fbest, shift + jig, 2)[2:] == r[2:], (mode, jig)

    # scans of one frequency from a small *freq with a step that is not exact in float32: f0 = *freq + ifreq * fstep
    # (wsprd.c:151) comes back, rounded once (contracted) or twice (exact)
    for k in range(-20, 21):
        r = demod(R.sync_and_demodulate, 0.37, shift, 1, ifmin=k, ifmax=k, fstep=0.0137)
        assert demod(G.sync_and_demodulate, 0.37, shift, 1, ifmin=k, ifmax=k, fstep=0.0137)[:3] == r[:3], (mode, k)

    sym = ol.channel_symbols(msg)[1]
    pairs = [(G.subtract_signal2, R.subtract_signal2)] + ([(G.subtract_signal, R.subtract_signal)] if mode == "exact" else [])
    for gfn, rfn in pairs:
        outs = []
        for fn in (gfn, rfn):
            Ic, Qc = I[0].copy(), Q[0].copy()
            fn(ol.ptr(Ic), ol.ptr(Qc), C.c_long(NS), C.c_float(f0), C.c_int(int(round(t0 * 375))), C.c_float(0.0), ol.ptr(sym))
            outs.append((Ic, Qc))
        assert not np.array_equal(outs[1][0], I[0])
        assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes(), mode


def test_streaming_decimator_against_the_compiled_callback(w):
    """The stream of test_streaming_decimator_any_chunking_equals_oracle in callbacks of 65536 bytes."""
    fe = ol.ref_front_end()
    if fe is None:
        pytest.skip("oracle/_ref/librtlsdr_front_ref.so is not built")
    rng = np.random.default_rng(21)
    nsamp = 6401 * 90 + 3206
    raw = _raw_stream(rng, nsamp)
    raw[1000:1256] = 0
    raw[70000:70512] = 255
    nbytes = raw.size
    GL = w.lib()
    GL.wspr_decimate_u8_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32,
                                           C.c_uint32, C.c_void_p]
    gi = np.zeros(NS, np.float32); gq = np.zeros(NS, np.float32)
    gs = _DecimState()
    GL.wspr_decim_stream_reset(C.byref(gs))
    gfill = C.c_uint32(0)
    for pos in range(0, nbytes, 65536):
        chunk = np.ascontiguousarray(raw[pos:pos + 65536])
        assert GL.wspr_decimate_u8_stream(C.byref(gs), ol.ptr(chunk), chunk.size, ol.ptr(gi), ol.ptr(gq), gfill.value, NS,
                                          C.byref(gfill)) == 0
        assert fe.feed(chunk) == gfill.value, pos
    ri, rq, n = fe.outputs()
    assert n == gfill.value == 90
    assert gi.tobytes() == ri.tobytes() and gq.tobytes() == rq.tobytes()
