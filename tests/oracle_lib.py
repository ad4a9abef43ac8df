"""ctypes bindings of the CPU oracle (oracle/liboracle.so) and of the real reference, compiled by oracle/Makefile
into oracle/_ref/: the message-layer objects (libwsprd_ref.so), the decoder wsprd.c in an exact and a clang-fused
build (libwsprd_dsp_ref.so, libwsprd_dsp_ref_fma.so) and the receiver's decimator callback and file readers
(librtlsdr_front_ref.so).  TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg (those two use the oracle alone)."""
import contextlib
import ctypes as C
import os
import shutil
import subprocess
import tempfile
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
GOLDEN = os.path.join(ROOT, "tests", "golden")

NSYM, MAXCAND, NSAMP = 162, 200, 45000


class Options(C.Structure):            # reference wsprd/wsprd.h:44-52
    _fields_ = [("freq", C.c_int), ("rcall", C.c_char * 13), ("rloc", C.c_char * 7),
                ("quickmode", C.c_int), ("usehashtable", C.c_int),
                ("npasses", C.c_int), ("subtraction", C.c_int)]


class Spot(C.Structure):               # reference wsprd/wsprd.h:62-74
    _fields_ = [("freq", C.c_double), ("sync", C.c_float), ("snr", C.c_float),
                ("dt", C.c_float), ("drift", C.c_float), ("jitter", C.c_int),
                ("message", C.c_char * 23), ("call", C.c_char * 13),
                ("loc", C.c_char * 7), ("pwr", C.c_char * 3), ("cycles", C.c_int)]

    def key(self):
        return (self.message.decode(), self.call.decode(), self.loc.decode(), self.pwr.decode())

    def as_dict(self):
        return dict(freq=self.freq, sync=self.sync, snr=self.snr, dt=self.dt, drift=self.drift,
                    jitter=self.jitter, message=self.message.decode(), call=self.call.decode(),
                    loc=self.loc.decode(), pwr=self.pwr.decode(), cycles=self.cycles)


class Cand(C.Structure):               # reference wsprd/wsprd.h:54-60
    _fields_ = [("freq", C.c_float), ("snr", C.c_float), ("shift", C.c_int),
                ("drift", C.c_float), ("sync", C.c_float)]


P = 3


class Trace(C.Structure):
    _fields_ = [("passes_run", C.c_int), ("blocks", C.c_int),
                ("noise_level", C.c_float * P), ("npk", C.c_int * P),
                ("smspec_raw", (C.c_float * 411) * P),
                ("cand_peaks", (Cand * MAXCAND) * P),
                ("cand_coarse", (Cand * MAXCAND) * P),
                ("cand_fine", (Cand * MAXCAND) * P),
                ("mode0_shift", (C.c_int * MAXCAND) * P),
                ("mode0_sync", (C.c_float * MAXCAND) * P),
                ("n_visited", C.c_int * P),
                ("attempts", (C.c_int * MAXCAND) * P),
                ("fano_calls", (C.c_int * MAXCAND) * P),
                ("decoded", (C.c_int * MAXCAND) * P),
                ("subtracted", (C.c_int * MAXCAND) * P),
                ("first_rms", (C.c_float * MAXCAND) * P),
                ("first_sync2", (C.c_float * MAXCAND) * P),
                ("first_symbols", ((C.c_ubyte * NSYM) * MAXCAND) * P),
                ("fano_metric", (C.c_uint * MAXCAND) * P),
                ("fano_cycles", (C.c_uint * MAXCAND) * P),
                ("fano_maxnp", (C.c_uint * MAXCAND) * P),
                ("decdata", ((C.c_ubyte * 11) * MAXCAND) * P),
                ("fano_cycles_total", C.c_long)]


class Stops(C.Structure):              # oracle/wspr_oracle.h: orc_stops
    _fields_ = [("reason", C.c_int * P), ("cand", C.c_int * P)]


def default_options(freq=144489000, npasses=2, subtraction=1, quickmode=0):
    """Decoder defaults of rtlsdr_wsprd.c:357-362; dial 144.489 MHz = the '2m' band."""
    return Options(freq=freq, quickmode=quickmode, usehashtable=0,
                   npasses=npasses, subtraction=subtraction)


def build_oracle():
    subprocess.run(["make", "-s", "-C", ORACLE_DIR], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


_lib = None
_ref = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(ORACLE_DIR, "liboracle.so")
        if not os.path.exists(path):
            build_oracle()
        L = C.CDLL(path)
        L.orc_wspr_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, Options,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
        L.orc_wspr_decode.restype = C.c_int
        L.orc_wspr_decode_stops.argtypes = [C.c_void_p, C.c_void_p, C.c_int, Options,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orc_wspr_decode_stops.restype = C.c_int
        L.orc_nhash.restype = C.c_uint32
        L.orc_nhash.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32]
        L.orc_pack_call.restype = C.c_ulong
        L.orc_pack_call.argtypes = [C.c_char_p]
        L.orc_pack_grid4_power.restype = C.c_ulong
        L.orc_fano.restype = C.c_int
        L.orc_unpk.restype = C.c_int
        L.orc_channel_symbols.restype = C.c_int
        L.orc_pick_peaks.restype = C.c_int
        L.orc_blocks_for.restype = C.c_int
        L.orc_decim_new.restype = C.c_void_p
        L.orc_decim_feed.restype = C.c_uint32
        L.orc_decim_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                     C.c_uint32, C.c_uint32]
        L.orc_decim_free.argtypes = [C.c_void_p]
        L.orc_sync_demod.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int,
                                     C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.orc_subtract.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_int,
                                   C.c_float, C.c_void_p]
        L.orc_iq_from_interleaved.restype = C.c_int
        _lib = L
    return _lib


def ref_lib():
    """Real reference objects (fano.c, nhash.c, wsprd_utils.c, wsprsim_utils.c, tab.c).
    Returns None when the prebuilt library is not present."""
    global _ref
    if _ref is None:
        path = os.path.join(ORACLE_DIR, "_ref", "libwsprd_ref.so")
        if not os.path.exists(path):
            return None
        R = C.CDLL(path)
        R.nhash.restype = C.c_uint32
        R.nhash.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32]
        R.pack_call.restype = C.c_ulong
        R.pack_call.argtypes = [C.c_char_p]
        R.pack_grid4_power.restype = C.c_ulong
        R.fano.restype = C.c_int
        R.unpk_.restype = C.c_int
        R.get_wspr_channel_symbols.restype = C.c_int
        _ref = R
    return _ref


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------- the compiled reference
# The reference is not re-entrant (wsprd.c keeps its FFT plan in a global), and wspr_decode leaves files in the working
# directory (an empty fftw_wisdom.dat; hashtable.txt under usehashtable): one lock around every call, and every call
# runs inside a temporary directory.
_ref_lock = threading.RLock()
_ref_tmp = None
_DEMOD_ARGS = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
               C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
_SUBTRACT_ARGS = [C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_int, C.c_float, C.c_void_p]


@contextlib.contextmanager
def working_directory(cwd=None):
    """Hold the reference lock and run inside cwd (default: one temporary directory kept for the process)."""
    global _ref_tmp
    with _ref_lock:
        if cwd is None:
            if _ref_tmp is None:
                _ref_tmp = tempfile.TemporaryDirectory(prefix="wspr_ref_cwd_")
            cwd = _ref_tmp.name
        back = os.getcwd()
        os.chdir(cwd)
        try:
            yield
        finally:
            os.chdir(back)


def _bind_dsp(R):
    R.wspr_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, Options, C.c_void_p, C.c_void_p]
    R.wspr_decode.restype = C.c_int
    R.sync_and_demodulate.argtypes = _DEMOD_ARGS
    R.sync_and_demodulate.restype = None
    for f in (R.subtract_signal, R.subtract_signal2):
        f.argtypes = _SUBTRACT_ARGS
        f.restype = None


class RefDsp:
    """The reference's own wsprd.c, compiled; the one thing substituted is the FFT (the oracle's orc_fft512 behind an
    <fftw3.h> stand-in).  Methods take what the C functions take."""

    def __init__(self, path):
        lib()                                                   # liboracle.so first: the library needs orc_fft512 from it
        self.path = path
        self._lib = C.CDLL(path, mode=C.RTLD_LOCAL)
        _bind_dsp(self._lib)

    def decode(self, I, Q, samples=None, opt=None, cwd=None):
        """wspr_decode on copies of I/Q: (spots, residual I, Q).  cwd: where hashtable.txt lives (usehashtable)."""
        I = np.ascontiguousarray(I, dtype=np.float32).copy()
        Q = np.ascontiguousarray(Q, dtype=np.float32).copy()
        n = int(samples if samples is not None else I.size)
        spots = (Spot * 100)()
        nres = C.c_int(0)
        with working_directory(cwd):
            self._lib.wspr_decode(ptr(I), ptr(Q), n, opt or default_options(), C.addressof(spots), C.addressof(nres))
        return [spots[i] for i in range(nres.value)], I, Q

    def sync_and_demodulate(self, *args):
        with working_directory():
            self._lib.sync_and_demodulate(*args)

    def subtract_signal(self, *args):
        with working_directory():
            self._lib.subtract_signal(*args)

    def subtract_signal2(self, *args):
        with working_directory():
            self._lib.subtract_signal2(*args)


_ref_dsp = {}


def _ref_dsp_named(name):
    if name not in _ref_dsp:
        path = os.path.join(ORACLE_DIR, "_ref", name)
        if not os.path.exists(path):
            return None
        _ref_dsp[name] = RefDsp(path)
    return _ref_dsp[name]


def ref_dsp_lib():
    """wsprd.c as gcc builds it for x86-64 (no fused multiply-add).  None when the library is not present."""
    return _ref_dsp_named("libwsprd_dsp_ref.so")


def cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma " in line + " " for line in f)
    except OSError:
        return False


def ref_dsp_fma_lib():
    """wsprd.c as clang builds it with -ffp-contract=on -mfma.  None when the library is not present or the CPU has
    no FMA instructions to run it."""
    return _ref_dsp_named("libwsprd_dsp_ref_fma.so") if cpu_has_fma() else None


class RefFrontEnd:
    """One instance of the reference's rtlsdr_wsprd.c: its decimator callback with state of its own, and its file
    readers and writer.  The callback's state is function-static and cannot be reset, so every instance is a fresh
    copy of the library (beside a link to liboracle.so, which its decoder half needs)."""

    def __init__(self, path):
        lib()
        self._dir = tempfile.TemporaryDirectory(prefix="wspr_front_ref_")
        os.mkdir(os.path.join(self._dir.name, "_ref"))
        os.symlink(os.path.join(ORACLE_DIR, "liboracle.so"), os.path.join(self._dir.name, "liboracle.so"))
        copy = os.path.join(self._dir.name, "_ref", os.path.basename(path))
        shutil.copy(path, copy)
        R = C.CDLL(copy, mode=C.RTLD_LOCAL)
        R.front_ref_feed.argtypes = [C.c_void_p, C.c_uint32]
        R.front_ref_feed.restype = None
        R.front_ref_count.restype = C.c_uint32
        R.front_ref_read.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        R.front_ref_read.restype = None
        for f in (R.readRawIQfile, R.readC2file, R.writeRawIQfile):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p]
            f.restype = C.c_int32
        R.decoderSelfTest.restype = C.c_int32
        self._lib = R

    def feed(self, chunk):
        """One callback's worth of interleaved u8 IQ; returns the number of outputs so far.  The callback rewrites
        its buffer in place, so it gets a copy."""
        buf = np.array(chunk, dtype=np.uint8, copy=True)
        with working_directory():
            self._lib.front_ref_feed(ptr(buf), buf.size)
            return self._lib.front_ref_count()

    def outputs(self):
        with working_directory():
            n = self._lib.front_ref_count()
            I = np.zeros(NSAMP, np.float32)
            Q = np.zeros(NSAMP, np.float32)
            self._lib.front_ref_read(ptr(I), ptr(Q), n)
        return I, Q, n

    def read_iq(self, path):
        return self._read(self._lib.readRawIQfile, path)

    def read_c2(self, path):
        return self._read(self._lib.readC2file, path)

    def _read(self, fn, path):
        I = np.zeros(NSAMP, np.float32)
        Q = np.zeros(NSAMP, np.float32)
        with working_directory():
            n = fn(ptr(I), ptr(Q), os.path.abspath(path).encode())
        return I, Q, n

    def write_iq(self, I, Q, path):
        I = np.ascontiguousarray(I, dtype=np.float32)
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        assert I.size == NSAMP and Q.size == NSAMP
        with working_directory():
            return self._lib.writeRawIQfile(ptr(I), ptr(Q), os.path.abspath(path).encode())

    def self_test(self):
        """decoderSelfTest() under the receiver's default decoder options: 1 when the reference decodes its own
        synthesised signal (it prints the spot and leaves selftest.iq in the temporary directory)."""
        with working_directory():
            self._lib.initDecoder_options()
            return self._lib.decoderSelfTest()


def ref_front_end():
    """A fresh instance of the compiled reference receiver.  None when the library is not present."""
    path = os.path.join(ORACLE_DIR, "_ref", "librtlsdr_front_ref.so")
    if not os.path.exists(path):
        return None
    return RefFrontEnd(path)


def read_iq_file(path):
    """.iq reader semantics of rtlsdr_wsprd.c:555-592 via the oracle."""
    raw = np.fromfile(path, dtype=np.float32)
    I = np.zeros(NSAMP, np.float32)
    Q = np.zeros(NSAMP, np.float32)
    n = lib().orc_iq_from_interleaved(ptr(raw), C.c_int(raw.size), ptr(I), ptr(Q))
    return I, Q, n


def decode(I, Q, samples=None, opt=None, trace=False):
    """Run the oracle decoder on copies of I/Q. Returns (spots, residual I, Q[, trace]); the trace also carries, per
    pass, where the candidate loop stopped early (stop_reason 0 none / 1 re-encode failed / 2 "A000AA", stop_cand)."""
    L = lib()
    I = np.ascontiguousarray(I, dtype=np.float32).copy()
    Q = np.ascontiguousarray(Q, dtype=np.float32).copy()
    n = int(samples if samples is not None else I.size)
    opt = opt or default_options()
    spots = (Spot * 100)()
    nres = C.c_int(0)
    tr = Trace() if trace else None
    if trace:
        st = Stops()
        L.orc_wspr_decode_stops(ptr(I), ptr(Q), n, opt, C.addressof(spots), C.addressof(nres), C.addressof(tr),
                                C.addressof(st))
        tr.stop_reason, tr.stop_cand = list(st.reason), list(st.cand)
    else:
        L.orc_wspr_decode(ptr(I), ptr(Q), n, opt, C.addressof(spots), C.addressof(nres), None)
    out = [spots[i] for i in range(nres.value)]
    return (out, I, Q, tr) if trace else (out, I, Q)


def channel_symbols(message, L=None):
    L = L or lib()
    hashtab = C.create_string_buffer(32768 * 13)
    loctab = C.create_string_buffer(32768 * 5)
    sym = (C.c_ubyte * NSYM)()
    msg = C.create_string_buffer(message.encode(), 32)
    ok = L.orc_channel_symbols(msg, hashtab, loctab, sym)
    return ok, np.frombuffer(sym, dtype=np.uint8).copy()


def spot_line(s):
    """-r print format, rtlsdr_wsprd.c:691-701."""
    return "Spot : %6.2f %6.2f %10.6f %2d %7s %6s %2s" % (
        s.snr, s.dt, s.freq, int(s.drift), s.call.decode(), s.loc.decode(), s.pwr.decode())
