"""rtlsdr-wsprd_amd -- MI355X-native WSPR decode path.

Thin ctypes mirror of the C ABI in include/wspr_mi355x.h (the product is the shared
library rtlsdr-wsprd_amd/libwspr_mi355x.so: hand-written HIP kernels for gfx950 + a
C++ host scheduler).  Names follow the reference's C interface
(wsprd/wsprd.h:44-111): decoder_options, decoder_results, wspr_decode.

There is NO CPU fallback: every entry point raises if the library is missing and
the library itself refuses to run without a HIP device.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwspr_mi355x.so")

NSAMPLES = 45000
NSYM = 162
MAX_CANDIDATES = 200


class decoder_options(C.Structure):          # wsprd/wsprd.h:44-52
    _fields_ = [("freq", C.c_int), ("rcall", C.c_char * 13), ("rloc", C.c_char * 7),
                ("quickmode", C.c_int), ("usehashtable", C.c_int),
                ("npasses", C.c_int), ("subtraction", C.c_int)]


class decoder_results(C.Structure):          # wsprd/wsprd.h:62-74
    _fields_ = [("freq", C.c_double), ("sync", C.c_float), ("snr", C.c_float),
                ("dt", C.c_float), ("drift", C.c_float), ("jitter", C.c_int),
                ("message", C.c_char * 23), ("call", C.c_char * 13),
                ("loc", C.c_char * 7), ("pwr", C.c_char * 3), ("cycles", C.c_int)]

    def as_dict(self):
        return dict(freq=self.freq, sync=self.sync, snr=self.snr, dt=self.dt, drift=self.drift,
                    jitter=self.jitter, message=self.message.decode(), call=self.call.decode(),
                    loc=self.loc.decode(), pwr=self.pwr.decode(), cycles=self.cycles)


class cand(C.Structure):                     # wsprd/wsprd.h:54-60
    _fields_ = [("freq", C.c_float), ("snr", C.c_float), ("shift", C.c_int),
                ("drift", C.c_float), ("sync", C.c_float)]


class wspr_synth_tx(C.Structure):            # include/wspr_mi355x.h: one transmission of a synthesised scene
    _fields_ = [("seg", C.c_int32), ("f0", C.c_float), ("t0", C.c_float), ("amp", C.c_float), ("drift", C.c_float),
                ("symbols", C.c_ubyte * 162), ("pad", C.c_ubyte * 2)]


# the same layout for numpy: a scene as one structured array (np.zeros(n, SYNTH_TX_DTYPE), fields filled columnwise)
SYNTH_TX_DTYPE = np.dtype([("seg", "<i4"), ("f0", "<f4"), ("t0", "<f4"), ("amp", "<f4"), ("drift", "<f4"),
                           ("symbols", "u1", (162,)), ("pad", "u1", (2,))])
assert SYNTH_TX_DTYPE.itemsize == C.sizeof(wspr_synth_tx) == 184


class wspr_synth_path(C.Structure):          # one path of a fading channel: linear gain, Doppler shift and spread in Hz
    _fields_ = [("gain", C.c_float), ("shift", C.c_float), ("sigma", C.c_float)]


class wspr_synth_channel(C.Structure):       # the channel of one transmission (wspr_synth_faded*()), 24 bytes
    _fields_ = [("path", wspr_synth_path * 2)]


SYNTH_CHANNEL_DTYPE = np.dtype([("path", [("gain", "<f4"), ("shift", "<f4"), ("sigma", "<f4")], (2,))])
assert SYNTH_CHANNEL_DTYPE.itemsize == C.sizeof(wspr_synth_channel) == 24
SYNTH_ACCUMULATE = 1
SYNTH_NORMALISE = 2

TRACE_PASSES = 3


class cand_trace(C.Structure):               # include/wspr_mi355x_bench.h: wspr_cand_trace
    _fields_ = [("visited", C.c_int), ("mode0_shift", C.c_int), ("mode0_sync", C.c_float),
                ("freq", C.c_float), ("shift", C.c_int), ("drift", C.c_float), ("sync", C.c_float),
                ("attempts", C.c_int), ("fano_calls", C.c_int), ("first_sync", C.c_float), ("first_rms", C.c_float),
                ("decoded", C.c_int), ("subtracted", C.c_int), ("jitter", C.c_int), ("cycles", C.c_uint),
                ("first_symbols", C.c_ubyte * NSYM), ("decdata", C.c_ubyte * 11), ("stop", C.c_ubyte), ("block", C.c_ubyte),
                ("pad", C.c_ubyte * 1)]


class trace(C.Structure):                    # include/wspr_mi355x_bench.h: wspr_trace
    _fields_ = [("passes_run", C.c_int), ("npk", C.c_int * TRACE_PASSES), ("n_visited", C.c_int * TRACE_PASSES),
                ("cand", (cand_trace * MAX_CANDIDATES) * TRACE_PASSES)]


WSPR_ARITH_EXACT, WSPR_ARITH_CONTRACTED = 0, 1    # include/wspr_mi355x.h: wspr_set_arithmetic()


def default_options(freq=144489000, npasses=2, subtraction=1, quickmode=0):
    """initDecoder_options(), rtlsdr_wsprd.c:357-362."""
    return decoder_options(freq=freq, quickmode=quickmode, usehashtable=0,
                           npasses=npasses, subtraction=subtraction)


def build(verbose=False):
    """Compile the HIP extension in-tree for gfx950 (works without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.run(["bash", os.path.join(_HERE, "csrc", "build.sh")], check=True, stdout=out, stderr=out)


LAB_PATH = os.path.join(_HERE, "libwspr_mi355x_lab.so")
_lib = None
_lab = None


def _bind(path):
    """CDLL + argument types of every entry point the library exports (the lab-only ones where present)."""
    L = C.CDLL(path)
    L.wspr_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, decoder_options, C.c_void_p, C.c_void_p]
    L.wspr_decode.restype = C.c_int
    L.wspr_decode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, decoder_options,
                                    C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.wspr_decode_batch.restype = C.c_int
    L.wspr_decode_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t,
                                           decoder_options, C.c_void_p, C.c_int, C.c_void_p]
    L.wspr_decode_batch_device.restype = C.c_int
    L.wspr_iq_stride.restype = C.c_size_t
    L.wspr_mi355x_version.restype = C.c_char_p
    L.wspr_device_ready.restype = C.c_int
    L.sync_and_demodulate.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_int]
    L.sync_and_demodulate.restype = None
    L.subtract_signal2.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_int, C.c_float, C.c_void_p]
    L.subtract_signal2.restype = None
    L.wspr_last_timings.argtypes = [C.c_void_p, C.c_int]
    L.wspr_decimate_u8.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.wspr_decimate_u8_batch_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.wspr_pin_host_buffer.argtypes = [C.c_void_p, C.c_size_t]
    L.wspr_unpin_host_buffer.argtypes = [C.c_void_p]
    L.wspr_release_buffers.restype = C.c_size_t
    L.wspr_set_fano_fast_budget.restype = C.c_uint
    L.wspr_set_arithmetic.argtypes = [C.c_int]
    L.wspr_set_arithmetic.restype = C.c_int
    L.wspr_set_osd_depth.argtypes = [C.c_int]
    L.wspr_set_osd_depth.restype = C.c_int
    L.wspr_osd_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.wspr_osd_batch_device.restype = C.c_int
    L.wspr_set_block_detection.argtypes = [C.c_int]
    L.wspr_set_block_detection.restype = C.c_int
    L.wspr_block_demod_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
    L.wspr_block_demod_batch.restype = C.c_int
    L.wspr_spread_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
    L.wspr_spread_batch.restype = C.c_int
    L.wspr_set_spread_estimate.argtypes = [C.c_int]
    L.wspr_set_spread_estimate.restype = C.c_int
    L.wspr_last_spreads.argtypes = [C.c_void_p, C.c_int]
    L.wspr_last_spreads.restype = C.c_int
    L.wspr_spot_quality_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.wspr_spot_quality_batch_device.restype = C.c_int
    L.wspr_set_spot_details.argtypes = [C.c_int]
    L.wspr_set_spot_details.restype = C.c_int
    L.wspr_last_spot_details.argtypes = [C.c_void_p, C.c_int]
    L.wspr_last_spot_details.restype = C.c_int
    L.wspr_format_spot_extended.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.wspr_format_spot_extended.restype = C.c_int
    L.wspr_set_message_list.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.wspr_set_message_list.restype = C.c_int
    L.wspr_message_list_entry.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.wspr_message_list_entry.restype = C.c_int
    L.wspr_list_match_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.wspr_list_match_batch_device.restype = C.c_int
    L.wspr_synth_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int,
                                          C.c_void_p, C.c_void_p]
    L.wspr_synth_batch_device.restype = C.c_int
    L.wspr_synth.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    L.wspr_synth.restype = C.c_int
    L.wspr_synth_faded_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64,
                                                C.c_int, C.c_void_p, C.c_void_p]
    L.wspr_synth_faded_batch_device.restype = C.c_int
    L.wspr_synth_faded.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    L.wspr_synth_faded.restype = C.c_int
    L.wspr_audio_batch_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.wspr_audio_batch_device.restype = C.c_int
    L.wspr_audio_to_iq.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.wspr_audio_to_iq.restype = C.c_int
    L.wspr_audio_constants.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.wspr_audio_constants.restype = None
    L.wspr_audio_blank_batch_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                C.c_size_t, C.c_void_p]
    L.wspr_audio_blank_batch_device.restype = C.c_int
    L.wspr_audio_blanked_batch_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                  C.c_void_p, C.c_int, C.c_void_p]
    L.wspr_audio_blanked_batch_device.restype = C.c_int
    L.wspr_audio_to_iq_blanked.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int, C.c_void_p]
    L.wspr_audio_to_iq_blanked.restype = C.c_int
    L.wspr_noise_default_windows.argtypes = [C.c_void_p]
    L.wspr_noise_default_windows.restype = None
    L.wspr_noise_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
    L.wspr_noise_batch_device.restype = C.c_int
    L.wspr_noise.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.wspr_noise.restype = C.c_int
    L.wspr_waterfall_default_params.argtypes = [C.c_void_p]
    L.wspr_waterfall_default_params.restype = None
    L.wspr_waterfall_shape.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.wspr_waterfall_shape.restype = C.c_int
    L.wspr_waterfall_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p,
                                              C.c_size_t, C.c_void_p]
    L.wspr_waterfall_batch_device.restype = C.c_int
    L.wspr_waterfall.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.wspr_waterfall.restype = C.c_int
    L.wspr_waterfall_palette.argtypes = [C.c_int, C.c_void_p]
    L.wspr_waterfall_palette.restype = None
    L.wspr_write_pgm_file.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    L.wspr_write_pgm_file.restype = C.c_int
    L.wspr_write_png_file.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.wspr_write_png_file.restype = C.c_int
    L.wspr_read_wav_file.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t]
    L.wspr_read_wav_file.restype = C.c_size_t
    L.wspr_write_wav_file.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t]
    L.wspr_write_wav_file.restype = C.c_int
    L.wspr_synth_audio_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64,
                                                C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    L.wspr_synth_audio_batch_device.restype = C.c_int
    L.wspr_synth_audio.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    L.wspr_synth_audio.restype = C.c_int
    L.wspr_iq_to_audio_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_float, C.c_void_p,
                                                C.c_size_t, C.c_void_p]
    L.wspr_iq_to_audio_batch_device.restype = C.c_int
    L.wspr_iq_to_audio.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    L.wspr_iq_to_audio.restype = C.c_int
    L.wspr_write_c2_file.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_double]
    L.wspr_write_c2_file.restype = C.c_int
    L.wspr_tune_step.argtypes = [C.c_double, C.c_void_p]
    L.wspr_tune_step.restype = C.c_uint32
    L.wspr_tune_u8_batch_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.wspr_tune_u8_batch_device.restype = C.c_int
    L.wspr_tune_u8.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.wspr_tune_u8.restype = C.c_int
    L.wspr_tune_constants.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.wspr_tune_constants.restype = None
    L.wspr_selftest.argtypes = [decoder_options, C.c_void_p]
    L.wspr_selftest.restype = C.c_int
    L.nhash.restype = C.c_uint32
    L.nhash.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32]
    L.pack_call.restype = C.c_ulong
    L.pack_call.argtypes = [C.c_char_p]
    L.pack_grid4_power.restype = C.c_ulong
    L.get_callsign_character_code.restype = C.c_byte
    L.get_locator_character_code.restype = C.c_byte
    L.fano.restype = C.c_int
    L.unpk_.restype = C.c_int
    L.get_wspr_channel_symbols.restype = C.c_int
    if hasattr(L, "wspr_stage_fft_bank"):            # include/wspr_mi355x_bench.h: the lab build only
        L.wspr_stage_fft_bank.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p]
        L.wspr_stage_fft_bank.restype = C.c_int
        L.wspr_stage_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.wspr_stage_candidates.restype = C.c_int
        L.wspr_stage_candidates_ps.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
        L.wspr_stage_candidates_ps.restype = C.c_int
        L.wspr_bench_fft_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_void_p]
        L.wspr_bench_valu.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_void_p]
        L.wspr_bench_decimate.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.wspr_calib_read.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        L.wspr_calib_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.wspr_calib_copy16.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        L.wspr_calib_valu.argtypes = [C.c_int, C.c_void_p]
        L.wspr_decode_batch_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, decoder_options,
                                              C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return L


def lib():
    """The PRODUCT library, libwspr_mi355x.so (raises if it has not been built).  WSPR_USE_LAB=1 makes this the lab
    library instead, for whole-suite runs of the lab build and for tests that need one of its environment switches."""
    global _lib
    if os.environ.get("WSPR_USE_LAB") == "1":
        return lab()
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libwspr_mi355x.so is not built: run rtlsdr-wsprd_amd/csrc/build.sh "
                               "(there is no CPU fallback)")
        _lib = _bind(LIB_PATH)
    return _lib


def lab():
    """The LAB build of the same sources, libwspr_mi355x_lab.so: everything the product exports plus the stage-level
    parity hooks, the per-candidate trace, kernel timings and calibration kernels of include/wspr_mi355x_bench.h.
    A separate library with its own contexts and streams: tests and bench.py use it for those calls only."""
    global _lab
    if _lab is None:
        if not os.path.exists(LAB_PATH):
            raise RuntimeError("libwspr_mi355x_lab.so is not built: run rtlsdr-wsprd_amd/csrc/build.sh")
        _lab = _bind(LAB_PATH)
    return _lab


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def wspr_set_arithmetic(mode, library=None):
    """Process-wide arithmetic of the signal-processing stages (include/wspr_mi355x.h): WSPR_ARITH_EXACT (default) or
    WSPR_ARITH_CONTRACTED.  Returns the previous mode, or -1 (nothing changed) for any other value.  The product and
    the lab library each keep their own setting: `library` (default: lib()) is the one set."""
    return (library or lib()).wspr_set_arithmetic(int(mode))


def set_osd_depth(depth, library=None):
    """wspr_set_osd_depth() of include/wspr_mi355x.h: -1 switches the ordered-statistics rescue stage off (the default),
    0..3 set its depth for every later decode call.  Returns the previous value, or -2 (nothing changed) for any other
    argument.  Like the arithmetic mode, the product and the lab library each keep their own setting."""
    return (library or lib()).wspr_set_osd_depth(int(depth))


def osd_batch(symbols, depth, library=None):
    """wspr_osd_batch_device(): ordered-statistics decoding of n vectors of 162 soft symbols (uint8 [n, 162], transmission
    order).  Returns (data uint8 [n, 11], dist, nhard, order as uint32 [n]); raises if the library refuses the call."""
    sym = np.ascontiguousarray(symbols, dtype=np.uint8).reshape(-1, NSYM)
    n = sym.shape[0]
    data = np.zeros((n, 11), np.uint8)
    dist, nhard, order = (np.zeros(n, np.uint32) for _ in range(3))
    rc = (library or lib()).wspr_osd_batch_device(_ptr(sym), n, int(depth), _ptr(data), _ptr(dist), _ptr(nhard), _ptr(order))
    if rc != 0:
        raise RuntimeError("wspr_osd_batch_device failed (rc %d: depth outside 0..3, or no usable HIP device)" % rc)
    return data, dist, nhard, order


# include/wspr_mi355x.h: wspr_block_item, one hypothesis of wspr_block_demod_batch()
BLOCK_ITEM_DTYPE = np.dtype([("seg", "<i4"), ("freq", "<f4"), ("shift", "<i4"), ("drift", "<f4")])


def set_block_detection(maxblock, library=None):
    """wspr_set_block_detection() of include/wspr_mi355x.h: 1 switches the noncoherent block-detection stage off (the
    default), 2 or 3 set the largest block size every later decode call tries.  Returns the previous value, or -2 (nothing
    changed) for any other argument.  The product and the lab library each keep their own setting."""
    return (library or lib()).wspr_set_block_detection(int(maxblock))


def block_demod(I, Q, items, library=None):
    """wspr_block_demod_batch(): host rows [nseg, samples] and n hypotheses (seg, freq, shift, drift) -- a numpy array of
    BLOCK_ITEM_DTYPE or a list of such tuples.  Returns uint8 [n, 3, 162]: the soft-symbol vectors of block sizes 1, 2, 3 in
    transmission order; raises if the library refuses the call."""
    I = np.ascontiguousarray(I, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    if I.ndim == 1:
        I, Q = I[None, :], Q[None, :]
    nseg, samples = I.shape
    it = items if isinstance(items, np.ndarray) and items.dtype == BLOCK_ITEM_DTYPE else np.array(
        [tuple(x) for x in items], BLOCK_ITEM_DTYPE)
    it = np.ascontiguousarray(it)
    n = int(it.size)
    sym = np.zeros((n, 3, NSYM), np.uint8)
    rc = (library or lib()).wspr_block_demod_batch(_ptr(I), _ptr(Q), nseg, samples, samples, _ptr(it), n, _ptr(sym))
    if rc != 0:
        raise RuntimeError("wspr_block_demod_batch failed (rc %d: bad arguments, or no usable HIP device)" % rc)
    return sym


# include/wspr_mi355x.h: wspr_spread_item (one job of wspr_spread_batch()) and wspr_spread (its result, and one record of
# wspr_last_spreads())
SPREAD_ITEM_DTYPE = np.dtype([("seg", "<i4"), ("f0", "<f4"), ("shift", "<i4"), ("drift", "<f4"), ("symbols", "u1", (NSYM,)),
                              ("pad", "u1", (2,))])
SPREAD_DTYPE = np.dtype([("w50", "<f4"), ("f50", "<f4"), ("ratio", "<f4"), ("valid", "<i4"), ("f0", "<f4"), ("shift", "<i4"),
                         ("drift", "<f4"), ("pad", "<i4")])


def set_spread_estimate(on, library=None):
    """wspr_set_spread_estimate() of include/wspr_mi355x.h: 1 adds a Doppler-spread figure per spot to every later decode
    call (read back with last_spreads()), 0 switches it off (the default).  Returns the previous value, or -2 (nothing
    changed) for any other argument.  The product and the lab library each keep their own setting."""
    return (library or lib()).wspr_set_spread_estimate(int(on))


def spread_batch(I, Q, items, samples=None, library=None):
    """wspr_spread_batch(): host rows [nseg, row length] of which `samples` count (default: all), and n jobs -- a numpy
    array of SPREAD_ITEM_DTYPE.  Returns a SPREAD_DTYPE array [n]; raises if the library refuses the call."""
    I = np.ascontiguousarray(I, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    if I.ndim == 1:
        I, Q = I[None, :], Q[None, :]
    nseg, width = I.shape
    it = np.ascontiguousarray(items, dtype=SPREAD_ITEM_DTYPE)
    out = np.zeros(int(it.size), SPREAD_DTYPE)
    rc = (library or lib()).wspr_spread_batch(_ptr(I), _ptr(Q), nseg, width if samples is None else int(samples), width,
                                              _ptr(it), int(it.size), _ptr(out))
    if rc != 0:
        raise RuntimeError("wspr_spread_batch failed (rc %d: bad arguments, or no usable HIP device)" % rc)
    return out


def last_spreads(nseg, max_results, library=None):
    """wspr_last_spreads() for a call of nseg segments and max_results spots each: a SPREAD_DTYPE array [nseg, max_results]
    (entries beyond a segment's spots are zero), or None where the library answers -1 (stage off for that call, or a
    call that does not record them)."""
    out = np.zeros((int(nseg), int(max_results)), SPREAD_DTYPE)
    n = (library or lib()).wspr_last_spreads(_ptr(out), int(out.size))
    return out if n == out.size else None


# include/wspr_mi355x.h: wspr_spot_quality (the figures of one job of wspr_spot_quality_batch_device()) and
# wspr_spot_detail (one record of wspr_last_spot_details(): the figures and the spot's provenance)
SPOT_QUALITY_DTYPE = np.dtype([("nhard", "<i4"), ("dist", "<i4"), ("rsum", "<i4"), ("v2", "<i4"), ("metric", "<i4")])
SPOT_DETAIL_DTYPE = np.dtype([("nhard", "<i4"), ("dist", "<i4"), ("rsum", "<i4"), ("v2", "<i4"), ("metric", "<i4"),
                              ("pass", "u1"), ("stage", "u1"), ("block", "u1"), ("valid", "u1"), ("cand", "<i4"), ("pad", "<i4")])
STAGE_LADDER, STAGE_BLOCK2, STAGE_BLOCK3, STAGE_LIST, STAGE_OSD = 1, 2, 3, 4, 5   # wspr_spot_detail.stage: WSPR_STAGE_*


def set_spot_details(on, library=None):
    """wspr_set_spot_details() of include/wspr_mi355x.h: 1 adds a record of decode-quality figures and provenance per spot
    to every later decode call (read back with last_spot_details()), 0 switches it off (the default).  Returns the previous
    value, or -2 (nothing changed) for any other argument.  The product and the lab library each keep their own setting."""
    return (library or lib()).wspr_set_spot_details(int(on))


def spot_quality_batch(symbols, decdata, library=None):
    """wspr_spot_quality_batch_device(): the figures of n vectors of 162 soft symbols (uint8 [n, 162], transmission order)
    against the code words of their decdata (uint8 [n, 11], as fano() leaves it).  Returns a SPOT_QUALITY_DTYPE array [n];
    raises if the library refuses the call."""
    sym = np.ascontiguousarray(symbols, dtype=np.uint8).reshape(-1, NSYM)
    dec = np.ascontiguousarray(decdata, dtype=np.uint8).reshape(-1, 11)
    if dec.shape[0] != sym.shape[0]:
        raise ValueError("one decdata per vector")
    out = np.zeros(sym.shape[0], SPOT_QUALITY_DTYPE)
    rc = (library or lib()).wspr_spot_quality_batch_device(_ptr(sym), _ptr(dec), sym.shape[0], _ptr(out))
    if rc != 0:
        raise RuntimeError("wspr_spot_quality_batch_device failed (rc %d: bad arguments, or no usable HIP device)" % rc)
    return out


def last_spot_details(nseg, max_results, library=None):
    """wspr_last_spot_details() for a call of nseg segments and max_results spots each: a SPOT_DETAIL_DTYPE array
    [nseg, max_results] (entries beyond a segment's spots are zero), or None where the library answers -1 (stage off for
    that call, or a call that does not record them)."""
    out = np.zeros((int(nseg), int(max_results)), SPOT_DETAIL_DTYPE)
    n = (library or lib()).wspr_last_spot_details(_ptr(out), int(out.size))
    return out if n == out.size else None


def format_spot_extended(result, detail, cap=160, library=None):
    """wspr_format_spot_extended(): the "Spot : ..." line of a decoder_results followed by pass, stage, block, nhard, dist
    and metric of its SPOT_DETAIL_DTYPE record.  Returns (text, length of the whole line); the text holds at most cap - 1
    characters."""
    rec = np.ascontiguousarray(np.asarray(detail, dtype=SPOT_DETAIL_DTYPE).reshape(1))
    buf = C.create_string_buffer(max(1, int(cap)))
    n = (library or lib()).wspr_format_spot_extended(C.byref(result), _ptr(rec), buf, int(cap))
    return buf.value.decode("ascii", "replace"), n


LIST_MAX = 65536                   # include/wspr_mi355x.h: WSPR_LIST_MAX
# include/wspr_mi355x.h: wspr_list_match, the result of K14 for one vector: winner, S1, S2, V
LIST_MATCH_DTYPE = np.dtype([("index", "<i4"), ("score", "<i4"), ("second", "<i4"), ("v2", "<i4")])


def set_message_list(messages, zmin16=96, library=None):
    """wspr_set_message_list() of include/wspr_mi355x.h: the texts every later decode call matches its failed candidates
    against (list decoding, K14), accepted at z >= zmin16 / 16.  None or an empty list switches the stage off (the
    default).  Returns the number of entries kept (repeats are dropped), or -1 with NOTHING CHANGED for a text that does
    not qualify, more than LIST_MAX texts, or zmin16 outside 1 .. 203.  The product and the lab library each keep their
    own list: `library` (default: lib()) is the one set."""
    L = library or lib()
    msgs = [m if isinstance(m, bytes) else str(m).encode() for m in (messages or [])]
    if not msgs:
        return L.wspr_set_message_list(None, 0, int(zmin16))
    arr = (C.c_char_p * len(msgs))(*msgs)
    return L.wspr_set_message_list(C.cast(arr, C.c_void_p), len(msgs), int(zmin16))


def message_list_entry(index, library=None):
    """wspr_message_list_entry(): (canonical text, decdata uint8 [11], channel symbols uint8 [162]) of entry `index` of the
    list in force, or None outside it."""
    text = C.create_string_buffer(23)
    dec, sym = np.zeros(11, np.uint8), np.zeros(NSYM, np.uint8)
    if (library or lib()).wspr_message_list_entry(int(index), text, _ptr(dec), _ptr(sym)) != 0:
        return None
    return text.value.decode(), dec, sym


def list_match(symbols, library=None):
    """wspr_list_match_batch_device(): n vectors of 162 soft symbols (uint8 [n, 162], transmission order) against the list
    in force.  Returns a LIST_MATCH_DTYPE array [n]; raises if the library refuses the call (no list, no device)."""
    sym = np.ascontiguousarray(symbols, dtype=np.uint8).reshape(-1, NSYM)
    out = np.zeros(sym.shape[0], LIST_MATCH_DTYPE)
    rc = (library or lib()).wspr_list_match_batch_device(_ptr(sym), sym.shape[0], _ptr(out))
    if rc != 0:
        raise RuntimeError("wspr_list_match_batch_device failed (rc %d: no list set, or no usable HIP device)" % rc)
    return out


def get_wspr_channel_symbols(message):
    """wsprsim_utils.h:9 -- returns (ok, symbols[162] uint8) with fresh hash tables."""
    hashtab = C.create_string_buffer(32768 * 13)
    loctab = C.create_string_buffer(32768 * 5)
    sym = (C.c_ubyte * NSYM)()
    ok = lib().get_wspr_channel_symbols(C.create_string_buffer(message.encode(), 32), hashtab, loctab, sym)
    return int(ok), np.frombuffer(sym, dtype=np.uint8).copy()


def synth_tx_list(items):
    """[(seg, f0, t0, amp, drift, symbols[162]), ...] sorted by seg -> ctypes array of wspr_synth_tx."""
    arr = (wspr_synth_tx * max(1, len(items)))()
    for k, (seg, f0, t0, amp, drift, sym) in enumerate(items):
        arr[k].seg, arr[k].f0, arr[k].t0, arr[k].amp, arr[k].drift = int(seg), f0, t0, amp, drift
        arr[k].symbols[:] = [int(v) for v in sym]
    return arr


def wspr_synth_batch_device(items, nseg, d_i, d_q, seg_index0=0, noise_sigma=0.0, seed=0, flags=0):
    """wspr_synth_batch_device() of include/wspr_mi355x.h: the scene `items` (a list as for synth_tx_list(), or a numpy
    array of SYNTH_TX_DTYPE) into nseg device rows of wspr_iq_stride() floats at the raw pointers d_i / d_q.
    Returns the library's code (0, or -1 with nothing written)."""
    tx, n, _keep = _synth_items(items)
    return lib().wspr_synth_batch_device(tx, n, nseg, seg_index0, noise_sigma, seed, flags, d_i, d_q)


def wspr_synth(items, noise_sigma=0.0, seed=0, flags=0, I=None, Q=None):
    """wspr_synth(): one segment into host rows of 45000 floats (given rows are copied and matter with SYNTH_ACCUMULATE).
    Returns (I, Q); raises if the library refuses the call."""
    I = np.zeros(NSAMPLES, np.float32) if I is None else np.array(I, np.float32).copy()
    Q = np.zeros(NSAMPLES, np.float32) if Q is None else np.array(Q, np.float32).copy()
    arr = synth_tx_list(items)
    if lib().wspr_synth(C.addressof(arr), len(items), noise_sigma, seed, flags, _ptr(I), _ptr(Q)) != 0:
        raise RuntimeError("wspr_synth failed (bad arguments, or no usable HIP device)")
    return I, Q


def synth_channel_list(channels):
    """[[(gain, shift, sigma), (gain, shift, sigma)], ...], one per transmission -> ctypes array of wspr_synth_channel."""
    arr = (wspr_synth_channel * max(1, len(channels)))()
    for k, ch in enumerate(channels):
        if len(ch) != 2:
            raise ValueError("a channel is two paths (gain, shift, sigma); a path with gain 0 is skipped")
        for p in range(2):
            arr[k].path[p].gain, arr[k].path[p].shift, arr[k].path[p].sigma = ch[p]
    return arr


def _synth_channels(channels, n):
    """(pointer or None, keep-alive) for the channels of n transmissions: None, a list, or a SYNTH_CHANNEL_DTYPE array."""
    if channels is None:
        return None, None
    if isinstance(channels, np.ndarray):
        assert channels.dtype == SYNTH_CHANNEL_DTYPE and channels.flags.c_contiguous and channels.size == n
        return channels.ctypes.data, channels
    if len(channels) != n:
        raise ValueError("one channel per transmission")
    arr = synth_channel_list(channels)
    return C.addressof(arr), arr


def wspr_synth_faded_batch_device(items, channels, nseg, d_i, d_q, seg_index0=0, noise_sigma=0.0, seed=0, flags=0):
    """wspr_synth_faded_batch_device(): wspr_synth_batch_device() with an HF fading channel per transmission (K13).
    channels: one [(gain, shift, sigma), (gain, shift, sigma)] per transmission (or a numpy array of SYNTH_CHANNEL_DTYPE);
    None is the unfaded call.  Returns the library's code (0, or -1 with nothing written)."""
    tx, n, _keep_tx = _synth_items(items)
    ch, _keep = _synth_channels(channels, n)
    return lib().wspr_synth_faded_batch_device(tx, ch, n, nseg, seg_index0, noise_sigma, seed, flags, d_i, d_q)


def wspr_synth_faded(items, channels, noise_sigma=0.0, seed=0, flags=0, I=None, Q=None):
    """wspr_synth_faded(): one faded segment into host rows of 45000 floats (given rows are copied and matter with
    SYNTH_ACCUMULATE).  Returns (I, Q); raises if the library refuses the call."""
    I = np.zeros(NSAMPLES, np.float32) if I is None else np.array(I, np.float32).copy()
    Q = np.zeros(NSAMPLES, np.float32) if Q is None else np.array(Q, np.float32).copy()
    arr = synth_tx_list(items)
    ch, _keep = _synth_channels(channels, len(items))
    if lib().wspr_synth_faded(C.addressof(arr), ch, len(items), noise_sigma, seed, flags, _ptr(I), _ptr(Q)) != 0:
        raise RuntimeError("wspr_synth_faded failed (bad arguments, or no usable HIP device)")
    return I, Q


AUDIO_RATE = 12000                 # include/wspr_mi355x.h: the 12 kHz audio front end (K12)
AUDIO_MAX_SAMPLES = 1440000
AUDIO_NTAPS = 511


def audio_batch_device(d_pcm, pcm_stride, nsamp, nseg, d_i, d_q, normalise=0):
    """wspr_audio_batch_device(): nseg records of nsamp int16 samples at the raw device pointer d_pcm (row stride pcm_stride
    samples) into nseg device rows of wspr_iq_stride() floats at d_i / d_q.  Returns the library's code (0; -1 with nothing
    written; -2 for nsamp > AUDIO_MAX_SAMPLES)."""
    return lib().wspr_audio_batch_device(d_pcm, int(pcm_stride), int(nsamp), int(nseg), d_i, d_q, int(normalise))


def audio_to_iq(pcm, normalise=0):
    """wspr_audio_to_iq(): one record (int16, 12 000 Hz, the band at 1 500 Hz) into host rows of 45000 floats, through the
    device.  Returns (I, Q, n_out); raises if the library refuses the call."""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    I = np.zeros(NSAMPLES, np.float32)
    Q = np.zeros(NSAMPLES, np.float32)
    n_out = C.c_uint32(0)
    rc = lib().wspr_audio_to_iq(_ptr(pcm), int(pcm.size), _ptr(I), _ptr(Q), C.addressof(n_out), int(normalise))
    if rc != 0:
        raise RuntimeError("wspr_audio_to_iq failed (rc %d: a record above 120 s, or no usable HIP device)" % rc)
    return I, Q, int(n_out.value)


def audio_blank_batch_device(d_pcm, pcm_stride, nsamp, nseg, thr16, guard, d_out, out_stride, n_blanked=None):
    """wspr_audio_blank_batch_device(): the impulse-noise blanker (K15) alone, PCM rows at the raw device pointer d_pcm into
    PCM rows at d_out.  n_blanked: an int32 numpy array of nseg that receives the blanked samples per record, or None.
    Returns the library's code (0; -1 with nothing written; -2 for nsamp > AUDIO_MAX_SAMPLES)."""
    return lib().wspr_audio_blank_batch_device(d_pcm, int(pcm_stride), int(nsamp), int(nseg), int(thr16), int(guard), d_out,
                                               int(out_stride), None if n_blanked is None else _ptr(n_blanked))


def audio_blanked_batch_device(d_pcm, pcm_stride, nsamp, nseg, thr16, guard, d_i, d_q, normalise=0, n_blanked=None):
    """wspr_audio_blanked_batch_device(): audio_batch_device() on blanked samples (K15 then K12); n_blanked as above."""
    return lib().wspr_audio_blanked_batch_device(d_pcm, int(pcm_stride), int(nsamp), int(nseg), int(thr16), int(guard), d_i,
                                                 d_q, int(normalise), None if n_blanked is None else _ptr(n_blanked))


def audio_to_iq_blanked(pcm, thr16, guard, normalise=0):
    """wspr_audio_to_iq_blanked(): audio_to_iq() on blanked samples.  Returns (I, Q, n_out, n_blanked); raises if the
    library refuses the call."""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    I = np.zeros(NSAMPLES, np.float32)
    Q = np.zeros(NSAMPLES, np.float32)
    n_out = C.c_uint32(0)
    n_blanked = C.c_int(0)
    rc = lib().wspr_audio_to_iq_blanked(_ptr(pcm), int(pcm.size), int(thr16), int(guard), _ptr(I), _ptr(Q),
                                        C.addressof(n_out), int(normalise), C.addressof(n_blanked))
    if rc != 0:
        raise RuntimeError("wspr_audio_to_iq_blanked failed (rc %d: settings out of range, a record above 120 s, or no usable "
                           "HIP device)" % rc)
    return I, Q, int(n_out.value), int(n_blanked.value)


# include/wspr_mi355x.h: wspr_noise_windows and struct wspr_noise, the band noise figures of a segment (K16)
NOISE_WINDOWS_DTYPE = np.dtype([("pre_b0", "<i4"), ("pre_b1", "<i4"), ("post_b0", "<i4"), ("post_b1", "<i4")])
NOISE_DTYPE = np.dtype([("pre_mean", "<f4"), ("pre_trough", "<f4"), ("post_mean", "<f4"), ("post_trough", "<f4"),
                        ("fft_floor", "<f4"), ("fft_p30", "<f4"), ("nframes", "<i4"), ("flags", "<i4")])
NOISE_PRE_USED, NOISE_POST_USED, NOISE_FFT_USED, NOISE_NONFINITE = 1, 2, 4, 8
NOISE_MAX_BLOCK = 2812


def _noise_windows(windows):
    """None (the library's default) or (pre_b0, pre_b1, post_b0, post_b1) as what the call takes."""
    if windows is None:
        return None, None
    w = np.array([tuple(int(x) for x in windows)], NOISE_WINDOWS_DTYPE)
    return w, _ptr(w)


def noise_default_windows():
    """wspr_noise_default_windows(): (pre_b0, pre_b1, post_b0, post_b1) in blocks of 16 samples.  Needs no device."""
    w = np.zeros(1, NOISE_WINDOWS_DTYPE)
    lib().wspr_noise_default_windows(_ptr(w))
    return tuple(int(x) for x in w[0])


def noise_batch_device(d_i, d_q, nseg, samples, seg_stride, windows=None, out=None):
    """wspr_noise_batch_device(): the band noise figures (K16) of nseg rows at the raw device pointers d_i / d_q (16-byte
    aligned, seg_stride floats apart).  The figures are UNCALIBRATED linear powers relative to the row's scale: log them
    from rows that were not normalised.  out: a NOISE_DTYPE array of nseg to write into, or None.  Returns (rc, records):
    rc is the library's code (0; -1 or -2 with nothing written)."""
    if out is None:
        out = np.zeros(max(int(nseg), 0), NOISE_DTYPE)
    keep, w = _noise_windows(windows)
    rc = lib().wspr_noise_batch_device(d_i, d_q, int(nseg), int(samples), int(seg_stride), w, _ptr(out))
    return rc, out


def noise(I, Q, windows=None, samples=None):
    """wspr_noise(): the figures of one host row as a NOISE_DTYPE record; raises if the library refuses the call."""
    I = np.ascontiguousarray(I, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    out = np.zeros(1, NOISE_DTYPE)
    keep, w = _noise_windows(windows)
    rc = lib().wspr_noise(_ptr(I), _ptr(Q), int(I.size if samples is None else samples), w, _ptr(out))
    if rc != 0:
        raise RuntimeError("wspr_noise failed (rc %d: a window out of range, more than 45000 samples, or no usable HIP "
                           "device)" % rc)
    return out[0]


def to_db(power):
    """10 log10 of a linear figure (a scalar or an array); 0 and below give -inf.  Still uncalibrated."""
    p = np.asarray(power, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(p > 0.0, 10.0 * np.log10(np.where(p > 0.0, p, 1.0)), -np.inf)


# include/wspr_mi355x.h: wspr_waterfall_params and wspr_waterfall_info, the waterfall of a segment (K20)
WATERFALL_PARAMS_DTYPE = np.dtype([("hop", "<i4"), ("tavg", "<i4"), ("j0", "<i4"), ("j1", "<i4"), ("ref_mode", "<i4"),
                                   ("ref", "<f4"), ("db_min", "<f4"), ("db_step", "<f4")])
WATERFALL_INFO_DTYPE = np.dtype([("ref", "<f4"), ("nframes", "<i4"), ("nrows", "<i4"), ("flags", "<i4")])
WF_REF_ABSOLUTE, WF_REF_FLOOR = 0, 1
WF_WRITTEN, WF_NO_REF, WF_NONFINITE = 1, 2, 8


def waterfall_default_params():
    """wspr_waterfall_default_params() as a dict: hop, tavg, j0, j1, ref_mode, ref, db_min, db_step.  Needs no device."""
    p = np.zeros(1, WATERFALL_PARAMS_DTYPE)
    lib().wspr_waterfall_default_params(_ptr(p))
    return {k: p[0][k].item() for k in WATERFALL_PARAMS_DTYPE.names}


def _waterfall_params(params):
    """None (the library's default), a dict that overrides some of the defaults, or a WATERFALL_PARAMS_DTYPE record, as what
    the call takes."""
    if params is None:
        return None, None
    if isinstance(params, dict):
        d = waterfall_default_params()
        unknown = set(params) - set(d)
        if unknown:
            raise KeyError("unknown waterfall parameter: %s" % sorted(unknown))
        d.update(params)
        p = np.zeros(1, WATERFALL_PARAMS_DTYPE)
        for k, v in d.items():
            p[0][k] = v
    else:
        p = np.array(params, WATERFALL_PARAMS_DTYPE).reshape(1)
    return p, _ptr(p)


def waterfall_shape(samples=NSAMPLES, params=None):
    """wspr_waterfall_shape(): (nrows, ncols) of the image of a row of `samples` samples; raises if the library refuses the
    parameters.  Needs no device."""
    keep, p = _waterfall_params(params)
    nrows, ncols = C.c_int(0), C.c_int(0)
    rc = lib().wspr_waterfall_shape(int(samples), p, C.addressof(nrows), C.addressof(ncols))
    if rc != 0:
        raise ValueError("wspr_waterfall_shape refused the call (rc %d)" % rc)
    return int(nrows.value), int(ncols.value)


def waterfall_batch_device(d_i, d_q, nseg, samples, seg_stride, d_img, img_stride, params=None, info=None):
    """wspr_waterfall_batch_device(): the waterfalls (K20) of nseg rows at the raw device pointers d_i / d_q (16-byte aligned,
    seg_stride floats apart) into nseg images of waterfall_shape() bytes at the raw device pointer d_img (16-byte aligned,
    img_stride bytes apart, a multiple of 16).  info: a WATERFALL_INFO_DTYPE array of nseg to write into, or None.  Returns
    (rc, info): rc is the library's code (0; -1 or -2 with nothing written)."""
    if info is None:
        info = np.zeros(max(int(nseg), 0), WATERFALL_INFO_DTYPE)
    keep, p = _waterfall_params(params)
    rc = lib().wspr_waterfall_batch_device(d_i, d_q, int(nseg), int(samples), int(seg_stride), p, d_img, int(img_stride),
                                           _ptr(info))
    return rc, info


def waterfall(I, Q, params=None, samples=None):
    """wspr_waterfall(): the waterfall of one host row as (image uint8 [nrows, ncols], WATERFALL_INFO_DTYPE record); raises if
    the library refuses the call."""
    I = np.ascontiguousarray(I, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    n = int(I.size if samples is None else samples)
    try:
        nrows, ncols = waterfall_shape(n, params)
    except ValueError as e:
        raise RuntimeError("wspr_waterfall: %s" % e) from None
    img = np.zeros((nrows, ncols), np.uint8)
    info = np.zeros(1, WATERFALL_INFO_DTYPE)
    keep, p = _waterfall_params(params)
    rc = lib().wspr_waterfall(_ptr(I), _ptr(Q), n, p, img.ctypes.data if img.size else None, _ptr(info))
    if rc != 0:
        raise RuntimeError("wspr_waterfall failed (rc %d: parameters out of range, more than 45000 samples, or no usable HIP "
                           "device)" % rc)
    return img, info[0]


def waterfall_palette(which=1):
    """wspr_waterfall_palette(): uint8 [256, 3], RGB of each level; 0 grey, 1 the colour ramp.  Needs no device."""
    rgb = np.zeros((256, 3), np.uint8)
    lib().wspr_waterfall_palette(int(which), _ptr(rgb))
    return rgb


def write_pgm_file(filename, img):
    """wspr_write_pgm_file(): a uint8 image [height, width] as a binary P5 file.  Raises if it cannot be written."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w_ = img.shape
    if lib().wspr_write_pgm_file(os.fsencode(filename), _ptr(img), int(w_), int(h)) != 0:
        raise OSError("wspr_write_pgm_file could not write %r" % (filename,))


def write_png_file(filename, img, palette=None):
    """wspr_write_png_file(): a uint8 image [height, width] as an uncompressed 8-bit PNG, grey or (palette: uint8 [256, 3])
    indexed.  Raises if it cannot be written."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w_ = img.shape
    pal = None if palette is None else np.ascontiguousarray(palette, dtype=np.uint8).reshape(768)
    if lib().wspr_write_png_file(os.fsencode(filename), _ptr(img), int(w_), int(h), None if pal is None else _ptr(pal)) != 0:
        raise OSError("wspr_write_png_file could not write %r" % (filename,))


def read_wav_file(filename, cap=AUDIO_MAX_SAMPLES):
    """wspr_read_wav_file(): the samples (int16) of a 12 000 Hz 16-bit mono PCM WAV file, at most `cap`; an empty array on
    any error or any other format.  Host code: needs no device."""
    pcm = np.zeros(max(1, int(cap)), np.int16)
    n = lib().wspr_read_wav_file(os.fsencode(filename), _ptr(pcm), int(cap))
    return pcm[:n].copy()


def write_wav_file(filename, pcm):
    """wspr_write_wav_file(): int16 samples as a 12 000 Hz 16-bit mono PCM WAV file, what read_wav_file() reads.  Raises if
    the file cannot be written.  Host code: needs no device."""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    if lib().wspr_write_wav_file(os.fsencode(filename), _ptr(pcm), int(pcm.size)) != 0:
        raise OSError("wspr_write_wav_file could not write %r" % (filename,))


def audio_amp(snr_db, noise_sigma):
    """The level convention of the audio scene synthesiser (K17): the amplitude, in PCM units, of a signal at snr_db (the
    decoder's convention: noise power in 2 500 Hz) over real noise of standard deviation noise_sigma at 12 000 samples per
    second, which has noise_sigma^2 * 2500/6000 of its power in those 2 500 Hz."""
    return float(noise_sigma) * math.sqrt(5000.0 / 6000.0) * 10.0 ** (float(snr_db) / 20.0)


def _synth_items(items):
    """(pointer, count, keep-alive) of a transmission list: a list as for synth_tx_list(), or a SYNTH_TX_DTYPE array."""
    if isinstance(items, np.ndarray):
        assert items.dtype == SYNTH_TX_DTYPE and items.flags.c_contiguous
        return items.ctypes.data, int(items.size), items
    arr = synth_tx_list(items)
    return C.addressof(arr), len(items), arr


def synth_audio_batch_device(items, nseg, nsamp, d_pcm, pcm_stride, seg_index0=0, noise_sigma=0.0, seed=0, flags=0,
                             n_clipped=None):
    """wspr_synth_audio_batch_device(): the scene `items` (a list as for synth_tx_list(), or a numpy array of
    SYNTH_TX_DTYPE; amp and noise_sigma in PCM units) into nseg records of nsamp int16 samples at the raw device pointer
    d_pcm (row stride pcm_stride samples), the rows audio_batch_device() takes.  n_clipped: an int32 numpy array of nseg that
    receives the clipped samples per record, or None.  Returns the library's code (0; -1 with nothing written; -2 for
    nsamp > AUDIO_MAX_SAMPLES)."""
    tx, n, _keep = _synth_items(items)
    return lib().wspr_synth_audio_batch_device(tx, n, int(nseg), int(seg_index0), int(nsamp), noise_sigma, seed, int(flags),
                                               d_pcm, int(pcm_stride), None if n_clipped is None else _ptr(n_clipped))


def synth_audio(items, nsamp=AUDIO_MAX_SAMPLES, noise_sigma=0.0, seed=0, flags=0, pcm=None):
    """wspr_synth_audio(): one record of nsamp int16 samples in host memory (a given record is copied and matters with
    SYNTH_ACCUMULATE).  Returns (pcm, n_clipped); raises if the library refuses the call."""
    pcm = np.zeros(int(nsamp), np.int16) if pcm is None else np.array(pcm, np.int16).copy()
    assert pcm.size == int(nsamp)
    tx, n, _keep = _synth_items(items)
    clipped = C.c_int(0)
    rc = lib().wspr_synth_audio(tx, n, int(nsamp), noise_sigma, seed, int(flags), _ptr(pcm), C.addressof(clipped))
    if rc != 0:
        raise RuntimeError("wspr_synth_audio failed (rc %d: bad arguments, a record above 120 s, or no usable HIP device)" % rc)
    return pcm, int(clipped.value)


IQ_AUDIO_INTERP = 32               # include/wspr_mi355x.h: IQ to audio (K18), output samples per input sample
IQ_AUDIO_GAIN = 32768.0            # the inverse of the audio front end's 2^-15: for rows normalised to a peak of 0.5


def iq_to_audio_batch_device(d_i, d_q, nseg, samples, seg_stride, d_pcm, pcm_stride, gain=IQ_AUDIO_GAIN, n_clipped=None):
    """wspr_iq_to_audio_batch_device(): nseg rows of `samples` floats at the raw device pointers d_i / d_q (16-byte aligned,
    seg_stride floats apart) into nseg records of 32 * samples int16 samples at the raw device pointer d_pcm (row stride
    pcm_stride samples), the rows audio_batch_device() takes.  n_clipped: an int32 numpy array of nseg that receives the
    clipped samples per record, or None.  Returns the library's code (0; -1 with nothing written; -2 for samples > 45000)."""
    return lib().wspr_iq_to_audio_batch_device(d_i, d_q, int(nseg), int(samples), int(seg_stride), gain, d_pcm,
                                               int(pcm_stride), None if n_clipped is None else _ptr(n_clipped))


def iq_to_audio(I, Q, gain=IQ_AUDIO_GAIN, samples=None):
    """wspr_iq_to_audio(): one host row (float32, 375 Hz) into a record of 32 * samples int16 samples at 12 000 Hz with the
    band at 1 500 Hz, through the device.  Returns (pcm, n_clipped); raises if the library refuses the call."""
    I = np.ascontiguousarray(I, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    n = int(min(I.size, Q.size) if samples is None else samples)
    assert 0 <= n <= min(I.size, Q.size)
    pcm = np.zeros(IQ_AUDIO_INTERP * n, np.int16)
    clipped = C.c_int(0)
    rc = lib().wspr_iq_to_audio(_ptr(I), _ptr(Q), n, gain, _ptr(pcm), C.addressof(clipped))
    if rc != 0:
        raise RuntimeError("wspr_iq_to_audio failed (rc %d: a non-finite gain, more than 45000 samples, or no usable HIP "
                           "device)" % rc)
    return pcm, int(clipped.value)


TUNE_MAX_BANDS = 16                # include/wspr_mi355x.h: the tunable multi-band front end (K21)
TUNE_SAMPLES_PER_OUTPUT = 6400     # 2.4 Msps in, 375.000 Hz out


def tune_step(offset_hz):
    """wspr_tune_step(): (the 32-bit oscillator step that brings a signal at +offset_hz of a 2.4 Msps capture to 0 Hz, the
    offset in Hz that step stands for).  Host code: needs no device."""
    realised = C.c_double(0.0)
    step = lib().wspr_tune_step(float(offset_hz), C.addressof(realised))
    return int(step), float(realised.value)


def tune_u8_batch_device(d_raw, bytes_per_seg, nseg, steps, d_i, d_q, normalise=1):
    """wspr_tune_u8_batch_device(): nseg rows of bytes_per_seg raw bytes at the raw device pointer d_raw (16-byte aligned,
    bytes_per_seg a multiple of 16) and the steps of len(steps) bands (1 .. 16, of tune_step()) into nseg * len(steps) device
    rows of wspr_iq_stride() floats at d_i / d_q: row s * nbands + b = segment s tuned by steps[b].  Returns the library's code
    (0; -1 with nothing written)."""
    st = None if steps is None else np.ascontiguousarray(steps, dtype=np.uint32)
    return lib().wspr_tune_u8_batch_device(d_raw, int(bytes_per_seg), int(nseg), None if st is None else _ptr(st),
                                           0 if st is None else int(st.size), d_i, d_q, int(normalise))


def tune_u8(iq, steps, normalise=1):
    """wspr_tune_u8(): one capture of unsigned-8-bit IQ bytes in host memory into len(steps) rows of 45000 floats, through the
    device.  Returns (I, Q float32 [nbands, 45000], n_out); raises if the library refuses the call."""
    iq = np.ascontiguousarray(iq, dtype=np.uint8)
    st = np.ascontiguousarray(steps, dtype=np.uint32)
    I = np.zeros((st.size, NSAMPLES), np.float32)
    Q = np.zeros((st.size, NSAMPLES), np.float32)
    n = C.c_uint32(0)
    rc = lib().wspr_tune_u8(_ptr(iq), int(iq.size), _ptr(st), int(st.size), _ptr(I), _ptr(Q), C.addressof(n), int(normalise))
    if rc != 0:
        raise RuntimeError("wspr_tune_u8 failed (rc %d: no steps, more than 16 bands, or no usable HIP device)" % rc)
    return I, Q, int(n.value)


def tune_constants():
    """wspr_tune_constants(): (C[256], F[256] as complex-valued int arrays [256, 2] of (re, im), input samples per output)."""
    c = np.zeros(512, np.int16)
    f = np.zeros(512, np.int16)
    r = C.c_int(0)
    lib().wspr_tune_constants(_ptr(c), _ptr(f), C.addressof(r))
    return c.reshape(256, 2), f.reshape(256, 2), int(r.value)


def write_c2_file(filename, I, Q, dial_hz):
    """wspr_write_c2_file(): 45000 samples of I and Q (shorter rows are padded with zeros) and the dial frequency in Hz as a
    .c2 file, what wspr_read_c2_file() reads.  Raises if the file cannot be written.  Host code: needs no device."""
    rows = []
    for x in (I, Q):
        x = np.ascontiguousarray(x, dtype=np.float32).ravel()
        if x.size > NSAMPLES:
            raise ValueError("a .c2 file holds 45000 samples")
        rows.append(np.concatenate((x, np.zeros(NSAMPLES - x.size, np.float32))))
    if lib().wspr_write_c2_file(os.fsencode(filename), _ptr(rows[0]), _ptr(rows[1]), float(dial_hz)) != NSAMPLES:
        raise OSError("wspr_write_c2_file could not write %r" % (filename,))


def audio_constants():
    """wspr_audio_constants(): (taps_i[511], taps_q[511], input samples per output)."""
    gi = np.zeros(AUDIO_NTAPS, np.float32)
    gq = np.zeros(AUDIO_NTAPS, np.float32)
    r = C.c_int(0)
    lib().wspr_audio_constants(_ptr(gi), _ptr(gq), C.addressof(r))
    return gi, gq, int(r.value)


def wspr_selftest(options=None):
    """The reference's `-t` (decoderSelfTest()) generated and decoded on the device: (1 / 0, first spot)."""
    first = decoder_results()
    rc = lib().wspr_selftest(options or default_options(), C.addressof(first))
    if rc < 0:
        raise RuntimeError("wspr_selftest failed (no usable HIP device?)")
    return rc, first


def wspr_decode(idat, qdat, samples=None, options=None):
    """The reference entry point (wsprd/wsprd.h:106-111) on one segment.
    Returns (spots, residual_i, residual_q); inputs are left untouched."""
    I = np.ascontiguousarray(idat, dtype=np.float32).copy()
    Q = np.ascontiguousarray(qdat, dtype=np.float32).copy()
    n = int(samples if samples is not None else I.size)
    out = (decoder_results * 100)()
    nres = C.c_int(0)
    rc = lib().wspr_decode(_ptr(I), _ptr(Q), n, options or default_options(), C.addressof(out), C.addressof(nres))
    if rc < 0:
        raise RuntimeError("wspr_decode failed (no usable HIP device?)")
    return [out[i] for i in range(nres.value)], I, Q


def wspr_decode_batch(I, Q, options=None, max_results=50):
    """Host arrays [nseg, samples] -> list of spot lists."""
    I = np.ascontiguousarray(I, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    nseg, samples = I.shape
    out = (decoder_results * (nseg * max_results))()
    nres = (C.c_int * nseg)()
    rc = lib().wspr_decode_batch(_ptr(I), _ptr(Q), nseg, samples, samples, options or default_options(),
                                 C.addressof(out), max_results, C.addressof(nres), 0)
    if rc < 0:
        raise RuntimeError("wspr_decode_batch failed (rc %d: no usable HIP device, or usehashtable on a batch)" % rc)
    return [[out[s * max_results + i] for i in range(nres[s])] for s in range(nseg)]


def wspr_decode_batch_trace(I, Q, options=None, max_results=50):
    """wspr_decode_batch() + the per-candidate trace of the fine search (what the production kernels produced for
    every candidate the reference's loop enters), through the LAB library (include/wspr_mi355x_bench.h).
    Returns (spot lists, trace array [nseg])."""
    I = np.ascontiguousarray(I, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    nseg, samples = I.shape
    out = (decoder_results * (nseg * max_results))()
    nres = (C.c_int * nseg)()
    tr = (trace * nseg)()
    L = lab()
    rc = L.wspr_decode_batch_trace(_ptr(I), _ptr(Q), nseg, samples, samples, options or default_options(),
                                   C.addressof(out), max_results, C.addressof(nres), C.addressof(tr))
    if rc < 0:
        raise RuntimeError("wspr_decode_batch_trace failed (rc %d)" % rc)
    return [[out[s * max_results + i] for i in range(nres[s])] for s in range(nseg)], tr


def sync_torch():
    """The library runs on streams of its own (include/wspr_mi355x.h, stream contract): whatever torch still has
    in flight for a tensor -- the index or fill kernel that built it a moment ago -- must have landed before a
    device pointer to it is handed over.  Call this between the torch code and a raw-pointer entry point."""
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.current_stream().synchronize()


class BatchDecoder:
    """Decodes segments already resident in HBM (torch tensors or raw device pointers)."""

    def __init__(self, nseg, max_results=16, options=None):
        self.nseg, self.max_results = nseg, max_results
        self.options = options or default_options()
        self.out = (decoder_results * (nseg * max_results))()
        self.nres = (C.c_int * nseg)()

    def decode_ptr(self, d_i, d_q, samples, stride):
        rc = lib().wspr_decode_batch_device(d_i, d_q, self.nseg, samples, stride, self.options,
                                            C.addressof(self.out), self.max_results, C.addressof(self.nres))
        if rc < 0:
            raise RuntimeError("wspr_decode_batch_device failed")
        return self.nres

    def decode(self, ti, tq):
        """ti, tq: contiguous float32 CUDA tensors [nseg, samples]."""
        assert ti.is_cuda and tq.is_cuda and ti.is_contiguous() and tq.is_contiguous()
        sync_torch()
        return self.decode_ptr(ti.data_ptr(), tq.data_ptr(), ti.shape[1], ti.stride(0))

    def spots(self, s):
        return [self.out[s * self.max_results + i] for i in range(self.nres[s])]

    def total_spots(self):
        return int(sum(self.nres))


# wspr_last_timings(): one name per value, in the order include/wspr_mi355x.h documents (csrc/host/wspr_pipeline.h: TimingSlot)
TIMING_NAMES = (
    "fft_sync_ms", "host_bookkeeping_ms", "device_fano_tail_ms", "demod_ms", "subtract_ms", "host_fano_ms",
    "total_ms", "fano_calls", "fano_timeouts", "fano_cycles", "candidates_refined", "gpu_waves",
    "fano_left_to_device", "segments_redecoded", "candidates_consumed", "subtractions",
    "cpu_ms_call", "cpu_ms_pass_start", "cpu_ms_build_wave", "cpu_ms_refine", "cpu_ms_ladder", "cpu_ms_books",
    "cpu_ms_subtract", "cpu_ms_finish", "message_cache_lookups", "message_cache_hits",
    "osd_ms", "osd_vectors", "osd_spots", "lag_pruned", "lag_exact_evals", "lag_fallbacks",
    "block_ms", "block_vectors", "block2_decodes", "block3_decodes",
    "spread_ms", "spread_jobs",
    "list_ms", "list_vectors", "list_spots",
    "lag_drift_pruned", "lag_drift_exact_evals", "lag_drift_fallbacks",
    "spot_detail_ms", "spot_detail_jobs")


def last_timings():
    ms = (C.c_double * len(TIMING_NAMES))()
    n = lib().wspr_last_timings(C.addressof(ms), len(TIMING_NAMES))
    return {TIMING_NAMES[i]: ms[i] for i in range(n)}
