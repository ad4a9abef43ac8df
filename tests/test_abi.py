"""The C-ABI library loads without a GPU and exports every symbol include/wspr_mi355x.h
declares; struct layouts match the reference's; no product file touches oracle/."""
import ctypes as C
import os
import re
import subprocess

import pytest

import rtlsdr_wsprd_amd as w

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(header="wspr_mi355x.h"):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    funcs = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", src))
    funcs.discard("defined")
    data = set(re.findall(r"extern\s+[^;(]*?\b([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[[^\]]*\])+\s*;", src))
    return funcs, data


def test_library_exports_every_declared_symbol():
    L = w.lib()
    funcs, data = declared_symbols()
    assert {"wspr_decode", "wspr_decode_batch", "wspr_decode_batch_device", "get_wspr_channel_symbols",
            "sync_and_demodulate", "subtract_signal2", "fano", "unpk_", "nhash", "wspr_decimate_u8", "wspr_decimate_u8_stream",
            "wspr_decim_stream_reset", "wspr_decimate_u8_batch_device_stateful", "wspr_set_fano_fast_budget"} <= funcs
    missing = [f for f in sorted(funcs | data) if not hasattr(L, f)]
    assert not missing, missing


def test_library_exports_nothing_but_the_declared_symbols():
    """The dynamic symbol table is the header: no helper, C++ or HIP-runtime symbol leaks out."""
    funcs, data = declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", w.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert exported == funcs | data, (sorted(exported - funcs - data), sorted((funcs | data) - exported))


def test_lab_library_is_the_product_plus_the_bench_header():
    """libwspr_mi355x_lab.so (the same sources with -DWSPR_LAB: what the parity suite uses for stage hooks, trace, kernel
    timings and calibration) exports the drop-in header AND include/wspr_mi355x_bench.h, nothing else; none of the bench
    header's functions is in the product."""
    funcs, data = declared_symbols()
    bfuncs, bdata = declared_symbols("wspr_mi355x_bench.h")
    assert {"wspr_decode_batch_trace", "wspr_stage_fft_bank", "wspr_stage_candidates", "wspr_stage_candidates_ps", "wspr_bench_fft_sync",
            "wspr_bench_valu",
            "wspr_bench_decimate", "wspr_calib_read", "wspr_calib_copy", "wspr_calib_copy16", "wspr_calib_valu",
            "wspr_set_front_end_cus", "wspr_fano_host_handovers"} == bfuncs and not bdata
    out = subprocess.run(["nm", "-D", "--defined-only", w.LAB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert exported == funcs | data | bfuncs
    prod = subprocess.run(["nm", "-D", "--defined-only", w.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not ({ln.split()[-1] for ln in prod.splitlines() if ln.strip()} & bfuncs)


def test_product_reads_five_environment_variables_and_no_kernel_switch():
    """The laboratory is out of the product (verdict of round 4): the product library carries the names of its five
    documented runtime knobs and of no kernel-selection / repeat / virtual-device switch; the lab library carries those."""
    prod = open(w.LIB_PATH, "rb").read()
    lab = open(w.LAB_PATH, "rb").read()
    knobs = [b"WSPR_HOST_THREADS", b"WSPR_SLOTS", b"WSPR_BLOCKING_SYNC", b"WSPR_FANO_DEVICE", b"WSPR_FANO_FAST"]
    switches = [b"WSPR_K0_KERNEL", b"WSPR_K0_RESIDENT", b"WSPR_K0_CUS", b"WSPR_K1_FUSED", b"WSPR_K3_KERNEL", b"WSPR_K4_LAG",
                b"WSPR_K4_FREQ", b"WSPR_K4_DRIFT", b"WSPR_REPEAT_LAG", b"WSPR_REPEAT_FREQ", b"WSPR_REPEAT_FANO",
                b"WSPR_FANO_WAVE_CAP", b"WSPR_NODE_VIRTUAL", b"WSPR_NODE_FAIL_PEER", b"WSPR_NODE_FAIL_SHARD"]
    assert all(k in prod for k in knobs)
    assert not [k for k in switches if k in prod]
    assert all(k in lab for k in switches)
    names = set(re.findall(rb"WSPR_[A-Z0-9_]+", prod))
    # (besides the knobs: a flag name in an error text, and the build macro the libm warning tells the user about)
    assert names <= set(knobs) | {b"WSPR_HASH_REVISIT", b"WSPR_SINCOS_FMA"}, names


def test_set_device_rejects_devices_that_do_not_exist():
    L = w.lib()
    L.wspr_device_count.restype = C.c_int
    n = L.wspr_device_count()
    assert n >= 0
    assert L.wspr_set_device(n + 7) == -1 and L.wspr_set_device(-1) == -1
    if n:
        assert L.wspr_set_device(0) == 0


def test_timing_names_cover_exactly_what_the_library_reports():
    """wspr_last_timings() writes min(capacity, its own count) values; the wrapper's TIMING_NAMES must name every one of
    them, in the order the public header documents ([0] .. [25]).  Needs no device: without a context the values are 0."""
    L = w.lib()
    ms = (C.c_double * 64)(*([-1.0] * 64))
    n = L.wspr_last_timings(C.addressof(ms), 64)
    assert n == len(w.TIMING_NAMES) == len(set(w.TIMING_NAMES))
    assert all(v >= 0.0 for v in ms[:n]) and all(v == -1.0 for v in ms[n:])      # nothing written past the count
    assert L.wspr_last_timings(C.addressof(ms), 3) == 3
    hdr = open(os.path.join(ROOT, "include", "wspr_mi355x.h")).read()
    doc = hdr[hdr.index("Timing of the stages of the most recent batch call"):hdr.index("int wspr_last_timings(")]
    assert sorted(set(int(i) for i in re.findall(r"\[(\d+)\]", doc))) == list(range(n))
    assert list(w.last_timings()) == list(w.TIMING_NAMES)


def test_struct_layouts_match_reference():
    assert C.sizeof(w.decoder_options) == 40 and C.alignment(w.decoder_options) == 4
    assert [getattr(w.decoder_options, f).offset for f in
            ("freq", "rcall", "rloc", "quickmode", "usehashtable", "npasses", "subtraction")] == [0, 4, 17, 24, 28, 32, 36]
    assert C.sizeof(w.decoder_results) == 80 and C.alignment(w.decoder_results) == 8
    assert [getattr(w.decoder_results, f).offset for f in
            ("freq", "sync", "snr", "dt", "drift", "jitter", "message", "call", "loc", "pwr", "cycles")] == \
           [0, 8, 12, 16, 20, 24, 28, 51, 64, 71, 76]
    assert C.sizeof(w.cand) == 20


def test_c_header_compiles_and_agrees_on_sizes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "wspr_mi355x.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(struct decoder_options),'
                   'sizeof(struct decoder_results), sizeof(struct cand),'
                   'offsetof(struct decoder_results, message), offsetof(struct decoder_results, cycles));return 0;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=gnu17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == ["40", "80", "20", "28", "76"]


def test_trace_mirrors_agree_with_the_c_structs(tmp_path):
    """The per-candidate traces of the product (wspr_trace) and of the oracle (orc_trace, orc_stops) as the ctypes mirrors
    see them.  The early-exit mark sits in what was padding of wspr_cand_trace: neither trace changed its size, so a
    caller built against the earlier layout still hands over buffers that are large enough."""
    import oracle_lib as ol
    src = tmp_path / "t.c"
    src.write_text('#include "wspr_mi355x_bench.h"\n#include "wspr_oracle.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(wspr_cand_trace),'
                   'offsetof(wspr_cand_trace, stop), offsetof(wspr_cand_trace, pad), sizeof(wspr_trace), sizeof(orc_trace),'
                   'sizeof(orc_stops), offsetof(orc_stops, cand));return 0;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=gnu17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"), str(src),
                    "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(w.cand_trace), w.cand_trace.stop.offset, w.cand_trace.pad.offset, C.sizeof(w.trace),
                   C.sizeof(ol.Trace), C.sizeof(ol.Stops), ol.Stops.cand.offset]
    assert w.cand_trace.stop.offset == w.cand_trace.decdata.offset + 11 and C.sizeof(w.cand_trace) == 236
    assert C.sizeof(w.trace) == 4 + 2 * 4 * 3 + 3 * 200 * 236 and C.sizeof(ol.Trace) == 171184


def test_device_entry_points_fail_loudly_without_gpu():
    """No CPU fallback: on a box without a HIP device the decode returns an error, not spots."""
    import numpy as np
    L = w.lib()
    if L.wspr_device_ready() == 1:
        pytest.skip("a GPU is present")
    z = np.zeros(45000, np.float32)
    with pytest.raises(RuntimeError):
        w.wspr_decode(z, z)


def test_product_never_references_the_oracle():
    pkg = os.path.join(ROOT, "rtlsdr-wsprd_amd")
    bad = []
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".hip", ".cpp", ".h", ".py", ".sh")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                if f.endswith((".hip", ".cpp", ".h")):      # code only: comments may cite the checker
                    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
                    txt = re.sub(r"//[^\n]*", "", txt)
                if re.search(r"liboracle|orc_|oracle/|oracle_lib", txt):
                    bad.append(os.path.join(dp, f))
    assert not bad, bad
    out = subprocess.run(["ldd", w.LIB_PATH], capture_output=True, text=True).stdout
    assert "oracle" not in out


def test_reference_unit_tests_pass_against_the_product_library():
    """the reference's own harness tests/test_wsprd.c, compiled where it lies and linked
    against libwspr_mi355x.so instead of the reference objects (oracle/Makefile, target dropin), must
    pass unchanged: 18 tests over character codes, call/grid packing, unpack50, interleaver, Fano
    round trip, nhash, comparators, channel symbols and unpk_."""
    import subprocess
    exe = os.path.join(ROOT, "oracle", "_ref", "test_wsprd_dropin")
    if not os.path.exists(exe):
        pytest.skip("drop-in harness not built (build() found no reference sources)")
    # the product library of THIS tree, wherever the harness was linked
    env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(
        p for p in (os.path.dirname(w.LIB_PATH), os.environ.get("LD_LIBRARY_PATH")) if p))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "18/18 passed, 0 failed" in r.stdout


def test_metric_tables_data_symbol():
    """metric_tables[5][256] (reference wsprd/metric_tables.h:8, a data symbol of the reference's wsprd.o) is exported
    with the reference's values in all five rows -- the committed fixture, read out of that header -- and row 2 yields
    the integer table wspr_decode derives (wsprd.c:467-473)."""
    import numpy as np
    L = w.lib()
    got = np.ctypeslib.as_array((C.c_float * 1280).in_dll(L, "metric_tables")).reshape(5, 256).copy()
    want = np.load(os.path.join(ROOT, "tests", "golden", "metric_tables_f32.npy"))
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    met = ((C.c_int * 256) * 2)()
    L.wspr_fano_metric_table(met)
    bias = np.float32(0.45)
    f = (10.0 * (got[2] - bias).astype(np.float32).astype(np.float64)).astype(np.float32)   # the double product, as a float
    r2 = (np.sign(f) * np.floor(np.abs(f).astype(np.float64) + 0.5)).astype(int)            # roundf: halves away from zero
    assert list(met[0]) == r2.tolist() and list(met[1]) == r2[::-1].tolist()


def test_shard_range_rule_is_the_drivers():
    """wspr_shard_range() (the node-level call's split) == rtlsdr-wsprd_amd/dist.py shard_range() (the ranks' split)."""
    from rtlsdr_wsprd_amd import dist as wd
    L = w.lib()
    for nseg in (0, 1, 7, 8, 65536, 1000):
        for n in (1, 2, 3, 8):
            for k in range(n):
                lo, hi = C.c_int(), C.c_int()
                L.wspr_shard_range(nseg, k, n, C.byref(lo), C.byref(hi))
                assert (lo.value, hi.value) == wd.shard_range(nseg, k, n)
