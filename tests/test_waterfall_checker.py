"""The waterfall (K20) on the CPU: the serial checker (tests/helpers/waterfall_check.c over
rtlsdr-wsprd_amd/csrc/kernels/waterfall.h and noise.h) against the shape formula, a crafted tone, a numpy float64
restatement, the noise figures' checker, crafted non-finite samples and crafted threshold edges; the library's file writers,
palette and refusals, which need no device; and the checker under AddressSanitizer as a stand-alone program.  No GPU."""
import ctypes as C
import struct
import subprocess
import zlib

import numpy as np
import pytest

import noise_lib as nl
import waterfall_lib as wl

import rtlsdr_wsprd_amd as w

NS = wl.NS


def test_bindings_agree_with_the_checker():
    assert w.WATERFALL_INFO_DTYPE == wl.INFO_DTYPE and w.WATERFALL_PARAMS_DTYPE == wl.PARAMS_DTYPE
    d = w.waterfall_default_params()
    assert {k: (float(v) if isinstance(v, float) else int(v)) for k, v in d.items()} == wl.DEFAULTS
    assert (w.WF_REF_ABSOLUTE, w.WF_REF_FLOOR, w.WF_WRITTEN, w.WF_NO_REF, w.WF_NONFINITE) == \
           (wl.REF_ABSOLUTE, wl.REF_FLOOR, wl.WRITTEN, wl.NO_REF, wl.NONFINITE)
    hdr = open(wl.ol.ROOT + "/include/wspr_mi355x.h").read()
    for name, value in (("WSPR_WF_REF_ABSOLUTE", 0), ("WSPR_WF_REF_FLOOR", 1), ("WSPR_WF_WRITTEN", 1), ("WSPR_WF_NO_REF", 2),
                        ("WSPR_WF_NONFINITE", 8)):
        assert ("#define %s" % name) in hdr and int(hdr.split("#define %s" % name)[1].split()[0]) == value


@pytest.mark.parametrize("hop", wl.HOPS)
@pytest.mark.parametrize("tavg", wl.TAVGS)
def test_shape_rule(hop, tavg):
    for cols in ((-150, 150), (-256, 255), (7, 7)):
        p = wl.params(hop=hop, tavg=tavg, j0=cols[0], j1=cols[1])
        for n in wl.lengths(hop, tavg):
            want = wl.shape_formula(n, p)
            assert wl.check_shape(n, p) == (0,) + want
            assert w.waterfall_shape(n, p[0]) == want, (n, hop, tavg)
            assert want[0] == ((n - 512) // hop + 1 if n >= 512 else 0) // tavg and want[1] == cols[1] - cols[0] + 1
    assert w.waterfall_shape(NS, dict(hop=hop, tavg=1))[0] == {128: 348, 256: 174}[hop]
    assert w.waterfall_shape(512 + hop * tavg - 1, dict(hop=hop, tavg=tavg))[0] == 1          # the incomplete group is dropped
    assert w.waterfall_shape(512 + hop * tavg, dict(hop=hop, tavg=tavg))[0] == (2 if tavg == 1 else 1)


def test_default_shape_and_span():
    assert w.waterfall_shape() == (348, 301) and wl.check_shape(NS, None) == (0, 348, 301)
    T = wl.levels(-10.0, 0.25)
    assert T[0] == 0.0 and np.all(np.diff(T[1:]) > 0) and T[40] == 1.0 and T[80] == 10.0 and T[120] == 100.0
    assert abs(10 * np.log10(T[1]) + 9.75) < 1e-12 and abs(10 * np.log10(T[255]) - 53.75) < 1e-12
    assert np.allclose(T[1:], wl.levels_numpy(-10.0, 0.25), rtol=1e-15, atol=0)
    for step in (0.05, 4.0):                                                 # the extremes stay strictly increasing and finite
        for lo in (-60.0, 60.0):
            T = wl.levels(lo, step)
            assert np.all(np.isfinite(T)) and np.all(np.diff(T[1:]) > 0)


@pytest.mark.parametrize("hop", wl.HOPS)
def test_orientation_of_a_tone_burst(hop):
    """+40 Hz (bin 54.6) present only in samples 10 000 .. 19 999 over noise of sigma 0.02, levels over 2 sigma^2.  The tone
    reads +45.8 dB in a frame it fills (0.09 * 256^2 / 192 over 8e-4); `bright` is within 6 dB of the brightest pixel: Hann
    puts the bins 53 and 56 (1.6 and 1.4 bins off) 16 and 11 dB below the peak.  `Noise` is below +13 dB: a pixel of tavg 1 is
    exponential, P(> 20 x mean) = 2e-9."""
    rng = np.random.default_rng(40)
    t = np.arange(NS) / 375.0
    z = wl.SIGMA * (rng.normal(0, 1, NS) + 1j * rng.normal(0, 1, NS))
    z[10000:20000] += 0.3 * np.exp(2j * np.pi * 40.0 * t[10000:20000])
    I, Q = z.real.astype(np.float32), z.imag.astype(np.float32)
    p = wl.params(hop=hop, ref_mode=wl.REF_ABSOLUTE, ref=2 * wl.SIGMA ** 2)
    img, info = wl.check_rows(I, Q, NS, p)
    img = img[0].astype(int)
    nrows, ncols = img.shape
    assert info[0]["flags"] == wl.WRITTEN and (nrows, ncols) == wl.shape_formula(NS, p)
    col = lambda j: j + 150
    peak = img.max()
    assert abs(peak - (45.8 + 10) / 0.25) < 12                              # within 3 dB of the closed form
    bright_rows, bright_cols = np.nonzero(img >= peak - 24)
    assert set(bright_cols.tolist()) <= {col(54), col(55)}
    touching = wl.rows_touching(10000, 19999, hop, 1, nrows)
    inside = [r for r in range(nrows) if hop * r >= 10000 and hop * r + 511 <= 19999]
    assert set(bright_rows.tolist()) <= set(touching) and set(inside) <= set(bright_rows.tolist()) and len(inside) > 15
    assert all(int(np.argmax(img[r])) in (col(54), col(55)) for r in inside)
    noise_ceiling = int((13 + 10) / 0.25)
    outside = np.setdiff1d(np.arange(nrows), touching)
    assert img[outside].max() < noise_ceiling                                # nowhere else above the noise
    assert img[:, [col(-55), col(-54)]].max() < noise_ceiling                # the mirror stays dark: +f is to the right
    assert touching[0] > 0 and img[touching[0] - 1].max() < noise_ceiling    # row 0 is the earliest
    assert hop * touching[0] + 511 >= 10000 > hop * (touching[0] - 1) + 511


def test_against_float64():
    """Eight scenes, both hops, default columns and levels, floor mode: every pixel within one level of the float64 statement
    and at most 1 pixel in 10 000 differs (a condition, not a measurement: a numpy float32 against float64 rehearsal gave 6 of
    628 488, none off by more than one).  The reference is the checker's own info.ref, a float32 both statements take."""
    I, Q = wl.scene_rows()
    total = differ = 0
    for hop in wl.HOPS:
        p = wl.params(hop=hop)
        img, info = wl.check_rows(I, Q, NS, p)
        assert np.all(info["flags"] == wl.WRITTEN) and np.all(info["ref"] > 0)
        for s in range(I.shape[0]):
            want = wl.image_float64(I[s], Q[s], NS, p, info[s]["ref"])
            d = np.abs(img[s].astype(int) - want.astype(int))
            assert d.max() <= 1, (hop, s, int(d.max()))
            total += d.size
            differ += int(np.count_nonzero(d))
            assert 30 < np.median(img[s]) < 60 and img[s].max() > 200        # the floor near 0 dB (level 40), the strong tone far up
    print("checker against float64: %d of %d pixels differ, none by more than one level" % (differ, total))
    assert total == 8 * (348 + 174) * 301 and differ * 10000 <= total, (differ, total)


def test_floor_mode_takes_the_noise_figures_p30():
    I, Q = wl.scene_rows()
    for n in (NS, 44999, 1000, 512):
        img, info = wl.check_rows(I[:3], Q[:3], n)
        k16 = nl.check_rows(I[:3, :n], Q[:3, :n], n)
        assert info["ref"].tobytes() == k16["fft_p30"].tobytes() and np.all(info["flags"] == wl.WRITTEN)
        other_hop = wl.check_rows(I[:3], Q[:3], n, wl.params(hop=256, tavg=2))[1]
        assert other_hop["ref"].tobytes() == info["ref"].tobytes()           # K16's own hop whatever hop is here
    # rows without a usable floor: all zeros (fft_p30 == 0), one NaN (K16's guard), fewer than 512 samples (no spectrum)
    zero = np.zeros(NS, np.float32)
    img, info = wl.check_rows(zero, zero, NS)
    assert info[0].tobytes() == np.array([(0.0, 348, 348, wl.WRITTEN | wl.NO_REF)], wl.INFO_DTYPE).tobytes() and not img.any()
    for k in (44990, 3):                                                     # (44990: behind every complete frame, K16 still guards)
        J = I[0].copy()
        J[k] = np.nan
        img, info = wl.check_rows(J, Q[0], NS)
        assert info[0]["flags"] == wl.WRITTEN | wl.NO_REF | wl.NONFINITE and info[0]["ref"] == 0 and not img.any()
    img, info = wl.check_rows(I[0], Q[0], 511)
    assert info[0].tobytes() == np.array([(0.0, 0, 0, wl.NO_REF)], wl.INFO_DTYPE).tobytes() and img.size == 0


@pytest.mark.parametrize("hop,tavg", [(128, 1), (256, 1), (128, 3), (256, 16)])
def test_row_guard_in_absolute_mode(hop, tavg):
    I, Q = (x[0].copy() for x in wl.scene_rows())
    p = wl.params(hop=hop, tavg=tavg, ref_mode=wl.REF_ABSOLUTE, ref=8e-4)
    clean, cinfo = wl.check_rows(I, Q, NS, p)
    nrows = clean.shape[1]
    assert cinfo[0]["flags"] == wl.WRITTEN and clean.max() < 255
    Q[20000] = np.inf
    img, info = wl.check_rows(I, Q, NS, p)
    white = wl.rows_touching(20000, 20000, hop, tavg, nrows)
    assert len(white) == (512 // hop if tavg == 1 else len(white)) and white
    assert info[0]["flags"] == wl.WRITTEN | wl.NONFINITE and info[0]["ref"] == np.float32(8e-4)
    assert np.all(img[0, white] == 255)
    rest = np.setdiff1d(np.arange(nrows), white)
    assert np.array_equal(img[0, rest], clean[0, rest])                      # exactly those rows, and nothing else moves
    # an Inf in samples that no complete row uses sets nothing
    Q[20000] = I[20000]
    used = hop * (nrows * tavg - 1) + 512
    if used < NS:
        I[used] = -np.inf
        img, info = wl.check_rows(I, Q, NS, p)
        assert info[0]["flags"] == wl.WRITTEN
        I[used - 1] = np.nan
        img, info = wl.check_rows(I, Q, NS, p)
        assert info[0]["flags"] == wl.WRITTEN | wl.NONFINITE and np.all(img[0, -1] == 255) and img[0, :-1].max() < 255


def test_threshold_edges():
    """r == T[i] exactly lands on i, its neighbour below on i - 1, its neighbour above on i; with db_min -10 and db_step 0.25
    T[40] = 1, T[80] = 10 and T[120] = 100 exactly, so float pixel powers reach them."""
    T = wl.levels(-10.0, 0.25)
    for i in (1, 2, 40, 80, 120, 127, 128, 129, 254, 255):
        assert wl.level_of_ratio(T[i], -10.0, 0.25) == i
        assert wl.level_of_ratio(np.nextafter(T[i], 0.0), -10.0, 0.25) == i - 1
        assert wl.level_of_ratio(np.nextafter(T[i], np.inf), -10.0, 0.25) == i
    assert wl.level_of_ratio(np.nan, -10.0, 0.25) == 0 and wl.level_of_ratio(np.inf, -10.0, 0.25) == 255
    assert wl.level_of_ratio(0.0, -10.0, 0.25) == 0 and wl.level_of_ratio(-1.0, -10.0, 0.25) == 0
    assert wl.level_of_ratio(-np.inf, -10.0, 0.25) == 0
    for m, ref, want in ((10.0, 1.0, 80), (np.nextafter(np.float32(10.0), np.float32(0)), 1.0, 79), (2.5, 0.25, 80),
                         (100.0, 1.0, 120), (1.0, 1.0, 40), (np.nextafter(np.float32(1.0), np.float32(0)), 1.0, 39),
                         (np.nan, 1.0, 0), (np.inf, 1.0, 255), (0.0, 1.0, 0)):
        assert wl.level(m, ref, -10.0, 0.25) == want, (m, ref)
    # the count of i with r >= T[i], stated as a count
    rng = np.random.default_rng(7)
    for db_min, db_step in ((-10.0, 0.25), (-60.0, 0.05), (60.0, 4.0), (3.3, 1.7)):
        T = wl.levels(db_min, db_step)
        for r in np.concatenate((10.0 ** rng.uniform(-8, 110, 200), T[1:40])):
            assert wl.level_of_ratio(r, db_min, db_step) == int(np.count_nonzero(r >= T[1:]))


def test_tavg_sums_in_rising_f():
    """m = (float)((((0.0 + P_f) + P_f+1) + P_f+2) / 3 / W2) from the checker's own frame powers, bit for bit, on a row whose
    level falls by 5 dB per 256 samples; the levels are the count against the checker's table."""
    rng = np.random.default_rng(3)
    n = 8192
    env = 10.0 ** (-np.arange(n) / 1024.0)
    I = (env * rng.normal(0, 1, n)).astype(np.float32)
    Q = (env * rng.normal(0, 1, n)).astype(np.float32)
    _, w2 = nl.tables()
    for hop in wl.HOPS:
        p = wl.params(hop=hop, tavg=3, j0=-256, j1=255, ref_mode=wl.REF_ABSOLUTE, ref=1e-6)
        img, info, m, P = wl.detail(I, Q, n, p)
        nrows = info["nrows"]
        assert nrows == ((n - 512) // hop + 1) // 3 and P.shape[0] >= 3 * nrows
        P64 = P[:3 * nrows].astype(np.float64).reshape(nrows, 3, 512)
        rising = ((0.0 + P64[:, 0]) + P64[:, 1]) + P64[:, 2]
        want = (rising / 3.0 / w2).astype(np.float32)
        assert np.array_equal(m.view(np.uint32), want.view(np.uint32))
        T = wl.levels(p[0]["db_min"], p[0]["db_step"])
        r = m.astype(np.float64) / np.float64(np.float32(1e-6))
        assert np.array_equal(img, np.searchsorted(T[1:], r, side="right").astype(np.uint8))
        # tavg 1 of the same row: the frame powers themselves
        p1 = wl.params(hop=hop, tavg=1, j0=-256, j1=255, ref_mode=wl.REF_ABSOLUTE, ref=1e-6)
        _, _, m1, P1 = wl.detail(I, Q, n, p1)
        assert np.array_equal(m1.view(np.uint32), (P1.astype(np.float64) / 1.0 / w2).astype(np.float32).view(np.uint32))


def test_batch_over_strided_rows_equals_row_by_row():
    I, Q = wl.scene_rows()
    for p in (None, wl.params(hop=256, tavg=3, j0=-149, j1=150, ref_mode=wl.REF_ABSOLUTE, ref=1e-3)):
        for n in (45000, 1291):
            img, info = wl.check_rows(I[:3], Q[:3], n, p)
            for s in range(3):
                one, oinfo, _, _ = wl.detail(I[s, :n], Q[s, :n], n, p)
                assert np.array_equal(img[s], one) and info[s].tobytes() == oinfo.tobytes()


# ---- files and palette: host code of the library ------------------------------------------------------------------------
def _parse_png(blob):
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(blob):
        (length,) = struct.unpack(">I", blob[at:at + 4])
        kind, data = blob[at + 4:at + 8], blob[at + 8:at + 8 + length]
        (crc,) = struct.unpack(">I", blob[at + 8 + length:at + 12 + length])
        assert crc == zlib.crc32(kind + data) & 0xffffffff, kind
        chunks.append((kind, data))
        at += 12 + length
    assert at == len(blob)
    return chunks


def _palette_formula(which):
    rgb = np.zeros((256, 3), np.uint8)
    for v in range(256):
        if which == 0:
            rgb[v] = (v, v, v)
            continue
        k = min(v // 51, 4)
        t = 5 * (v - 51 * k)
        rgb[v] = [(0, 0, t), (0, t, 255), (t, 255, 255 - t), (255, 255 - t, 0), (255, t, t)][k]
    return rgb


def test_palette_equals_the_formula():
    for which in (0, 1):
        assert np.array_equal(w.waterfall_palette(which), _palette_formula(which))
    ramp = w.waterfall_palette(1)
    assert [tuple(ramp[v]) for v in (0, 51, 102, 153, 204, 255)] == \
           [(0, 0, 0), (0, 0, 255), (0, 255, 255), (255, 255, 0), (255, 0, 0), (255, 255, 255)]
    assert len({tuple(c) for c in ramp}) == 256                             # every level its own colour


@pytest.mark.parametrize("shape", [(1, 1), (348, 301), (348, 512)])
def test_png_files_parse_and_give_back_the_pixels(tmp_path, shape):
    rng = np.random.default_rng(shape[1])
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    h, wd = shape
    for palette in (None, w.waterfall_palette(1)):
        path = tmp_path / "x.png"
        w.write_png_file(path, img, palette)
        chunks = _parse_png(path.read_bytes())
        kinds = [k for k, _ in chunks]
        assert kinds == ([b"IHDR", b"IDAT", b"IEND"] if palette is None else [b"IHDR", b"PLTE", b"IDAT", b"IEND"])
        by = dict(chunks)
        assert struct.unpack(">IIBBBBB", by[b"IHDR"]) == (wd, h, 8, 0 if palette is None else 3, 0, 0, 0)
        if palette is not None:
            assert by[b"PLTE"] == palette.tobytes()
        assert by[b"IEND"] == b""
        raw = zlib.decompress(by[b"IDAT"])
        assert len(raw) == h * (wd + 1)
        lines = np.frombuffer(raw, np.uint8).reshape(h, wd + 1)
        assert not lines[:, 0].any() and np.array_equal(lines[:, 1:], img)  # filter 0 on every scan line
        # stored blocks only: nothing but headers around the raw bytes (2 zlib + 5 per block + 4 Adler-32)
        assert len(by[b"IDAT"]) == len(raw) + 2 + 5 * -(-len(raw) // 65535) + 4


def test_pgm_round_trip_and_unwritable_paths(tmp_path):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (348, 301), dtype=np.uint8)
    path = tmp_path / "x.pgm"
    w.write_pgm_file(path, img)
    blob = path.read_bytes()
    head = b"P5\n301 348\n255\n"
    assert blob[:len(head)] == head and blob[len(head):] == img.tobytes()
    L = w.lib()
    missing = str(tmp_path / "no_such_directory" / "x").encode()
    assert L.wspr_write_pgm_file(missing, img.ctypes.data, 301, 348) == -1
    assert L.wspr_write_png_file(missing, img.ctypes.data, 301, 348, None) == -1
    ok = str(tmp_path / "y").encode()
    for width, height in ((0, 348), (301, 0), (-1, 5)):
        assert L.wspr_write_pgm_file(ok, img.ctypes.data, width, height) == -1
        assert L.wspr_write_png_file(ok, img.ctypes.data, width, height, None) == -1
    assert L.wspr_write_png_file(ok, None, 301, 348, None) == -1 and L.wspr_write_png_file(None, img.ctypes.data, 301, 348, None) == -1
    with pytest.raises(OSError):
        w.write_png_file(tmp_path / "no_such_directory" / "x.png", img)
    with pytest.raises(OSError):
        w.write_pgm_file(tmp_path / "no_such_directory" / "x.pgm", img)


# ---- refusals that need no device ---------------------------------------------------------------------------------------
SENTINEL = 0x5a


def test_refusals_of_the_one_row_call_write_nothing():
    L = w.lib()
    I = np.zeros(NS + 1, np.float32)
    img = np.full(348 * 512, SENTINEL, np.uint8)
    info = np.zeros(1, wl.INFO_DTYPE)
    info.view(np.uint8)[:] = SENTINEL

    def refused(code, n=NS, rows=(I, I), image=img, record=info, **kw):
        p = wl.params(**kw)
        rc = L.wspr_waterfall(None if rows[0] is None else rows[0].ctypes.data, None if rows[1] is None else rows[1].ctypes.data,
                              n, p.ctypes.data, None if image is None else image.ctypes.data,
                              None if record is None else record.ctypes.data)
        assert rc == code, (rc, code, n, kw)
        assert np.all(img == SENTINEL) and np.all(info.view(np.uint8) == SENTINEL), kw
        rows_cols = C.c_int(-7), C.c_int(-7)
        if record is not None and image is not None and rows[0] is not None and rows[1] is not None:   # the shape call takes the same checks
            assert L.wspr_waterfall_shape(n, p.ctypes.data, C.addressof(rows_cols[0]), C.addressof(rows_cols[1])) == code
            assert rows_cols[0].value == -7 and rows_cols[1].value == -7
    nan, inf = float("nan"), float("inf")
    refused(-1, n=-1)
    refused(-2, n=45001)
    refused(-2, n=45001, hop=100)                                            # the length is looked at before the parameters
    for hop in (0, 64, 127, 129, 255, 512, -128):
        refused(-1, hop=hop)
    for tavg in (0, -1, 17, 1 << 20):
        refused(-1, tavg=tavg)
    for j0, j1 in ((-257, 0), (0, 256), (5, 4), (256, 256), (-300, -257)):
        refused(-1, j0=j0, j1=j1)
    for mode in (2, -1, 255):
        refused(-1, ref_mode=mode)
    for ref in (0.0, -1.0, nan, inf, -inf):
        refused(-1, ref_mode=wl.REF_ABSOLUTE, ref=ref)
    for db_min in (nan, inf, -inf, -60.5, 60.5):
        refused(-1, db_min=db_min)
    for db_step in (nan, inf, 0.0, 0.04, 4.5, -0.25):
        refused(-1, db_step=db_step)
    refused(-1, record=None)
    refused(-1, rows=(None, I))
    refused(-1, rows=(I, None))
    refused(-1, image=None)
    with pytest.raises(ValueError):
        w.waterfall_shape(NS, dict(hop=100))
    with pytest.raises(KeyError):
        w.waterfall_shape(NS, dict(hopp=128))
    # floor mode does not look at ref: garbage there is no refusal (the shape call stands for the device call here)
    assert w.waterfall_shape(NS, dict(ref=nan)) == (348, 301)


def test_checker_refuses_what_the_library_refuses():
    I = np.zeros((1, 600), np.float32)
    img = np.zeros(4096, np.uint8)
    info = np.zeros(1, wl.INFO_DTYPE)
    X = wl.checker()
    call = lambda n, p, stride=600, istride=4096, rec=info: X.waterfall_check_rows(
        wl.ol.ptr(I), wl.ol.ptr(I), 1, n, stride, wl.ol.ptr(p), wl.ol.ptr(img), istride, None if rec is None else wl.ol.ptr(rec))
    assert call(600, wl.params()) == 0
    assert call(-1, wl.params()) == -1 and call(45001, wl.params()) == -2 and call(600, wl.params(), stride=599) == -1
    assert call(600, wl.params(), istride=300) == -1 and call(600, wl.params(), rec=None) == -1
    for kw in (dict(hop=100), dict(tavg=0), dict(tavg=17), dict(j0=-257), dict(j1=256), dict(j0=3, j1=2), dict(ref_mode=2),
               dict(ref_mode=0, ref=0.0), dict(ref_mode=0, ref=float("nan")), dict(db_min=61.0), dict(db_step=0.01),
               dict(db_step=float("nan"))):
        assert call(600, wl.params(**kw)) == -1, kw


def test_checker_is_clean_under_the_sanitizers(tmp_path):
    """The checker as a stand-alone program (its own main) under AddressSanitizer and UBSan over rows and images exactly as
    large as the contract allows."""
    exe = wl.sanitizer_program(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("waterfall_check: ok"), (r.returncode, r.stdout, r.stderr[-2000:])
