"""examples/wspr_host.c --waterfall FILE.png: the option's parsing (CPU), and on a GPU the picture of the decoded slot -- a
PNG that parses, holds the colour ramp and the pixels of wspr_waterfall() on the file's samples with the default parameters --
beside an unchanged stdout, and exit status 4 where the picture cannot be written."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from test_examples import GOLDEN, REPORT_LINE, exe, run  # noqa: F401  (exe: the fixture that builds the program)
from test_waterfall_checker import _parse_png


def test_waterfall_option_needs_a_value_and_a_mode(exe):  # noqa: F811
    assert run(exe, "--waterfall").returncode == 2
    assert run(exe, "-r", "--waterfall").returncode != 0
    r = run(exe, "--waterfall", "x.png")
    assert r.returncode == 2 and "--waterfall FILE.png" in r.stderr             # no mode: the usage line, which names the option


@pytest.mark.gpu
def test_waterfall_of_the_played_back_slot(exe, tmp_path):  # noqa: F811
    import rtlsdr_wsprd_amd as w
    png = tmp_path / "slot.png"
    plain = run(exe, "-f", "144489000", "-r", GOLDEN)
    r = run(exe, "-f", "144489000", "--waterfall", str(png), "-r", GOLDEN)
    assert r.returncode == 0 and plain.returncode == 0, r.stderr
    assert r.stdout == plain.stdout and r.stdout.splitlines()[2:] == [REPORT_LINE]  # stdout is what it always was
    assert "301 x 348" in r.stderr
    chunks = _parse_png(png.read_bytes())
    assert [k for k, _ in chunks] == [b"IHDR", b"PLTE", b"IDAT", b"IEND"]
    by = dict(chunks)
    assert struct.unpack(">IIBBBBB", by[b"IHDR"]) == (301, 348, 8, 3, 0, 0, 0)
    assert by[b"PLTE"] == w.waterfall_palette(1).tobytes()
    lines = np.frombuffer(zlib.decompress(by[b"IDAT"]), np.uint8).reshape(348, 302)
    I, Q = np.zeros(45000, np.float32), np.zeros(45000, np.float32)          # the program's own reader
    n = w.lib().wspr_read_iq_file(C.c_char_p(GOLDEN.encode()), C.c_void_p(I.ctypes.data), C.c_void_p(Q.ctypes.data))
    want, info = w.waterfall(I, Q, samples=n)                                    # the slot as read, BEFORE the decode
    assert n == 45000 and info["flags"] == w.WF_WRITTEN and not lines[:, 0].any()
    assert np.array_equal(lines[:, 1:], want)
    # the reference's recording: one signal 0 dB in 2 500 Hz near +50 Hz -- the brightest column of the picture is there
    col = int(np.argmax(lines[:, 1:].astype(int).sum(axis=0))) - 150
    assert 60 <= col <= 76, col


@pytest.mark.gpu
def test_waterfall_that_cannot_be_written_is_status_4(exe, tmp_path):  # noqa: F811
    r = run(exe, "--waterfall", str(tmp_path / "no_such_directory" / "x.png"), "-r", GOLDEN)
    assert r.returncode == 4 and "cannot write" in r.stderr and "Spot" not in r.stdout
    r = run(exe, "--waterfall", str(tmp_path / "t.png"), "-t", cwd=tmp_path)
    assert r.returncode == 0 and "Self-test SUCCESS!" in r.stdout and (tmp_path / "t.png").stat().st_size > 348 * 301
