"""ctypes bindings of the impulse-noise blanker's checker (tests/helpers/blank_check.c: the contract of wspr_audio_blank_*() in
plain serial C over rtlsdr-wsprd_amd/csrc/kernels/audio_blank.h), built on demand; a numpy restatement of the same rule as
a second, independent statement; the crafted cases and the spiky scenes the blanker's tests share.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import audio_lib as al
import oracle_lib as ol

BLOCK = 8192
THR, GUARD = 96, 4              # the settings the end-to-end figures were taken with
SENTINEL = 0x7FFF

_lib = None
_SRC = os.path.join(ol.ROOT, "tests", "helpers", "blank_check.c")
_INC = os.path.join(ol.ROOT, "rtlsdr-wsprd_amd", "csrc", "kernels")


def checker():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="wspr_blank_"), "libblankcheck.so")
        subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-Wall", "-I", _INC, "-shared", "-o", out, _SRC], check=True)
        X = C.CDLL(out)
        X.blank_check_rows.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                       C.c_void_p]
        X.blank_check_rows.restype = C.c_int
        X.blank_check_level.argtypes = [C.c_void_p, C.c_int, C.c_int]
        X.blank_check_level.restype = C.c_int
        X.blank_check_block.restype = C.c_int
        assert X.blank_check_block() == BLOCK
        _lib = X
    return _lib


def sanitizer_program(directory):
    """The checker as a stand-alone program (its own main) under AddressSanitizer and UBSan: the path of the executable."""
    exe = os.path.join(str(directory), "blank_check_asan")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DBLANK_CHECK_MAIN", "-I", _INC, "-o", exe, _SRC], check=True)
    return exe


def round8(n):
    return (n + 7) & ~7


def check_rows(pcm, nsamp, thr16, guard, out_stride=None):
    """The checker on int16 records [nseg, stride], of which the first nsamp samples count.  Returns (out [nseg, out_stride]
    pre-filled with SENTINEL, n_blanked [nseg])."""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    if pcm.ndim == 1:
        pcm = pcm[None, :]
    nseg, stride = pcm.shape
    out_stride = round8(nsamp) if out_stride is None else out_stride
    out = np.full((nseg, out_stride), SENTINEL, np.int16)
    count = np.full(nseg, -1, np.int32)
    rc = checker().blank_check_rows(ol.ptr(pcm), stride, int(nsamp), nseg, int(thr16), int(guard), ol.ptr(out), out_stride,
                                    ol.ptr(count))
    assert rc == 0, rc
    return out, count


def level(pcm, b):
    """The checker's level of block b of one record."""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    return int(checker().blank_check_level(ol.ptr(pcm), int(pcm.size), int(b)))


def blank_numpy(pcm, thr16, guard):
    """The rule of audio_blank.h restated with numpy (sorted medians, window counts from a running sum): (out, n_blanked)
    for one record."""
    pcm = np.asarray(pcm, np.int16)
    n = pcm.size
    a = np.abs(pcm.astype(np.int64))
    out = pcm.copy()
    blanked = 0
    for lo in range(0, n, BLOCK):
        hi = min(lo + BLOCK, n)
        lev = int(np.sort(a[lo:hi])[(hi - lo - 1) // 2])
        if lev == 0:
            continue
        w0, w1 = max(0, lo - guard), min(n, hi + guard)           # the samples any window of this block can reach
        run = np.concatenate(([0], np.cumsum(16 * a[w0:w1] > thr16 * lev)))
        idx = np.arange(lo, hi)
        first = np.maximum(idx - guard, 0) - w0
        last = np.minimum(idx + guard, n - 1) - w0
        cond = run[last + 1] - run[first] > 0
        out[lo:hi][cond] = 0
        blanked += int(cond.sum())
    return out, blanked


def random_rows(nsamp, seed):
    """Three records of nsamp samples with different contents: full-scale noise; quiet noise with one loud sample in 16;
    quiet noise with rare spikes, runs of -32768 and a stretch of digital silence."""
    rng = np.random.default_rng(seed)
    n = max(nsamp, 1)
    rows = np.zeros((3, n), np.int16)
    rows[0] = rng.integers(-32768, 32768, n)
    quiet = rng.integers(-32768, 32768, n) // 64
    rows[1] = np.where(rng.integers(0, 16, n) == 0, rng.integers(-32768, 32768, n), quiet)
    r2 = rng.integers(-300, 301, n)
    r2[rng.integers(0, 400, n) == 0] = 32767
    r2[rng.integers(0, 400, n) == 0] = -32768
    if n > 40:
        r2[n // 3:n // 3 + 9] = -32768
        r2[n // 2:n // 2 + min(n // 4, 6000)] = 0
    rows[2] = r2
    rows[:, 0] = -32768
    return rows[:, :nsamp] if nsamp else rows[:, :0]


# ---- crafted cases: (name, records [rows, nsamp], thr16, guard, expected output, expected counts), by hand ---------------
def _tone(n, amp):
    """n samples of magnitude amp with alternating signs: every |sample| is amp, so the level is amp."""
    return (amp * (1 - 2 * (np.arange(n) & 1))).astype(np.int16)


def _zeroed(pcm, idx):
    out = pcm.copy()
    out[0, list(idx)] = 0
    return out


@functools.lru_cache(maxsize=None)
def crafted_cases():
    cases = []
    # a spike at the last sample of block 0 (level 10); block 1 is ten times louder (level 100).  thr16 = 160: a hit is
    # a > 100 by block 0's level, a > 1000 by block 1's.  The spike of 1000 blanks 8187 .. 8191; 8192 .. 8195 are judged by
    # block 1's level, by which it is no hit (16 * 1000 == 160 * 100).  Block 1's samples of 100 are no hits for block 0.
    p = np.concatenate((_tone(BLOCK, 10), _tone(BLOCK, 100)))[None, :].copy()
    p[0, 8191] = 1000
    cases.append(("spike_at_8191_louder_block_behind", p, 160, 4, _zeroed(p, range(8187, 8192)), [5]))
    # the mirror image: the spike at the first sample of block 1 (level 10), block 0 the louder one
    p = np.concatenate((_tone(BLOCK, 100), _tone(BLOCK, 10)))[None, :].copy()
    p[0, 8192] = -1000
    cases.append(("spike_at_8192_louder_block_in_front", p, 160, 4, _zeroed(p, range(8192, 8197)), [5]))
    # equality is no hit: level 16, thr16 = 32: 16 a > 512 holds for 33 and not for 32
    p = _tone(100, 16)[None, :].copy()
    p[0, 50], p[0, 70] = 32, -33
    cases.append(("equality_is_no_hit", p, 32, 0, _zeroed(p, [70]), [1]))
    # an even count takes the lower middle value: |1, 3, 60, -2| sorted is 1 2 3 60, level 2; thr16 = 400: 16 * 60 = 960
    # is above 400 * 2 and would not be above 400 * 3
    p = np.array([[1, 3, 60, -2]], np.int16)
    cases.append(("even_count_takes_the_lower_median", p, 400, 0, _zeroed(p, [2]), [1]))
    # a short last block: its level (4) is that of its own five samples -- not 0 from an empty rest of the block, not 1000
    # from block 0.  guard 1: 300 at 8195 blanks 8194 .. 8196, and the loud sample 8191 of block 0, judged by level 4, blanks 8192
    p = np.concatenate((_tone(BLOCK, 1000), np.array([4, -4, 4, 300, 4], np.int16)))[None, :].copy()
    cases.append(("short_last_block", p, 96, 1, _zeroed(p, [8192, 8194, 8195, 8196]), [4]))
    # digital silence for more than half of the block: level 0, copied, spikes included
    p = np.zeros((1, 1000), np.int16)
    p[0, 600:] = _tone(400, 30000)
    cases.append(("silent_block_is_copied", p, 16, 64, p.copy(), [0]))
    # -32768 counts as 32768: level 32767, thr16 = 16: a hit is a > 32767
    p = _tone(64, 32767)[None, :].copy()
    p[0, 10] = -32768
    cases.append(("minus_32768_is_32768", p, 16, 0, _zeroed(p, [10]), [1]))
    # ... and as a level: five of nine samples are -32768, level 32768, nothing can exceed it
    p = np.array([[-32768, 100, -32768, 100, -32768, 100, -32768, 100, -32768]], np.int16)
    cases.append(("level_32768", p, 16, 2, p.copy(), [0]))
    # guard 64 at both ends of a record of 1003 samples (level 10): 0 .. 64 and 938 .. 1002 go; the second record has no
    # spike and keeps every sample -- unless something is read from the first record's padding in front of it
    p = np.stack((_tone(1003, 10), _tone(1003, 10)))
    p[0, 0], p[0, 1002] = 5000, -5000
    want = p.copy()
    want[0, :65] = 0
    want[0, 938:] = 0
    cases.append(("guard_64_at_both_ends", p, 96, 64, want, [130, 0]))
    for c in cases:
        c[1].setflags(write=False)
        c[4].setflags(write=False)
    return cases


# ---- spiky scenes -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _unit_signals():
    """(sample indices, cos of the phase) of the three signals every spiky scene holds: audio_lib.audio_scene()'s waveform for
    SCENE_MESSAGES[0] at the offsets and times of SIGNALS, at unit amplitude (the same for every seed: computed once)."""
    out = []
    for j, msg in enumerate(al.SCENE_MESSAGES[0]):
        ok, sym = ol.channel_symbols(msg)
        assert ok, msg
        f0, t0 = al.SIGNALS[j][1], al.SIGNALS[j][2]
        f = 1500.0 + f0 + (np.repeat(np.asarray(sym, np.float64), al.SPS) - 1.5) * (al.RATE / al.SPS)
        phi = np.concatenate(([0.0], np.cumsum(2.0 * np.pi * f / al.RATE)[:-1]))
        idx = int(round(t0 * al.RATE)) + np.arange(phi.size)
        keep = (idx >= 0) & (idx < al.NSAMP)
        out.append((idx[keep], np.cos(phi[keep])))
    return out


def dirty_scene(seed, rate, blen, snr=-20.0):
    """audio_lib's scene recipe scaled by 500 instead of 2000 (head-room for the spikes): SCENE_MESSAGES[0] at `snr` dB with
    the offsets and times of SIGNALS over the same noise, then int(rate * 120) bursts at positions drawn from the scene's own
    generator after the noise, each blen samples of +-32767 with random signs, added before rounding and clipping."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, np.sqrt(2.4), al.NSAMP)
    for idx, wave in _unit_signals():
        x[idx] += np.sqrt(2.0) * 10.0 ** (snr / 20.0) * wave
    x *= 500.0
    nburst = int(rate * 120)
    if nburst:
        pos = rng.integers(0, al.NSAMP - blen + 1, nburst)
        sign = rng.integers(0, 2, (nburst, blen)) * 2 - 1
        for j in range(blen):
            np.add.at(x, pos + j, 32767.0 * sign[:, j])
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def dirty_items(snr=-20.0):
    return [(al.SCENE_MESSAGES[0][j], snr, al.SIGNALS[j][1], al.SIGNALS[j][2]) for j in range(3)]


@functools.lru_cache(maxsize=None)
def e2e_scene(rate):
    """The scene of the end-to-end tests: seed 9100, bursts of 3 samples, `rate` per second (read-only)."""
    pcm = dirty_scene(9100, rate, 3)
    pcm.setflags(write=False)
    return pcm



@functools.lru_cache(maxsize=None)
def scene_blanked(rate):
    """(the checker's blanked record of e2e_scene(rate) at (THR, GUARD), samples blanked), read-only."""
    out, count = check_rows(e2e_scene(rate), al.NSAMP, THR, GUARD)
    out.setflags(write=False)
    return out[0], int(count[0])


@functools.lru_cache(maxsize=None)
def scene_oracle(rate, blanked):
    """The CPU oracle's spots for the checker's K12 rows (normalised) of e2e_scene(rate), blanked by the checker or not."""
    pcm = scene_blanked(rate)[0] if blanked else e2e_scene(rate)
    I, Q = al.check_rows(pcm, normalise=1)
    return ol.decode(I[0], Q[0])[0]
