"""The impulse-noise blanker (K15) on the CPU: the serial checker (tests/helpers/blank_check.c over
rtlsdr-wsprd_amd/csrc/kernels/audio_blank.h) against a numpy restatement of the rule and against crafted cases written out by
hand, the checker under AddressSanitizer as a stand-alone program, and what the blanker buys end to end: checker blanker ->
checker front end (K12) -> CPU oracle.  No GPU."""
import subprocess

import numpy as np
import pytest

import audio_lib as al
import blank_lib as bl
import oracle_lib as ol

LENGTHS = [0, 1, 2, 8191, 8192, 8193, 8196, 16383, 16385, 24581]
THRS = [16, 96, 4096]
GUARDS = [0, 1, 4, 64]


@pytest.mark.parametrize("nsamp", LENGTHS)
def test_checker_equals_the_numpy_restatement(nsamp):
    rows = bl.random_rows(nsamp, 500 + nsamp)
    assert (rows == -32768).any() or nsamp == 0
    for thr16 in THRS:
        for guard in GUARDS:
            out, count = bl.check_rows(rows, nsamp, thr16, guard, out_stride=bl.round8(nsamp) + 8)
            for s in range(3):
                want, n = bl.blank_numpy(rows[s], thr16, guard)
                assert np.array_equal(out[s, :nsamp], want), (thr16, guard, s)
                assert count[s] == n, (thr16, guard, s)
                assert not out[s, nsamp:bl.round8(nsamp)].any()                       # the padding of the last chunk: zeros
                assert np.all(out[s, bl.round8(nsamp):] == bl.SENTINEL)              # behind it: left alone
    if nsamp >= 8192:                                                                 # the settings do something
        assert 0 < bl.check_rows(rows, nsamp, 96, 4)[1][1] < nsamp


@pytest.mark.parametrize("case", bl.crafted_cases(), ids=[c[0] for c in bl.crafted_cases()])
def test_crafted_cases(case):
    name, pcm, thr16, guard, want, counts = case
    nsamp = pcm.shape[1]
    # the records sit in a sentinel-filled buffer, stride = nsamp rounded up to 8, plus 16
    stride = bl.round8(nsamp) + 16
    host = np.full((pcm.shape[0], stride), bl.SENTINEL, np.int16)
    host[:, :nsamp] = pcm
    out, count = bl.check_rows(host, nsamp, thr16, guard, out_stride=stride)
    assert np.array_equal(out[:, :nsamp], want) and count.tolist() == counts
    assert not out[:, nsamp:bl.round8(nsamp)].any() and np.all(out[:, bl.round8(nsamp):] == bl.SENTINEL)
    for s in range(pcm.shape[0]):
        got, n = bl.blank_numpy(pcm[s], thr16, guard)
        assert np.array_equal(got, want[s]) and n == counts[s]


def test_levels_of_the_crafted_cases():
    by_name = {c[0]: c[1] for c in bl.crafted_cases()}
    assert [bl.level(by_name["spike_at_8191_louder_block_behind"][0], b) for b in (0, 1)] == [10, 100]
    assert bl.level(by_name["even_count_takes_the_lower_median"][0], 0) == 2
    assert [bl.level(by_name["short_last_block"][0], b) for b in (0, 1)] == [1000, 4]
    assert bl.level(by_name["silent_block_is_copied"][0], 0) == 0
    assert bl.level(by_name["minus_32768_is_32768"][0], 0) == 32767
    assert bl.level(by_name["level_32768"][0], 0) == 32768


def test_checker_refuses_what_the_library_refuses():
    chk = bl.checker()
    pcm = np.zeros(64, np.int16)
    out = np.full(64, bl.SENTINEL, np.int16)
    p, o = ol.ptr(pcm), ol.ptr(out)
    for thr16, guard in ((15, 4), (4097, 4), (96, -1), (96, 65)):
        assert chk.blank_check_rows(p, 64, 64, 1, thr16, guard, o, 64, None) == -1
    assert chk.blank_check_rows(p, 64, -1, 1, 96, 4, o, 64, None) == -1
    assert chk.blank_check_rows(p, 56, 64, 1, 96, 4, o, 64, None) == -1
    assert chk.blank_check_rows(p, 1440008, 1440001, 0, 96, 4, o, 1440008, None) == -2
    assert np.all(out == bl.SENTINEL)
    assert chk.blank_check_rows(p, 64, 64, 1, 96, 4, o, 64, None) == 0 and not out.any()      # n_blanked may be NULL


def test_checker_under_the_address_sanitizer(tmp_path):
    """A stand-alone program with its own main (no LD_PRELOAD, nothing loaded into Python): rows exactly as large as the
    contract allows, lengths 0, 1, 8191, 8192, 8193 and 20000, guard 0, 4 and 64."""
    r = subprocess.run([bl.sanitizer_program(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "blank_check: ok" in r.stdout and not r.stderr.strip()


def test_the_highest_threshold_leaves_a_scene_alone():
    out, count = bl.check_rows(al.scene(0), al.NSAMP, 4096, 64)
    assert count[0] == 0 and np.array_equal(out[0], al.scene(0))


def test_end_to_end_on_the_cpu():
    """Seed 9100: 50 bursts per second of 3 samples at +-32767 over three signals at -20 dB.  Without the blanker the oracle
    finds none of them on the front end's rows, after it all three; the blanker costs a spike-free scene nothing."""
    items = bl.dirty_items()
    dirty = al.find_sent(bl.scene_oracle(50, False), items)
    assert [s is not None for s in dirty] == [False, False, False]
    blanked = al.find_sent(bl.scene_oracle(50, True), items)
    share = bl.scene_blanked(50)[1] / al.NSAMP
    print("blanked share %.5f; spots %s" % (share, [(s.message, s.snr) for s in blanked if s is not None]))
    assert all(s is not None for s in blanked)
    assert 0.03 < share < 0.06
    clean = al.find_sent(bl.scene_oracle(0, True), items)
    clean_share = bl.scene_blanked(0)[1] / al.NSAMP
    print("spike-free: blanked share %.5f" % clean_share)
    assert all(s is not None for s in clean) and clean_share < 0.002
