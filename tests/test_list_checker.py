"""List decoding against known messages WITHOUT a GPU: the serial checker tests/helpers/list_check.c (what the kernel K14 is
held to, tests/test_gpu_list.py) against an independent int64 numpy statement of the definition in
rtlsdr-wsprd_amd/csrc/kernels/listmatch.h, against the ordered-statistics cost of the same code word, on inputs whose
answer is known; the gate's integer inequality at its edge; and how wspr_set_message_list() builds a list (host code)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import list_lib as ll
import osd_lib as ol
import rtlsdr_wsprd_amd as w


@pytest.fixture(scope="module")
def sym():
    return ll.all_symbols()


@pytest.fixture(autouse=True)
def list_off():
    yield
    for L in (w.lib(), w.lab()):
        w.set_message_list(None, library=L)


def test_checker_equals_the_numpy_statement(sym):
    vec = ll.match_vectors()
    for m in (1, 2, 33, 300, 7600):
        got, want = ll.check(sym[:m], vec), ll.numpy_match(sym[:m], vec)
        assert np.array_equal(got, want), (m, np.flatnonzero((got != want).any(axis=1))[:5])
    one = ll.check(sym[:1], vec)
    assert np.all(one[:, 0] == 0) and np.all(one[:, 2] == ll.NO_SECOND)
    assert ll.checker().list_check(sym.ctypes.data, 0, vec.ctypes.data, 1, None) == -1
    assert ll.checker().list_check(sym.ctypes.data, 1, vec.ctypes.data, -1, None) == -1


def test_degenerate_and_clean_vectors_have_the_answers_the_definition_gives(sym):
    deg = ll.degenerate_vectors()
    B = (2 * (sym.astype(int) >> 1) - 1).sum(axis=1)              # B_m
    got = ll.check(sym, deg)
    # all 0: v = -255 everywhere, S = -255 B; all 255: S = 255 B; all 128: v = 1, S = B; all 127: S = -B
    for row, scale in ((0, -255), (1, 255), (2, 1), (3, -1)):
        S = scale * B
        assert got[row, 1] == S.max() and got[row, 0] == int(np.argmax(S)), row        # argmax: the first of equals
        assert got[row, 2] == np.sort(S)[-2]
    assert list(got[:, 3]) == [ll.V_MAX, ll.V_MAX, 162, 162, ll.V_MAX]
    for k in (0, 31, 32, 7599):
        r = ll.check(sym, np.stack([ll.clean(sym[k]), 255 - ll.clean(sym[k])]))
        assert tuple(r[0, [0, 1, 3]]) == (k, ll.S_CLEAN, ll.V_MAX) and r[0, 2] < ll.S_CLEAN
        assert ll.gate(r[0, 1], r[0, 3], 203) == 1                 # z = sqrt(162) = 12.73 >= 203 / 16
        assert r[1, 1] < ll.S_CLEAN                                # the complement is no code word's clean vector
        assert -ll.S_CLEAN == int((2 * (255 - ll.clean(sym[k])).astype(int) - 255) @ (2 * (sym[k].astype(int) >> 1) - 1))


def test_tie_vectors_tie_and_the_lower_index_wins(sym):
    for a, b, v in ll.tie_cases():
        c = 2 * (sym.astype(int) >> 1) - 1
        x = 2 * v.astype(int) - 255
        assert int(c[a] @ x) == int(c[b] @ x)
        r = ll.check(sym, v[None])[0]
        assert r[0] == min(a, b) and r[2] == r[1] == int(c[a] @ x), (a, b, r)
        # in a list that ends before the later member the earlier one wins alone
        lo, hi = min(a, b), max(a, b)
        r = ll.check(sym[:hi], v[None])[0]
        assert r[0] == lo and r[2] < r[1]


def test_score_is_r_minus_twice_the_osd_cost(sym):
    """S = R - 2 D with D the ordered-statistics cost of the entry's code word (osd.h: the sum of the reliabilities where
    the code word differs from the hard decisions), computed the way tests/test_osd_checker.py does."""
    vec = ll.match_vectors()
    for k in (0, 33, 4000, 7599):
        assert w.set_message_list([ll.all_messages()[k]]) == 1
        _, dec, s = w.message_list_entry(0)
        assert np.array_equal(s, sym[k])
        cw = ol.encode_bits(dec) > 0                               # deinterleaved code bits of the entry's decdata
        for t in (0, 4, 9, 40, 100, 200, 256):
            d = vec[t].astype(int)[ol.PERM]
            h, r = d >= 128, np.abs(2 * d - 255)
            D = int(r[cw != h].sum())
            assert ll.check(sym[k:k + 1], vec[t][None])[0, 1] == int(r.sum()) - 2 * D, (k, t)


def test_gate_at_its_edge():
    """256 S^2 >= zmin16^2 V in 64-bit integers.  On integers the equality is reached (S = 6 k, V = k^2 at zmin16 = 96); no
    VECTOR reaches it: S is a sum of 162 odd numbers (even), V = 2 mod 8, so 256 S^2 holds an even and zmin16^2 V an odd
    number of factors 2.  A vector is therefore held to the two neighbouring thresholds."""
    for k in (1, 7, 541, 3245):                                    # 6 * 3245 = 19 470, V = 10 530 025 <= V_MAX
        s, v = 6 * k, k * k
        assert ll.gate(s, v, 96) == 1 and ll.gate(s, v, 97) == 0 and ll.gate(s - 1, v, 96) == 0 and ll.gate(s, v + 1, 96) == 0
    assert ll.gate(0, 162, 1) == 0 and ll.gate(-41310, ll.V_MAX, 1) == 0 and ll.gate(1, ll.V_MAX, 1) == 0
    assert ll.gate(41310, ll.V_MAX, 203) == 1                      # the largest products: 256 * 41310^2 = 4.4e11
    rng = np.random.default_rng(3)
    for _ in range(2000):
        s, v, z = int(rng.integers(-41310, 41311)), int(rng.integers(162, ll.V_MAX + 1)), int(rng.integers(1, 204))
        assert ll.gate(s, v, z) == ll.gate_exact(s, v, z)
    sym = ll.all_symbols()
    vec = np.clip(np.where(sym[5] >> 1, 150, 105) + rng.normal(0, 40, 162), 0, 255).astype(np.uint8)
    _, s, _, v = ll.check(sym[:64], vec[None])[0]
    z = int(np.floor(16 * s / np.sqrt(v)))                         # the largest threshold the vector passes
    assert 1 < z < 203 and 256 * int(s) ** 2 != z * z * int(v)
    assert ll.gate(s, v, z) == 1 and ll.gate(s, v, z + 1) == 0


def _canonical(msg):
    c, g, p = msg.split()
    return "%s %s %02d" % (c, g, int(p))


def test_list_construction():
    msgs = ll.all_messages()
    assert w.message_list_entry(0) is None                         # off by default
    # the canonical text: a type-1 power prints with two digits
    assert w.set_message_list(["K1JT FN20 0"]) == 1
    text, dec, s = w.message_list_entry(0)
    assert text == "K1JT FN20 00" and np.array_equal(s, w.get_wspr_channel_symbols("K1JT FN20 0")[1])
    assert dec[6] & 0x3F == 0 and not dec[7:].any()
    assert w.message_list_entry(1) is None and w.message_list_entry(-1) is None
    # a type-2 text is an entry; its decdata decodes to itself
    assert w.set_message_list(["PJ4/K1ABC 37", "K1ABC/7 30"]) == 2
    assert [w.message_list_entry(k)[0] for k in range(2)] == ["PJ4/K1ABC 37", "K1ABC/7 30"]
    # dedupe: the first occurrence stays, the order of the rest is kept ("K1JT FN20 00" repeats the 50 bits of "K1JT FN20 0")
    given = [msgs[7], "K1JT FN20 0", msgs[9], msgs[7], "K1JT FN20 00", msgs[8], msgs[9]]
    assert w.set_message_list(given, 88) == 4
    assert [w.message_list_entry(k)[0] for k in range(4)] == [_canonical(m) for m in (msgs[7], "K1JT FN20 0", msgs[9], msgs[8])]
    assert w.message_list_entry(4) is None
    # refusals change nothing: a type-3 text, a text channel_symbols() refuses, bad counts, bad thresholds
    held = [w.message_list_entry(k)[0] for k in range(4)]
    assert w.set_message_list([msgs[0], "<K1JT> FN20QI 37"]) == -1
    assert w.set_message_list([msgs[0], msgs[1], "HELLO"]) == -1
    assert w.set_message_list([msgs[0]], 0) == -1 and w.set_message_list([msgs[0]], 204) == -1
    arr = (C.c_char_p * 1)(msgs[0].encode())
    assert w.lib().wspr_set_message_list(C.cast(arr, C.c_void_p), -1, 96) == -1
    assert w.lib().wspr_set_message_list(C.cast(arr, C.c_void_p), w.LIST_MAX + 1, 96) == -1
    assert [w.message_list_entry(k)[0] for k in range(4)] == held and w.message_list_entry(4) is None
    assert w.set_message_list([msgs[0]], 1) == 1 and w.set_message_list([msgs[0]], 203) == 1
    # n == 0 / NULL switch the stage off
    assert w.set_message_list([]) == 0 and w.message_list_entry(0) is None
    assert w.set_message_list(msgs[:3]) == 3 and w.lib().wspr_set_message_list(None, 3, 96) == 0 and w.message_list_entry(0) is None
    # every one of the 7 600 qualifies, is distinct, and holds the symbols the encoder gives for its text
    assert w.set_message_list(msgs) == 7600
    for k in (0, 1, 18, 19, 380, 7599):
        text, _, s = w.message_list_entry(k)
        c, g, p = msgs[k].split()
        assert text == "%s %s %02d" % (c, g, int(p)) and np.array_equal(s, ll.all_symbols()[k])


def test_refusal_names_the_offending_index(tmp_path):
    """The line on stderr (a child process: the library writes to the C stream)."""
    code = ("import sys; sys.path.insert(0, %r); import rtlsdr_wsprd_amd as w\n"
            "assert w.set_message_list(['K1JT FN20 37', 'W1AW FN31 30', '<K1JT> FN20QI 37']) == -1\n" % ll.ROOT)
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "wspr_set_message_list" in r.stderr and "entry 2" in r.stderr


def test_device_entry_needs_a_list_and_a_sane_count():
    """The argument checks of wspr_list_match_batch_device() come before anything touches a device."""
    vec = np.zeros((1, 162), np.uint8)
    guard = np.full(8, 0x5A5A5A5A, np.int32)
    for L in (w.lib(), w.lab()):
        assert L.wspr_list_match_batch_device(vec.ctypes.data, 1, guard.ctypes.data) == -1      # no list
        assert L.wspr_list_match_batch_device(vec.ctypes.data, 0, guard.ctypes.data) == -1
        assert w.set_message_list(ll.all_messages()[:5], library=L) == 5
        assert L.wspr_list_match_batch_device(vec.ctypes.data, -1, guard.ctypes.data) == -1     # n < 0
        assert L.wspr_list_match_batch_device(vec.ctypes.data, 0, guard.ctypes.data) == 0       # n == 0: nothing happens
        assert np.all(guard == 0x5A5A5A5A)


def test_checker_runs_clean_as_a_sanitized_standalone_program(tmp_path):
    """list_check.c with its own main under AddressSanitizer and UBSan: a host program, nothing loaded into Python."""
    exe = tmp_path / "list_check"
    cc = subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-DLIST_CHECK_MAIN", "-o", str(exe), os.path.join(ll.ROOT, "tests", "helpers", "list_check.c")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("list_check ok"), (r.stdout, r.stderr)
