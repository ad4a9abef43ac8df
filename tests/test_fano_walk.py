"""The one statement of "search every gated vector, keep the first success in walk order" (csrc/host/wspr_fano_walk.h),
driven by a scripted search in a stand-alone program (tests/helpers/fano_walk_check.cpp): walks of 1, 2, 43 and 86 ranks
over 1, 3 and 300 candidates, gating densities from none to all, with and without the budget split, in the device
placement and in the host placement on one thread and on real pools of 4 and 16 threads whose tasks complete out of
order -- against the serial walk written out in the program: winning rank and record per candidate, the pending set,
the trace's attempts and fano_calls, both counter rules, and that no attempt above the winner changes any of them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_equals_the_serial_walk_in_every_placement(tmp_path):
    exe = tmp_path / "fano_walk_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", "-o", str(exe),
                    os.path.join(ROOT, "tests", "helpers", "fano_walk_check.cpp")], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok:"), r.stdout[-4000:]
