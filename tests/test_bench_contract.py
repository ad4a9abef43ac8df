"""bench.py pieces that can be checked without a GPU: the algorithmic byte counts behind the roofline
(SURVEY 8d), the CPU-share helper, and the command-line contract."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_algorithmic_bytes_are_the_surveys():
    import bench
    assert bench.K1_BYTES == 360000 + 4 * 417 * 347 == 938796          # IQ read once + ps rows 48..464 written
    assert bench.STAGE_BYTES == 1517592                                   # K1 + (ps read once by K2/K3)
    assert bench.HBM_PEAK_GBS == 8000.0
    assert bench.NS == 45000


def test_cpu_share_is_positive_and_bounded():
    import bench
    n = bench.usable_cpus()
    assert 1 <= n <= (os.cpu_count() or 1)


def test_command_line_contract():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--config", "--inflight", "--full", "--dump-outputs"):
        assert flag in out.stdout


def test_dump_outputs_writes_the_records_in_float_arrays(tmp_path):
    """--dump-outputs: the spot counts and the decoder_results records of a step as float32 / float64 .npy files, the
    records flattened in (segment, spot) order, only the slots below each segment's count; over the 64 MB cap a fixed
    sample of segments, the same one every time."""
    import ctypes as C
    import numpy as np
    import bench
    import rtlsdr_wsprd_amd as w
    nseg, k = 64, 4
    out = (w.decoder_results * (nseg * k))()
    cnt = np.array([s % (k + 1) for s in range(nseg)], np.int32)
    for s in range(nseg):
        for i in range(k):                                  # slots past the count hold stale records: never dumped
            r = out[s * k + i]
            r.freq, r.snr, r.cycles, r.message = 14.0956 + s * 1e-6, -float(i), s * 10 + i, ("CALL%d FN20 %d" % (s, i)).encode()
    recs = np.frombuffer(out, dtype=np.uint8).view(np.dtype(w.decoder_results)).reshape(nseg, k)
    n = bench.dump_outputs(str(tmp_path / "a"), cnt, recs)
    assert n == int(cnt.sum())
    got = {f.name[:-4]: np.load(f) for f in (tmp_path / "a").iterdir()}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["segments"].tolist() == list(range(nseg)) and got["spots_per_segment"].tolist() == cnt.tolist()
    seg = got["spot_segment"].astype(int)
    idx = np.concatenate([np.arange(c) for c in cnt])
    assert seg.tolist() == np.repeat(np.arange(nseg), cnt).tolist()
    assert got["cycles"].tolist() == (seg * 10 + idx).tolist() and got["snr"].tolist() == (-idx).astype(np.float32).tolist()
    text = [bytes(m.astype(np.uint8)).rstrip(b"\0").decode() for m in got["message"]]
    assert text == ["CALL%d FN20 %d" % (s, i) for s, i in zip(seg, idx)]
    # over the cap: a seeded sample of segments, in index order, identical from call to call, within the cap
    cap = bench.DUMP_CAP_BYTES
    try:
        bench.DUMP_CAP_BYTES = 20000
        bench.dump_outputs(str(tmp_path / "b"), cnt, recs)
        bench.dump_outputs(str(tmp_path / "c"), cnt, recs)
    finally:
        bench.DUMP_CAP_BYTES = cap
    sel = np.load(tmp_path / "b" / "segments.npy")
    assert 0 < len(sel) < nseg and np.all(np.diff(sel) > 0)
    assert sum(f.stat().st_size for f in (tmp_path / "b").iterdir()) <= 20000 + 128 * 15       # + the .npy headers
    for f in (tmp_path / "b").iterdir():
        assert np.array_equal(np.load(f), np.load(tmp_path / "c" / f.name))


def _bench(*argv, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), capture_output=True, text=True,
                          env=env, timeout=300)


def test_gpus_flag_spawns_ranks_or_fails_loudly():
    """`--gpus N` is honoured by bench.py itself (round-2 verdict: it used to be parsed and ignored).  Without a
    launcher around it the script re-executes as N ranks; on a node with fewer GPUs it says so and exits non-zero."""
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("this node could really run two ranks")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = _bench("--gpus", "2", "--steps", "1", "--warmup", "0", env=env)
    assert r.returncode != 0
    assert "--gpus 2 but only" in r.stderr and "HIP device(s) visible" in r.stderr


def test_gpus_flag_must_agree_with_the_launcher():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = _bench("--gpus", "4", env=env)
    assert r.returncode != 0 and "--gpus 4 but WORLD_SIZE=2" in r.stderr
