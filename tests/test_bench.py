"""bench.py itself: what --dump-outputs writes, and what a plain run (no --full) does and prints."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _check_dump(arrays, stream):
    assert sorted(arrays) == ["stream_len", "stream_sample", "stream_sample_pos", "stream_sha256"]
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["stream_len"].tolist() == [stream.size]
    pos = arrays["stream_sample_pos"].astype(np.int64)
    assert np.array_equal(arrays["stream_sample_pos"], pos) and (np.diff(pos) > 0).all()
    assert np.array_equal(arrays["stream_sample"], stream[pos].astype(np.float32))
    assert bytes(arrays["stream_sha256"].astype(np.uint8)) == hashlib.sha256(stream.tobytes()).digest()
    return pos


def test_dump_outputs_samples_a_long_stream_the_same_way_every_time(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    stream = np.random.default_rng(5).integers(0, 256, bench.DUMP_SAMPLE * 2 + 12345, dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / "a"), stream)
    bench.dump_outputs(str(tmp_path / "b"), stream)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    pos = _check_dump(a, stream)
    assert pos.size == bench.DUMP_SAMPLE and pos[-1] < stream.size
    assert all(np.array_equal(a[k], b[k]) for k in a)
    short = stream[:1000]
    bench.dump_outputs(str(tmp_path / "c"), short)
    assert _check_dump(_load(str(tmp_path / "c")), short).size == short.size      # a short stream is stored whole


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    # no --full: the headline keys from the timed steps, none of the checks / baselines / extra configs; the dumped stream is
    # the reference's (10 MB golden: length + sha256 of the whole stream)
    g = support.load_golden("golden_big_bzip2_9_10m.json")["cases"][0]
    d = str(tmp_path / "out")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--mb", "10", "--dump-outputs", d]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert all(k in line for k in HEADLINE_KEYS) and line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(10_000_000 / (line["ms_per_step"] / 1e3) / 1e6, rel=1e-2)
    assert line["cpu_baseline"] is None and line["verify"] == {} and line["stage_ms_per_step"] == {}
    assert "bzip2_9_decompress" not in line and "e2e_host_buffer" not in line
    arrays = _load(d)
    assert arrays["stream_len"].tolist() == [g["out_len"]] and arrays["stream_sample"].size == g["out_len"]
    stream = arrays["stream_sample"].astype(np.uint8)
    assert hashlib.sha256(stream.tobytes()).hexdigest() == g["out_sha256"]
    _check_dump(arrays, stream)
