"""The indexed compress through the JavaScript front (Bzip2.compressFileIndexed over the addon's bzip2CompressIndexed, bzip2EncCreate
with flags and bzip2EncIndex) and cli.js -z --index --line-index on the GPU: the tables equal buildIndex / buildLineIndex of the
output, the output equals the plain call's and the oracle's, readLines through the returned tables gives numpy's lines."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import recipes
import support
from test_gpu_enc_stream import _norun

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "compressjs-flattened_amd", "js", "cli.js")


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _inputs():
    cap = 100000 - 19
    return {"text": recipes.textgen(300000, 11),
            "nl_run_on_boundary": np.concatenate([_norun(cap - 4), np.full(300, 0x0A, np.uint8), _norun(5000, 3)])}


def _start(nl, total, k):
    return 0 if k == 0 else (int(nl[k - 1]) + 1 if k <= nl.size else total)


def test_js_compress_file_indexed(tmp_path):
    oracle = support.Oracle()
    cases, datas = [], []
    for name, data in _inputs().items():
        src = str(tmp_path / (name + ".bin"))
        data.tofile(src)
        nl = np.flatnonzero(data == 10)
        N = int(nl.size)
        at = int(np.searchsorted(nl, 100000 - 19 - 4, "left"))          # the line around the first block boundary
        spans = [[0, 1], [max(at - 1, 0), 3], [at, 200], [N - 1, 1], [N, 1], [N + 3, 2]]
        cases.append(dict(path=src, level=1, spans=spans))
        datas.append((data, nl))
    job = str(tmp_path / "job.json")
    json.dump({"cases": cases}, open(job, "w"))
    env = dict(os.environ, CJS_ENC_CHUNK_BYTES="100000")               # the stream form goes in several steps
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js_enc_index_check.js"), job], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    for c, r, (data, nl) in zip(cases, rep["cases"], datas):
        rc, want = oracle.bzip2_compress(data, 1)
        assert rc == 0 and r["plain"] == _sha(want)
        assert r["returnedSink"] is True
        total = int(data.size)
        for name in ("bytes", "streams", "noLines"):
            f = r["forms"][name]
            assert f["output"] == r["plain"] and f["index"] == r["index"], name
            if name == "noLines":
                assert f["lineIndex"] is None and f["spans"] is None
                continue
            assert f["lineIndex"] == r["lineIndex"], name
            for (a, n), got in zip(c["spans"], f["spans"]):
                lo, hi = _start(nl, total, a), _start(nl, total, a + n)
                assert got == data[lo:hi].tobytes().hex(), (name, a, n)


def test_cli_writes_the_tables(tmp_path):
    data = recipes.textgen(300000, 11)
    src, dst, dst2 = str(tmp_path / "in.txt"), str(tmp_path / "out.bz2"), str(tmp_path / "plain.bz2")
    ix, ln = str(tmp_path / "out.ix"), str(tmp_path / "out.ln")
    data.tofile(src)
    env = dict(os.environ, CJS_ENC_CHUNK_BYTES="100000")
    o = subprocess.run(["node", CLI, "-z", "-t", "bzip2", "-1", "--index", ix, "--line-index", ln, src, dst], capture_output=True, timeout=600, env=env)
    assert o.returncode == 0, o.stderr[-2000:]
    p = subprocess.run(["node", CLI, "-z", "-t", "bzip2", "-1", src, dst2], capture_output=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    got, plain = np.fromfile(dst, dtype=np.uint8), np.fromfile(dst2, dtype=np.uint8)
    rc, want = support.Oracle().bzip2_compress(data, 1)
    assert rc == 0 and np.array_equal(got, want) and np.array_equal(plain, want)
    script = r"""
      const fs = require('fs'), path = require('path');
      const Bzip2 = require(path.join(process.argv[1], 'compressjs-flattened_amd', 'js', 'Bzip2.js'));
      const s = fs.readFileSync(process.argv[2]);
      const index = Bzip2.buildIndex(s, false), lineIndex = Bzip2.buildLineIndex(s, index);
      console.log(JSON.stringify({ index: Buffer.from(index).toString('hex'), lineIndex: Buffer.from(lineIndex).toString('hex') }));
    """
    a = subprocess.run(["node", "-e", script, ROOT, dst], capture_output=True, text=True, timeout=600)
    assert a.returncode == 0, a.stderr[-2000:]
    r = json.loads(a.stdout.strip().splitlines()[-1])
    assert open(ix, "rb").read().hex() == r["index"] and open(ln, "rb").read().hex() == r["lineIndex"]
    # the index alone
    ix2 = str(tmp_path / "only.ix")
    o = subprocess.run(["node", CLI, "-z", "-t", "bzip2", "-1", "--index", ix2, src, dst], capture_output=True, timeout=600, env=env)
    assert o.returncode == 0, o.stderr[-2000:]
    assert open(ix2, "rb").read().hex() == r["index"]


def test_cli_rejects_the_flags_elsewhere(tmp_path):
    ix = str(tmp_path / "x.ix")

    def run(*args):
        return subprocess.run(["node", CLI] + list(args), input=b"", capture_output=True, timeout=60)
    for args, text in ((("-d", "-t", "bzip2", "--index", ix), b"can only be used with compression"),
                       (("-z", "-t", "bwtc", "--index", ix, "--line-index", ix), b"need -t bzip2"),
                       (("--recover", "-t", "bzip2", "--index", ix), b"cannot be used with --recover"),
                       (("--repair", "-t", "bzip2", "--line-index", ix), b"cannot be used with --repair"),
                       (("-d", "-t", "bzip2", "--line-index", ix), b"can only be used with compression")):
        o = run(*args)
        assert o.returncode != 0 and text in o.stderr, (args, o.stderr)
        assert not os.path.exists(ix)
