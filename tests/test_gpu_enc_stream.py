"""Streaming Bzip2 encoder on the GPU box: cjs_bzip2_enc_* through the Python front, the N-API front and cli.js.  Every
comparison is with a golden or with the oracle."""
import hashlib
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

import recipes
import support

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    return importlib.import_module("compressjs-flattened_amd")


def _splits(n, seed, max_piece):
    """write sizes of a fixed seed: many small, some large, some empty"""
    rng = np.random.default_rng(seed)
    out, left = [], n
    while left:
        k = int(rng.integers(0, 4))
        piece = 0 if k == 0 else int(rng.integers(1, max(2, max_piece >> (4 * (k - 1)))))
        piece = min(piece, left)
        out.append(piece)
        left -= piece
    return out or [0]


def encode(pkg, data, level, chunk_bytes, writes=None, read_max=None, track=None):
    """the whole stream through an encoder: `writes` = write sizes (default: one write), draining after each write with reads of
    at most read_max bytes; track(enc, bytes_written) is called after each write"""
    data = support.as_u8(data)
    parts, pos = [], 0
    with pkg.Bzip2Encoder(level, chunk_bytes) as enc:
        for w in (writes if writes is not None else [data.size]):
            enc.write(data[pos: pos + w])
            pos += w
            if track:
                track(enc, pos)
            while enc.pending:
                parts.append(enc.read(read_max))
        assert pos == data.size
        enc.finish()
        enc.finish()
        while enc.pending:
            parts.append(enc.read(read_max))
        assert enc.read().size == 0
    return np.concatenate(parts) if parts else np.empty(0, np.uint8)


def _small_cases():
    g = support.load_golden("golden_small.json")
    return [c for c in g["cases"] if c["algo"] == "Bzip2"]


@pytest.mark.parametrize("case", _small_cases(), ids=lambda c: "%s-%d" % (c["name"], c["level"]))
def test_small_goldens_in_several_steps(pkg, case):
    data = recipes.build(case["recipe"])
    chunk = 300000 if case["level"] < 5 else 500000       # multi-block cases take several steps
    seed = int(hashlib.sha256(("%s-%d" % (case["name"], case["level"])).encode()).hexdigest()[:8], 16)
    out = encode(pkg, data, case["level"], chunk, _splits(data.size, seed, 400000), read_max=70001)
    assert out.size == case["out_len"] and support.sha256(out) == case["out_sha256"]


def _norun(n, seed=0):
    return ((np.arange(n, dtype=np.int64) * 7 + seed) & 255).astype(np.uint8)


def _edge_inputs(level):
    from test_enc_stream_host import _run_mix
    cap = level * 100000 - 19
    return {
        "zeros_12m": (np.zeros(12000000, np.uint8), 1 << 20, None),            # no complete block for many steps; the buffer grows
        "run_mix": (_run_mix(3000000, 5), 400000, None),
        "q2_probe": (np.concatenate([_norun(cap - 4), np.full(300, 0x55, np.uint8), _norun(5000, 3)]), 200000, None),
        "one_full_block": (_norun(cap), 150000, None),
        "two_full_blocks": (_norun(2 * cap), 150000, None),
        "empty": (np.empty(0, np.uint8), 1 << 20, None),
        "one_byte": (np.array([0x42], np.uint8), 1 << 20, None),
        "bytewise_300k": (recipes.textgen(300000, 11), 100000, [1] * 300000),
    }


@pytest.mark.parametrize("level", [1, 9])
@pytest.mark.parametrize("name", ["zeros_12m", "run_mix", "q2_probe", "one_full_block", "two_full_blocks", "empty", "one_byte", "bytewise_300k"])
def test_edge_inputs_against_the_oracle(pkg, oracle, name, level):
    data, chunk, writes = _edge_inputs(level)[name]
    if writes is None:
        writes = _splits(data.size, level * 100 + len(name), 700000)
    rc, want = oracle.bzip2_compress(data, level)
    assert rc == 0
    out = encode(pkg, data, level, chunk, writes)
    assert out.size == want.size and np.array_equal(out, want)


@pytest.mark.parametrize("level", list(range(1, 10)))
def test_every_level(pkg, oracle, level):
    data = recipes.textgen(2500000, 21)
    rc, want = oracle.bzip2_compress(data, level)
    assert rc == 0
    out = encode(pkg, data, level, 600000, _splits(data.size, level, 900000), read_max=99991)
    assert out.size == want.size and np.array_equal(out, want)


def test_100m_golden_in_bounded_memory(pkg):
    import torch
    case = support.load_golden("golden_big_bzip2_9_100m.json")["cases"][0]
    data = recipes.build(case["recipe"])
    chunk = 16 << 20

    def in_use():
        free, total = torch.cuda.mem_get_info()
        return total - free

    in_use()
    used, pend = {}, []
    h = hashlib.sha256()
    n_out = pos = 0
    with pkg.Bzip2Encoder(9, chunk) as enc:
        piece = 4 << 20
        while pos < data.size:
            enc.write(data[pos: pos + piece])
            pos += piece
            # write() puts bytes only into a free staging chunk, and the worker frees the one that chunk 6 (counted from 1) goes to
            # when step 4 begins: once a write that reaches into chunk 6 has returned, steps 1..3 are done
            if pos == 5 * chunk + piece:
                used[3] = in_use()
            pend.append(enc.pending)
            while enc.pending:                       # read in 1 MiB pieces between the writes
                p = enc.read(1 << 20)
                assert 0 < p.size <= 1 << 20
                h.update(p.tobytes())
                n_out += p.size
        enc.finish()                                 # 100 MB in 16 MiB chunks: step 6 is the last one
        used[6] = in_use()
        at_finish = enc.pending
        while enc.pending:
            p = enc.read(1 << 20)
            h.update(p.tobytes())
            n_out += p.size
    print("device bytes in use after steps 3 / 6: %r; largest pending after a write %d B, after finish %d B" % (used, max(pend), at_finish))
    assert n_out == case["out_len"] and h.hexdigest() == case["out_sha256"]
    assert set(used) == {3, 6} and used[3] == used[6]
    # drained after each write: never more than one step's output, however far the worker lags behind the writes (the worker puts
    # a step's bytes into the queue only when it is empty or the caller waits for the worker).  A step takes at most one chunk
    # and the carried block's input (under 2 x 900,000 bytes of this text); the golden gives the ratio of the whole stream; 10 %
    # for the spread between blocks
    ratio = case["out_len"] / data.size
    step_out = 1.1 * ratio * (chunk + 1800000)
    assert max(pend) <= step_out
    # finish is no write: it returns when the whole stream can be read, and that is the output of every step still under way,
    # which the two staging chunks keep to four: the step whose bytes are still coming down, the chunk in work, the chunk staged
    # behind it, and the final one
    assert at_finish <= 4 * step_out


@pytest.mark.slow
def test_1gib_golden_with_the_default_chunk(pkg):
    case = support.load_golden("golden_big_bzip2_9_1g.json")["cases"][0]
    data = recipes.build(case["recipe"])
    h = hashlib.sha256()
    n_out = 0
    with pkg.Bzip2Encoder(9) as enc:
        for pos in range(0, data.size, 32 << 20):
            enc.write(data[pos: pos + (32 << 20)])
            while enc.pending:
                p = enc.read(8 << 20)
                h.update(p.tobytes())
                n_out += p.size
        enc.finish()
        while enc.pending:
            p = enc.read(8 << 20)
            h.update(p.tobytes())
            n_out += p.size
    assert n_out == case["out_len"] and h.hexdigest() == case["out_sha256"]


def test_two_encoders_on_two_threads_beside_one_shot_calls(pkg, oracle):
    datas = [recipes.textgen(4000000, 31), np.concatenate([recipes.textgen(1500000, 32), np.zeros(2000000, np.uint8), recipes.textgen(700000, 33)])]
    levels = [9, 2]
    wants = [oracle.bzip2_compress(d, lv)[1] for d, lv in zip(datas, levels)]
    other = recipes.textgen(1200000, 34)
    want_other = oracle.bzip2_compress(other, 5)[1]
    outs, errs = [None, None], []
    gate = threading.Barrier(3)

    def run(k):
        try:
            gate.wait()
            outs[k] = encode(pkg, datas[k], levels[k], 500000, _splits(datas[k].size, 40 + k, 300000), read_max=50000)
        except Exception as e:      # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    gate.wait()
    mids = [pkg.Bzip2.compressFile(other, None, 5) for _ in range(2)]       # the cached context of the one-shot path, meanwhile
    for t in th:
        t.join()
    assert not errs, errs
    for k in range(2):
        assert np.array_equal(outs[k], wants[k]), k
    for m in mids:
        assert np.array_equal(m, want_other)


def test_python_generator(pkg, oracle):
    data = recipes.textgen(1800000, 41)
    cuts = [0, 1, 70000, 70000, 900000, 1234567, data.size]
    chunks = [bytes(data[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    pieces = list(pkg.Bzip2.compressStream(iter(chunks), 3, chunk_bytes=400000))
    assert len(pieces) > 1
    got = np.concatenate(pieces)
    one = pkg.Bzip2.compressFile(data, None, 3)
    rc, want = oracle.bzip2_compress(data, 3)
    assert rc == 0 and np.array_equal(one, want) and np.array_equal(got, want)


NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_front_streams_in_and_out():
    g = support.load_golden("golden_small.json")
    case = [c for c in g["cases"] if c["algo"] == "Bzip2" and c["name"] == "sample5" and c["level"] == 9][0]
    src = os.path.join(recipes.DATA, "sample5.ref")
    script = r"""
      const fs = require('fs'), crypto = require('crypto');
      const m = require(process.argv[1]);
      const data = fs.readFileSync(process.argv[2]);
      const sha = (b) => crypto.createHash('sha256').update(Buffer.from(b)).digest('hex');
      const r = {};
      let pos = 0, reads = 0;
      const inS = { readByte: function () { reads++; return pos < data.length ? data[pos++] : -1; } };
      const chunks = [];
      const outS = { writeByte: function (b) { chunks.push(b); } };
      try { m.Bzip2.compressFile(inS, outS, 0); } catch (e) { r.level0 = e.message; }
      r.reads_before_throw = reads;
      r.returned = m.Bzip2.compressFile(inS, outS, 9) === outS;
      r.stream = sha(Uint8Array.from(chunks)); r.stream_len = chunks.length;
      const b = m.Bzip2.compressFile(data, null, 9);
      r.buffer = sha(b); r.buffer_len = b.length;
      let p2 = 0;
      const inR = { readByte: function () { return p2 < data.length ? data[p2++] : -1; },
                    read: function (buf, off, len) { const n = Math.min(len, data.length - p2, 300001); data.copy(Buffer.from(buf.buffer, buf.byteOffset + off, n), 0, p2, p2 + n); p2 += n; return n; } };
      const c = m.Bzip2.compressFile(inR);
      r.read_api = sha(c);
      console.log(JSON.stringify(r));
    """
    env = dict(os.environ, CJS_ENC_CHUNK_BYTES="700000")
    out = subprocess.run([NODE, "-e", script, os.path.join(ROOT, "compressjs-flattened_amd", "js", "index.js"), src],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["level0"] == "Invalid block size multiplier" and r["reads_before_throw"] == 0
    assert r["returned"] is True
    assert r["stream_len"] == case["out_len"] and r["stream"] == case["out_sha256"]
    assert r["buffer_len"] == case["out_len"] and r["buffer"] == case["out_sha256"]
    assert r["read_api"] == case["out_sha256"]


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_cli_streams_file_and_pipe():
    g = support.load_golden("golden_small.json")
    case = [c for c in g["cases"] if c["algo"] == "Bzip2" and c["name"] == "sample5" and c["level"] == 9][0]
    cli = os.path.join(ROOT, "compressjs-flattened_amd", "js", "cli.js")
    src = os.path.join(recipes.DATA, "sample5.ref")
    tmp = tempfile.mkdtemp()
    dst = os.path.join(tmp, "out.bz2")
    env = dict(os.environ, CJS_DEBUG="1", CJS_ENC_CHUNK_BYTES="700000")
    o = subprocess.run([NODE, cli, "-z", "-t", "bzip2", "-9", src, dst], capture_output=True, timeout=600, env=env)
    assert o.returncode == 0, o.stderr[-2000:]
    got = np.fromfile(dst, dtype=np.uint8)
    assert got.size == case["out_len"] and support.sha256(got) == case["out_sha256"]
    steps = [ln for ln in o.stderr.decode().splitlines() if ln.startswith("[cjs] enc step ")]
    assert len(steps) > 1, o.stderr[-2000:]                   # one line per step; the input is larger than the chunk
    with open(src, "rb") as f:
        o = subprocess.run([NODE, cli, "-z", "-t", "bzip2", "-9"], stdin=subprocess.PIPE if False else f, capture_output=True, timeout=600)
    assert o.returncode == 0, o.stderr[-2000:]
    with open(src, "rb") as f:
        p = subprocess.run("cat | %s %s -z -t bzip2 -9" % (NODE, cli), shell=True, stdin=f, capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    for res in (o, p):
        b = np.frombuffer(res.stdout, dtype=np.uint8)
        assert b.size == case["out_len"] and support.sha256(b) == case["out_sha256"]
