"""Batched Bzip2 compression on the GPU (cjs_bzip2_compress_batch*, Bzip2.compressFiles): every stream of a batch is
byte-identical to the reference's Bzip2.compressFile of its input -- the golden fixtures, the oracle and the single-stream
entry point -- whatever the mix of sizes, and the device-resident form leaves d_out untouched when the streams do not fit."""
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import recipes
import support

pytestmark = pytest.mark.gpu


def _pkg():
    import importlib
    return importlib.import_module("compressjs-flattened_amd")


def _cap(level):
    return level * 100000 - 19


def _norun(n, seed=0):
    """n bytes without any run of equal bytes: RLE1 output == input"""
    return ((np.arange(n, dtype=np.int64) * 7 + seed) % 251).astype(np.uint8)


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8).copy()


@pytest.fixture(scope="module")
def golden_bzip2():
    cases = [c for c in support.load_golden("golden_small.json")["cases"] if c["algo"] == "Bzip2"]
    assert len(cases) == 64
    return [(c, recipes.build(c["recipe"])) for c in cases]


def test_golden_cases_one_batch_per_level(golden_bzip2):
    pkg = _pkg()
    by_level = {}
    for c, data in golden_bzip2:
        by_level.setdefault(c["level"], []).append((c, data))
    assert sorted(by_level) == [1, 2, 5, 9]
    for level, items in by_level.items():
        outs = pkg.Bzip2.compressFiles([d for _, d in items], level)
        assert len(outs) == len(items)
        for (c, _), o in zip(items, outs):
            assert o.size == c["out_len"] and support.sha256(o) == c["out_sha256"], (c["name"], level)


def test_golden_cases_shuffled_with_duplicates(golden_bzip2):
    pkg = _pkg()
    rng = random.Random(5)
    for level in (1, 2, 5, 9):
        items = [(c, d) for c, d in golden_bzip2 if c["level"] == level]
        order = items + rng.sample(items, min(7, len(items)))
        rng.shuffle(order)
        outs = pkg.Bzip2.compressFiles([d for _, d in order], level)
        for (c, _), o in zip(order, outs):
            assert support.sha256(o) == c["out_sha256"], (c["name"], level)


def _mixture(level, seed):
    """inputs of every kind the batch path tells apart, neighbours chosen so that a run could leak from one into the next"""
    rng = np.random.default_rng(seed)
    cap = _cap(level)
    # runs of 4, 5, 255+ bytes that end at the input's end, each followed by an input that starts with the same byte: kept in
    # this order (outside the shuffle below), so a run that leaked into the next input would change that input's stream
    fixed = [_u8(b"xyz" + b"a" * 4), _u8(b"a" * 9 + b"bcd"), _u8(b"p" * 5), _u8(b"p" * 5), _u8(b"q" * 300), _u8(b"q" * 300 + b"r"),
             _u8(b"r" * 255), _u8(b"r" * 260), _u8(b"rs" * 40), _u8(b"s"), _u8(b"ssss"), _u8(b"s" * 3)]
    ins = [np.empty(0, np.uint8), _u8(b"a"), _u8(b"ab")]
    ins += [_norun(cap), _norun(cap + 1, 3)]                            # RLE1 output fills a block exactly / one byte past it
    ins.append(np.concatenate([_norun(cap - 5, 1), _u8(b"zzzzzz")]))    # block full at the run-length byte, bytes left: two blocks
    ins.append(np.concatenate([_norun(cap - 5, 2), _u8(b"zzzz")]))      # block full at the run-length byte, nothing left: one block
    ins += [np.tile(_u8(b"ab"), 3000), np.tile(_u8(b"abc"), 1001), np.tile(_u8(b"abcd"), 77), _u8(b"z" * 5000),
            np.tile(_u8(b"hello "), 20000)]                             # periodic: equal rotations (Q4)
    for k in range(10):
        n = int(rng.integers(0, 200000)) if k < 7 else int(rng.integers(0, 3000000))
        ins.append(recipes.textgen(n, seed * 100 + k))
    ins.append(recipes.xorshift_bytes(70000, seed, mask=3))           # many short runs
    tail = recipes.textgen(150000, seed)
    ins.append(np.concatenate([_norun(cap - 4, 4), _u8(b"z" * 10), tail]))      # block ends between a 4th 'z' and its run-length byte
    ins.append(np.concatenate([_norun(cap - 5, 5), _u8(b"z" * 9), tail]))       # block full at the run-length byte, the run goes on
    ins.append(np.concatenate([_norun(cap - 2, 6), _u8(b"y" * 600), tail]))     # a run across the block boundary
    perm = rng.permutation(len(ins))
    return fixed + [ins[i] for i in perm]


@pytest.mark.parametrize("level", list(range(1, 10)))
def test_oracle_mixture(level, oracle, hip):
    pkg = _pkg()
    ins = _mixture(level, 11 + level)
    outs = pkg.Bzip2.compressFiles(ins, level)
    assert len(outs) == len(ins)
    for k, (d, o) in enumerate(zip(ins, outs)):
        rc, want = oracle.bzip2_compress(d, level)
        assert rc == 0
        assert np.array_equal(o, want), "input %d (%d bytes) differs from the oracle at level %d" % (k, d.size, level)
        rc, single = hip.bzip2_compress(d, level)
        assert rc == 0 and np.array_equal(o, single), "input %d differs from cjs_bzip2_compress" % k


def test_run_seams_one_batch():
    """The stage-0 seam inputs (recipes.rle_seam_inputs: one run of 3..511 bytes ending at a lane, tile or two-tile border) as ONE
    batch: stream k is compressFile of input k -- the batch kernels' tile carry and their share of the chunk rule."""
    pkg = _pkg()
    cases = sorted(recipes.rle_seam_inputs().items())
    assert len(cases) == 43
    outs = pkg.Bzip2.compressFiles([d for _, d in cases], 1)
    assert len(outs) == len(cases)
    for ((L, E), d), o in zip(cases, outs):
        assert np.array_equal(o, pkg.Bzip2.compressFile(d, None, 1)), "run of %d ending at %d" % (L, E)


def test_scale_many_tiny_and_one_large(oracle, hip):
    pkg = _pkg()
    rng = np.random.default_rng(3)
    ins = []
    for k in range(20000):
        n = int(rng.integers(0, 301))
        ins.append(recipes.textgen(n, 1000 + k) if k % 3 else rng.integers(0, 4, n).astype(np.uint8))
    big = recipes.textgen(10 * 1000 * 1000, 77)
    ins.insert(12345, big)
    outs = pkg.Bzip2.compressFiles(ins, 9)
    assert len(outs) == len(ins)
    for k, (d, o) in enumerate(zip(ins, outs)):
        rc, want = oracle.bzip2_compress(d, 9)
        assert rc == 0 and np.array_equal(o, want), "input %d (%d bytes)" % (k, d.size)
    rc, single = hip.bzip2_compress(big, 9)
    assert rc == 0 and np.array_equal(outs[12345], single)
    # round trip of all streams at once through the existing decoder (multistream)
    rc, back = hip.bzip2_decompress(np.concatenate(outs), 1)
    assert rc == 0 and np.array_equal(back, np.concatenate(ins))


def _passes(script):
    """runs `script` in a child process with CJS_DEBUG set and returns the batch path's pass count line"""
    env = dict(os.environ, CJS_DEBUG="1")
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600, env=env, cwd=support.ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stderr.splitlines() if l.startswith("[cjs batch]")]
    assert len(lines) == 1, out.stderr[-2000:]
    return lines[0]


_PASS_SCRIPT = """
import sys, numpy as np
sys.path.insert(0, "tests"); sys.path.insert(0, ".")
import importlib, recipes
pkg = importlib.import_module("compressjs-flattened_amd")
rng = np.random.default_rng(9)
%s
outs = pkg.Bzip2.compressFiles(ins, %d)
assert len(outs) == len(ins)
"""


def test_tiny_inputs_share_one_pass():
    # 10,000 inputs of 1-300 bytes: every stage runs ONCE over all of them (not once per length class or per input)
    line = _passes(_PASS_SCRIPT % ("ins = [recipes.textgen(int(n), k) for k, n in enumerate(rng.integers(1, 301, 10000))]", 9))
    assert " 1 passes (10000 one-block inputs, 0 blocks of 0 inputs" in line, line


# (the text inputs are slices of ONE generated text: the generator's start-up would cost 20,000 calls a quarter of a minute)
_TINY_40000 = ("text = recipes.textgen(1 << 20, 5); "
               "ins = [text[21 * k: 21 * k + int(n)].copy() if k % 2 else (rng.integers(0, 2, int(n)) + 48).astype(np.uint8) "
               "for k, n in enumerate(rng.integers(1, 41, 40000))]")


def test_more_than_32768_tiny_inputs_share_one_pass(oracle):
    # 40,000 inputs of 1-40 bytes, text and 2-symbol bytes: one pass of 40,000 blocks, so the block id and the hole bit leave the
    # suffix sort's round 1 five symbols of depth (more than 32768 blocks; tests/test_gpu_bwt_var.py has the stage on its own)
    line = _passes(_PASS_SCRIPT % (_TINY_40000, 9))
    assert " 1 passes (40000 one-block inputs, 0 blocks of 0 inputs" in line, line
    scope = {"np": np, "recipes": recipes, "rng": np.random.default_rng(9)}
    exec(_TINY_40000, scope)
    ins = scope["ins"]
    assert len(ins) == 40000 and min(d.size for d in ins) == 1 and max(d.size for d in ins) == 40
    outs = _pkg().Bzip2.compressFiles(ins, 9)
    assert len(outs) == len(ins)
    for k, (d, o) in enumerate(zip(ins, outs)):
        rc, want = oracle.bzip2_compress(d, 9)
        assert rc == 0 and np.array_equal(o, want), "input %d (%d bytes)" % (k, d.size)


def test_multi_block_inputs_are_batched():
    # 24 inputs of 150-400 kB at level 1 (100 kB blocks): their blocks share a few passes (length classes), not one pipeline per input
    line = _passes(_PASS_SCRIPT % ("ins = [recipes.textgen(int(n), k) for k, n in enumerate(rng.integers(150000, 400001, 24))]", 1))
    import re
    m = re.search(r" (\d+) passes \((\d+) one-block inputs, (\d+) blocks of (\d+) inputs", line)
    assert m, line
    passes, one, blocks, multi = (int(x) for x in m.groups())
    assert one == 0 and multi == 24 and blocks >= 48 and passes <= 8, line


def _device_batch(ins):
    import torch
    off = np.zeros(len(ins) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([d.size for d in ins])
    packed = np.concatenate(ins + [np.zeros(1, np.uint8)])
    return torch.from_numpy(packed).to("cuda:0"), off


def test_device_form_output_too_small_leaves_d_out_untouched(oracle):
    import torch
    pkg = _pkg()
    ins = [recipes.textgen(n, 40 + n) for n in (0, 1, 5000, 70000, 300000)] + [_norun(_cap(1) + 10)]
    d_in, off = _device_batch(ins)
    ctx = pkg.DeviceContext.batch(0, int(off[-1]), len(ins), 1)
    try:
        d_out = torch.full((int(off[-1]) * 2 + 4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
        so, sl = ctx.compress_batch(d_in.data_ptr(), off, d_out.data_ptr(), d_out.numel())
        need = int(max(so + sl))
        host = d_out.cpu().numpy()
        for k, d in enumerate(ins):
            assert so[k] % 4 == 0
            rc, want = oracle.bzip2_compress(d, 1)
            assert np.array_equal(host[int(so[k]): int(so[k] + sl[k])], want), k
        sentinel = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(pkg.CjsError) as e:         # one byte short of the end of the last stream
            ctx.compress_batch(d_in.data_ptr(), off, sentinel.data_ptr(), need - 1)
        assert e.value.errorCode == -33
        assert bool((sentinel == 0x5A).all())
        so2, sl2 = ctx.compress_batch(d_in.data_ptr(), off, sentinel.data_ptr(), need)      # exactly the end: fits
        assert np.array_equal(so2, so) and np.array_equal(sl2, sl)
        back = sentinel.cpu().numpy()
        for k in range(len(ins)):
            assert np.array_equal(back[int(so[k]): int(so[k] + sl[k])], host[int(so[k]): int(so[k] + sl[k])]), k
        assert bool((sentinel[need:] == 0x5A).all())
    finally:
        ctx.close()


def test_device_context_reused_across_batch_shapes(oracle):
    import torch
    pkg = _pkg()
    ctx = pkg.DeviceContext.batch(0, 4 << 20, 3000, 5)
    try:
        shapes = [[recipes.textgen(64 * 1024, s) for s in range(40)],
                  [recipes.textgen(int(n), 7 + i) for i, n in enumerate(np.random.default_rng(1).integers(0, 2000, 2500))],
                  [recipes.textgen(1200000, 9), np.empty(0, np.uint8), _u8(b"x")],
                  [recipes.textgen(64 * 1024, s) for s in range(40)]]
        first = None
        for ins in shapes:
            d_in, off = _device_batch(ins)
            d_out = torch.zeros(int(off[-1]) * 2 + 65536, dtype=torch.uint8, device="cuda:0")
            so, sl = ctx.compress_batch(d_in.data_ptr(), off, d_out.data_ptr(), d_out.numel())
            host = d_out.cpu().numpy()
            got = [host[int(so[k]): int(so[k] + sl[k])].copy() for k in range(len(ins))]
            for k, d in enumerate(ins):
                rc, want = oracle.bzip2_compress(d, 5)
                assert rc == 0 and np.array_equal(got[k], want), k
            if first is None:
                first = got
        assert all(np.array_equal(a, b) for a, b in zip(first, got))
    finally:
        ctx.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_front_compress_files_golden(golden_bzip2):
    if not os.path.exists(os.path.join(support.PKG, "js", "cjs_napi.node")):
        pytest.skip("N-API addon not built")
    with tempfile.TemporaryDirectory() as td:
        jobs = {}
        for i, (c, d) in enumerate(golden_bzip2):
            p = os.path.join(td, "in%d" % i)
            d.tofile(p)
            jobs.setdefault(str(c["level"]), []).append(p)
        jf = os.path.join(td, "jobs.json")
        json.dump(jobs, open(jf, "w"))
        script = r"""
          const fs = require('fs'), crypto = require('crypto');
          const m = require(process.argv[1]);
          const jobs = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
          const res = {};
          for (const lv of Object.keys(jobs)) {
            const outs = m.Bzip2.compressFiles(jobs[lv].map(p => fs.readFileSync(p)), Number(lv));
            res[lv] = outs.map(o => (o instanceof Uint8Array ? '' : 'not-u8:') + crypto.createHash('sha256').update(o).digest('hex'));
          }
          console.log(JSON.stringify(res));
        """
        out = subprocess.run(["node", "-e", script, os.path.join(support.PKG, "js", "index.js"), jf], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr
        res = json.loads(out.stdout.strip().splitlines()[-1])
    want = {}
    for c, _ in golden_bzip2:
        want.setdefault(str(c["level"]), []).append(c["out_sha256"])
    assert res == want
