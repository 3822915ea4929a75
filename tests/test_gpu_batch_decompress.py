"""Batched Bzip2 decompression on the GPU (cjs_bzip2_decompress_batch, Bzip2.decompressFiles): every input of a batch gets
exactly what cjs_bzip2_decompress gives it alone -- the same code, the same bytes, the same detail text -- whatever its
neighbours hold, across groups, budgets and threads."""
import ctypes
import json
import os
import random
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest

import recipes
import support

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8p = ctypes.POINTER(ctypes.c_uint8)
S = ctypes.c_size_t


def _pkg():
    import importlib
    sys.path.insert(0, ROOT)
    return importlib.import_module("compressjs-flattened_amd")


def _lib():
    L = ctypes.CDLL(_pkg().LIB_PATH)
    L.cjs_bzip2_decompress_batch.argtypes = [ctypes.POINTER(u8p), ctypes.POINTER(S), S, ctypes.c_int, ctypes.POINTER(u8p),
                                             ctypes.POINTER(S), ctypes.POINTER(S), ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p]
    L.cjs_bzip2_decompress.argtypes = [u8p, S, ctypes.c_int, ctypes.POINTER(u8p), ctypes.POINTER(S), ctypes.c_void_p]
    L.cjs_last_error_detail.restype = ctypes.c_char_p
    L.cjs_free.argtypes = [ctypes.c_void_p]
    L.cjs_free.restype = None
    return L


def _u8(x):
    return np.frombuffer(x, dtype=np.uint8).copy() if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=np.uint8)


def batch(L, inputs, multi=0):
    """-> (rc, [(status, bytes)], detail)"""
    arrs = [_u8(x) for x in inputs]
    cnt = len(arrs)
    ptrs = (u8p * max(cnt, 1))(*[a.ctypes.data_as(u8p) if a.size else u8p() for a in arrs])
    lens = (S * max(cnt, 1))(*[a.size for a in arrs])
    off, ln, st = (S * max(cnt, 1))(), (S * max(cnt, 1))(), (ctypes.c_int32 * max(cnt, 1))()
    out = u8p()
    rc = L.cjs_bzip2_decompress_batch(ptrs, lens, cnt, multi, ctypes.byref(out), off, ln, st, None)
    detail = L.cjs_last_error_detail().decode()
    res = []
    if rc == 0:
        for k in range(cnt):
            assert k == 0 or off[k] >= off[k - 1]
            assert st[k] == 0 or ln[k] == 0
            res.append((st[k], ctypes.string_at(ctypes.addressof(out.contents) + off[k], ln[k]) if ln[k] else b""))
        L.cjs_free(out)
    return rc, res, detail


def single(L, data, multi=0):
    a = _u8(data)
    keep = a if a.size else np.zeros(1, np.uint8)
    out, n = u8p(), S(0)
    rc = L.cjs_bzip2_decompress(keep.ctypes.data_as(u8p), a.size, multi, ctypes.byref(out), ctypes.byref(n), None)
    detail = L.cjs_last_error_detail().decode()
    b = ctypes.string_at(out, n.value) if rc == 0 and n.value else b""
    if rc == 0:
        L.cjs_free(out)
    return rc, b, detail


def damaged_mixture(oracle, seed):
    """>= 120 damaged streams (as in test_bzip2_decompress_fuzz_matches_oracle) interleaved with good ones"""
    rng = np.random.default_rng(seed)
    data = np.concatenate([recipes.textgen(120000, 31), np.zeros(3000, np.uint8), rng.integers(0, 256, 20000, dtype=np.uint8)])
    small = [recipes.textgen(int(rng.integers(1, 3000)), 100 + i) for i in range(8)]
    out = []
    for level in (1, 9):
        rc, good = oracle.bzip2_compress(data, level)
        assert rc == 0
        for trial in range(64):
            bad = good.copy()
            for _ in range(int(rng.integers(1, 4))):
                bad[int(rng.integers(0, bad.size))] ^= 1 << int(rng.integers(0, 8))
            if trial % 10 == 9:
                bad = bad[: int(rng.integers(8, bad.size))]
            out.append(bad)
            if trial % 4 == 0:
                rc, g = oracle.bzip2_compress(small[trial % 8], level)
                out.append(g)
    return out


def check_parity(L, oracle, inputs, multi):
    rc, res, _ = batch(L, inputs, multi)
    assert rc == 0
    for k, x in enumerate(inputs):
        rc1, b1, _ = single(L, x, multi)
        rco, bo = oracle.bzip2_decompress(x, multi)
        assert res[k][0] == rc1 == rco, (k, res[k][0], rc1, rco)
        if rc1 == 0:
            assert res[k][1] == b1 == bo.tobytes(), k


@pytest.fixture(scope="module")
def L():
    return _lib()


def test_round_trip_golden_small_shuffled(L):
    pkg = _pkg()
    cases = [c for c in support.load_golden("golden_small.json")["cases"] if c["algo"] == "Bzip2"]
    items = [(recipes.build(c["recipe"]), c["level"]) for c in cases]
    assert sorted({lv for _, lv in items}) == [1, 2, 5, 9]
    streams = []
    for lv in (1, 2, 5, 9):
        sel = [d for d, l in items if l == lv]
        streams += list(zip(sel, pkg.Bzip2.compressFiles(sel, lv)))
    random.Random(5).shuffle(streams)
    streams = streams + streams[::3]
    outs = pkg.Bzip2.decompressFiles([s for _, s in streams])
    assert len(outs) == len(streams)
    for (d, _), o in zip(streams, outs):
        assert np.array_equal(o, d)


def test_samples_one_batch(L):
    pkg = _pkg()
    names = ["sample%d" % i for i in range(5)]
    data = os.path.join(ROOT, "tests", "golden", "data")
    ins = [np.fromfile(os.path.join(data, n + ".bz2"), dtype=np.uint8) for n in names]
    outs = pkg.Bzip2.decompressFiles(ins)
    for n, o in zip(names, outs):
        assert np.array_equal(o, np.fromfile(os.path.join(data, n + ".ref"), dtype=np.uint8)), n


@pytest.mark.parametrize("multi", [0, 1])
def test_parity_input_by_input(L, oracle, multi):
    check_parity(L, oracle, damaged_mixture(oracle, 7 + multi), multi)


def _bad_cases(oracle):
    text = recipes.textgen(60000, 3)
    rc, good = oracle.bzip2_compress(text, 9)
    g = good.copy()
    bad_block_crc = g.copy(); bad_block_crc[10] ^= 0x01              # stored block CRC (bytes 10..13)
    bad_stream_crc = g.copy(); bad_stream_crc[-2] ^= 0x10
    # origPointer beyond the block: the 24 bits behind the CRC and the randomised bit
    oob = g.copy()
    bits = np.unpackbits(oob)
    bits[32 + 48 + 32 + 1: 32 + 48 + 32 + 1 + 24] = 1
    oob = np.packbits(bits)
    return {"bad magic": _u8(b"BZx9" + bytes(g[4:])), "level out of range": _u8(b"BZh0" + bytes(g[4:])),
            "block crc": bad_block_crc, "stream crc": bad_stream_crc, "initial position": oob}, g


def test_detail_text_of_single_bad_input(L, oracle):
    bad, g = _bad_cases(oracle)
    rng = np.random.default_rng(3)
    goods = [oracle.bzip2_compress(recipes.textgen(int(rng.integers(10, 5000)), 50 + i), 9)[1] for i in range(4)]
    for name, b in bad.items():
        rc1, _, d1 = single(L, b)
        assert rc1 != 0, name
        if name == "initial position":
            assert d1 == "initial position out of bounds"
        for where in ("first", "middle", "last"):
            ins = [b] + goods if where == "first" else goods[:2] + [b] + goods[2:] if where == "middle" else goods + [b]
            rc, res, d = batch(L, ins)
            k = {"first": 0, "middle": 2, "last": len(goods)}[where]
            assert rc == 0 and res[k][0] == rc1 and d == d1, (name, where, res[k][0], rc1, d, d1)
            assert all(s == 0 for i, (s, _) in enumerate(res) if i != k)


def _expect_single(L, ins, multi=0):
    """every input: the single call's code and bytes; the batch's detail: the single call's detail of the lowest failing input"""
    rc, res, d = batch(L, ins, multi)
    assert rc == 0
    want_detail = None
    for k, x in enumerate(ins):
        rc1, b1, d1 = single(L, x, multi)
        assert res[k][0] == rc1 and res[k][1] == b1, (k, res[k][0], rc1)
        if rc1 and want_detail is None:
            want_detail = d1
    assert d == (want_detail or ""), (d, want_detail)
    return res


def _split(L, oracle, full, cut, multi=0):
    """input = full[:cut], its neighbour = full[cut:] (cut % 4 == 0: in the batch's upload the neighbour's bytes follow at once,
    so the group holds `full` unbroken).  The oracle fails the input alone and decodes `full`: an input that read its
    neighbour's bytes instead of zeros past its end would come back decoded."""
    assert cut % 4 == 0
    head, rest = full[:cut], full[cut:]
    rc_alone, _ = oracle.bzip2_decompress(head, multi)
    rc_joined, want = oracle.bzip2_decompress(full, multi)
    assert rc_alone != 0 and rc_joined == 0
    res = _expect_single(L, [head, rest, head], multi)
    assert res[0][0] == rc_alone and res[2][0] == rc_alone
    rc, res2, _ = batch(L, [full, head], multi)                      # (and the whole stream in front of it still decodes)
    assert rc == 0 and res2[0] == (0, want.tobytes()) and res2[1][0] == rc_alone


def test_no_leakage_between_neighbours(L, oracle):
    rng = np.random.default_rng(11)
    _, s9 = oracle.bzip2_compress(recipes.textgen(400000, 9), 9)
    _, s1 = oracle.bzip2_compress(recipes.textgen(150000, 12), 1)
    _, small = oracle.bzip2_compress(recipes.textgen(3000, 4), 9)
    # truncated inside a block's Huffman data (level 9: the first block; level 1: inside the stream)
    _split(L, oracle, s9, (s9.size // 2) & ~3)
    _split(L, oracle, s1, (s1.size // 3) & ~3)
    # cut inside the end-of-stream marker / stream CRC
    _split(L, oracle, small, (small.size - 2) & ~3)
    # multistream: cut inside the second member's first block magic
    two = np.concatenate([small, s1])
    _split(L, oracle, two, (small.size + 5 + 3) & ~3, 1)
    # the issue's shapes: truncated Huffman data before a large random input; a cut stream CRC before a 0xff-led input
    big_random = rng.integers(0, 256, 3 << 20, dtype=np.uint8)
    _expect_single(L, [s9[:4000], big_random])
    _expect_single(L, [small[:-2], _u8(b"\xff" + bytes(range(1, 200)))])
    # multistream: a valid stream, then BZh9 and 3 bytes of the block magic; the next input starts with the other 3
    head = _u8(bytes(small) + b"BZh9" + bytes([0x31, 0x41, 0x59]))
    tail = _u8(bytes([0x26, 0x53, 0x59]) + bytes(small[10:]))
    _expect_single(L, [head, tail], 1)
    # non-multistream input with a second stream appended: ignored
    _expect_single(L, [_u8(bytes(small) + bytes(small)), small], 0)
    empty14 = oracle.bzip2_compress(np.zeros(0, np.uint8), 9)[1]
    assert empty14.size == 14
    for multi in (0, 1):
        _expect_single(L, [b"", b"BZh", b"BZh0", empty14, small, b"", empty14], multi)


def test_several_failing_inputs_lowest_index_wins(L, oracle):
    pkg = _pkg()
    bad, _ = _bad_cases(oracle)
    goods = [oracle.bzip2_compress(recipes.textgen(2000 + 300 * i, 90 + i), 9)[1] for i in range(3)]
    for first, second in (("stream crc", "bad magic"), ("block crc", "initial position"), ("level out of range", "stream crc")):
        ins = [goods[0], bad[first], goods[1], bad[second], goods[2]]
        _expect_single(L, ins)
        with pytest.raises(pkg.CjsError) as e_single:
            pkg.Bzip2.decompressFile(bad[first])
        with pytest.raises(pkg.CjsError) as e_batch:
            pkg.Bzip2.decompressFiles(ins)
        assert str(e_batch.value) == str(e_single.value), (first, str(e_batch.value), str(e_single.value))
        assert e_batch.value.errorCode == e_single.value.errorCode and e_batch.value.index == 1
    # reversed order: the other input is the lowest failing one
    ins = [goods[0], bad["bad magic"], bad["stream crc"]]
    with pytest.raises(pkg.CjsError) as e_batch:
        pkg.Bzip2.decompressFiles(ins)
    assert e_batch.value.index == 1 and "bad magic" in str(e_batch.value)


def _debug_child(code, env_extra):
    env = dict(os.environ, CJS_DEBUG="1", **env_extra)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout, [l for l in r.stderr.splitlines() if l.startswith("[cjs dec batch]")]


_SCALE = r"""
import sys, numpy as np
sys.path.insert(0, "tests"); sys.path.insert(0, ".")
import importlib, recipes
pkg = importlib.import_module("compressjs-flattened_amd")
rng = np.random.default_rng(1)
xs = [recipes.textgen(int(rng.integers(1, 301)), 1000 + i) for i in range(20000)]
for lv in (9, 1):
    ss = pkg.Bzip2.compressFiles(xs, lv)
    outs = pkg.Bzip2.decompressFiles(ss)
    assert all(np.array_equal(a, b) for a, b in zip(xs, outs)), lv
print("ok")
"""


def test_scale_20000_tiny_streams():
    out, lines = _debug_child(_SCALE, {})
    assert out.strip().endswith("ok")
    assert len(lines) == 2, lines                                    # one group per level
    for l in lines:
        assert "20000 inputs" in l and " 1 inverse-BWT batches" in l, l


def test_level_change_between_members(L, oracle):
    parts = []
    for i, lv in enumerate((1, 9, 3, 9, 2)):
        parts.append(oracle.bzip2_compress(recipes.textgen(150000 + 1000 * i, 70 + i), lv)[1])
    ms = _u8(b"".join(bytes(p) for p in parts))
    ms2 = _u8(b"".join(bytes(p) for p in parts[2:]))
    rc, res, _ = batch(L, [ms, parts[0], ms2], 1)
    assert rc == 0
    for k, x in enumerate([ms, parts[0], ms2]):
        rco, bo = oracle.bzip2_decompress(x, 1)
        assert rco == 0 and res[k] == (0, bo.tobytes())


_SHRUNK = r"""
import sys, numpy as np
sys.path.insert(0, "tests"); sys.path.insert(0, ".")
import support, test_gpu_batch_decompress as t
L = t._lib(); o = support.Oracle()
rng = np.random.default_rng(4)
_, big = o.bzip2_compress(rng.integers(0, 256, 300000, dtype=np.uint8), 1)      # larger than a group: the single-stream path
bad_big = big.copy(); bad_big[5000] ^= 4
for multi in (0, 1):
    t.check_parity(L, o, t.damaged_mixture(o, 21 + multi) + [big, bad_big, big[:1000]], multi)
print("ok")
"""


def test_shrunk_budgets_and_groups():
    out, lines = _debug_child(_SHRUNK, {"CJS_DEC_ROW_BYTES": str(60 << 20), "CJS_DEC_BATCH_ELEMS": str(300000),
                                        "CJS_DEC_GROUP_BYTES": str(200000)})
    assert out.strip().endswith("ok")
    assert len(lines) > 2, lines                                      # several groups


def test_threads_match_single_thread(L, oracle):
    rng = np.random.default_rng(5)
    batches = []
    for t in range(4):
        xs = [recipes.textgen(int(rng.integers(1, 40000)), 300 + 50 * t + i) for i in range(40)]
        batches.append([oracle.bzip2_compress(x, 1 + 2 * t)[1] for x in xs])
    batches[2][5] = batches[2][5][:100]
    big = oracle.bzip2_compress(recipes.textgen(2000000, 77), 9)[1]
    want = [batch(L, b) for b in batches]
    want_big = single(L, big)
    got = [None] * 4
    got_big = []

    def run(i):
        for _ in range(3):
            got[i] = batch(L, batches[i])

    def run_big():
        for _ in range(3):
            got_big.append(single(L, big))
    ths = [threading.Thread(target=run, args=(i,)) for i in range(4)] + [threading.Thread(target=run_big)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    for i in range(4):
        assert got[i][0] == 0 and got[i][1] == want[i][1], i
    assert all(g[:2] == want_big[:2] for g in got_big)


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_front_under_node(oracle):
    addon = os.path.join(ROOT, "compressjs-flattened_amd", "js", "cjs_napi.node")
    if not os.path.exists(addon):
        pytest.skip("N-API addon not built")
    script = r"""
      const m = require(process.argv[1]);
      const xs = [];
      for (let i = 0; i < 50; i++) { const a = new Uint8Array(1 + i * 37); for (let j = 0; j < a.length; j++) a[j] = (j * 7 + i) % 26 + 97; xs.push(a); }
      const ss = m.Bzip2.compressFiles(xs, 9);
      const outs = m.Bzip2.decompressFiles(ss);
      let same = outs.length === xs.length;
      for (let i = 0; i < xs.length && same; i++) same = Buffer.compare(Buffer.from(outs[i]), Buffer.from(xs[i])) === 0;
      const bad = ss.map((s) => new Uint8Array(s));
      bad[7][bad[7].length - 3] ^= 0x40;
      let single = null, batch = null;
      try { m.Bzip2.decompressFile(bad[7]); } catch (e) { single = {message: e.message, code: e.errorCode}; }
      try { m.Bzip2.decompressFiles(bad); } catch (e) { batch = {message: e.message, code: e.errorCode, index: e.index, type: e.constructor.name}; }
      console.log(JSON.stringify({same, single, batch}));
    """
    r = subprocess.run(["node", "-e", script, os.path.join(ROOT, "compressjs-flattened_amd", "js", "index.js")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["same"] is True
    assert res["single"] is not None and res["batch"]["message"] == res["single"]["message"]
    assert res["batch"]["code"] == res["single"]["code"] and res["batch"]["index"] == 7 and res["batch"]["type"] == "TypeError"
