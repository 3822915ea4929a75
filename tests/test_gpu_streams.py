"""Whole-stream parity on the GPU box: larger goldens through the C ABI, the JS fronts under Node, the
device-resident entry points, sharded ranges, and size-independent properties at full size."""
import hashlib
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import recipes
import support

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["golden_big_bzip2_9_10m.json", "golden_big_bzip2_1_10m.json"])
def test_10m_goldens(hip, name):
    case = support.load_golden(name)["cases"][0]
    data = recipes.build(case["recipe"])
    rc, out = hip.bzip2_compress(data, case["level"])
    assert rc == 0
    assert out.size == case["out_len"] and support.sha256(out) == case["out_sha256"]


def test_100m_level1_golden_and_round_trip(hip, oracle):
    # BASELINE.json configs[1]: bzip2 -1 on 100 MB (1001 blocks)
    case = support.load_golden("golden_big_bzip2_1_100m.json")["cases"][0]
    data = recipes.build(case["recipe"])
    rc, out = hip.bzip2_compress(data, 1)
    assert rc == 0
    assert out.size == case["out_len"] and support.sha256(out) == case["out_sha256"]


def test_device_range_assembly_equals_whole_stream(oracle):
    sys.path.insert(0, ROOT)
    import torch
    pkg = importlib.import_module("compressjs-flattened_amd")
    shard = importlib.import_module("compressjs-flattened_amd.shard")
    data = recipes.textgen(3000000, 5)
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(data.copy()).to(dev)
    d_out = torch.zeros(4 << 20, dtype=torch.uint8, device=dev)
    ctx = pkg.DeviceContext(0, data.size, 1, 12)
    _, total, _ = ctx.compress_range(d_in.data_ptr(), data.size, 0, 0, d_out.data_ptr(), d_out.numel())
    parts, crcs_all = [], None
    for first, count in shard.plan_ranges(total, 3):
        bits, _, crcs = ctx.compress_range(d_in.data_ptr(), data.size, first, count, d_out.data_ptr(), d_out.numel())
        parts.append((d_out[: (bits + 7) // 8].cpu().numpy().copy(), bits))
        crcs_all = crcs.copy() if crcs_all is None else np.where(np.arange(total) >= first, crcs, crcs_all)
    ctx.close()
    stream = shard.assemble(1, parts, crcs_all)
    rc, want = oracle.bzip2_compress(data, 1)
    assert rc == 0 and np.array_equal(stream, want)


def test_device_output_too_small_is_refused_without_writing(oracle):
    # the size check of the device-resident entry point runs on the device (huff_offsets): a buffer that cannot hold the
    # stream gives CJS_E_OUTPUT_TOO_SMALL and stays untouched, one that just fits gives the stream
    sys.path.insert(0, ROOT)
    import torch
    pkg = importlib.import_module("compressjs-flattened_amd")
    data = recipes.textgen(700000, 9)
    rc, want = oracle.bzip2_compress(data, 2)
    assert rc == 0
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(data.copy()).to(dev)
    ctx = pkg.DeviceContext(0, data.size, 2)
    d_out = torch.full((want.size + 64,), 0xAB, dtype=torch.uint8, device=dev)
    small = (want.size // 2) & ~3
    with pytest.raises(pkg.CjsError) as e:
        ctx.compress(d_in.data_ptr(), data.size, d_out.data_ptr(), small)
    assert e.value.errorCode == -33
    back = d_out.cpu().numpy()
    assert (back == 0xAB).all()
    st = pkg.Stats()
    ctx.set_stage_times(False)         # events only: no per-stage synchronisation (what bench.py's timed loop uses)
    n = ctx.compress(d_in.data_ptr(), data.size, d_out.data_ptr(), (want.size + 8 + 3) & ~3, st)
    assert n == want.size and np.array_equal(d_out[:n].cpu().numpy(), want)
    assert st.ms_total > 0 and st.ms_bwt == 0 and st.bwt_dominant_launches > 0 and st.blocks == 4
    ctx.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_front_matches_goldens():
    g = support.load_golden("golden_small.json")
    wanted = {(c["name"], c["level"]): c for c in g["cases"] if c["algo"] == "Bzip2"}
    jobs = []
    tmp = tempfile.mkdtemp()
    for (name, level), c in wanted.items():
        if name in ("sample1", "sample3", "textgen_65536_s1", "tiny_banana", "tiny_empty", "zeros_300000", "q2_run_at_block_end"):
            path = os.path.join(tmp, "%s.bin" % name)
            recipes.build(c["recipe"]).tofile(path)
            jobs.append({"name": name, "path": path, "level": level, "algo": "Bzip2"})
    jf = os.path.join(tmp, "jobs.json")
    json.dump(jobs, open(jf, "w"))
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js_front_check.js"), jf], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["devices"] >= 1
    for r in rep["results"]:
        c = wanted[(r["name"], r["level"])]
        assert r["isU8"] and r["len"] == c["out_len"] and r["sha256"] == c["out_sha256"], r
    banana = "425a6839314159265359efb6ec01000001810030012000218f506610bc5dc914e14243bedbb004"
    api = rep["api"]
    assert api["array_input"] == banana and api["buffer_input"] == banana and api["stream_input"] == banana
    assert api["sink_returned"] is True and api["sink_hex"] == banana and api["default_level"] == banana
    assert api["level0"] == "Invalid block size multiplier"
    assert api["short_out"] == "TypeError:outputsize does not match decoded input"


def _bwtc_cases():
    g = support.load_golden("golden_small.json")
    return [c for c in g["cases"] if c["algo"] == "BWTC"]


@pytest.mark.parametrize("case", _bwtc_cases(), ids=lambda c: "%s-%d" % (c["name"], c["level"]))
def test_bwtc_compress_golden(hip, case):
    data = recipes.build(case["recipe"])
    rc, out = hip.bwtc_compress(data, case["level"])
    assert rc == 0, hip.L.cjs_strerror(rc)
    assert out.size == case["out_len"], "length %d want %d" % (out.size, case["out_len"])
    assert support.sha256(out) == case["out_sha256"]


def test_bwtc_10m_golden(hip):
    case = support.load_golden("golden_big_bwtc_9_10m.json")["cases"][0]
    data = recipes.build(case["recipe"])
    rc, out = hip.bwtc_compress(data, 9)
    assert rc == 0 and out.size == case["out_len"] and support.sha256(out) == case["out_sha256"]


@pytest.mark.parametrize("name", ["sample0", "sample1", "sample2", "sample3", "sample4"])
def test_bzip2_decoder_goldens(hip, name):
    # NPM/test/bzip2-basic.js: streams produced by the real bzip2
    comp = np.fromfile(os.path.join(recipes.DATA, name + ".bz2"), dtype=np.uint8)
    ref = np.fromfile(os.path.join(recipes.DATA, name + ".ref"), dtype=np.uint8)
    rc, out = hip.bzip2_decompress(comp)
    assert rc == 0, hip.L.cjs_strerror(rc)
    assert out.size == ref.size and np.array_equal(out, ref)


def _bz_cases():
    g = support.load_golden("golden_small.json")
    return [c for c in g["cases"] if c["algo"] == "Bzip2" and c["level"] in (1, 9)]


@pytest.mark.parametrize("case", _bz_cases(), ids=lambda c: "%s-%d" % (c["name"], c["level"]))
def test_bzip2_decompress_round_trip(hip, oracle, case):
    data = recipes.build(case["recipe"])
    rc, comp = oracle.bzip2_compress(data, case["level"])       # == the reference's stream (pinned)
    assert rc == 0
    rc, out = hip.bzip2_decompress(comp)
    assert rc == 0, hip.L.cjs_strerror(rc)
    assert out.size == data.size and np.array_equal(out, data)


def test_bzip2_decompress_errors_and_multistream(hip, oracle):
    assert hip.bzip2_decompress(b"garbage data here")[0] == -2
    assert hip.bzip2_decompress(b"BZh0")[0] == -2
    comp = np.fromfile(os.path.join(recipes.DATA, "sample1.bz2"), dtype=np.uint8).copy()
    comp[2000] ^= 0x10
    assert hip.bzip2_decompress(comp)[0] == -5
    a = oracle.bzip2_compress(b"first stream ", 1)[1]
    b = oracle.bzip2_compress(b"second stream", 1)[1]
    both = np.concatenate([a, b])
    assert hip.bzip2_decompress(both, 0)[1].tobytes() == b"first stream "
    assert hip.bzip2_decompress(both, 1)[1].tobytes() == b"first stream second stream"


def test_bzip2_decompress_fuzz_matches_oracle(hip, oracle):
    # damaged streams: the GPU decoder must come back (no hang, no fault) with the reference's verdict -- same code, and the
    # same bytes where the damage happens to leave a decodable stream (the oracle is pinned on the reference's error cases)
    rng = np.random.default_rng(2024)
    data = np.concatenate([recipes.textgen(250000, 31), np.zeros(3000, np.uint8), rng.integers(0, 256, 20000, dtype=np.uint8)])
    for level in (1, 9):
        rc, good = oracle.bzip2_compress(data, level)
        assert rc == 0
        for trial in range(60):
            bad = good.copy()
            for _ in range(int(rng.integers(1, 4))):
                bad[int(rng.integers(0, bad.size))] ^= 1 << int(rng.integers(0, 8))
            if trial % 10 == 9:
                bad = bad[: int(rng.integers(8, bad.size))]
            rc_o, out_o = oracle.bzip2_decompress(bad, trial & 1)
            rc_h, out_h = hip.bzip2_decompress(bad, trial & 1)
            assert rc_h == rc_o, (level, trial, rc_h, rc_o)
            if rc_o == 0:
                assert np.array_equal(out_h, out_o), (level, trial)


def test_bzip2_decompress_10m(hip, oracle):
    data = recipes.textgen(10000000, 1)
    rc, comp = hip.bzip2_compress(data, 9)
    assert rc == 0
    rc, out = hip.bzip2_decompress(comp)
    assert rc == 0 and np.array_equal(out, data)


@pytest.mark.parametrize("name", ["sample0", "sample1", "sample2", "sample3", "sample4"])
def test_bzip2_table_goldens(hip, name):
    # NPM/test/bzip2-table.js
    comp = np.fromfile(os.path.join(recipes.DATA, name + ".bz2"), dtype=np.uint8)
    rc, table = hip.bzip2_table(comp)
    assert rc == 0
    text = "".join("%d\t%d\n" % (p, s) for p, s in table)
    assert text == open(os.path.join(recipes.DATA, name + ".bzt")).read()


@pytest.mark.parametrize("name,bitpos", [("sample0", 32), ("sample2", 544888), ("sample4", 32), ("sample4", 1596228), ("sample4", 2342106)])
def test_bzip2_decompress_block_goldens(hip, oracle, name, bitpos):
    # NPM/test/bzip2-block.js
    comp = np.fromfile(os.path.join(recipes.DATA, name + ".bz2"), dtype=np.uint8)
    rc, out = hip.bzip2_decompress_block(comp, bitpos)
    assert rc == 0
    if name == "sample0":
        assert out.tobytes() == b"This is a test\n"
    else:
        ref = np.fromfile(os.path.join(recipes.DATA, "%s.%d" % (name, bitpos)), dtype=np.uint8)
        assert np.array_equal(out, ref)


@pytest.mark.parametrize("case", [c for c in _bwtc_cases() if c["level"] in (1, 9)], ids=lambda c: "%s-%d" % (c["name"], c["level"]))
def test_bwtc_decompress_round_trip(hip, oracle, case):
    data = recipes.build(case["recipe"])
    rc, comp = oracle.bwtc_compress(data, case["level"])       # == the reference's stream (pinned by the goldens)
    assert rc == 0 and support.sha256(comp) == case["out_sha256"]
    rc, out = hip.bwtc_decompress(comp)
    assert rc == 0, hip.L.cjs_strerror(rc)
    assert out.size == data.size and np.array_equal(out, data)


def test_bwtc_errors(hip):
    assert hip.bwtc_decompress(b"nope, not bwtc")[0] == -21


def test_multi_device_host_path_equals_single(hip, oracle, monkeypatch):
    # CJS_DEVICES=3: three worker shards (all on GPU 0 here), each packs at its final bit offset, fragments land in place == the single stream
    data = recipes.textgen(1500000, 9)
    rc, want = oracle.bzip2_compress(data, 1)
    monkeypatch.setenv("CJS_DEVICES", "3")
    rc, out = hip.bzip2_compress(data, 1)
    monkeypatch.delenv("CJS_DEVICES")
    assert rc == 0 and np.array_equal(out, want)


def _mixed_input(seed):
    """text, binary noise, low-entropy noise, long runs and periodic stretches in one stream (sizes from the seed)"""
    rng = np.random.RandomState(seed)
    parts = []
    for _ in range(int(rng.randint(3, 9))):
        kind = int(rng.randint(0, 6))
        n = int(rng.randint(1, 400000))
        if kind == 0:
            parts.append(recipes.textgen(n, int(rng.randint(1, 1 << 30))))
        elif kind == 1:
            parts.append(rng.randint(0, 256, n).astype(np.uint8))
        elif kind == 2:
            parts.append((rng.randint(0, 4, n) + 97).astype(np.uint8))
        elif kind == 3:
            parts.append(np.full(int(rng.randint(1, 3000)), int(rng.randint(0, 256)), dtype=np.uint8))
        elif kind == 4:
            unit = rng.randint(0, 256, int(rng.randint(1, 40))).astype(np.uint8)
            parts.append(np.tile(unit, n // len(unit) + 1)[:n])
        else:
            page = recipes.textgen(int(rng.randint(50, 3000)), int(rng.randint(1, 1 << 30)))
            parts.append(np.tile(page, int(rng.randint(2, 60))))
    return np.concatenate(parts)


@pytest.mark.parametrize("seed", range(12))
def test_mixed_content_vs_oracle(hip, oracle, seed):
    # random mixtures, random level: Bzip2 and BWTC streams equal the oracle's, and both decoders give the input back
    data = _mixed_input(1000 + seed)
    level = 1 + (seed * 5) % 9
    rc, want = oracle.bzip2_compress(data, level)
    rc2, got = hip.bzip2_compress(data, level)
    assert rc == 0 and rc2 == 0 and np.array_equal(got, want), "bzip2 level %d, %d bytes" % (level, data.size)
    rc3, back = hip.bzip2_decompress(got)
    assert rc3 == 0 and np.array_equal(back, data)
    rc, want = oracle.bwtc_compress(data, level)
    rc2, got = hip.bwtc_compress(data, level)
    assert rc == 0 and rc2 == 0 and np.array_equal(got, want), "bwtc level %d, %d bytes" % (level, data.size)
    rc3, back = hip.bwtc_decompress(got)
    assert rc3 == 0 and np.array_equal(back, data)


def test_cached_workspace_across_calls(hip, oracle):
    # cjs_bzip2_compress keeps its per-device workspace: growing / shrinking inputs, a level change, cjs_trim in between
    seq = [(300000, 9, 21), (2500000, 9, 22), (1000, 9, 23), (700000, 1, 24), (0, 1, 25), (1200000, 5, 26)]
    for i, (n, level, seed) in enumerate(seq):
        data = recipes.textgen(n, seed) if n else np.empty(0, dtype=np.uint8)
        rc, want = oracle.bzip2_compress(data, level)
        rc2, out = hip.bzip2_compress(data, level)
        assert rc == 0 and rc2 == 0 and np.array_equal(out, want), "call %d (n=%d level=%d)" % (i, n, level)
        if i == 2:
            hip.L.cjs_trim()
    hip.L.cjs_trim()
    rc2, out = hip.bzip2_compress(recipes.textgen(50000, 27), 9)
    assert rc2 == 0 and np.array_equal(out, oracle.bzip2_compress(recipes.textgen(50000, 27), 9)[1])


def test_chunked_large_input_path_is_bit_exact(oracle):
    # inputs above CJS_CHUNK_BYTES are compressed as block ranges one after the other (bounded workspace) and stitched
    # on the host: forced here with a tiny threshold (the variable is read once per process, hence the subprocess)
    data = recipes.textgen(3000000, 12)
    rc, want = oracle.bzip2_compress(data, 2)
    import subprocess, sys as _sys
    code = ("import sys; sys.path.insert(0, 'tests'); import torch, support, recipes, numpy as np; "
            "d = recipes.textgen(3000000, 12); rc, out = support.HipLib().bzip2_compress(d, 2); "
            "print(rc, support.sha256(out))")
    env = dict(os.environ, CJS_CHUNK_BYTES="500000")
    out = subprocess.run([_sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr[-1500:]
    rc_s, sha = out.stdout.split()
    assert rc == 0 and rc_s == "0" and sha == support.sha256(want)


@pytest.mark.parametrize("expr,level", [("recipes.textgen(1200000, 14)", 1), ("recipes.textgen(1200000, 14)", 9),
                                        ("np.full(1200000, 0x61, dtype=np.uint8)", 1)], ids=["text-1", "text-9", "one-byte-1"])
def test_waves_of_two_ranges_and_empty_ranges_are_bit_exact(oracle, expr, level):
    # CJS_CHUNK_BYTES=500000 cuts 1,200,000 bytes into five ranges, CJS_DEVICES=2 runs them two at a time (waves of 2, 2, 1), the
    # host stitches their bit strings.  Level 1: ~12 blocks over the five ranges; level 9: 2 blocks, so three ranges have no block
    # and add 0 bits to the stitch; one repeated byte: blocks of a few hundred bits, the stitch is mostly shared edge bytes.
    data = eval(expr)
    rc, want = oracle.bzip2_compress(data, level)
    code = ("import sys; sys.path.insert(0, 'tests'); import torch, support, recipes, numpy as np; "
            "d = %s; rc, out = support.HipLib().bzip2_compress(d, %d); print(rc, support.sha256(out))" % (expr, level))
    env = dict(os.environ, CJS_CHUNK_BYTES="500000", CJS_DEVICES="2")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr[-1500:]
    rc_s, sha = out.stdout.split()
    assert rc == 0 and rc_s == "0" and sha == support.sha256(want)


@pytest.mark.parametrize("n", [50000, 250000])
def test_more_shards_than_blocks_all_at_once(hip, oracle, monkeypatch, n):
    # CJS_DEVICES=5 on one block and on three: the shards without blocks publish empty metas and write nothing, the last shard
    # WITH blocks ends the stream (trailer and combined CRC)
    data = recipes.textgen(n, 15)
    rc, want = oracle.bzip2_compress(data, 1)
    monkeypatch.setenv("CJS_DEVICES", "5")
    rc2, out = hip.bzip2_compress(data, 1)
    monkeypatch.delenv("CJS_DEVICES")
    assert rc == 0 and rc2 == 0 and np.array_equal(out, want)


def _run_variant(env, n, seed, level):
    """HipLib().bzip2_compress in a fresh process under `env` (the toggles are read once per process) -> (rc, sha256)"""
    import subprocess, sys as _sys
    code = ("import sys; sys.path.insert(0, 'tests'); import torch, support, recipes, numpy as np; "
            "d = recipes.textgen(%d, %d); rc, out = support.HipLib().bzip2_compress(d, %d); "
            "print(rc, support.sha256(out))" % (n, seed, level))
    out = subprocess.run([_sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env), cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr[-1500:]
    rc_s, sha = out.stdout.split()
    return int(rc_s), sha


@pytest.mark.parametrize("env", [{}, {"CJS_NO_SEGMENTED_SORT": "1"}], ids=["default", "unsegmented-fallback"])
def test_suffix_sort_paths_are_bit_exact(oracle, env):
    # the paths the sorter picks by itself, each in a fresh process: packed two-phase round 1 with the two-sweep regroup (>= 8
    # blocks) and without (3 blocks), both tile sorters (radix while groups are large, counting / bitonic later), the Huffman
    # refinement as one kernel per block (< 8 blocks or < 8 MB) and as a chain of kernels (10 level-9 blocks); and the fallback
    # for inputs of more segments than the workspace was carved for (keys materialised, one plain radix sort; forced here)
    cases = [(2500000, 4, 9), (1200000, 6, 1), (9100000, 8, 9)]
    for n, seed, level in cases:
        rc, want = oracle.bzip2_compress(recipes.textgen(n, seed), level)
        rc_v, sha = _run_variant(env, n, seed, level)
        assert rc == 0 and rc_v == 0 and sha == support.sha256(want), (env, n, level)


def test_bwtc_100m_golden(hip):
    # BASELINE.json configs[3] at 100 MB: BWTC -9, golden cut by the reference JS
    case = support.load_golden("golden_big_bwtc_9_100m.json")["cases"][0]
    data = recipes.build(case["recipe"])
    rc, out = hip.bwtc_compress(data, 9)
    assert rc == 0, hip.L.cjs_strerror(rc)
    assert out.size == case["out_len"] and support.sha256(out) == case["out_sha256"]


def test_bzip2_100m_compress_golden_then_decompress(hip):
    # BASELINE.json configs[4] at 100 MB: the reference-identical -9 stream decompressed on the GPU gives the input back
    case = support.load_golden("golden_big_bzip2_9_100m.json")["cases"][0]
    data = recipes.build(case["recipe"])
    rc, comp = hip.bzip2_compress(data, 9)
    assert rc == 0 and comp.size == case["out_len"] and support.sha256(comp) == case["out_sha256"]
    rc, back = hip.bzip2_decompress(comp)
    assert rc == 0, hip.L.cjs_strerror(rc)
    assert back.size == data.size and support.sha256(back) == case["in_sha256"]
    rc, tab = hip.bzip2_table(comp)
    assert rc == 0 and len(tab) == 112 and sum(sz for _, sz in tab) == data.size


def test_sharded_decompress_equals_single(hip, oracle, monkeypatch):
    # CJS_DEVICES=3: three byte-range shares (all on GPU 0 here), each scans / decodes the candidates that start in its
    # share; chain walk and offsets on the host.  Level 9 (few big blocks per share), level 1 (many) and a mixed multistream.
    m = support.load_golden("golden_api.json")["mixed_level_multistream"]
    cases = []
    for n, seed, level in ((10000000, 1, 9), (4000000, 3, 1)):
        d = recipes.textgen(n, seed)
        rc, comp = hip.bzip2_compress(d, level)
        assert rc == 0
        cases.append((comp, d, 0))
    parts = [recipes.build(p["recipe"]) for p in m["parts"]]
    cat = np.concatenate([hip.bzip2_compress(d, p["level"])[1] for d, p in zip(parts, m["parts"])])
    cases.append((cat, np.concatenate(parts), 1))
    for ndev in ("2", "3", "5"):
        monkeypatch.setenv("CJS_DEVICES", ndev)
        for comp, want, multi in cases:
            rc, out = hip.bzip2_decompress(comp, multi)
            assert rc == 0, (ndev, hip.L.cjs_strerror(rc))
            assert out.size == want.size and np.array_equal(out, want), ndev
        # a damaged block in the middle share is reported with the reference's code
        bad = cases[0][0].copy()
        bad[bad.size // 2] ^= 0x40
        assert hip.bzip2_decompress(bad)[0] in (-5, -2)
        monkeypatch.delenv("CJS_DEVICES")


def test_sharded_bwtc_compress_equals_golden(hip, monkeypatch):
    # CJS_DEVICES=3: three device slots (all GPU 0 here) produce the step lists of their block ranges, the single host coder
    # consumes them in block order; output == the reference's stream
    case = support.load_golden("golden_big_bwtc_9_10m.json")["cases"][0]
    data = recipes.build(case["recipe"])
    for ndev in ("2", "3"):
        monkeypatch.setenv("CJS_DEVICES", ndev)
        rc, out = hip.bwtc_compress(data, 9)
        monkeypatch.delenv("CJS_DEVICES")
        assert rc == 0 and out.size == case["out_len"] and support.sha256(out) == case["out_sha256"], ndev
    # small first batch / single batch give the same stream too, and so does the one-thread form of the range coder (the
    # default runs the range chain and the low chain on two host threads)
    for env in ({"CJS_BWTC_FIRST_BATCH": "0"}, {"CJS_BWTC_FIRST_BATCH": "1"}, {"CJS_BWTC_FIRST_BATCH": "3"}, {"CJS_BWTC_SPLIT_CODER": "0"}):
        import subprocess, sys as _sys
        code = ("import sys; sys.path.insert(0, 'tests'); import torch, support, recipes; "
                "d = recipes.textgen(10000000, 1); rc, out = support.HipLib().bwtc_compress(d, 9); print(rc, support.sha256(out))")
        o = subprocess.run([_sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env), cwd=ROOT, timeout=300)
        assert o.returncode == 0 and o.stdout.split() == ["0", case["out_sha256"]], (env, o.stderr[-800:])


def test_multistream_with_more_than_65535_blocks(hip, oracle):
    # many tiny concatenated streams: the per-block kernels run in slabs of 65535 blocks
    one = oracle.bzip2_compress(b"x", 1)[1]
    two = oracle.bzip2_compress(b"yz", 1)[1]
    reps = 35000
    cat = np.concatenate([np.tile(np.concatenate([one, two]), reps)])
    rc, out = hip.bzip2_decompress(cat, 1)
    assert rc == 0, hip.L.cjs_strerror(rc)
    assert out.size == 3 * reps and out.tobytes() == b"xyz" * reps
    hip.L.cjs_trim()


def test_many_tiny_members_under_level9_headers(hip, oracle):
    # 70,000 member streams that announce level 9: a scratch row is sized for a 900 kB block whatever the member holds, so the
    # block decode runs in row batches under a byte budget (a row per candidate at once would be ~440 GB here; the reference
    # decodes the file trivially).  With several batches each batch's decoded bytes are packed and the rows reused.
    one = oracle.bzip2_compress(b"x", 9)[1]
    two = oracle.bzip2_compress(b"yz", 9)[1]
    reps = 35000
    cat = np.tile(np.concatenate([one, two]), reps)
    rc, out = hip.bzip2_decompress(cat, 1)
    assert rc == 0, hip.L.cjs_strerror(rc)
    assert out.size == 3 * reps and out.tobytes() == b"xyz" * reps
    rc, tab = hip.bzip2_table(cat, 1, cap=2 * reps + 8)
    assert rc == 0 and len(tab) == 2 * reps
    hip.L.cjs_trim()


def test_decode_row_batches_match_the_single_batch(oracle):
    # the same file decoded with room for all rows at once and with room for two rows per batch (CJS_DEC_ROW_BYTES): text blocks
    # of three levels, a damaged block (error reported as before) and a table listing
    code = ("import sys; sys.path.insert(0, 'tests'); import torch, support, recipes, numpy as np; h = support.HipLib(); o = support.Oracle(); "
            "parts = [recipes.textgen(2600000, 3), recipes.textgen(950000, 4), recipes.textgen(400000, 5)]; "
            "cat = np.concatenate([o.bzip2_compress(d, l)[1] for d, l in zip(parts, (9, 3, 1))]); "
            "rc, out = h.bzip2_decompress(cat, 1); rc2, tab = h.bzip2_table(cat, 1); "
            "bad = cat.copy(); bad[bad.size // 3] ^= 0x10; rc3, _ = h.bzip2_decompress(bad, 1); "
            "print(rc, support.sha256(out), support.sha256(np.concatenate(parts)), rc2, len(tab), rc3, h.last_error_detail().split(' (')[0])")
    res = []
    # ... and with the inverse BWT in batches of <= 1,000,000 / 2,000,000 elements (CJS_DEC_BATCH_ELEMS): batches of one block, of
    # blocks of one size (one segmented radix pass) and of mixed sizes (the block number sorted on too)
    for env in ({}, {"CJS_DEC_ROW_BYTES": str(14 * 900000)}, {"CJS_DEC_BATCH_ELEMS": "1000000"}, {"CJS_DEC_BATCH_ELEMS": "2000000"}):
        o = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env), cwd=ROOT, timeout=300)
        assert o.returncode == 0, o.stderr[-1500:]
        res.append(o.stdout.split())
    assert all(r == res[0] for r in res[1:]), res
    assert res[0][0] == "0" and res[0][1] == res[0][2] and res[0][3] == "0" and res[0][5] in ("-5", "-2")


def test_bwtc_decompress_negative_inputs(hip, oracle):
    # truncated / bit-flipped streams (DefSum model at level 1, Fenwick model at level 9): an error code or different
    # bytes, never a crash; a stream of thousands of empty blocks decodes to nothing
    data = recipes.textgen(400000, 13)
    for level in (1, 9):
        rc, comp = oracle.bwtc_compress(data, level)
        assert rc == 0
        assert np.array_equal(hip.bwtc_decompress(comp)[1], data)
        for cut in (comp.size - 5, comp.size // 2, 9):
            rc, out = hip.bwtc_decompress(comp[:cut])
            assert rc != 0 or not np.array_equal(out, data)
        rng = np.random.default_rng(level)
        for _ in range(8):
            bad = comp.copy()
            bad[int(rng.integers(8, comp.size - 8))] ^= 1 << int(rng.integers(0, 8))
            rc, out = hip.bwtc_decompress(bad)
            assert rc in (0, -5)
    from test_host_logic import _forged_empty_blocks
    rc, out = hip.bwtc_decompress(_forged_empty_blocks(60000))
    assert rc == 0 and out.size == 0


@pytest.mark.slow
def test_1gib_goldens_compress_and_decompress(hip):
    # BASELINE.json north_star / configs[3] / configs[4] at full size: bit-identical .bz2 and .bwtc on the 1 GiB
    # enwik8-shaped input (goldens cut by the reference JS), and the .bz2 decompressed on the GPU gives the input back
    case = support.load_golden("golden_big_bzip2_9_1g.json")["cases"][0]
    data = recipes.build(case["recipe"])
    assert support.sha256(data) == case["in_sha256"]
    rc, comp = hip.bzip2_compress(data, 9)
    assert rc == 0, hip.L.cjs_strerror(rc)
    assert comp.size == case["out_len"] and support.sha256(comp) == case["out_sha256"]
    hip.L.cjs_trim()
    rc, back = hip.bzip2_decompress(comp)
    assert rc == 0, hip.L.cjs_strerror(rc)
    assert back.size == data.size and support.sha256(back) == case["in_sha256"]
    del back, comp
    hip.L.cjs_trim()
    wcase = support.load_golden("golden_big_bwtc_9_1g.json")["cases"][0]
    rc, out = hip.bwtc_compress(data, 9)
    assert rc == 0, hip.L.cjs_strerror(rc)
    assert out.size == wcase["out_len"] and support.sha256(out) == wcase["out_sha256"]


@pytest.mark.slow
def test_bzip2_round_trip_above_4gib(hip):
    # every size_t path end to end: compress takes block ranges one after the other (CJS_CHUNK_BYTES), decompress takes
    # batches of blocks; 4910 blocks x 3516 tiles is also more workgroups x threads than one launch may carry (2^32), so
    # the decoder's stage kernels must go in slabs.
    n = (1 << 32) + 123456789
    data = recipes.textgen(n, 1)
    want = support.sha256(data)
    rc, comp = hip.bzip2_compress(data, 9)
    assert rc == 0, hip.L.cjs_strerror(rc)
    hip.L.cjs_trim()
    rc, back = hip.bzip2_decompress(comp)
    assert rc == 0, (hip.L.cjs_strerror(rc), hip.last_error_detail())
    assert back.size == n and support.sha256(back) == want


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_cli_round_trips_a_reference_fixture(oracle):
    # js/cli.js over the two fronts (NPM/bin/compressjs:7-25,60-120,175): file -> file and stdin -> stdout, both algorithms;
    # a file input knows its size, a pipe does not (BWTC then writes varint(0), like the reference for a stream without .size)
    cli = os.path.join(ROOT, "compressjs-flattened_amd", "js", "cli.js")
    src = os.path.join(ROOT, "tests", "golden", "data", "sample1.ref")
    data = np.fromfile(src, dtype=np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        for t, level in (("bzip2", 9), ("bwtc", 5), ("bzip", 1)):
            comp, back = os.path.join(tmp, "c." + t), os.path.join(tmp, "b." + t)
            r = subprocess.run(["node", cli, "-z", "-t", t, "-%d" % level, src, comp], capture_output=True, timeout=120)
            assert r.returncode == 0, r.stderr
            got = np.fromfile(comp, dtype=np.uint8)
            rc, want = (oracle.bwtc_compress if t == "bwtc" else oracle.bzip2_compress)(data, level)
            assert rc == 0 and np.array_equal(got, want), t
            r = subprocess.run(["node", cli, "-d", "-t", t, comp, back], capture_output=True, timeout=120)
            assert r.returncode == 0, r.stderr
            assert np.array_equal(np.fromfile(back, dtype=np.uint8), data), t
        # pipes; default level 7
        r = subprocess.run(["node", cli, "-z", "-t", "bzip2"], input=data.tobytes(), capture_output=True, timeout=120)
        assert r.returncode == 0 and np.array_equal(np.frombuffer(r.stdout, dtype=np.uint8), oracle.bzip2_compress(data, 7)[1])
        r2 = subprocess.run(["node", cli, "-d", "-t", "bzip2"], input=r.stdout, capture_output=True, timeout=120)
        assert r2.returncode == 0 and r2.stdout == data.tobytes()
        w = subprocess.run(["node", cli, "-z", "-t", "bwtc", "-9"], input=data.tobytes(), capture_output=True, timeout=120)
        assert w.returncode == 0 and w.stdout[:5] == b"bwtc\x80"                      # size unknown: varint(0)
        w2 = subprocess.run(["node", cli, "-d", "-t", "bwtc"], input=w.stdout, capture_output=True, timeout=120)
        assert w2.returncode == 0 and w2.stdout == data.tobytes()
        # one block by bit position (Bzip2.decompressBlock): the first block starts at bit 32
        comp = os.path.join(tmp, "c.bzip2")
        b = subprocess.run(["node", cli, "-d", "-t", "bzip2", "-b", "32", comp], capture_output=True, timeout=120)
        assert b.returncode == 0 and b.stdout == data.tobytes()                        # sample1 at level 9 is one block
        bad = subprocess.run(["node", cli, "-d", "-t", "bzip2"], input=b"not a bzip2 file at all", capture_output=True, timeout=120)
        assert bad.returncode == 1 and b"Not bzip data" in bad.stderr
