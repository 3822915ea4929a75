"""Device-resident Bzip2 decompression on the GPU (cjs_bzip2_decompress_device, decompress_device): for the same bytes the device
call gives exactly what the host-buffer cjs_bzip2_decompress gives -- code, bytes, detail text -- writes nothing at or past the
bound it owns, reads nothing past the input, refuses host memory, and moves only metadata across PCIe."""
import ctypes
import os
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
    L.cjs_bzip2_decompress.argtypes = [u8p, S, ctypes.c_int, ctypes.POINTER(u8p), ctypes.POINTER(S), ctypes.c_void_p]
    L.cjs_bzip2_decompress_device.argtypes = [ctypes.c_void_p, S, ctypes.c_int, ctypes.c_void_p, S, ctypes.POINTER(S), ctypes.c_void_p]
    L.cjs_last_error_detail.restype = ctypes.c_char_p
    L.cjs_free.argtypes = [ctypes.c_void_p]
    L.cjs_free.restype = None
    return L


def _u8(x):
    return np.frombuffer(x, dtype=np.uint8).copy() if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=np.uint8)


def host(L, data, multi=0):
    a = _u8(data)
    keep = a if a.size else np.zeros(1, np.uint8)
    out, n = u8p(), S(0)
    rc = L.cjs_bzip2_decompress(keep.ctypes.data_as(u8p), a.size, multi, ctypes.byref(out), ctypes.byref(n), None)
    detail = L.cjs_last_error_detail().decode()
    b = ctypes.string_at(out, n.value) if rc == 0 and n.value else b""
    if rc == 0:
        L.cjs_free(out)
    return rc, b, detail


def device(L, data, multi=0, in_shift=0, out_shift=0, tail=b"", cap=None):
    """-> (rc, bytes, detail, out_n, the whole output tensor, out_shift): d_in at byte in_shift of a tensor, `tail` behind the
    input's n bytes; d_out at byte out_shift of a 0xA5-filled tensor with `cap` bytes for the call"""
    import torch
    a = _u8(data)
    buf = torch.from_numpy(np.concatenate([np.zeros(in_shift, np.uint8), a, _u8(tail), np.zeros(1, np.uint8)])).cuda()
    if cap is None:
        cap = 3 * a.size + (1 << 16)
    out = torch.full((cap + out_shift + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = S(0)
    rc = L.cjs_bzip2_decompress_device(buf.data_ptr() + in_shift, a.size, multi, out.data_ptr() + out_shift, cap, ctypes.byref(n), None)
    detail = L.cjs_last_error_detail().decode()
    got = out[out_shift: out_shift + n.value].cpu().numpy().tobytes() if rc == 0 else b""
    return rc, got, detail, n.value, out, out_shift


def same_as_host(L, data, multi=0, **kw):
    want = host(L, data, multi)
    # (room for whatever a damaged stream decodes to before its verdict: a size above the capacity is -33 first, by contract)
    got = device(L, data, multi, cap=max(len(want[1]), 8 * len(data)) + 65536, **kw)
    assert got[:3] == want, (got[0], want[0], got[2], want[2])
    return got


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


def _bad_cases(oracle):
    text = recipes.textgen(60000, 3)
    rc, good = oracle.bzip2_compress(text, 9)
    g = good.copy()
    bad_block_crc = g.copy(); bad_block_crc[10] ^= 0x01              # stored block CRC (bytes 10..13)
    bad_stream_crc = g.copy(); bad_stream_crc[-2] ^= 0x10
    oob = g.copy()                                                    # origPointer beyond the block
    bits = np.unpackbits(oob)
    bits[32 + 48 + 32 + 1: 32 + 48 + 32 + 1 + 24] = 1
    oob = np.packbits(bits)
    return {"bad magic": _u8(b"BZx9" + bytes(g[4:])), "level out of range": _u8(b"BZh0" + bytes(g[4:])),
            "block crc": bad_block_crc, "stream crc": bad_stream_crc, "initial position": oob}, g


@pytest.fixture(scope="module")
def L():
    return _lib()


def test_golden_round_trips(L):
    pkg = _pkg()
    cases = [c for c in support.load_golden("golden_small.json")["cases"] if c["algo"] == "Bzip2"]
    assert len(cases) == 64
    for c in cases:
        d = recipes.build(c["recipe"])
        s = pkg.Bzip2.compressFiles([d], c["level"])[0]
        rc, got, _, n, _, _ = device(L, s, cap=d.size)
        assert rc == 0 and n == d.size and got == d.tobytes(), c["name"]
    data = os.path.join(ROOT, "tests", "golden", "data")
    for i in range(5):
        s = np.fromfile(os.path.join(data, "sample%d.bz2" % i), dtype=np.uint8)
        ref = np.fromfile(os.path.join(data, "sample%d.ref" % i), dtype=np.uint8)
        rc, got, _, _, _, _ = device(L, s, cap=ref.size)
        assert rc == 0 and got == ref.tobytes(), i


@pytest.mark.parametrize("multi", [0, 1])
def test_parity_on_damaged_input(L, oracle, multi):
    bad, _ = _bad_cases(oracle)
    inputs = damaged_mixture(oracle, 7 + multi) + list(bad.values())
    codes = []
    for k, x in enumerate(inputs):
        rc, b, d, _, _, _ = same_as_host(L, x, multi)
        rco, bo = oracle.bzip2_decompress(x, multi)
        assert rc == rco, (k, rc, rco)
        if rc == 0:
            assert b == bo.tobytes(), k
        codes.append(rc)
    assert codes.count(0) >= 25 and sum(1 for c in codes if c) >= 100, codes
    assert {0, -2, -5} <= set(codes), sorted(set(codes))
    assert same_as_host(L, bad["initial position"], multi)[2] == "initial position out of bounds"


def test_multistream(L, oracle):
    parts = [oracle.bzip2_compress(recipes.textgen(150000 + 1000 * i, 70 + i), lv)[1] for i, lv in enumerate((1, 9, 3))]
    ms = _u8(b"".join(bytes(p) for p in parts))
    for x in (ms, _u8(bytes(ms) + b"trailing garbage"), _u8(bytes(ms) + b"BZh9" + bytes(20))):
        for multi in (0, 1):
            same_as_host(L, x, multi)
    rc, got, _, _, _, _ = device(L, ms, 1)
    assert rc == 0 and got == oracle.bzip2_decompress(ms, 1)[1].tobytes()


def test_output_bounds(L, oracle):
    import torch
    pkg = _pkg()
    text = recipes.textgen(700000, 21)
    s = _u8(oracle.bzip2_compress(text, 1)[1])
    need = text.size
    d_in = torch.from_numpy(s).cuda()
    # the size query
    with pytest.raises(pkg.CjsError) as e:
        pkg.decompress_device(d_in.data_ptr(), s.size, 0, 0)
    assert e.value.errorCode == -33 and e.value.need == need
    # one byte short: -33 with need, every byte untouched
    rc, _, _, n, out, _ = device(L, s, cap=need - 1)
    assert rc == -33 and n == need and bool((out == 0xA5).all())
    # exactly enough: the bytes, nothing behind them
    rc, got, _, n, out, sh = device(L, s, cap=need, out_shift=3)
    assert rc == 0 and got == text.tobytes() and bool((out[sh + need:] == 0xA5).all()) and bool((out[:sh] == 0xA5).all())
    # bad stream CRC: all untouched; bad block CRC: untouched at and past need
    bad, g = _bad_cases(oracle)
    rc, _, d, _, out, _ = device(L, bad["stream crc"])
    assert rc == -5 and d.startswith("Bad stream CRC") and bool((out == 0xA5).all())
    rc, _, d, _, out, _ = device(L, bad["block crc"], out_shift=1)
    assert rc == -5 and d.startswith("Bad block CRC") and bool((out[1 + 60000:] == 0xA5).all()) and int(out[0]) == 0xA5


def test_alignment_and_isolation(L, oracle):
    rng = np.random.default_rng(9)
    text = recipes.textgen(300000, 5)
    s = _u8(oracle.bzip2_compress(text, 9)[1])
    other = _u8(oracle.bzip2_compress(recipes.textgen(5000, 6), 3)[1])
    cut = s[: s.size - 7]                                            # a truncated stream: what lies behind it must not matter
    for shift in (0, 1, 2, 3):
        for tail in (bytes(other), rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()):
            for x in (s, cut):
                for multi in (0, 1):
                    same_as_host(L, x, multi, in_shift=shift, tail=tail, out_shift=(1, 3)[shift & 1])


def test_pinned_memory_is_refused(L, oracle):
    import torch
    s = _u8(oracle.bzip2_compress(recipes.textgen(10000, 2), 9)[1])
    pinned = torch.from_numpy(s).pin_memory()
    out = torch.zeros(20000, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = S(0)
    assert L.cjs_bzip2_decompress_device(pinned.data_ptr(), s.size, 0, out.data_ptr(), out.numel(), ctypes.byref(n), None) == -32
    d_in = torch.from_numpy(s).cuda()
    pout = torch.zeros(20000, dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()
    assert L.cjs_bzip2_decompress_device(d_in.data_ptr(), s.size, 0, pout.data_ptr(), pout.numel(), ctypes.byref(n), None) == -32


_NO_HOST_COPY = r"""
import sys, hashlib, numpy as np, torch
sys.path.insert(0, "tests"); sys.path.insert(0, ".")
import torch; torch.zeros(1, device="cuda")      # (CUDA up in torch before the library's first call)
import importlib, recipes, support
pkg = importlib.import_module("compressjs-flattened_amd")
g = support.load_golden("golden_big_bzip2_9_100m.json")["cases"][0]
data = recipes.build(g["recipe"])
d_in = torch.from_numpy(data).cuda()
d_s = torch.empty(data.size // 2 + (1 << 20), dtype=torch.uint8, device="cuda")
ctx = pkg.DeviceContext(0, data.size, 9)
m = ctx.compress(d_in.data_ptr(), data.size, d_s.data_ptr(), d_s.numel())
ctx.close()
assert m == g["out_len"] and hashlib.sha256(d_s[:m].cpu().numpy().tobytes()).hexdigest() == g["out_sha256"]
d_out = torch.empty(data.size, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
n = pkg.decompress_device(d_s.data_ptr(), m, d_out.data_ptr(), d_out.numel())
assert n == data.size and torch.equal(d_out, d_in)
print("ok")
"""


def test_no_host_copy_100m():
    env = dict(os.environ, CJS_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", _NO_HOST_COPY], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().endswith("ok")
    lines = [l for l in r.stderr.splitlines() if l.startswith("[cjs dec dev]")]
    assert len(lines) == 1, lines
    w = lines[0].split()
    h2d, d2h, cands = int(w[w.index("H2D") + 1]), int(w[w.index("D2H") + 1]), int(w[w.index("candidates") + 1])
    print(lines[0])
    assert h2d + d2h <= 64 * 1024 + 1024 * cands, lines[0]


def test_threads(L, oracle):
    streams = [(_u8(oracle.bzip2_compress(recipes.textgen(20000 + 7000 * t, 400 + t), 1 + 2 * t)[1]), t) for t in range(4)]
    want = [host(L, s) for s, _ in streams]
    errors = []

    def run(i):
        try:
            for j in range(20):
                got = device(L, streams[i][0], 0, in_shift=j & 3, out_shift=(j >> 2) & 3)
                if got[:3] != want[i]:
                    errors.append((i, j, got[0]))
        except Exception as e:                                       # (reported below: an exception in a thread is not a failure)
            errors.append((i, repr(e)))
    ths = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors, errors[:5]


# ---------------------------------------------------------------- batch (cjs_bzip2_decompress_batch_device)
def _blib(L):
    PS = ctypes.POINTER(S)
    L.cjs_bzip2_decompress_batch.argtypes = [ctypes.POINTER(u8p), PS, S, ctypes.c_int, ctypes.POINTER(u8p), PS, PS, ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p]
    L.cjs_bzip2_decompress_batch_device.argtypes = [ctypes.c_void_p, PS, S, ctypes.c_int, ctypes.c_void_p, S, PS, PS, ctypes.POINTER(ctypes.c_int32), PS,
                                                    ctypes.c_void_p]
    return L


def host_batch(L, inputs, multi=0):
    """-> (rc, [(status, off, len, bytes)], detail)"""
    arrs = [_u8(x) for x in inputs]
    cnt = len(arrs)
    ptrs = (u8p * cnt)(*[a.ctypes.data_as(u8p) if a.size else u8p() for a in arrs])
    lens = (S * cnt)(*[a.size for a in arrs])
    off, ln, st = (S * cnt)(), (S * cnt)(), (ctypes.c_int32 * cnt)()
    out = u8p()
    rc = _blib(L).cjs_bzip2_decompress_batch(ptrs, lens, cnt, multi, ctypes.byref(out), off, ln, st, None)
    detail = L.cjs_last_error_detail().decode()
    res = []
    if rc == 0:
        base = ctypes.addressof(out.contents) if out else 0
        res = [(st[k], off[k], ln[k], ctypes.string_at(base + off[k], ln[k]) if ln[k] else b"") for k in range(cnt)]
        L.cjs_free(out)
    return rc, res, detail


def device_batch(L, inputs, multi=0, cap=None, shift=1):
    """-> (rc, [(status, off, len, bytes)], detail, need, the 0xA5-filled output tensor): the inputs packed back to back in one
    device buffer from byte `shift` on"""
    import torch
    arrs = [_u8(x) for x in inputs]
    cnt = len(arrs)
    offs = np.zeros(cnt + 1, np.uint64)
    offs[1:] = np.cumsum([a.size for a in arrs]) + shift
    offs[0] = shift
    buf = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8)] + arrs + [np.zeros(1, np.uint8)])).cuda()
    if cap is None:
        cap = 8 * int(offs[-1]) + (1 << 16)
    out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    io = (S * (cnt + 1))(*[int(x) for x in offs])
    off, ln, st, need = (S * cnt)(), (S * cnt)(), (ctypes.c_int32 * cnt)(), S(0)
    rc = _blib(L).cjs_bzip2_decompress_batch_device(buf.data_ptr(), io, cnt, multi, out.data_ptr(), cap, off, ln, st, ctypes.byref(need), None)
    detail = L.cjs_last_error_detail().decode()
    res = []
    if rc == 0:
        host_out = out[: need.value].cpu().numpy().tobytes()
        res = [(st[k], off[k], ln[k], host_out[off[k]: off[k] + ln[k]]) for k in range(cnt)]
    return rc, res, detail, need.value, out


def batch_parity(L, inputs, multi=0):
    rc_h, want, d_h = host_batch(L, inputs, multi)
    rc, got, d, need, out = device_batch(L, inputs, multi)
    assert rc == rc_h == 0
    for k in range(len(inputs)):
        assert got[k] == want[k], (k, got[k][:3], want[k][:3])
    assert d == d_h, (d, d_h)
    assert need >= max([o + n for _, o, n, _ in want] + [0])
    assert bool((out[need:] == 0xA5).all())
    return got


def test_batch_parity(L, oracle):
    import random
    pkg = _pkg()
    cases = [c for c in support.load_golden("golden_small.json")["cases"] if c["algo"] == "Bzip2"]
    goldens = []
    for lv in (1, 2, 5, 9):
        sel = [recipes.build(c["recipe"]) for c in cases if c["level"] == lv]
        goldens += pkg.Bzip2.compressFiles(sel, lv)
    bad, _ = _bad_cases(oracle)
    for multi in (0, 1):
        ins = list(goldens) + goldens[::3] + [b"", b"", b"BZh"] + damaged_mixture(oracle, 7 + multi) + list(bad.values())
        random.Random(3 + multi).shuffle(ins)
        got = batch_parity(L, ins, multi)
        codes = [g[0] for g in got]
        assert {0, -2, -5} <= set(codes)


def test_batch_output_bounds(L, oracle):
    pkg = _pkg()
    ins = [oracle.bzip2_compress(recipes.textgen(30000 + 1000 * i, 60 + i), 9)[1] for i in range(5)]
    rc, _, _, need, _ = device_batch(L, ins)
    assert rc == 0 and need == sum(30000 + 1000 * i for i in range(5))
    rc, _, _, need2, out = device_batch(L, ins, cap=need - 1)
    assert rc == -33 and need2 == need and bool((out == 0xA5).all())
    rc, got, _, _, out = device_batch(L, ins, cap=need)
    assert rc == 0 and bool((out[need:] == 0xA5).all())
    for i, g in enumerate(got):
        assert g[0] == 0 and g[3] == recipes.textgen(30000 + 1000 * i, 60 + i).tobytes()
    import torch
    d = torch.from_numpy(np.concatenate([_u8(x) for x in ins])).cuda()
    offs = np.concatenate([[0], np.cumsum([len(x) for x in ins])])
    with pytest.raises(pkg.CjsError) as e:                           # the size query
        pkg.decompress_batch_device(d.data_ptr(), offs, 0, 0)
    assert e.value.errorCode == -33 and e.value.need == need


def _child(code, env_extra):
    env = dict(os.environ, CJS_DEBUG="1", **env_extra)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-2000:]
    return [l for l in r.stderr.splitlines() if l.startswith("[cjs dec dev]")]


_TINY = r"""
import sys, numpy as np
sys.path.insert(0, "tests"); sys.path.insert(0, ".")
import torch; torch.zeros(1, device="cuda")      # (CUDA up in torch before the library's first call)
import importlib, recipes, test_gpu_dec_device as t
pkg = importlib.import_module("compressjs-flattened_amd")
L = t._lib()
rng = np.random.default_rng(1)
xs = [recipes.textgen(int(rng.integers(1, 301)), 1000 + i) for i in range(20000)]
for lv in (9, 1):
    ss = pkg.Bzip2.compressFiles(xs, lv)
    rc, res, d, need, _ = t.device_batch(L, ss)
    assert rc == 0 and all(r[0] == 0 and r[3] == x.tobytes() for r, x in zip(res, xs)), lv
print("ok")
"""


def test_batch_20000_tiny_streams():
    lines = _child(_TINY, {})
    assert len(lines) == 2 and all("20000 inputs, 1 units" in l for l in lines), lines


_SHRUNK_GROUPS = r"""
import sys, numpy as np
sys.path.insert(0, "tests"); sys.path.insert(0, ".")
import torch; torch.zeros(1, device="cuda")      # (CUDA up in torch before the library's first call)
import support, test_gpu_dec_device as t
L = t._lib(); o = support.Oracle()
rng = np.random.default_rng(4)
_, big = o.bzip2_compress(rng.integers(0, 256, 300000, dtype=np.uint8), 1)      # larger than a group: the single device path
bad_big = big.copy(); bad_big[5000] ^= 4
for multi in (0, 1):
    t.batch_parity(L, t.damaged_mixture(o, 21 + multi) + [big, bad_big, big[:1000], big], multi)
print("ok")
"""


def test_batch_shrunk_groups_and_oversized_inputs():
    lines = _child(_SHRUNK_GROUPS, {"CJS_DEC_GROUP_BYTES": str(200000)})
    assert len(lines) == 2 and all(int(l.split(" units")[0].split()[-1]) > 3 for l in lines), lines


_SHRUNK_BATCHES = r"""
import sys, hashlib, numpy as np, torch
sys.path.insert(0, "tests"); sys.path.insert(0, ".")
import torch; torch.zeros(1, device="cuda")      # (CUDA up in torch before the library's first call)
import importlib, recipes, support, test_gpu_dec_device as t
pkg = importlib.import_module("compressjs-flattened_amd")
g = support.load_golden("golden_big_bzip2_9_10m.json")["cases"][0]
data = recipes.build(g["recipe"])
s = pkg.Bzip2.compressFile(data, None, 9)
assert hashlib.sha256(s.tobytes()).hexdigest() == g["out_sha256"]
d_in = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), s])).cuda()
d_out = torch.full((data.size + 7,), 0xA5, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
n = pkg.decompress_device(d_in.data_ptr() + 3, s.size, d_out.data_ptr() + 5, data.size)
assert n == data.size and np.array_equal(d_out[5:5 + n].cpu().numpy(), data) and bool((d_out[:5] == 0xA5).all())
offs = [3, 3 + s.size]
off, ln, st, d = pkg.decompress_batch_device(d_in.data_ptr(), offs, d_out.data_ptr(), data.size)
assert st[0] == 0 and ln[0] == data.size and np.array_equal(d_out[:n].cpu().numpy(), data)
print("ok")
"""


def test_several_phase_batches_10m():
    lines = _child(_SHRUNK_BATCHES, {"CJS_DEC_ROW_BYTES": str(60 << 20), "CJS_DEC_BATCH_ELEMS": str(2000000)})
    assert len(lines) == 2, lines


_BIG = r"""
import sys, hashlib, numpy as np, torch
sys.path.insert(0, "tests"); sys.path.insert(0, ".")
import torch; torch.zeros(1, device="cuda")      # (CUDA up in torch before the library's first call)
import importlib, recipes, support
pkg = importlib.import_module("compressjs-flattened_amd")
g = support.load_golden("golden_big_bzip2_9_1g.json")["cases"][0]
data = recipes.build(g["recipe"])
d_in = torch.from_numpy(data).cuda()
del data
d_s = torch.empty(g["out_len"] + (1 << 20), dtype=torch.uint8, device="cuda")
ctx = pkg.DeviceContext(0, g["in_len"], 9)
m = ctx.compress(d_in.data_ptr(), g["in_len"], d_s.data_ptr(), d_s.numel())
ctx.close()
assert m == g["out_len"] and hashlib.sha256(d_s[:m].cpu().numpy().tobytes()).hexdigest() == g["out_sha256"]
pkg.trim()
d_out = torch.empty(g["in_len"], dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
n = pkg.decompress_device(d_s.data_ptr(), m, d_out.data_ptr(), d_out.numel())
assert n == g["in_len"] and torch.equal(d_out, d_in)
print("ok")
"""


@pytest.mark.slow
def test_round_trip_1g_on_device():
    _child(_BIG, {})


def test_threads_single_and_batch(L, oracle):
    streams = [_u8(oracle.bzip2_compress(recipes.textgen(20000 + 7000 * t, 400 + t), 1 + 2 * t)[1]) for t in range(4)]
    groups = [[_u8(oracle.bzip2_compress(recipes.textgen(100 + 37 * i + t, 500 + 10 * t + i), 9)[1]) for i in range(30)] for t in range(4)]
    groups[1][4] = groups[1][4][:50]
    want = [host(L, s) for s in streams]
    want_b = [host_batch(L, g) for g in groups]
    errors = []

    def run(i):
        try:
            for j in range(20):
                if j % 2 == 0:
                    got = device(L, streams[i], 0, in_shift=j & 3, out_shift=(j >> 2) & 3)
                    if got[:3] != want[i]:
                        errors.append((i, j, got[0]))
                else:
                    rc, res, d, _, _ = device_batch(L, groups[i], shift=j & 3)
                    if rc or res != want_b[i][1] or d != want_b[i][2]:
                        errors.append((i, j, "batch", rc))
        except Exception as e:
            errors.append((i, repr(e)))
    ths = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors, errors[:5]
