"""Bzip2 recovery (cjs_bzip2_recover, Bzip2.recoverFile): the checks that need no GPU -- the C ABI exports and declares both entry
points, they refuse bad arguments and answer n < 6 before a device is touched and fail with CJS_E_NO_DEVICE otherwise, the fronts
carry them, the CLI refuses what it must; and the model of tests/recover_cases.py reproduces, with the oracle alone, what every
damaged input of the GPU tests was built to give."""
import ctypes
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import recover_cases as rc_
import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "compressjs-flattened_amd")
LIB = os.path.join(PKG, "libcjs_hip.so")
JS = os.path.join(PKG, "js")
S = ctypes.c_size_t
u8p = ctypes.POINTER(ctypes.c_uint8)
BOGUS = 0x7F0000001000                   # never dereferenced: every check that uses it comes before any device use
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(JS, "cjs_napi.node")), reason="node or the addon is missing")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _pkg():
    sys.path.insert(0, ROOT)
    return importlib.import_module("compressjs-flattened_amd")


@pytest.fixture(scope="module")
def L():
    return rc_.bind(LIB)


# ---------------------------------------------------------------- exports and surface
def test_symbols_are_exported_and_declared():
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "cjs_bzip2_recover") and hasattr(lib, "cjs_bzip2_recover_device")
    hdr = open(os.path.join(ROOT, "include", "cjs_hip.h")).read()
    assert "int cjs_bzip2_recover(const uint8_t *in, size_t n, int as_stream, uint8_t **out, size_t *out_n," in hdr
    assert "int cjs_bzip2_recover_device(const uint8_t *d_in, size_t n, int as_stream, uint8_t *d_out, size_t out_cap, size_t *out_n," in hdr
    assert "typedef struct cjs_bz_found {" in hdr and "#define CJS_REC_SHADOWED 1" in hdr
    assert ctypes.sizeof(rc_.Found) == 40


def test_python_front_has_recover():
    pkg = _pkg()
    assert callable(pkg.Bzip2.recoverFile) and callable(pkg.recover_device)
    assert ctypes.sizeof(pkg.Found) == 40 and pkg.REC_SHADOWED == 1


@needs_node
def test_js_front_has_recover():
    out = subprocess.run(["node", "-e", "var a = require('./common.js').addon(), B = require('./Bzip2.js');"
                          "console.log(typeof a.bzip2Recover, typeof B.recoverFile, B.REC_SHADOWED)"], cwd=JS, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["function", "function", "1"]


# ---------------------------------------------------------------- call behaviour without a device
def test_bad_arguments_are_refused_before_the_device(L):
    f = L.cjs_bzip2_recover
    data = (ctypes.c_uint8 * 100)()
    out, n, nf = u8p(), S(7), ctypes.c_long(9)
    found = (rc_.Found * 4)()
    assert f(data, 100, 0, None, ctypes.byref(n), found, 4, ctypes.byref(nf), None) == -32           # out NULL
    assert f(data, 100, 0, ctypes.byref(out), None, found, 4, ctypes.byref(nf), None) == -32         # out_n NULL
    assert f(data, 100, 1, ctypes.byref(out), ctypes.byref(n), found, 4, None, None) == -32          # n_found NULL
    assert f(None, 100, 0, ctypes.byref(out), ctypes.byref(n), found, 4, ctypes.byref(nf), None) == -32      # in NULL with n > 0
    assert f(data, 100, 0, ctypes.byref(out), ctypes.byref(n), None, 4, ctypes.byref(nf), None) == -32       # found NULL with cap > 0
    assert n.value == 7 and nf.value == 9 and not out
    g = L.cjs_bzip2_recover_device
    assert g(BOGUS, 100, 0, BOGUS, 1000, None, found, 4, ctypes.byref(nf), None) == -32              # out_n NULL
    assert g(BOGUS, 100, 0, BOGUS, 1000, ctypes.byref(n), found, 4, None, None) == -32               # n_found NULL
    assert g(None, 100, 0, BOGUS, 1000, ctypes.byref(n), found, 4, ctypes.byref(nf), None) == -32    # d_in NULL with n > 0
    assert g(BOGUS, 100, 1, None, 1000, ctypes.byref(n), found, 4, ctypes.byref(nf), None) == -32    # d_out NULL with out_cap > 0
    assert g(BOGUS, 100, 0, BOGUS, 1000, ctypes.byref(n), None, 4, ctypes.byref(nf), None) == -32    # found NULL with cap > 0
    assert n.value == 7 and nf.value == 9


@pytest.mark.parametrize("size", [0, 1, 5])
def test_too_short_for_a_magic_is_success_without_a_device(L, size):
    assert rc_.recover_host(L, bytes(size), 0) == (0, b"", [])
    assert rc_.recover_host(L, b"\x31\x41\x59\x26\x53"[:size], 1) == (0, rc_.EMPTY_STREAM, [])
    n, nf = S(3), ctypes.c_long(3)
    assert L.cjs_bzip2_recover_device(BOGUS, size, 0, None, 0, ctypes.byref(n), None, 0, ctypes.byref(nf), None) == 0
    assert n.value == 0 and nf.value == 0


def test_no_device_gives_no_device_error(L):
    if _has_gpu():
        pytest.skip("a GPU is present")
    assert rc_.recover_host(L, bytes(100), 0)[0] == -30
    assert rc_.recover_host(L, bytes(6), 1)[0] == -30
    n, nf = S(0), ctypes.c_long(0)
    assert L.cjs_bzip2_recover_device(BOGUS, 100, 0, BOGUS, 1000, ctypes.byref(n), None, 0, ctypes.byref(nf), None) == -30
    assert L.cjs_bzip2_recover_device(BOGUS, 100, 1, None, 0, ctypes.byref(n), None, 0, ctypes.byref(nf), None) == -30      # the size query
    pkg = _pkg()
    with pytest.raises(pkg.CjsError) as e:
        pkg.Bzip2.recoverFile(bytes(100))
    assert e.value.errorCode == -30
    with pytest.raises(pkg.CjsError) as e:
        pkg.recover_device(BOGUS, 100, BOGUS, 1000)
    assert e.value.errorCode == -30


@needs_node
@pytest.mark.parametrize("args, text", [
    (["--recover", "-z", "-t", "bzip2"], "--recover can only be used alone with -t bzip2"),
    (["--repair", "-z", "-t", "bzip2"], "--repair can only be used alone with -t bzip2"),
    (["--recover", "-b", "32", "-t", "bzip2"], "--recover can only be used alone with -t bzip2"),
    (["--repair", "-b", "32", "-t", "bzip2"], "--repair can only be used alone with -t bzip2"),
    (["--recover", "-9", "-t", "bzip2"], "--recover can only be used alone with -t bzip2"),
    (["--repair", "-1", "-t", "bzip2"], "--repair can only be used alone with -t bzip2"),
    (["--recover"], "--recover can only be used alone with -t bzip2"),
    (["--repair", "-t", "bwtc"], "--repair can only be used alone with -t bzip2"),
])
def test_cli_refusals(args, text):
    out = subprocess.run(["node", os.path.join(JS, "cli.js")] + args, input=b"", capture_output=True, timeout=60)
    assert out.returncode == 1 and out.stdout == b""
    assert out.stderr.decode().strip() == text


# ---------------------------------------------------------------- the model on the inputs of the GPU tests
def _positions(m):
    return [r[0] for r in m.recovered]


def test_model_on_undamaged_input(oracle):
    s = rc_.stream250(oracle)
    assert s.size == 96108 and rc_.magics(s) == [p for p, _ in rc_.BLOCKS250] and rc_.magics(s, rc_.MAGIC_END) == [rc_.EOS250]
    assert oracle.bzip2_table(s, 0) == (0, rc_.BLOCKS250)
    m = rc_.model(oracle, s)
    assert [(p, len(d)) for p, _, d, _ in m.recovered] == rc_.BLOCKS250 and m.data == rc_.text250().tobytes()
    assert [e for _, e, _, _ in m.recovered] == [299452, 604689, rc_.EOS250]
    want = s.copy(); want[3] = ord("9")
    assert m.stream == want.tobytes()
    s9 = rc_.stream250_l9(oracle)
    m = rc_.model(oracle, s9)
    assert m.stream == s9.tobytes() and m.data == rc_.text250().tobytes() and len(m.recovered) == 1
    m = rc_.model(oracle, rc_.EMPTY_STREAM)
    assert m.hits == [] and m.data == b"" and m.stream == rc_.EMPTY_STREAM
    ms, payload = rc_.members(oracle)
    m = rc_.model(oracle, ms)
    rc, tab = oracle.bzip2_table(ms, 1)
    assert rc == 0 and [(p, len(d)) for p, _, d, _ in m.recovered] == tab and m.data == payload and len(tab) >= 4
    assert oracle.bzip2_decompress(ms, 0)[1].tobytes() != payload           # the reference stops after the first member ...
    rc, back = oracle.bzip2_decompress(rc_.u8(m.stream), 0)
    assert rc == 0 and back.tobytes() == payload                             # ... the repaired form is one stream


def test_model_on_damage(oracle):
    t = rc_.text250().tobytes()
    for make in (rc_.damage_a, rc_.damage_b):
        bad = make(oracle)
        assert oracle.bzip2_decompress(bad, 1)[0] != 0
        m = rc_.model(oracle, bad)
        assert _positions(m) == [32, 604689] and m.data == t[:99898] + t[99898 + 99897:]
    m = rc_.model(oracle, rc_.damage_c(oracle))
    assert _positions(m) == [299444] and m.data == t[99898: 99898 + 99897]
    bad = rc_.damage_d(oracle)
    assert oracle.bzip2_decompress(bad, 1)[0] == -2
    m = rc_.model(oracle, bad)
    assert _positions(m) == [32, 299452, 604689, 768960] and m.data == t + t[:1000]
    base = rc_.model(oracle, rc_.stream250(oracle))
    for k in (1, 7, 8, 31):
        m = rc_.model(oracle, rc_.shifted(oracle, k))
        assert _positions(m) == [p + k for p, _ in rc_.BLOCKS250] and m.stream == base.stream and m.data == t


@pytest.mark.parametrize("which", sorted(rc_.FORTY_DAMAGE))
def test_model_on_forty_blocks(oracle, which):
    s, want, tab = rc_.forty(oracle)
    assert s.size == 2284 and len(want) == 820 and [z for _, z in tab] == list(range(1, 41))
    bad, keep = rc_.forty_damaged(oracle, which)
    m = rc_.model(oracle, bad)
    assert m.data == keep and _positions(m) == [p for k, (p, _) in enumerate(tab) if k not in rc_.FORTY_DAMAGE[which]]
    assert len(m.recovered) == {"every-third": 27, "first": 39, "last": 39, "all": 0, "none": 40}[which]
    if which == "all":
        assert m.stream == rc_.EMPTY_STREAM
    rc, back = oracle.bzip2_decompress(rc_.u8(m.stream), 0)
    assert rc == 0 and back.tobytes() == keep


def test_model_on_shadowing(oracle):
    s, data = rc_.magic_in_map(oracle)
    assert rc_.magics(s) == [32, 137] and oracle.bzip2_table(s, 0) == (0, [(32, 3000)])
    m = rc_.model(oracle, s)
    assert _positions(m) == [32] and m.shadowed == [137] and m.data == data
    as9 = rc_.flip(s, 32 + 53)
    assert oracle.bzip2_decompress_block(as9, 137)[0] == -7
    m = rc_.model(oracle, as9)
    assert m.recovered == [] and m.shadowed == [] and m.stream == rc_.EMPTY_STREAM


def test_model_on_level_limit(oracle):
    s, data = rc_.level_limit(oracle)
    assert oracle.bzip2_decompress(s, 0)[0] == -5 and oracle.bzip2_decompress(s, 1)[0] == -5
    m = rc_.model(oracle, s)
    assert _positions(m) == [32] and m.data == data


def test_model_on_random_damage(oracle):
    """every seeded input is damaged, and together the seeds lose every block at least once and keep every block at least once"""
    lost, kept = set(), set()
    for seed in rc_.SEEDS:
        bad = rc_.random_damage(oracle, seed)
        assert bad.tobytes() != rc_.stream250(oracle).tobytes()
        m = rc_.model(oracle, bad)
        sizes = [len(r[2]) for r in m.recovered]
        assert len(sizes) <= 3 and set(sizes) <= {z for _, z in rc_.BLOCKS250}
        kept |= set(sizes)
        lost |= {z for _, z in rc_.BLOCKS250} - set(sizes)
        rc, back = oracle.bzip2_decompress(rc_.u8(m.stream), 0)
        assert rc == 0 and back.tobytes() == m.data
    assert kept == lost == {z for _, z in rc_.BLOCKS250}
