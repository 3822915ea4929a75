"""Batched Bzip2 compression (cjs_bzip2_compress_batch*, Bzip2.compressFiles): the checks that need no GPU -- the C ABI
exports the batch entry points, refuses bad levels before it touches a device, succeeds on an empty batch, and fails
with CJS_E_NO_DEVICE (no CPU fallback) otherwise; the Python and JS fronts carry compressFiles."""
import ctypes
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "compressjs-flattened_amd")
LIB = os.path.join(PKG, "libcjs_hip.so")
u8p = ctypes.POINTER(ctypes.c_uint8)


def _lib():
    L = ctypes.CDLL(LIB)
    S, I, V = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    L.cjs_bzip2_compress_batch.argtypes = [ctypes.POINTER(u8p), ctypes.POINTER(S), S, I, ctypes.POINTER(u8p), ctypes.POINTER(S),
                                           ctypes.POINTER(S), V]
    L.cjs_bzip2_compress_batch.restype = I
    L.cjs_ctx_create_batch.argtypes = [ctypes.POINTER(V), I, S, S, I]
    L.cjs_ctx_create_batch.restype = I
    L.cjs_free.argtypes = [V]
    L.cjs_free.restype = None
    return L


def _batch(L, inputs, level):
    arrs = [np.frombuffer(x, dtype=np.uint8) if isinstance(x, bytes) else x for x in inputs]
    cnt = len(arrs)
    ptrs = (u8p * max(cnt, 1))(*[a.ctypes.data_as(u8p) for a in arrs])
    lens = (ctypes.c_size_t * max(cnt, 1))(*[a.size for a in arrs])
    off = (ctypes.c_size_t * max(cnt, 1))()
    ln = (ctypes.c_size_t * max(cnt, 1))()
    out = u8p()
    rc = L.cjs_bzip2_compress_batch(ptrs, lens, cnt, level, ctypes.byref(out), off, ln, None)
    return rc, out


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_batch_symbols_are_exported():
    L = ctypes.CDLL(LIB)
    for name in ("cjs_bzip2_compress_batch", "cjs_ctx_create_batch", "cjs_bzip2_compress_batch_device"):
        assert hasattr(L, name), name


@pytest.mark.parametrize("level", [0, 10, -1])
def test_bad_level_is_refused_before_the_device(level):
    L = _lib()
    rc, out = _batch(L, [b"abc", b""], level)
    assert rc == -20 and not out
    ctx = ctypes.c_void_p()
    assert L.cjs_ctx_create_batch(ctypes.byref(ctx), 0, 1 << 16, 4, level) == -20 and not ctx.value


def test_empty_batch_succeeds():
    L = _lib()
    rc, out = _batch(L, [], 9)
    assert rc == 0 and not out
    L.cjs_free(out)


def test_no_device_gives_no_device_error():
    if _has_gpu():
        pytest.skip("a GPU is present")
    L = _lib()
    rc, out = _batch(L, [b"hello", b"", b"world" * 100], 9)
    assert rc == -30 and not out          # CJS_E_NO_DEVICE: no CPU fallback
    ctx = ctypes.c_void_p()
    assert L.cjs_ctx_create_batch(ctypes.byref(ctx), 0, 1 << 16, 4, 9) == -30


def test_python_front_has_compress_files():
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("compressjs-flattened_amd")
    assert callable(pkg.Bzip2.compressFiles)
    assert callable(pkg.DeviceContext.batch) and callable(pkg.DeviceContext.compress_batch)
    assert pkg.Bzip2.compressFiles([]) == []
    for bad in (0, 10, 2.5):
        with pytest.raises(pkg.CjsError) as e:
            pkg.Bzip2.compressFiles([b"abc"], bad)
        assert e.value.errorCode == -20
    if not _has_gpu():
        with pytest.raises(pkg.CjsError) as e:
            pkg.Bzip2.compressFiles([b"abc", b"de"], 9)
        assert e.value.errorCode == -30


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_front_has_compress_files():
    addon = os.path.join(PKG, "js", "cjs_napi.node")
    if not os.path.exists(addon):
        pytest.skip("N-API addon not built (node_api.h missing)")
    script = r"""
      const m = require(process.argv[1]);
      const r = {fn: typeof m.Bzip2.compressFiles, native: typeof m.native().bzip2CompressBatch};
      try { m.Bzip2.compressFiles([new Uint8Array(3)], 0); r.level0 = 'no throw'; } catch (e) { r.level0 = e.message; }
      const empty = m.Bzip2.compressFiles([], 9);
      r.empty = Array.isArray(empty) && empty.length === 0;
      console.log(JSON.stringify(r));
    """
    out = subprocess.run(["node", "-e", script, os.path.join(PKG, "js", "index.js")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    import json
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r == {"fn": "function", "native": "function", "level0": "Invalid block size multiplier", "empty": True}
