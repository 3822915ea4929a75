"""Batched Bzip2 decompression (cjs_bzip2_decompress_batch, Bzip2.decompressFiles): the checks that need no GPU -- the C ABI
exports the entry point, succeeds on an empty batch, refuses bad arguments before it touches a device, and fails with
CJS_E_NO_DEVICE (no CPU fallback) otherwise; the Python, N-API and JS fronts carry the batch form."""
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
S = ctypes.c_size_t


def _lib():
    L = ctypes.CDLL(LIB)
    L.cjs_bzip2_decompress_batch.argtypes = [ctypes.POINTER(u8p), ctypes.POINTER(S), S, ctypes.c_int, ctypes.POINTER(u8p),
                                             ctypes.POINTER(S), ctypes.POINTER(S), ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p]
    L.cjs_bzip2_decompress_batch.restype = ctypes.c_int
    L.cjs_free.argtypes = [ctypes.c_void_p]
    L.cjs_free.restype = None
    return L


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _args(inputs):
    arrs = [np.frombuffer(x, dtype=np.uint8) if isinstance(x, bytes) else x for x in inputs]
    cnt = len(arrs)
    ptrs = (u8p * max(cnt, 1))(*[a.ctypes.data_as(u8p) if a is not None and a.size else u8p() for a in arrs])
    lens = (S * max(cnt, 1))(*[0 if a is None else a.size for a in arrs])
    return arrs, ptrs, lens, (S * max(cnt, 1))(), (S * max(cnt, 1))(), (ctypes.c_int32 * max(cnt, 1))()


def test_symbol_is_exported():
    assert hasattr(ctypes.CDLL(LIB), "cjs_bzip2_decompress_batch")


def test_empty_batch_succeeds():
    L = _lib()
    out = u8p()
    assert L.cjs_bzip2_decompress_batch(None, None, 0, 0, ctypes.byref(out), None, None, None, None) == 0 and not out
    _, ptrs, lens, off, ln, st = _args([])
    assert L.cjs_bzip2_decompress_batch(ptrs, lens, 0, 1, ctypes.byref(out), off, ln, st, None) == 0 and not out


def test_bad_arguments_are_refused_before_the_device():
    L = _lib()
    keep, ptrs, lens, off, ln, st = _args([b"BZh9", b""])
    out = u8p()
    f = L.cjs_bzip2_decompress_batch
    assert f(ptrs, lens, 2, 0, None, off, ln, st, None) == -32
    for args in ((None, lens, 2, 0, ctypes.byref(out), off, ln, st, None), (ptrs, None, 2, 0, ctypes.byref(out), off, ln, st, None),
                 (ptrs, lens, 2, 0, ctypes.byref(out), None, ln, st, None), (ptrs, lens, 2, 0, ctypes.byref(out), off, None, st, None),
                 (ptrs, lens, 2, 0, ctypes.byref(out), off, ln, None, None)):
        assert f(*args) == -32 and not out
    ptrs[0] = u8p()                      # n[0] = 4 with in[0] == NULL
    assert f(ptrs, lens, 2, 0, ctypes.byref(out), off, ln, st, None) == -32 and not out


def test_no_device_gives_no_device_error():
    if _has_gpu():
        pytest.skip("a GPU is present")
    L = _lib()
    keep, ptrs, lens, off, ln, st = _args([b"BZh9", b"", b"not bzip"])
    ptrs[1] = u8p()                      # n[1] = 0: in[1] may be NULL
    out = u8p()
    assert L.cjs_bzip2_decompress_batch(ptrs, lens, 3, 0, ctypes.byref(out), off, ln, st, None) == -30 and not out


def test_python_front_has_decompress_files():
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("compressjs-flattened_amd")
    assert callable(pkg.Bzip2.decompressFiles)
    assert pkg.Bzip2.decompressFiles([]) == []
    if not _has_gpu():
        with pytest.raises(pkg.CjsError) as e:
            pkg.Bzip2.decompressFiles([b"BZh9", b""])
        assert e.value.errorCode == -30


def test_js_front_has_decompress_files():
    src = open(os.path.join(PKG, "js", "Bzip2.js")).read()
    assert "Bzip2.decompressFiles = function" in src and "bzip2DecompressBatch" in src
    cc = open(os.path.join(PKG, "js", "cjs_napi.cc")).read()
    assert '"bzip2DecompressBatch"' in cc and 'SYM(bzip2_decompress_batch, "cjs_bzip2_decompress_batch")' in cc
    addon = os.path.join(PKG, "js", "cjs_napi.node")
    if shutil.which("node") is None or not os.path.exists(addon):
        return
    script = r"""
      const m = require(process.argv[1]);
      const r = {fn: typeof m.Bzip2.decompressFiles, native: typeof m.native().bzip2DecompressBatch};
      const empty = m.Bzip2.decompressFiles([], 0);
      r.empty = Array.isArray(empty) && empty.length === 0;
      console.log(JSON.stringify(r));
    """
    out = subprocess.run(["node", "-e", script, os.path.join(PKG, "js", "index.js")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    import json
    assert json.loads(out.stdout.strip().splitlines()[-1]) == {"fn": "function", "native": "function", "empty": True}
