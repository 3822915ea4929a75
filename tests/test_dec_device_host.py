"""Device-resident Bzip2 decompression (cjs_bzip2_decompress_device, decompress_device): the checks that need no GPU -- the C ABI
exports and declares the entry point, refuses bad arguments before it touches a device, and fails with CJS_E_NO_DEVICE (no CPU
fallback) otherwise; the Python front carries it."""
import ctypes
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "compressjs-flattened_amd")
LIB = os.path.join(PKG, "libcjs_hip.so")
S = ctypes.c_size_t
V = ctypes.c_void_p
BOGUS = 0x7F0000001000                   # never dereferenced: every check below comes before any device use


def _lib():
    L = ctypes.CDLL(LIB)
    L.cjs_bzip2_decompress_device.argtypes = [V, S, ctypes.c_int, V, S, ctypes.POINTER(S), V]
    L.cjs_bzip2_decompress_device.restype = ctypes.c_int
    return L


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _pkg():
    sys.path.insert(0, ROOT)
    return importlib.import_module("compressjs-flattened_amd")


def test_symbol_is_exported_and_declared():
    assert hasattr(ctypes.CDLL(LIB), "cjs_bzip2_decompress_device")
    hdr = open(os.path.join(ROOT, "include", "cjs_hip.h")).read()
    assert "int cjs_bzip2_decompress_device(const uint8_t *d_in, size_t n, int multistream" in hdr


def test_python_front_has_decompress_device():
    assert callable(_pkg().decompress_device)


def test_bad_arguments_are_refused_before_the_device():
    f = _lib().cjs_bzip2_decompress_device
    n = S(7)
    assert f(BOGUS, 100, 0, BOGUS, 1000, None, None) == -32           # out_n NULL
    assert f(None, 100, 0, BOGUS, 1000, ctypes.byref(n), None) == -32  # d_in NULL with n > 0
    assert n.value == 7
    assert f(BOGUS, 100, 1, None, 1000, ctypes.byref(n), None) == -32  # d_out NULL with out_cap > 0


def _blib():
    L = ctypes.CDLL(LIB)
    PS = ctypes.POINTER(S)
    L.cjs_bzip2_decompress_batch_device.argtypes = [V, PS, S, ctypes.c_int, V, S, PS, PS, ctypes.POINTER(ctypes.c_int32), PS, V]
    L.cjs_bzip2_decompress_batch_device.restype = ctypes.c_int
    return L


def test_batch_symbol_is_exported_and_declared():
    assert hasattr(ctypes.CDLL(LIB), "cjs_bzip2_decompress_batch_device")
    hdr = open(os.path.join(ROOT, "include", "cjs_hip.h")).read()
    assert "int cjs_bzip2_decompress_batch_device(const uint8_t *d_in, const size_t *in_off, size_t count" in hdr
    assert callable(_pkg().decompress_batch_device)


def test_batch_bad_arguments_are_refused_before_the_device():
    f = _blib().cjs_bzip2_decompress_batch_device
    off = (S * 4)(0, 10, 10, 30)
    o, ln, need = (S * 3)(), (S * 3)(), S(5)
    st = (ctypes.c_int32 * 3)()
    ok = [BOGUS, off, 3, 0, BOGUS, 100, o, ln, st, ctypes.byref(need), None]
    for i in (1, 6, 7, 8, 9):                                        # in_off / out_off / out_len / status / out_need NULL
        args = list(ok)
        args[i] = None
        assert f(*args) == -32, i
    args = list(ok); args[0] = None                                  # d_in NULL with input bytes
    assert f(*args) == -32
    args = list(ok); args[4] = None                                  # d_out NULL with out_cap > 0
    assert f(*args) == -32
    bad = (S * 4)(0, 10, 9, 30)                                      # not ascending
    args = list(ok); args[1] = bad
    assert f(*args) == -32
    # count == 0: success, *out_need = 0
    assert f(None, None, 0, 0, None, 0, None, None, None, ctypes.byref(need), None) == 0 and need.value == 0


def test_no_device_gives_no_device_error():
    if _has_gpu():
        pytest.skip("a GPU is present")
    f = _lib().cjs_bzip2_decompress_device
    n = S(0)
    assert f(BOGUS, 100, 0, BOGUS, 1000, ctypes.byref(n), None) == -30
    assert f(BOGUS, 100, 1, None, 0, ctypes.byref(n), None) == -30     # the size query is a well-formed call too
    pkg = _pkg()
    with pytest.raises(pkg.CjsError) as e:
        pkg.decompress_device(BOGUS, 100, BOGUS, 1000)
    assert e.value.errorCode == -30
    fb = _blib().cjs_bzip2_decompress_batch_device
    off = (S * 3)(0, 10, 30)
    o, ln, need = (S * 2)(), (S * 2)(), S(0)
    st = (ctypes.c_int32 * 2)()
    assert fb(BOGUS, off, 2, 1, BOGUS, 100, o, ln, st, ctypes.byref(need), None) == -30
    with pytest.raises(pkg.CjsError) as e:
        pkg.decompress_batch_device(BOGUS, [0, 10, 30], BOGUS, 100)
    assert e.value.errorCode == -30
