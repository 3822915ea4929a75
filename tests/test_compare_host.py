"""What cjs_bzip2_compare[_device] and cjs_bzip2_compare_streams[_device] decide before a device is touched, without a GPU: every
refusal of the contract, the spans that touch no block, the size of the two structs, and the logic of CompareResult.equal /
cmp_text on hand-made infos.  The index is made of imaginary entries (rg.create)."""
import ctypes
import importlib

import numpy as np
import pytest

import compare_cases as cc
import range_cases as rg

N = 5000                                                    # bytes of the imaginary stream the entries describe
# decoded offsets: block 0 [0, 1000), blocks 1 and 2 of size zero, block 3 [1000, 1500)
ENTRIES = [(32, 9000, 1000, 0x11223344, 1, 0), (9000, 9200, 0, 0xFFFFFFFF, 1, 0), (9300, 9500, 0, 7, 1, 0), (20007, 39899, 500, 0, 9, 0)]
TOTAL = 1500
FORMS = ["host", "device", "streams", "streams_device"]


@pytest.fixture(scope="module")
def L():
    return cc.bind()


@pytest.fixture(scope="module")
def h(L):
    rc, h = rg.create(L, ENTRIES, N, 0)
    assert rc == 0
    return h


def test_struct_sizes():
    assert ctypes.sizeof(cc.Diff) == 16 == cc.DIFF.itemsize and ctypes.sizeof(cc.Info) == 64
    assert (cc.Diff.off.offset, cc.Diff.a.offset, cc.Diff.b.offset, cc.Diff.reserved.offset) == (0, 8, 9, 10)
    pkg = importlib.import_module("compressjs-flattened_amd")
    assert ctypes.sizeof(pkg.Diff) == 16 and ctypes.sizeof(pkg.CompareInfo) == 64
    assert [f[0] for f in pkg.CompareInfo._fields_] == [f[0] for f in cc.Info._fields_]


def _fn(L, form):
    return {"host": L.cjs_bzip2_compare, "device": L.cjs_bzip2_compare_device, "streams": L.cjs_bzip2_compare_streams,
            "streams_device": L.cjs_bzip2_compare_streams_device}[form]


def _ptr(form, a):
    return a.ctypes.data_as(rg.u8p) if form in ("host", "streams") else ctypes.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("form", FORMS)
def test_refusals_before_the_device_is_touched(L, h, form):
    """off >= total makes every call one that would succeed without a device: a refusal is then the argument check's"""
    fn = _fn(L, form)
    stream, other = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    info = cc.Info()
    diffs = (cc.Diff * 4)()
    two = form.startswith("streams")
    ok = dict(first=_ptr(form, stream), n=N, h=h, other=_ptr(form, other), other_n=N, third=h if two else 0, off=TOTAL, ln=10,
              diffs=ctypes.cast(diffs, rg.V), cap=4, info=ctypes.byref(info))

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a["first"], a["n"], a["h"], a["other"], a["other_n"], a["third"], a["off"], a["ln"], a["diffs"], a["cap"], a["info"], None)
    assert call() == 0
    assert call(h=None) == rg.E_INVALID
    assert call(info=None) == rg.E_INVALID
    assert call(first=None) == rg.E_INVALID                  # NULL in with n > 0
    assert call(other=None) == rg.E_INVALID                  # NULL other with other_n > 0
    assert call(diffs=None) == rg.E_INVALID                  # NULL diffs with cap > 0
    assert call(diffs=None, cap=0) == 0
    assert call(n=N - 1) == rg.E_INVALID and rg.detail(L) == "the index is of a stream of 5000 bytes"
    assert call() == 0 and rg.detail(L) == ""
    if two:
        assert call(third=None) == rg.E_INVALID
        assert call(other_n=N + 1) == rg.E_INVALID and rg.detail(L) == "the index is of a stream of 5000 bytes"
    else:
        assert call(other=None, other_n=0) == 0
    assert all(bytes(diffs[i]) == bytes(16) for i in range(4))
    # the same refusals when the span is not empty: still before the device is looked for (no CJS_E_NO_DEVICE)
    assert call(off=0, h=None) == rg.E_INVALID and call(off=0, info=None) == rg.E_INVALID and call(off=0, n=N - 1) == rg.E_INVALID
    assert call(off=0, diffs=None) == rg.E_INVALID and call(off=0, first=None) == rg.E_INVALID and call(off=0, other=None) == rg.E_INVALID


@pytest.mark.parametrize("form", FORMS)
def test_an_empty_span_needs_no_device(L, form):
    """len = 0, off >= total, an other side that ends in front of the window or starts behind it, an index without blocks and one
    of zero-size blocks only: 0, zeros, nothing decoded"""
    stream, other = np.zeros(N, np.uint8), np.zeros(300, np.uint8)
    two = form.startswith("streams")

    def run(h, off, ln, other_off=0, other_n=300):
        if form == "host":
            return cc.compare_host(L, stream, h, other[:other_n], other_off, off, ln, 3)
        if form == "device":
            return cc.compare_device(L, ctypes.c_void_p(stream.ctypes.data), N, h, ctypes.c_void_p(other.ctypes.data), other_n, other_off, off, ln, 3)      # (never looked at)
        if form == "streams":
            return cc.streams_host(L, stream, h, stream, h, off, ln, 3)
        return cc.streams_device(L, ctypes.c_void_p(stream.ctypes.data), N, h, ctypes.c_void_p(stream.ctypes.data), N, h, off, ln, 3)
    rc, h = rg.create(L, ENTRIES, N, 0)
    assert rc == 0
    spans = [(0, 0, 0, 300), (700, 0, 0, 300), (TOTAL, 5, 0, 300), (TOTAL + 1, cc.ALL, 0, 300), (2 ** 64 - 1, cc.ALL, 0, 300), (2 ** 63, 2 ** 63, 0, 300)]
    if not two:
        spans += [(300, cc.ALL, 0, 300), (0, 100, 100, 300), (0, cc.ALL, TOTAL, 300), (0, cc.ALL, 0, 0), (0, cc.ALL, 2 ** 64 - 10, 300)]
    for off, ln, o_off, o_n in spans:
        rc, m, info, d = run(h, off, ln, o_off, o_n)
        assert rc == 0 and m == [] and cc.info_tuple(info) == cc.ZERO_INFO and d == "", (off, ln, o_off, o_n)
    L.cjs_bzip2_index_destroy(h)
    for entries in ([], [e for e in ENTRIES if e[2] == 0]):
        rc, h = rg.create(L, entries, N, 0)
        assert rc == 0
        for off, ln in ((0, cc.ALL), (0, 10), (5, 0)):
            rc, m, info, d = run(h, off, ln)
            assert rc == 0 and m == [] and cc.info_tuple(info) == cc.ZERO_INFO, (len(entries), off, ln)
        L.cjs_bzip2_index_destroy(h)


@pytest.mark.parametrize("form", FORMS)
def test_a_span_with_bytes_needs_a_device(L, h, form):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    stream, other = np.zeros(N, np.uint8), np.zeros(300, np.uint8)
    if form == "host":
        rc = cc.compare_host(L, stream, h, other, 0, 0, cc.ALL, 3)[0]
    elif form == "device":
        rc = cc.compare_device(L, ctypes.c_void_p(stream.ctypes.data), N, h, ctypes.c_void_p(other.ctypes.data), 300, 0, 0, cc.ALL, 3)[0]
    elif form == "streams":
        rc = cc.streams_host(L, stream, h, stream, h, 0, cc.ALL, 3)[0]
    else:
        rc = cc.streams_device(L, ctypes.c_void_p(stream.ctypes.data), N, h, ctypes.c_void_p(stream.ctypes.data), N, h, 0, cc.ALL, 3)[0]
    assert rc == rg.E_NO_DEVICE


def test_expected_list_helper():
    """the reference the GPU tests compare with"""
    plain = np.frombuffer(b"abcdefghij", np.uint8)
    other = np.frombuffer(b"abXdeYghiZkl", np.uint8)
    assert cc.expected(plain, other) == ([(2, 99, 88), (5, 102, 89), (9, 106, 90)], 10)
    assert cc.expected(plain, other[2:8], other_off=2) == ([(2, 99, 88), (5, 102, 89)], 6)
    assert cc.expected(plain, other, off=3, ln=3) == ([(5, 102, 89)], 3)
    assert cc.expected(plain, other, runs=[(0, 2), (6, 10)]) == ([(9, 106, 90)], 6)
    assert cc.expected(plain, other[:0], other_off=4) == ([], 0)
    f = cc.flipped(plain, [0, 9, 9, 4])
    assert np.nonzero(f != plain)[0].tolist() == [0, 4, 9]


def _result(pkg, n_diffs=0, first=cc.NONE, compared=0, bad=0, bad_b=0, len_a=0, len_b=0, detail=""):
    info = pkg.CompareInfo(n_diffs, first, compared, bad, 3 if bad else cc.NONE, 1, bad_b, 2 if bad_b else cc.NONE)
    return pkg.CompareResult([], info, detail, len_a, len_b)


def test_compare_result_logic():
    pkg = importlib.import_module("compressjs-flattened_amd")
    r = _result(pkg, compared=100, len_a=100, len_b=100)
    assert r.equal and r.cmp_text() == "" and r.first_diff is None and r.first_bad_block is None and r.first_bad_block_b is None
    r = _result(pkg, n_diffs=2, first=41, compared=100, len_a=100, len_b=100)
    assert not r.equal and r.cmp_text() == "differ: byte 42" and r.first_diff == 41 and r.total == 2
    r = _result(pkg, n_diffs=1, first=0, compared=90, len_a=100, len_b=90)      # a difference goes before an EOF
    assert not r.equal and r.cmp_text() == "differ: byte 1"
    r = _result(pkg, compared=90, len_a=90, len_b=100)
    assert not r.equal and r.cmp_text() == "EOF on a"
    r = _result(pkg, compared=90, len_a=100, len_b=90)
    assert not r.equal and r.cmp_text() == "EOF on b"
    r = _result(pkg, compared=0, len_a=0, len_b=0)
    assert r.equal and r.cmp_text() == ""
    r = _result(pkg, compared=0, len_a=0, len_b=5)
    assert not r.equal and r.cmp_text() == "EOF on a"
    # equal lengths, but only a window was compared: not `equal`, and cmp has no answer
    r = _result(pkg, compared=60, len_a=100, len_b=100)
    assert not r.equal
    with pytest.raises(pkg.CjsError):
        r.cmp_text()
    # bad blocks on either side: never equal, no answer without a difference, the difference with one
    for kw in (dict(bad=1), dict(bad_b=1)):
        r = _result(pkg, compared=70, len_a=100, len_b=100, detail="index does not match the stream at block 3", **kw)
        assert not r.equal and (r.first_bad_block, r.first_bad_block_b) == ((3, None) if "bad" in kw else (None, 2))
        with pytest.raises(pkg.CjsError) as e:
            r.cmp_text()
        assert "block 3" in str(e.value)
        r = _result(pkg, n_diffs=1, first=9, compared=70, len_a=100, len_b=100, **kw)
        assert not r.equal and r.cmp_text() == "differ: byte 10"
    r = _result(pkg, compared=100, len_a=100, len_b=100, bad=1)      # (cannot happen: a bad block is not compared) still not equal
    assert not r.equal
