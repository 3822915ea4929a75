"""What cjs_bzip2_search[_device] decide before a device is touched, without a GPU: every refusal of the contract, the windows that
touch no block, and the size of the two structs.  The index is made of imaginary entries (rg.create)."""
import ctypes

import numpy as np
import pytest

import range_cases as rg
import search_cases as sc

N = 5000                                                    # bytes of the imaginary stream the entries describe
# decoded offsets: block 0 [0, 1000), blocks 1 and 2 of size zero, block 3 [1000, 1500)
ENTRIES = [(32, 9000, 1000, 0x11223344, 1, 0), (9000, 9200, 0, 0xFFFFFFFF, 1, 0), (9300, 9500, 0, 7, 1, 0), (20007, 39899, 500, 0, 9, 0)]
TOTAL = 1500


@pytest.fixture(scope="module")
def L():
    return sc.bind()


@pytest.fixture(scope="module")
def h(L):
    rc, h = rg.create(L, ENTRIES, N, 0)
    assert rc == 0
    return h


def _raw(L, fn, first, n, h, pat, pat_off, npat, flags, off, ln, found, cap, info):
    return fn(first, n, h, pat, pat_off, npat, flags, off, ln, found, cap, info, None)


def _args(pats):
    blob, p_off = sc.pattern_arrays(pats)
    return blob, p_off, blob.ctypes.data_as(rg.u8p), p_off.ctypes.data_as(ctypes.POINTER(sc.U32))


def test_struct_sizes():
    assert ctypes.sizeof(sc.Match) == 16 == sc.MATCH.itemsize and ctypes.sizeof(sc.Info) == 32
    assert (sc.Match.off.offset, sc.Match.pattern.offset, sc.Match.reserved.offset) == (0, 8, 12)


@pytest.mark.parametrize("form", ["host", "device"])
def test_refusals_before_the_device_is_touched(L, h, form):
    """off >= total makes every call one that would succeed without a device: a refusal is then the argument check's"""
    fn = L.cjs_bzip2_search if form == "host" else L.cjs_bzip2_search_device
    stream = np.zeros(N, np.uint8)
    first = stream.ctypes.data_as(rg.u8p) if form == "host" else ctypes.c_void_p(stream.ctypes.data)
    keep, keep2, pat, p_off = _args([b"abc", b"d"])
    info = sc.Info()
    found = (sc.Match * 4)()
    ok = dict(first=first, n=N, h=h, pat=pat, pat_off=p_off, npat=2, flags=0, off=TOTAL, ln=10, found=ctypes.cast(found, rg.V), cap=4, info=ctypes.byref(info))

    def call(**kw):
        a = dict(ok, **kw)
        return _raw(L, fn, a["first"], a["n"], a["h"], a["pat"], a["pat_off"], a["npat"], a["flags"], a["off"], a["ln"], a["found"], a["cap"], a["info"])
    assert call() == 0
    assert call(h=None) == rg.E_INVALID
    assert call(info=None) == rg.E_INVALID
    assert call(pat=None) == rg.E_INVALID
    assert call(pat_off=None) == rg.E_INVALID
    assert call(first=None) == rg.E_INVALID                  # NULL in with n > 0
    assert call(found=None) == rg.E_INVALID                  # NULL found with cap > 0
    assert call(found=None, cap=0) == 0
    assert call(n=N - 1) == rg.E_INVALID and "5000" in rg.detail(L)
    assert call(npat=0) == rg.E_INVALID
    for flags in (2, 4, 0x80000000, 3):
        assert call(flags=flags) == rg.E_INVALID, flags
    assert call(flags=sc.NOCASE) == 0
    # 65 patterns; 64 are fine
    k1, k2, p65, o65 = _args([b"x"] * 65)
    assert call(pat=p65, pat_off=o65, npat=65) == rg.E_INVALID
    assert call(pat=p65, pat_off=o65, npat=64) == 0
    # lengths 0 and 257; 256 is fine
    for pats, want in (([b"ab", b"", b"c"], rg.E_INVALID), ([b"a" * 257], rg.E_INVALID), ([b"a" * 256, b"b"], 0)):
        k3, k4, pp, oo = _args(pats)
        assert call(pat=pp, pat_off=oo, npat=len(pats)) == want, [len(p) for p in pats]
    # offsets that do not ascend, and a first offset that is not 0
    desc = np.array([0, 3, 2], np.uint32)
    assert call(pat_off=desc.ctypes.data_as(ctypes.POINTER(sc.U32))) == rg.E_INVALID
    one = np.array([1, 3, 4], np.uint32)
    assert call(pat_off=one.ctypes.data_as(ctypes.POINTER(sc.U32))) == rg.E_INVALID
    assert all(bytes(found[i]) == bytes(16) for i in range(4))


@pytest.mark.parametrize("form", ["host", "device"])
def test_a_window_without_a_touched_block_needs_no_device(L, form):
    """len = 0, off >= total, an index without blocks and one of zero-size blocks only: 0, no match, nothing decoded"""
    stream = np.zeros(N, np.uint8)

    def run(h, off, ln):
        if form == "host":
            return sc.search_host(L, stream, h, [b"a", b"bc"], off, ln, 0, 3)
        return sc.search_device(L, ctypes.c_void_p(stream.ctypes.data), N, h, [b"a", b"bc"], off, ln, 0, 3)      # (never looked at)
    rc, h = rg.create(L, ENTRIES, N, 0)
    assert rc == 0
    for off, ln in ((0, 0), (700, 0), (TOTAL, 5), (TOTAL + 1, sc.ALL), (2 ** 64 - 1, sc.ALL), (2 ** 63, 2 ** 63)):
        rc, m, info, d = run(h, off, ln)
        assert rc == 0 and m == [] and sc.info_tuple(info) == (0, 0, 2 ** 64 - 1, 0) and d == "", (off, ln)
    L.cjs_bzip2_index_destroy(h)
    for entries in ([], [e for e in ENTRIES if e[2] == 0]):
        rc, h = rg.create(L, entries, N, 0)
        assert rc == 0
        for off, ln in ((0, sc.ALL), (0, 10), (5, 0)):
            rc, m, info, d = run(h, off, ln)
            assert rc == 0 and m == [] and sc.info_tuple(info) == (0, 0, 2 ** 64 - 1, 0), (len(entries), off, ln)
        L.cjs_bzip2_index_destroy(h)


def test_expected_list_helper():
    """the reference the GPU tests compare with: overlaps, equal patterns, the window's two rules, A..Z folding only, runs"""
    plain = np.frombuffer(b"aaaa@A[a`b{B\xc1\xe1aa", np.uint8)
    assert sc.expected(plain, [b"aa", b"a", b"aa"]) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (3, 1), (7, 1), (14, 0), (14, 1), (14, 2), (15, 1)]
    assert sc.expected(plain, [b"aa"], 1, 2) == [(1, 0)] and sc.expected(plain, [b"aa"], 1, 1) == [] and sc.expected(plain, [b"aa"], 14, sc.ALL) == [(14, 0)]
    assert sc.expected(plain, [b"A", b"\xc1", b"["], nocase=True) == [(0, 0), (1, 0), (2, 0), (3, 0), (5, 0), (6, 2), (7, 0), (12, 1), (14, 0), (15, 0)]
    assert sc.expected(plain, [b"aa"], runs=[(0, 2), (2, 4), (15, 16)]) == [(0, 0), (2, 0)]
