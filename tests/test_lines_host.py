"""What the line table (cjs_bzip2_lines_*) decides without a GPU: the table itself (create, save, load, info, counts, every refusal),
the refusals of the two questions before a device is touched, and the questions the table alone answers.  The index is made of
imaginary entries (rg.create)."""
import ctypes
import os
import re

import numpy as np
import pytest

import lines_cases as lc
import range_cases as rg

N = 5000                                                    # bytes of the imaginary stream the entries describe
# decoded offsets: block 0 [0, 1000), blocks 1 and 2 of size zero, block 3 [1000, 1500)
ENTRIES = [(32, 9000, 1000, 0x11223344, 1, 0), (9000, 9200, 0, 0xFFFFFFFF, 1, 0), (9300, 9500, 0, 7, 1, 0), (20007, 39899, 500, 0x80000001, 9, 0)]
TOTAL = 1500
COUNTS = [40, 0, 0, 500]                                    # block 3: newlines only
NL = 540
FOLD = lc.crc_fold(ENTRIES)


@pytest.fixture(scope="module")
def L():
    return lc.bind()


@pytest.fixture(scope="module")
def h(L):
    rc, h = rg.create(L, ENTRIES, N, 0)
    assert rc == 0
    return h


@pytest.fixture(scope="module")
def t(L, h):
    rc, t = lc.create(L, h, COUNTS)
    assert rc == 0, rg.detail(L)
    return t


def test_create_save_load_round_trip(L, h, t):
    c = 0                                                   # the fold the image is built with, by hand
    for crc in (0x11223344, 0xFFFFFFFF, 7, 0x80000001):
        c = ((c << 1) & 0xFFFFFFFF | (c >> 31)) ^ crc
    assert FOLD == c and lc.HEADER.itemsize == 40
    raw = lc.save(L, t)
    assert raw == lc.image(COUNTS, TOTAL, FOLD) and len(raw) == 40 + 4 * 4
    rc, t2 = lc.load(L, raw, h)
    assert rc == 0 and lc.save(L, t2) == raw and lc.counts(L, t2) == COUNTS and lc.info(L, t2) == (4, NL, TOTAL)
    L.cjs_bzip2_lines_destroy(t2)
    L.cjs_bzip2_lines_destroy(None)


def test_info_and_counts(L, t):
    assert lc.info(L, t) == (4, NL, TOTAL)
    assert L.cjs_bzip2_lines_info(t, None, None, None) == 0 and L.cjs_bzip2_lines_info(None, None, None, None) == rg.E_INVALID
    assert lc.counts(L, t) == COUNTS
    c = np.full(4, 77, np.uint32)
    assert L.cjs_bzip2_lines_counts(t, c.ctypes.data_as(lc.PU32), 2) == 4 and c.tolist() == [40, 0, 77, 77]
    assert L.cjs_bzip2_lines_counts(t, c.ctypes.data_as(lc.PU32), 9) == 4 and c.tolist() == COUNTS
    assert L.cjs_bzip2_lines_counts(t, None, 0) == 4 and L.cjs_bzip2_lines_counts(t, None, 1) == rg.E_INVALID
    assert L.cjs_bzip2_lines_counts(None, None, 0) == rg.E_INVALID


def test_create_refusals(L, h):
    rc, t = lc.create(L, h, COUNTS[:3])
    assert rc == rg.E_INVALID and not t and rg.detail(L) == lc.FOREIGN
    rc, t = lc.create(L, h, COUNTS + [0])
    assert rc == rg.E_INVALID and rg.detail(L) == lc.FOREIGN
    for bad in ([1001, 0, 0, 500], [40, 1, 0, 500], [40, 0, 0, 501]):
        rc, t = lc.create(L, h, bad)
        assert rc == rg.E_INVALID and not t and "block" in rg.detail(L), bad
    rc, t = lc.create(L, h, [1000, 0, 0, 0])                # as many newlines as bytes is fine
    assert rc == 0 and lc.info(L, t) == (4, 1000, TOTAL)
    L.cjs_bzip2_lines_destroy(t)
    out = rg.V()
    c = np.array(COUNTS, np.uint32)
    assert L.cjs_bzip2_lines_create(None, c.ctypes.data_as(lc.PU32), 4, ctypes.byref(out)) == rg.E_INVALID
    assert L.cjs_bzip2_lines_create(h, None, 4, ctypes.byref(out)) == rg.E_INVALID
    assert L.cjs_bzip2_lines_create(h, c.ctypes.data_as(lc.PU32), 4, None) == rg.E_INVALID


def test_load_refusals(L, h):
    good = lc.image(COUNTS, TOTAL, FOLD)
    rc, t = lc.load(L, good, h)
    assert rc == 0
    L.cjs_bzip2_lines_destroy(t)
    cases = {
        "magic": (lc.image(COUNTS, TOTAL, FOLD, magic=b"CJSBZIX1"), "magic"),
        "version": (lc.image(COUNTS, TOTAL, FOLD, version=2), "version"),
        "flags": (lc.image(COUNTS, TOTAL, FOLD, flags=1), "flag"),
        "reserved": (lc.image(COUNTS, TOTAL, FOLD, reserved=1), "reserved"),
        "short header": (good[:39], "magic"),
        "one byte short": (good[:-1], "length"),
        "one byte long": (good + b"\0", "length"),
        "one count long": (good + bytes(4), "length"),
        "blocks field": (lc.image(COUNTS, TOTAL, FOLD, blocks=3), "length"),
        "empty": (b"", "magic"),
        "foreign blocks": (lc.image(COUNTS + [0], TOTAL, FOLD), lc.FOREIGN),
        "foreign total": (lc.image(COUNTS, TOTAL + 1, FOLD), lc.FOREIGN),
        "foreign fold": (lc.image(COUNTS, TOTAL, FOLD ^ 0x100), lc.FOREIGN),
        "count above size": (lc.image([40, 0, 1, 500], TOTAL, FOLD), "block 2"),
    }
    for name, (raw, word) in cases.items():
        rc, t = lc.load(L, raw, h)
        assert rc == rg.E_INVALID and not t and word in rg.detail(L), (name, rg.detail(L))
    a = np.frombuffer(good, np.uint8).copy()
    out = rg.V()
    assert L.cjs_bzip2_lines_load(a.ctypes.data_as(rg.u8p), a.size, None, ctypes.byref(out)) == rg.E_INVALID
    assert L.cjs_bzip2_lines_load(None, a.size, h, ctypes.byref(out)) == rg.E_INVALID
    assert L.cjs_bzip2_lines_load(a.ctypes.data_as(rg.u8p), a.size, h, None) == rg.E_INVALID
    assert L.cjs_bzip2_lines_save(None, None, None) == rg.E_INVALID


def _first(form, stream):
    return stream.ctypes.data_as(rg.u8p) if form == "host" else ctypes.c_void_p(stream.ctypes.data)      # (never looked at)


@pytest.mark.parametrize("kind", ["locate", "number"])
@pytest.mark.parametrize("form", ["host", "device"])
def test_refusals_before_the_device_is_touched(L, h, t, form, kind):
    """the question is one the table alone answers: a refusal is then the argument check's"""
    fn = getattr(L, "cjs_bzip2_lines_" + kind + ("" if form == "host" else "_device"))
    stream = np.zeros(N, np.uint8)
    q, out, st = np.zeros(2, np.uint64), np.full(2, 9, np.uint64), np.full(2, 9, np.int32)
    ok = dict(first=_first(form, stream), n=N, h=h, t=t, q=q.ctypes.data, count=2, out=out.ctypes.data, st=st.ctypes.data)

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a["first"], a["n"], a["h"], a["t"], a["q"], a["count"], a["out"], a["st"], None)
    assert call() == 0 and out.tolist() == [0, 0] and st.tolist() == [0, 0]
    for name in ("h", "t", "first", "q", "out", "st"):
        assert call(**{name: None}) == rg.E_INVALID, name
    assert call(q=None, out=None, st=None, count=0) == 0
    assert call(n=N - 1) == rg.E_INVALID and "5000" in rg.detail(L)
    # a table of another index: one block more, another total, another CRC
    for entries in (ENTRIES + [(39899, 39990, 0, 0, 1, 0)], ENTRIES[:3] + [(20007, 39899, 501, 0x80000001, 9, 0)],
                    ENTRIES[:3] + [(20007, 39899, 500, 0x80000000, 9, 0)]):
        rc, h2 = rg.create(L, entries, N, 0)
        assert rc == 0
        rc, t2 = lc.create(L, h2, [0] * len(entries))
        assert rc == 0
        assert call(t=t2) == rg.E_INVALID and rg.detail(L) == lc.FOREIGN
        assert call(h=h2) == rg.E_INVALID and rg.detail(L) == lc.FOREIGN
        assert call(h=h2, t=t2) == 0
        L.cjs_bzip2_lines_destroy(t2); L.cjs_bzip2_index_destroy(h2)


@pytest.mark.parametrize("form", ["host", "device"])
def test_build_refusals(L, h, form):
    fn = L.cjs_bzip2_lines_build if form == "host" else L.cjs_bzip2_lines_build_device
    stream = np.zeros(N, np.uint8)
    out = rg.V()
    assert fn(_first(form, stream), N, None, ctypes.byref(out), None) == rg.E_INVALID
    assert fn(_first(form, stream), N, h, None, None) == rg.E_INVALID
    assert fn(None, N, h, ctypes.byref(out), None) == rg.E_INVALID
    assert fn(_first(form, stream), N + 1, h, ctypes.byref(out), None) == rg.E_INVALID and "5000" in rg.detail(L) and not out


@pytest.mark.parametrize("form", ["host", "device"])
def test_the_table_alone_answers(L, h, t, form):
    stream = np.zeros(N, np.uint8)

    def ask(kind, hh, tt, qs):
        if form == "host":
            rc, out, st, d = lc.ask_host(L, kind, stream, hh, tt, qs)
        else:
            rc, out, st, d = lc.ask_device(L, kind, ctypes.c_void_p(stream.ctypes.data), N, hh, tt, qs)
        assert rc == 0 and d == "" and not st.any()
        return out.tolist()
    # line 0 and lines above N (N itself needs block 3: it is not asked here)
    assert ask("locate", h, t, [0, NL + 1, NL + 2, 2 ** 63, lc.TOP, 0]) == [0, TOTAL, TOTAL, TOTAL, TOTAL, 0]
    # offsets at block starts (the blocks of size zero start where block 3 does) and at or behind the end
    assert ask("number", h, t, [0, 1000, TOTAL, TOTAL + 7, lc.TOP, 1000, 0]) == [0, 40, NL, NL, NL, 40, 0]
    assert ask("locate", h, t, []) == [] and ask("number", h, t, []) == []
    # without a GPU a question that needs a block says so
    import torch
    if not torch.cuda.is_available() and form == "host":
        assert lc.ask_host(L, "locate", stream, h, t, [0, 1])[0] == rg.E_NO_DEVICE
        assert lc.ask_host(L, "number", stream, h, t, [0, 1])[0] == rg.E_NO_DEVICE


@pytest.mark.parametrize("form", ["host", "device"])
def test_empty_stream_and_blocks_of_size_zero(L, form):
    """an index without blocks (an empty stream) and one of zero-size blocks only: the build and every question without a device"""
    stream = np.zeros(N, np.uint8)
    for entries in ([], [e for e in ENTRIES if e[2] == 0]):
        rc, h = rg.create(L, entries, N, 0)
        assert rc == 0
        if form == "host":
            rc, t, d = lc.build_host(L, stream, h)
        else:
            rc, t, d = lc.build_device(L, ctypes.c_void_p(stream.ctypes.data), N, h)
        assert rc == 0 and d == "" and lc.counts(L, t) == [0] * len(entries) and lc.info(L, t) == (len(entries), 0, 0)
        assert lc.save(L, t) == lc.image([0] * len(entries), 0, lc.crc_fold(entries))
        for kind, qs in (("locate", [0, 1, 5, lc.TOP]), ("number", [0, 1, lc.TOP])):
            if form == "host":
                rc, out, st, d = lc.ask_host(L, kind, stream, h, t, qs)
            else:
                rc, out, st, d = lc.ask_device(L, kind, ctypes.c_void_p(stream.ctypes.data), N, h, t, qs)
            assert rc == 0 and out.tolist() == [0] * len(qs) and not st.any()
        L.cjs_bzip2_lines_destroy(t); L.cjs_bzip2_index_destroy(h)


def test_expectation_helpers_agree_with_the_table(L):
    """the reference the GPU tests compare with, against values written by hand; the table's questions on the same text"""
    plain = np.frombuffer(b"ab\n\ncd\x0b\n\x8ae", np.uint8)
    nl = lc.newlines(plain)
    assert nl.tolist() == [2, 3, 7]
    assert [lc.start(nl, 10, k) for k in (0, 1, 2, 3, 4, lc.TOP)] == [0, 3, 4, 8, 10, 10]
    assert [lc.number(nl, 10, o) for o in (0, 2, 3, 4, 7, 8, 10, 17, lc.TOP)] == [0, 0, 1, 2, 2, 3, 3, 3, 3]
    assert lc.block_counts(plain, [0, 3, 3, 10]) == [1, 0, 2]
    # an imaginary index of that text (blocks [0, 3), [3, 3), [3, 10)): the answers the table alone gives are the helpers'
    rc, h = rg.create(L, [(32, 200, 3, 1, 1, 0), (200, 300, 0, 2, 1, 0), (300, 500, 7, 3, 1, 0)], 100, 0)
    assert rc == 0
    rc, t = lc.create(L, h, [1, 0, 2])
    assert rc == 0
    stream = np.zeros(100, np.uint8)
    rc, out, st, d = lc.ask_host(L, "locate", stream, h, t, [0, 4, 9])
    assert rc == 0 and out.tolist() == [lc.start(nl, 10, k) for k in (0, 4, 9)]
    rc, out, st, d = lc.ask_host(L, "number", stream, h, t, [0, 3, 10, 17])
    assert rc == 0 and out.tolist() == [lc.number(nl, 10, o) for o in (0, 3, 10, 17)]
    L.cjs_bzip2_lines_destroy(t); L.cjs_bzip2_index_destroy(h)


def test_the_abi_is_declared_and_exported(L):
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cjs_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = ["build", "build_device", "create", "save", "load", "info", "counts", "destroy", "locate", "locate_device", "number", "number_device"]
    for name in names:
        assert re.search(r"\bcjs_bzip2_lines_%s\s*\(" % name, src) and hasattr(L, "cjs_bzip2_lines_" + name), name
    assert "typedef struct cjs_bz_lines cjs_bz_lines;" in src and not re.search(r"struct cjs_bz_lines\s*\{", src)
