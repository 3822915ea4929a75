"""The host side of the line sort, without a GPU: cjs_stage_text_sort (the rounds of csrc/sort_plan.h) against the Python
restatement sort_text and against sorted() over the real lines on random texts, the refusals of the four GPU entry points before a
device is touched, n == 0 and an empty window without a device, and the argument handling of the Python front."""
import ctypes
import importlib

import numpy as np
import pytest

import lines_cases as lc
import range_cases as rg
import sort_cases as sc


@pytest.fixture(scope="module")
def L():
    return sc.bind()


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("compressjs-flattened_amd")


def random_text(rng, k):
    alphabet = (b"ab", b"a\x00\xff", bytes(x for x in range(256) if x != 10))[k % 3]
    out = []
    for _ in range(int(rng.randint(0, 80))):
        base = (0, 6, 7, 8, 14)[rng.randint(0, 5)]
        n = int(base - 1 + rng.randint(0, 3)) if base else int(rng.randint(0, 2))
        out.append(bytes(alphabet[i] for i in rng.randint(0, len(alphabet), n)))
    text = b"\n".join(out) + (b"\n" if out and k % 4 else b"")
    return text


def test_stage_sort_against_the_restatement_on_300_random_texts(L, pkg):
    rng = np.random.RandomState(4321)
    for k in range(300):
        text = random_text(rng, k)
        flags = k & 3
        want_lines, want_counts, winfo, _ = sc.sort_ref(sc.split_lines(text), flags)
        assert pkg.sort_text(text, bool(flags & sc.REVERSE), bool(flags & sc.UNIQUE)) == (want_lines, want_counts)
        rc, lines, counts, info = sc.stage_sort(L, text, flags)
        assert rc == 0 and sc.info5(info) == winfo and (lines, counts) == (want_lines, want_counts), (k, text)
        assert info.rounds <= (max([len(x) for x in sc.split_lines(text)] + [0]) + 8) // 7
        cap = int(rng.randint(0, 5))
        rc, lines, counts, info = sc.stage_sort(L, text, flags ^ 3, cap, counts=bool(k & 4))
        w2 = sc.sort_ref(sc.split_lines(text), flags ^ 3)
        assert rc == 0 and sc.info5(info) == w2[2] and lines == w2[0][:cap] and counts == (w2[1][:cap] if k & 4 else [])


def test_the_restatement_is_the_issues_rule(pkg):
    text = b"b\nab\x00\nab\nb\nab\x00\x00\nab\x01\n\nb"
    assert sc.split_lines(text) == [b"b", b"ab\x00", b"ab", b"b", b"ab\x00\x00", b"ab\x01", b"", b"b"]
    assert pkg.sort_text(text) == ([6, 2, 1, 4, 5, 0, 3, 7], [1] * 8)
    assert pkg.sort_text(text, reverse=True) == ([0, 3, 7, 5, 4, 1, 2, 6], [1] * 8)          # descending content, ties still ascending
    assert pkg.sort_text(text, unique=True) == ([6, 2, 1, 4, 5, 0], [1, 1, 1, 1, 1, 3])
    assert pkg.sort_text(text, reverse=True, unique=True) == ([0, 5, 4, 1, 2, 6], [3, 1, 1, 1, 1, 1])
    assert pkg.sort_text(b"") == ([], []) and pkg.sort_text(b"\n") == ([0], [1]) and pkg.sort_text(b"x") == ([0], [1])
    assert sc.sort_ref(sc.split_lines(text))[2] == (8, 8, 6, len(text) + 1, 1)
    assert sc.sort_ref([b"abcdefg", b"abcdefg"])[2][4] == 2 and sc.sort_ref([b"abcdefgh", b"abcdefgi"])[2][4] == 2 and sc.sort_ref([b"abcdef", b"abcdef"])[2][4] == 1
    assert sc.sort_ref([])[2] == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("name", ("cjs_text_sort", "cjs_text_sort_device"))
def test_argument_errors_arrive_before_the_device_is_touched(L, name):
    fn = getattr(L, name)
    text = np.frombuffer(b"b\na\nc\nd\n", dtype=np.uint8)           # (host memory: the device form would refuse it, but only behind these)
    lines, counts = np.zeros(8, np.uint64), np.zeros(8, np.uint64)
    info = sc.SortInfo()
    out, tn = rg.u8p(), rg.S(0)
    t, lo, co, i = text.ctypes.data, lines.ctypes.data, counts.ctypes.data, ctypes.byref(info)
    none = (None, None) if name == "cjs_text_sort" else (None, 0, None)
    assert fn(t, 8, 0, lo, co, 8, *none, None, None) == sc.E_INVALID                 # NULL info
    assert fn(None, 8, 0, lo, co, 8, *none, i, None) == sc.E_INVALID                 # NULL text with n
    assert fn(t, 8, 0, None, co, 8, *none, i, None) == sc.E_INVALID                  # NULL lines_out with cap
    assert fn(t, 8, 4, lo, co, 8, *none, i, None) == sc.E_INVALID                    # an unknown flag
    assert fn(t, sc.MAX + 1, 0, None, None, 0, *none, i, None) == sc.E_UNSUPPORTED
    if name == "cjs_text_sort":
        assert fn(t, 8, 0, lo, co, 8, ctypes.byref(out), None, i, None) == sc.E_INVALID      # one of text_out / text_n without the other
        assert fn(t, 8, 0, lo, co, 8, None, ctypes.byref(tn), i, None) == sc.E_INVALID
    else:
        assert fn(t, 8, 0, lo + 4, co, 7, *none, i, None) == sc.E_INVALID            # lines_out not 8-byte aligned
        assert fn(t, 8, 0, lo, co + 4, 7, *none, i, None) == sc.E_INVALID
        assert fn(t, 8, 0, lo, co, 8, None, 16, ctypes.byref(tn), i, None) == sc.E_INVALID       # NULL d_text_out with text_cap
        assert fn(t, 8, 0, lo, co, 8, t, 16, None, i, None) == sc.E_INVALID                      # d_text_out without text_n


@pytest.mark.parametrize("name", ("cjs_text_sort", "cjs_text_sort_device", "cjs_stage_text_sort"))
def test_no_text_is_answered_without_a_device(L, name):
    info = sc.SortInfo(*([7] * 8))
    lines = np.full(2, sc.CANARY64, np.uint64)
    out, tn = rg.u8p(), rg.S(5)
    for t, lo, cap in ((None, None, 0), (lines.ctypes.data, lines.ctypes.data, 2)):
        if name == "cjs_text_sort":
            assert L.cjs_text_sort(t, 0, 3, lo, None, cap, ctypes.byref(out), ctypes.byref(tn), ctypes.byref(info), None) == 0
            assert tn.value == 0 and out
            L.cjs_free(out)
        elif name == "cjs_text_sort_device":
            assert L.cjs_text_sort_device(t, 0, 3, lo, None, cap, None, 0, ctypes.byref(tn), ctypes.byref(info), None) == 0 and tn.value == 0
        else:
            assert L.cjs_stage_text_sort(t, 0, 3, lo, None, cap, ctypes.byref(info)) == 0
        assert sc.info_all(info) == (0, 0, 0, 0, 0, 0, 0, sc.M64) and (lines == sc.CANARY64).all()


N_STREAM = 5000                                             # bytes of the imaginary stream the entries describe
ENTRIES = [(32, 9000, 1000, 0x11223344, 1, 0), (9000, 9200, 0, 0xFFFFFFFF, 1, 0), (9300, 9500, 0, 7, 1, 0), (20007, 39899, 500, 0x80000001, 9, 0)]
COUNTS = [40, 0, 0, 500]


@pytest.mark.parametrize("name", ("cjs_bzip2_sort", "cjs_bzip2_sort_device"))
def test_stream_argument_errors_arrive_before_the_device_is_touched(L, name):
    rc, h = rg.create(L, ENTRIES, N_STREAM, 0)
    assert rc == 0
    rc, t = lc.create(L, h, COUNTS)
    assert rc == 0
    rc, h2 = rg.create(L, ENTRIES[:3], N_STREAM, 0)
    assert rc == 0
    rc, t2 = lc.create(L, h2, COUNTS[:3])
    assert rc == 0
    stream = np.zeros(N_STREAM, np.uint8)
    lines = np.zeros(4, np.uint64)
    info = sc.SortInfo()
    host = name == "cjs_bzip2_sort"
    # (the device form gets a host address for d_in: no call here may come as far as looking at it)
    src = stream.ctypes.data_as(rg.u8p) if host else stream.ctypes.data
    fn = getattr(L, name)
    one = np.array([(1, 1)], dtype=sc.RANGE)
    text_args = [None, None] if host else [None, 0, None]
    ok = [src, N_STREAM, h, t, 0, 5, sc.LINES, 0, None, 0, 0, lines.ctypes.data, None, 4] + text_args + [ctypes.byref(info), None]
    at_info = len(ok) - 2
    for at, value in ((0, None), (1, N_STREAM - 1), (2, None), (3, None), (3, t2), (6, 3), (10, 4), (11, None), (at_info, None)):
        a = list(ok)
        a[at] = value
        assert fn(*a) == sc.E_INVALID, at
    out, tn = rg.u8p(), rg.S(0)
    if host:
        for pair in ((ctypes.byref(out), None), (None, ctypes.byref(tn))):
            a = list(ok)
            a[14:16] = pair
            assert fn(*a) == sc.E_INVALID
    else:
        for triple in ((None, 8, ctypes.byref(tn)), (stream.ctypes.data, 8, None)):
            a = list(ok)
            a[14:17] = triple
            assert fn(*a) == sc.E_INVALID
    # the selection of a cut mode is checked as the cut checks it
    for mode, d, sel, nsel in ((sc.FIELDS, 9, None, 1), (sc.FIELDS, 9, one.ctypes.data, 0), (sc.FIELDS, 9, one.ctypes.data, 65), (sc.FIELDS, 10, one.ctypes.data, 1),
                               (sc.BYTES, 256, one.ctypes.data, 1)):
        a = list(ok)
        a[6:10] = [mode, d, sel, nsel]
        assert fn(*a) == sc.E_INVALID, (mode, d, nsel)
    assert rg.detail(L) == "" and fn(*(ok[:3] + [t2] + ok[4:])) == sc.E_INVALID and rg.detail(L) == lc.FOREIGN
    # an empty window is answered without a device; windows above the limits are refused before one is touched
    a = list(ok)
    a[4], a[5] = 541, 9
    if host:
        a[14:16] = [ctypes.byref(out), ctypes.byref(tn)]
    assert fn(*a) == 0 and sc.info_all(info) == (0, 0, 0, 0, 0, 0, 0, sc.M64)
    if host:
        assert out and tn.value == 0
        L.cjs_free(out)
    pair = (stream.ctypes.data, None) if host else (None, stream.ctypes.data)
    limit = lambda mb, ml, p=pair: L.cjs_stage_bzip2_sort_limit(p[0], p[1], N_STREAM, h, t, 0, 5, mb, ml, 0, lines.ctypes.data, None, 4, ctypes.byref(info), None)
    assert limit(2 ** 40, 4) == sc.E_UNSUPPORTED and limit(999, 2 ** 40) == sc.E_UNSUPPORTED
    assert limit(2 ** 40, 2 ** 40, (None, None)) == sc.E_INVALID and limit(2 ** 40, 2 ** 40, (stream.ctypes.data, stream.ctypes.data)) == sc.E_INVALID
    for x in (t, t2):
        L.cjs_bzip2_lines_destroy(x)
    for x in (h, h2):
        L.cjs_bzip2_index_destroy(x)


def test_the_python_front_checks_its_arguments(pkg):
    with pytest.raises(ValueError):
        pkg.text_sort(b"a\nb\n", limit=-1)
    res = pkg.text_sort(b"", want_text=True)                 # no text: no device
    assert (res.n_lines, res.n_out, res.n_distinct, res.text_bytes, res.rounds) == (0, 0, 0, 0, 0)
    assert res.lines.dtype == np.uint64 and res.lines.size == 0 and res.counts.size == 0 and res.text == b""
    assert ctypes.sizeof(pkg.SortInfo) == 64 and (pkg.SORT_REVERSE, pkg.SORT_UNIQUE, pkg.SORT_LINES) == (1, 2, 2)
