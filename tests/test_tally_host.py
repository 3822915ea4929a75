"""The host side of the key tally, without a GPU: cjs_stage_keys_tally (csrc/tally_plan.h) against the restatement
tally_cases.tally_ref on random key lists, the refusals of both GPU entry points before a device is touched, n == 0 without a
device, and the argument handling of the Python front."""
import ctypes
import importlib

import numpy as np
import pytest

import lines_cases as lc
import range_cases as rg
import tally_cases as tc


@pytest.fixture(scope="module")
def L():
    return tc.bind()


def _agree(L, tuples, order, lo, hi, cap=None):
    want, winfo = tc.tally_ref(tuples, order, lo, hi)
    rc, got, info = tc.stage_tally(L, tc.key_array(tuples), order, lo, hi, cap)
    assert rc == 0 and tc.info_tuple(info) == winfo, (order, lo, hi)
    assert tc.groups_as_tuples(got) == want[:len(tuples) if cap is None else cap], (order, lo, hi, cap)


def test_stage_tally_against_the_restatement_on_300_random_lists(L):
    rng = np.random.RandomState(1234)
    filters = ((1, 0), (2, 0), (1, 1), (2, 3), (0, 0))
    for k in range(300):
        tuples = tc.random_keys(rng, int(rng.randint(0, 500)), 1 + int(rng.randint(0, 60)), bad_share=(0.0, 0.05, 0.5)[k % 3])
        lo, hi = filters[k % 5]
        _agree(L, tuples, k & 1, lo, hi)
        _agree(L, tuples, 1 - (k & 1), lo, hi, cap=int(rng.randint(0, 5)))


def test_the_restatement_is_the_issues_rule():
    a, b, c = (1, 2, 3), (1, 2, 4), (9, 2, 3)
    items = [b, a, tc.ONES, a, c, b, a]
    assert tc.tally_ref(items, tc.BY_COUNT) == ([(a, 1, 3), (b, 0, 2), (c, 4, 1)], (7, 1, 3, 3, 3))
    assert tc.tally_ref(items, tc.BY_FIRST) == ([(b, 0, 2), (a, 1, 3), (c, 4, 1)], (7, 1, 3, 3, 3))
    assert tc.tally_ref(items, tc.BY_FIRST, 2) == ([(b, 0, 2), (a, 1, 3)], (7, 1, 3, 2, 3))          # uniq -d
    assert tc.tally_ref(items, tc.BY_FIRST, 1, 1) == ([(c, 4, 1)], (7, 1, 3, 1, 3))                 # uniq -u
    assert tc.tally_ref([b, b, a, a], tc.BY_COUNT)[0] == [(b, 0, 2), (a, 2, 2)]                      # a count tie: by first occurrence
    assert tc.tally_ref([], tc.BY_COUNT) == ([], (0, 0, 0, 0, 0))


@pytest.mark.parametrize("name", ("cjs_keys_tally", "cjs_keys_tally_device"))
def test_argument_errors_arrive_before_the_device_is_touched(L, name):
    fn = getattr(L, name)
    keys = np.zeros(8, dtype=tc.KEY)                      # (host memory: the device form would refuse it, but only behind these)
    out = np.zeros(8, dtype=tc.TALLY)
    info = tc.TallyInfo()
    k, o, i = keys.ctypes.data, out.ctypes.data, ctypes.byref(info)
    assert fn(k, 8, tc.BY_COUNT, 1, 0, o, 8, None, None) == tc.E_INVALID                 # NULL info
    assert fn(None, 8, tc.BY_COUNT, 1, 0, o, 8, i, None) == tc.E_INVALID                 # NULL keys with n
    assert fn(k, 8, tc.BY_COUNT, 1, 0, None, 8, i, None) == tc.E_INVALID                 # NULL out with cap
    assert fn(k, 8, 2, 1, 0, o, 8, i, None) == tc.E_INVALID                              # an unknown order
    assert fn(k, 8, tc.BY_FIRST, 3, 2, o, 8, i, None) == tc.E_INVALID                    # max_count below min_count
    assert fn(k, tc.MAX_KEYS + 1, tc.BY_FIRST, 1, 0, None, 0, i, None) == tc.E_UNSUPPORTED
    if name.endswith("_device"):
        assert fn(k + 4, 7, tc.BY_FIRST, 1, 0, o, 7, i, None) == tc.E_INVALID            # keys not 8-byte aligned
        assert fn(k, 8, tc.BY_FIRST, 1, 0, o + 8, 7, i, None) == tc.E_INVALID            # out not 16-byte aligned


@pytest.mark.parametrize("name", ("cjs_keys_tally", "cjs_keys_tally_device", "cjs_stage_keys_tally"))
def test_no_keys_are_answered_without_a_device(L, name):
    info = tc.TallyInfo(7, 7, 7, 7, 7)
    out = np.full(2 * tc.TALLY.itemsize, tc.CANARY, np.uint8)
    tail = () if name.startswith("cjs_stage") else (None,)
    for keys, o, cap in ((None, None, 0), (out.ctypes.data, out.ctypes.data, 2)):
        assert getattr(L, name)(keys, 0, tc.BY_COUNT, 1, 0, o, cap, ctypes.byref(info), *tail) == 0
        assert tc.info_tuple(info) == (0, 0, 0, 0, 0) and (out == tc.CANARY).all()


N_STREAM = 5000                                             # bytes of the imaginary stream the entries describe
ENTRIES = [(32, 9000, 1000, 0x11223344, 1, 0), (9000, 9200, 0, 0xFFFFFFFF, 1, 0), (9300, 9500, 0, 7, 1, 0), (20007, 39899, 500, 0x80000001, 9, 0)]
COUNTS = [40, 0, 0, 500]


@pytest.mark.parametrize("name", ("cjs_bzip2_tally", "cjs_bzip2_tally_device"))
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
    out = np.zeros(4, dtype=tc.TALLY)
    info = tc.StreamInfo()
    # (the device form gets a host address for d_in: no call here may come as far as looking at it)
    src = stream.ctypes.data_as(rg.u8p) if name == "cjs_bzip2_tally" else stream.ctypes.data
    fn = getattr(L, name)
    one = np.array([(1, 1)], dtype=np.dtype([("lo", "<u4"), ("hi", "<u4")]))
    ok = [src, N_STREAM, h, t, 0, 5, 0, tc.LINES, 0, None, 0, tc.BY_COUNT, 1, 0, out.ctypes.data, 4, ctypes.byref(info), None]
    for at, value in ((0, None), (1, N_STREAM - 1), (2, None), (3, None), (3, t2), (7, 3), (11, 2), (13, None), (14, None), (16, None)):
        a = list(ok)
        a[at] = value
        if at == 13:
            a[12], a[13] = 3, 2                             # max_count below min_count
        assert fn(*a) == tc.E_INVALID, at
    # the selection of a cut mode is checked as the cut checks it
    for mode, d, sel, nsel in ((tc.FIELDS, 9, None, 1), (tc.FIELDS, 9, one.ctypes.data, 0), (tc.FIELDS, 9, one.ctypes.data, 65), (tc.FIELDS, 10, one.ctypes.data, 1),
                               (tc.BYTES, 256, one.ctypes.data, 1)):
        a = list(ok)
        a[7:11] = [mode, d, sel, nsel]
        assert fn(*a) == tc.E_INVALID, (mode, d, nsel)
    assert rg.detail(L) == "" and fn(*(ok[:3] + [t2] + ok[4:])) == tc.E_INVALID and rg.detail(L) == lc.FOREIGN
    # an empty window is answered without a device; a window above the line limit is refused before one is touched
    a = list(ok)
    a[4], a[5] = 541, 9
    assert fn(*a) == 0 and tc.stream_info_tuple(info) == (0, 0, 0, 0, 0, 0, 0, tc.M64)
    pair = (stream.ctypes.data, None) if name == "cjs_bzip2_tally" else (None, stream.ctypes.data)
    assert L.cjs_stage_bzip2_tally_limit(pair[0], pair[1], N_STREAM, h, t, 0, 5, 4, out.ctypes.data, 4, ctypes.byref(info), None) == tc.E_UNSUPPORTED
    assert L.cjs_stage_bzip2_tally_limit(None, None, N_STREAM, h, t, 0, 5, 4, out.ctypes.data, 4, ctypes.byref(info), None) == tc.E_INVALID
    size = rg.S(0)
    assert L.cjs_stage_text_keys_device(None, 5, 0, None, 0, ctypes.byref(size), 0, None) == tc.E_INVALID          # NULL text with n
    assert L.cjs_stage_text_keys_device(stream.ctypes.data, 5, 0, None, 4, ctypes.byref(size), 0, None) == tc.E_INVALID          # NULL keys with cap
    assert L.cjs_stage_text_keys_device(stream.ctypes.data, 5, 0, None, 0, None, 0, None) == tc.E_INVALID
    for x in (t, t2):
        L.cjs_bzip2_lines_destroy(x)
    for x in (h, h2):
        L.cjs_bzip2_index_destroy(x)


def test_the_python_front_checks_its_arguments():
    pkg = importlib.import_module("compressjs-flattened_amd")
    keys = np.zeros(3, dtype=pkg.LINE_KEY_DTYPE)
    for kw in ({"order": "content"}, {"min_count": -1}, {"min_count": 3, "max_count": 2}, {"limit": -1}):
        with pytest.raises(ValueError):
            pkg.tally_keys(keys, **kw)
    res = pkg.tally_keys(keys[:0])                        # no keys: no device
    assert (res.n_lines, res.n_bad_lines, res.n_distinct, res.n_groups, res.max_count) == (0, 0, 0, 0, 0)
    assert res.groups.dtype == pkg.TALLY_DTYPE and res.groups.size == 0 and pkg.TALLY_DTYPE.itemsize == 32
    assert ctypes.sizeof(pkg.TallyInfo) == 40
