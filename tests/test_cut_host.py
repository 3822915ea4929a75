"""The host side of the column cut, without a GPU: cjs_stage_cut (csrc/cut_plan.h walked over a plain buffer) and cjs_cut_list_parse
against the restatement cut_cases.cut_ref, the refusals of both GPU entry points before a device is touched (the index is made of
imaginary entries), and cut_ref itself against GNU cut where that is on the path."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import cut_cases as ct
import lines_cases as lc
import range_cases as rg

LISTS = ("1", "2", "1,3", "2-", "-2", "3-5,9", "65,300", "1-", "400", "7,2,2-4,3-3", "2,4,70-90")


@pytest.fixture(scope="module")
def L():
    return ct.bind()


def _random_texts():
    rng = np.random.RandomState(77)
    out = []
    for i in range(300):
        d = (ord(","), 0, 0xFF, ord("\t"))[i % 4]
        alphabet = np.array([d, d, 10, 97, 98, 0x0B][:4 + i % 3], np.uint8)
        out.append((d, bytes(rng.choice(alphabet, int(rng.randint(0, 2001))))))
    return out


def _corners():
    wide = b",".join(b"f%d" % k for k in range(1, 301))
    return {"empty": b"", "only newlines": b"\n\n\n\n", "only delimiters": b",,,,", "delimiters, then a newline": b",,,\n,\n",
            "no final newline": b"a,b,c\nd,e", "a final newline": b"a,b,c\nd,e\n", "a delimiter first and last": b",a,b,\n,\n,x\nx,\n",
            "a line of 300 fields": b"x\n" + wide + b"\n" + wide[:-1], "no delimiter": b"abc\ndefgh\n\nij"}


def _check(L, text, d, lists=LISTS):
    for spec in lists:
        rc, sel = ct.parse(L, spec)
        assert rc == 0 and sel == ct.ref_list(spec), spec
        for mode in (ct.FIELDS, ct.BYTES):
            want = ct.cut_ref(text, mode, d, sel)
            rc, got, n = ct.stage_cut(L, text, mode, d, sel)
            assert rc == 0 and n == len(want) and got == want, (spec, mode, d, text[:80])


def test_random_texts_against_the_restatement(L):
    for k, (d, text) in enumerate(_random_texts()):
        _check(L, text, d, LISTS[k % 3::3])


@pytest.mark.parametrize("name", sorted(_corners()))
def test_corner_texts(L, name):
    _check(L, _corners()[name], ord(","))


@pytest.mark.parametrize("d", (0x00, 0xFF))
def test_delimiters_at_the_ends_of_the_byte_range(L, d):
    text = _corners()["a delimiter first and last"].replace(b",", bytes([d])) + _corners()["a line of 300 fields"].replace(b",", bytes([d]))
    _check(L, text, d)


def test_the_restatement_is_the_issues_rule():
    f = lambda text, spec, mode=ct.FIELDS: ct.cut_ref(text, mode, ord(","), ct.ref_list(spec))
    assert f(b"a,b,c\nd\n\ne,f", "2") == b"b\n\n\nf\n"                  # a line without the delimiter is a line of one field
    assert f(b"a,b,c\nd\n\ne,f", "1,3") == b"a,c\nd\n\ne\n"
    assert f(b"a,b,c\n", "2-") == b"b,c\n" and f(b",,\n", "2-") == b",\n" and f(b",,\n", "1-") == b",,\n" and f(b"a\n", "400") == b"\n"
    assert f(b"abcdef\ngh\n", "2,4-", ct.BYTES) == b"bdef\nh\n" and f(b"", "1") == b"" and f(b"\n", "1") == b"\n" and f(b"x", "1") == b"x\n"
    assert ct.cut_ref(b"a\nb\nc", ct.FIELDS, 44, [(1, 1)], first=1, count=1) == b"b\n" and ct.cut_ref(b"a\nb\nc", ct.FIELDS, 44, [(1, 1)], first=2) == b"c\n"
    assert ct.cut_ref(b"a\nb\n", ct.FIELDS, 44, [(1, 1)], first=2) == b"" and ct.normal([(7, 7), (2, 2), (2, 4), (3, 3), (5, ct.TO_END)]) == [(2, ct.TO_END)]


def test_unordered_and_overlapping_ranges_equal_their_normal_form(L):
    text = _corners()["a line of 300 fields"] + b"\n" + _random_texts()[9][1].replace(b"\0", b",")
    for sel in ([(7, 7), (2, 2), (2, 4), (3, 3)], [(70, 90), (1, 1), (80, 300), (65, 66)], [(5, ct.TO_END), (1, 2), (3, 3)], [(2, 2)] * 64):
        for mode in (ct.FIELDS, ct.BYTES):
            rc, got, n = ct.stage_cut(L, text, mode, 44, sel)
            rc2, got2, n2 = ct.stage_cut(L, text, mode, 44, ct.normal(sel))
            assert rc == rc2 == 0 and got == got2 == ct.cut_ref(text, mode, 44, sel)


def test_a_cap_one_byte_short(L):
    text = _corners()["a final newline"] * 30 + b"tail,of,it"
    for spec, mode in (("2", ct.FIELDS), ("1-", ct.FIELDS), ("2-3", ct.BYTES)):
        sel = ct.ref_list(spec)
        want = ct.cut_ref(text, mode, 44, sel)
        rc, got, n = ct.stage_cut(L, text, mode, 44, sel, cap=len(want) - 1)      # (stage_cut checks the canaries behind the cap)
        assert rc == rg.E_TOO_SMALL and n == len(want) and got == want[:-1]
        rc, got, n = ct.stage_cut(L, text, mode, 44, sel, cap=len(want))
        assert rc == 0 and got == want
        rc, got, n = ct.stage_cut(L, text, mode, 44, sel, cap=0)
        assert rc == rg.E_TOO_SMALL and n == len(want) and got == b""


def test_parser_refusals(L):
    for spec in ("", ",", "1,", ",1", "0", "5-3", "-", "1--2", "a", "1 ,2", "4294967295", "1-2-3"):
        assert ct.parse(L, spec) == (rg.E_INVALID, []), spec
    assert ct.parse(L, "1,2,3", cap=2)[0] == rg.E_INVALID and ct.parse(L, "1,2", cap=2) == (0, [(1, 1), (2, 2)])
    assert ct.parse(L, ",".join(str(k) for k in range(1, 65))) == (0, [(k, k) for k in range(1, 65)])
    n = ct.U32(0)
    assert L.cjs_cut_list_parse(None, None, 0, ctypes.byref(n)) == rg.E_INVALID and L.cjs_cut_list_parse(b"1", None, 4, ctypes.byref(n)) == rg.E_INVALID


def test_stage_cut_argument_errors(L):
    n = rg.S(0)
    out = np.zeros(16, np.uint8)
    one = ct.sel_array([(1, 1)])
    ok = [b"a,b\n", 4, ct.FIELDS, 44, one.ctypes.data, 1, out.ctypes.data, 16, ctypes.byref(n)]
    assert L.cjs_stage_cut(*ok) == 0 and n.value == 2
    for at, value in ((0, None), (2, 2), (3, 256), (3, 10), (4, None), (5, 0), (5, 65), (6, None), (8, None)):
        a = list(ok)
        a[at] = value
        assert L.cjs_stage_cut(*a) == rg.E_INVALID, (at, value)
    for bad in ([(0, 1)], [(3, 2)], [(1, 1), (0, ct.TO_END)]):
        r = ct.sel_array(bad)
        assert L.cjs_stage_cut(b"a,b\n", 4, ct.FIELDS, 44, r.ctypes.data, len(bad), out.ctypes.data, 16, ctypes.byref(n)) == rg.E_INVALID
    assert L.cjs_stage_cut(b"a\nb\n", 4, ct.BYTES, 10, one.ctypes.data, 1, out.ctypes.data, 16, ctypes.byref(n)) == 0       # bytes mode ignores delim = newline


# ---------------------------------------------------------------- the GPU entry points' refusals, before a device is touched
N = 5000                                                    # bytes of the imaginary stream the entries describe
ENTRIES = [(32, 9000, 1000, 0x11223344, 1, 0), (9000, 9200, 0, 0xFFFFFFFF, 1, 0), (9300, 9500, 0, 7, 1, 0), (20007, 39899, 500, 0x80000001, 9, 0)]
COUNTS = [40, 0, 0, 500]


@pytest.mark.parametrize("form", ("host", "device"))
def test_argument_errors_arrive_before_the_device_is_touched(L, form):
    rc, h = rg.create(L, ENTRIES, N, 0)
    assert rc == 0
    rc, t = lc.create(L, h, COUNTS)
    assert rc == 0
    rc, h2 = rg.create(L, ENTRIES[:3], N, 0)
    assert rc == 0
    rc, t2 = lc.create(L, h2, COUNTS[:3])
    assert rc == 0
    stream = np.zeros(N, np.uint8)
    one = ct.sel_array([(1, 1)])
    many = ct.sel_array([(k, k) for k in range(1, 66)])
    info = ct.CutInfo()
    out, n = rg.u8p(), rg.S(0)
    # (the device form gets a host address for d_in and d_out: no call here may come as far as looking at them)
    if form == "host":
        fn = L.cjs_bzip2_cut
        ok = [stream.ctypes.data_as(rg.u8p), N, h, t, 0, 5, ct.FIELDS, 9, one.ctypes.data, 1, ctypes.byref(out), ctypes.byref(n), ctypes.byref(info), None]
        nulls = (0, 2, 3, 8, 10, 11, 12)
    else:
        fn = L.cjs_bzip2_cut_device
        ok = [stream.ctypes.data, N, h, t, 0, 5, ct.FIELDS, 9, one.ctypes.data, 1, stream.ctypes.data, 16, ctypes.byref(n), ctypes.byref(info), None]
        nulls = (0, 2, 3, 8, 10, 12, 13)
    cases = [(at, None) for at in nulls] + [(1, N - 1), (3, t2), (6, 2), (6, 0xFFFFFFFF), (7, 256), (7, 10), (9, 0), (9, 65)]
    for at, value in cases:
        a = list(ok)
        a[at] = value
        if (at, value) == (9, 65):
            a[8] = many.ctypes.data
        assert fn(*a) == rg.E_INVALID, (form, at, value)
        assert not out
    for bad in ([(0, 1)], [(3, 2)], [(1, 1), (0, 5)]):
        a = list(ok)
        r = ct.sel_array(bad)
        a[8], a[9] = r.ctypes.data, len(bad)
        assert fn(*a) == rg.E_INVALID, (form, bad)
    a = list(ok)
    a[3] = t2
    assert fn(*a) == rg.E_INVALID and rg.detail(L) == lc.FOREIGN
    # an empty window is answered by the table alone, without a device
    a = list(ok)
    a[4], a[5] = 3, 0
    if form == "device":
        a[10], a[11] = None, 0
    assert fn(*a) == 0 and info.n_lines == 0 and info.out_bytes == 0 and info.blocks_decoded == 0
    if form == "host":
        assert out and n.value == 0
        L.cjs_free(out)
    for x in (t, t2):
        L.cjs_bzip2_lines_destroy(x)
    for x in (h, h2):
        L.cjs_bzip2_index_destroy(x)


# ---------------------------------------------------------------- the restatement against GNU cut
def _cut_fixture():
    """about 20 KB in which EVERY line holds the delimiter and ends in a newline: the one stated difference from GNU cut (a line
    without the delimiter) cannot occur"""
    rng = np.random.RandomState(5)
    lines = []
    while sum(len(x) for x in lines) < 20000:
        k = int(rng.randint(2, 13))
        fields = [bytes(rng.randint(97, 123, int(rng.randint(0, 9))).astype(np.uint8)) for _ in range(k)]
        lines.append(b",".join(fields) + b"\n")
    lines += [b",\n", b",,,,\n", b"a,\n", b",b\n"]
    return b"".join(lines)


GNU_LISTS = ("1", "2", "1,3", "2-", "-2", "3-5,9")


@pytest.mark.skipif(shutil.which("cut") is None, reason="no cut on the path")
def test_the_restatement_is_what_cut_writes():
    text = _cut_fixture()
    assert all(b"," in ln for ln in text.split(b"\n")[:-1]) and text.endswith(b"\n")
    env = dict(os.environ, LC_ALL="C")
    for spec in GNU_LISTS:
        for mode, flags in ((ct.FIELDS, ["-d,", "-f", spec]), (ct.BYTES, ["-b", spec])):
            run = subprocess.run(["cut"] + flags, input=text, capture_output=True, env=env, timeout=60)
            assert run.returncode == 0, run.stderr
            assert ct.cut_ref(text, mode, ord(","), ct.ref_list(spec)) == run.stdout, (spec, mode)
