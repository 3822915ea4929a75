"""The regex search without a GPU: the compiler and the per-position walk through cjs_regex_check and cjs_stage_regex_scan against
Python's `re` (fixed patterns of the contract, with and without NOCASE, and a few hundred random ones), every refusal with its code
and a detail text, and what cjs_bzip2_search_regex[_device] decide before a device is touched.  The index is made of imaginary
entries (rg.create), as in test_search_host.py."""
import ctypes

import numpy as np
import pytest

import range_cases as rg
import regex_cases as rc_
import search_cases as sc

N = 5000
ENTRIES = [(32, 9000, 1000, 0x11223344, 1, 0), (9000, 9200, 0, 0xFFFFFFFF, 1, 0), (9300, 9500, 0, 7, 1, 0), (20007, 39899, 500, 0, 9, 0)]
TOTAL = 1500


@pytest.fixture(scope="module")
def L():
    return rc_.bind()


@pytest.fixture(scope="module")
def h(L):
    rc, h = rg.create(L, ENTRIES, N, 0)
    assert rc == 0
    return h


def _text():
    """6,000 bytes in which every fixed pattern finds something: digits and dashes, letters of both cases next to @ [ ` {, dots,
    newlines, bytes >= 0x80 that differ by 0x20, a run of 300 x and 0xF7 markers 200, 255, 256 and 400 bytes apart"""
    rng = np.random.RandomState(11)
    alphabet = np.frombuffer(b"abcABCXxzZ019-.@[`{ \n\xc1\xe1\xe2\xda\xfa", np.uint8)
    t = bytearray(alphabet[rng.randint(0, alphabet.size, 6000)].tobytes())
    t[1000:1300] = b"x" * 300
    t[500:520] = b"19-0 919-10-9 1-1 00-"[:20]
    at = 2000
    for gap in (200, 255, 256, 400):
        t[at:at + gap + 1] = b"\xf7" + bytes(rng.randint(0x30, 0x3A, gap).astype(np.uint8))
        at += gap + 1
    t[at] = 0xF7
    return bytes(t)


@pytest.mark.parametrize("nocase", [False, True])
def test_fixed_patterns_against_re(L, nocase):
    text = _text()
    pats = [p for p, letters in rc_.FIXED if letters or not nocase]
    want = rc_.expected(text, pats, nocase=nocase)
    rc, got, n, d = rc_.stage_scan(L, pats, text, nocase)
    assert rc == 0 and n == len(got) and got == want, d
    by = lambda j: [(o, l) for o, k, l in want if k == j]
    assert all(by(j) for j in range(len(pats))), [len(by(j)) for j in range(len(pats))]
    x = pats.index(rb"x{256}")
    if not nocase:
        assert by(x) == [(1000 + k, 256) for k in range(45)]                     # every start with 256 x behind it, none after
        f7 = pats.index(rb"\xF7[^\xF7]{254,}")
        assert by(f7) == [(2201, 256), (2457, 256), (2714, 256), (3115, 256)]      # gaps of 255, 256, 400 and more bytes: clamped to 256; 200: nothing
        hi = pats.index(b"\xc1[\xe1-\xe3]+|\xda\xfa")
        assert by(hi) == [(o, l) for o, k, l in rc_.expected(text, [pats[hi]], nocase=True)]      # bytes >= 0x80 do not fold
    else:
        assert len(by(x)) > 45 or b"X" not in text[990:1310]


def test_nocase_classes(L):
    text = b"zZ[`aA\\]^_bB@{\nb9 B9 dd9 AB9 aD9"
    rc, got, n, d = rc_.stage_scan(L, [rb"[Z-a]", rb"[^A-C]{2}9"], text, True)
    assert rc == 0 and got == rc_.expected(text, [rb"[Z-a]", rb"[^A-C]{2}9"], nocase=True)
    hit = [o for o, j, l in got if j == 0]
    assert hit[:10] == list(range(10)) and {text[o] for o in hit} == set(b"zZ[`aA\\]^_")      # and neither b nor B, @ nor {
    assert (text.index(b"dd9"), 1, 3) in got and not any(j == 1 and text[o:o + 1] in b"bB" for o, j, l in got)


def test_cap_and_count_of_the_stage(L):
    text = b"abcabcabc"
    rc, got, n, d = rc_.stage_scan(L, [b"abc", b"b"], text, cap=2)
    assert rc == 0 and n == 6 and got == [(0, 0, 3), (1, 1, 1)]
    rc, got, n, d = rc_.stage_scan(L, [b"abc", b"b"], b"")
    assert rc == 0 and n == 0 and got == []


def test_random_patterns_against_re(L):
    rng = np.random.RandomState(2024)
    done = empties = hits = 0
    for it in range(400):
        nocase = bool(rng.randint(3) == 0)
        pats = [rc_.random_pattern(rng) for _ in range(1 + (rng.randint(4) == 0) * (1 + rng.randint(3)))]
        flags = rc_.re.IGNORECASE if nocase else 0
        empty = any(rc_.re.compile(p, flags).fullmatch(b"") for p in pats)
        text = rc_.random_text(rng, 60)
        rc, got, n, d = rc_.stage_scan(L, pats, text, nocase)
        if empty:
            assert rc == rg.E_INVALID and "empty" in d, (pats, rc, d)
            empties += 1
            continue
        assert rc == 0, (pats, rc, d)
        want = rc_.expected(text, pats, nocase=nocase)
        assert got == want, (pats, nocase, text)
        done += 1
        hits += len(want)
    assert done > 200 and empties > 10 and hits > 3000


REFUSALS = [(rb"^a", rc_.E_UNSUPPORTED), (rb"a$", rc_.E_UNSUPPORTED), (rb"\bfoo", rc_.E_UNSUPPORTED), (rb"(a)\1", rc_.E_UNSUPPORTED), (rb"a*?", rc_.E_UNSUPPORTED),
            (rb"a*", rg.E_INVALID), (rb"(", rg.E_INVALID), (rb"[a", rg.E_INVALID), (rb"a{3,2}", rg.E_INVALID), (rb"a{257}", rg.E_INVALID), (rb"\q", rc_.E_UNSUPPORTED)]


def test_refusals(L):
    for pat, code in REFUSALS:
        for pats, j in (([pat], 0), ([b"fine", b"x+y", pat], 2)):
            rc, res, d = rc_.check(L, pats)
            assert rc == code and d.startswith("pattern %d, byte " % j) and len(d) > 20, (pat, rc, d)
            rc, got, n, d2 = rc_.stage_scan(L, pats, b"some text")
            assert rc == code and d2 == d, (pat, rc, d2)
    # the byte position
    assert rc_.check(L, [rb"ab$"])[2].startswith("pattern 0, byte 2: ") and rc_.check(L, [rb"abc\bfoo"])[2].startswith("pattern 0, byte 3: ")
    # an empty pattern, a text of 1025 bytes, 65 patterns; 1024 bytes and 64 patterns are fine
    rc, res, d = rc_.check(L, [b"a", b""])
    assert rc == rg.E_INVALID and d.startswith("pattern 1, byte 0: ")
    rc, res, d = rc_.check(L, [b"a" * 1025])
    assert rc == rg.E_INVALID and d.startswith("pattern 0, byte 0: ")
    assert rc_.check(L, [b"(?:" + b"a|" * 509 + b"bc)"])[0] == 0
    rc, res, d = rc_.check(L, [b"a"] * 65)
    assert rc == rg.E_INVALID and d
    rc, res, d = rc_.check(L, [b"a"] * 64)
    assert rc == 0 and res == [(1, 1)] * 64
    rc, res, d = rc_.check(L, [])
    assert rc == rg.E_INVALID and d


def test_state_limit_and_table_budget(L):
    """The tables hold 8-bit states: 255 values besides the dead state's, for the states a transition enters.  Acceptance stands on
    the transition, so of `(a|b)*a(a|b){k}` the last k bytes are the state: 2^k states.  k = 7 is accepted with 128, k = 8 has 256
    and is refused (the state-per-acceptance count of the issue, 2^(k+1), would have refused 7)."""
    rc, res, d = rc_.check(L, [rb"(a|b)*a(a|b){7}"])
    assert rc == 0 and res == [(128, 256)]
    rc, res, d = rc_.check(L, [rb"(a|b)*a(a|b){8}"])
    assert rc == rc_.E_UNSUPPORTED and "255 states" in d and d.startswith("pattern 0, byte ")
    text = rc_.random_text(np.random.RandomState(5), 600).replace(b"\n", b"a").replace(b"c", b"b").replace(b"B", b"b")
    rc, got, n, d = rc_.stage_scan(L, [rb"(a|b)*a(a|b){7}"], text)
    assert rc == 0 and got == rc_.expected(text, [rb"(a|b)*a(a|b){7}"])
    # every pattern of the contract that needs 256 bytes fits
    rc, res, d = rc_.check(L, [rb"x{256}", rb"\xF7[^\xF7]{254,}", rb"b[ab]{0,255}", rb"\xF7\xF7[^\xF7]{254}", rb"\xF7+[^\xF7]{1,255}"])
    assert rc == 0 and [m for s, m in res] == [256] * 5 and all(s <= 256 for s, m in res)
    rc, res, d = rc_.check(L, [rb"abc", rb"a{2,5}", rb"ab|cd", rb"\d{4}-\d{2}-\d{2}"])
    assert rc == 0 and res == [(3, 3), (5, 5), (3, 2), (10, 10)]
    # 64 copies of [a-z]{200}: over the table budget; 16 copies are not
    rc, res, d = rc_.check(L, [rb"[a-z]{200}"] * 64)
    assert rc == rc_.E_UNSUPPORTED and "32768" in d and d.startswith("pattern ")
    rc, res, d = rc_.check(L, [rb"[a-z]{200}"] * 16)
    assert rc == 0 and res == [(200, 200)] * 16


@pytest.mark.parametrize("form", ["host", "device"])
def test_refusals_before_the_device_is_touched(L, h, form):
    """off >= total makes every call one that would succeed without a device: a refusal is then the argument check's"""
    fn = L.cjs_bzip2_search_regex if form == "host" else L.cjs_bzip2_search_regex_device
    stream = np.zeros(N, np.uint8)
    first = stream.ctypes.data_as(rg.u8p) if form == "host" else ctypes.c_void_p(stream.ctypes.data)
    keep, keep2, pat, p_off = rc_._pat_args([rb"ab+c", rb"\d"])
    info = sc.Info()
    found = (sc.Match * 4)()
    ok = dict(first=first, n=N, h=h, pat=pat, pat_off=p_off, npat=2, flags=0, off=TOTAL, ln=10, found=ctypes.cast(found, rg.V), cap=4, info=ctypes.byref(info))

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a["first"], a["n"], a["h"], a["pat"], a["pat_off"], a["npat"], a["flags"], a["off"], a["ln"], a["found"], a["cap"], a["info"], None)
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
    k1, k2, p65, o65 = rc_._pat_args([b"x"] * 65)
    assert call(pat=p65, pat_off=o65, npat=65) == rg.E_INVALID
    assert call(pat=p65, pat_off=o65, npat=64) == 0
    desc = np.array([0, 3, 2], np.uint32)
    assert call(pat_off=desc.ctypes.data_as(ctypes.POINTER(sc.U32))) == rg.E_INVALID
    one = np.array([1, 3, 4], np.uint32)
    assert call(pat_off=one.ctypes.data_as(ctypes.POINTER(sc.U32))) == rg.E_INVALID
    for pat_, code in REFUSALS + [(b"", rg.E_INVALID), (rb"(a|b)*a(a|b){8}", rc_.E_UNSUPPORTED)]:
        k3, k4, pp, oo = rc_._pat_args([b"ok", pat_])
        assert call(pat=pp, pat_off=oo, npat=2) == code and rg.detail(L).startswith("pattern 1, byte "), pat_
    k5, k6, pp, oo = rc_._pat_args([rb"[a-z]{200}"] * 64)
    assert call(pat=pp, pat_off=oo, npat=64) == rc_.E_UNSUPPORTED and "32768" in rg.detail(L)
    assert all(bytes(found[i]) == bytes(16) for i in range(4))


@pytest.mark.parametrize("form", ["host", "device"])
def test_a_window_without_a_touched_block_needs_no_device(L, h, form):
    stream = np.zeros(N, np.uint8)
    for off, ln in ((0, 0), (700, 0), (TOTAL, 5), (TOTAL + 1, sc.ALL), (2 ** 64 - 1, sc.ALL)):
        if form == "host":
            rc, m, info, d = rc_.regex_host(L, stream, h, [rb"a+", rb"b|c"], off, ln, 0, 3)
        else:
            rc, m, info, d = rc_.regex_device(L, ctypes.c_void_p(stream.ctypes.data), N, h, [rb"a+", rb"b|c"], off, ln, 0, 3)
        assert rc == 0 and m == [] and sc.info_tuple(info) == (0, 0, 2 ** 64 - 1, 0) and d == "", (off, ln)


def test_expected_list_helper():
    """the reference of the GPU tests: longest match at every start, the clamp at 256, the window and the runs"""
    assert rc_.expected(b"aab ab", [rb"a+b", rb"a"]) == [(0, 0, 3), (0, 1, 1), (1, 0, 2), (1, 1, 1), (4, 0, 2), (4, 1, 1)]
    assert rc_.expected(b"x" * 300, [rb"x+"])[40:50] == [(o, 0, min(256, 300 - o)) for o in range(40, 50)]
    assert rc_.expected(b"aaaa", [rb"a+"], 1, 2) == [(1, 0, 2), (2, 0, 1)]
    assert rc_.expected(b"aaaa", [rb"a+"], runs=[(0, 2), (2, 3)]) == [(0, 0, 2), (1, 0, 1), (2, 0, 1)]
    assert rc_.expected(b"Ab", [rb"aB"], nocase=True) == [(0, 0, 2)] and rc_.expected(b"Ab", [rb"aB"]) == []
