"""Shared pieces of the regex-search tests (test_regex_host.py, test_gpu_regex.py, test_gpu_regex_js.py): the ctypes binding of
cjs_bzip2_search_regex[_device], cjs_regex_check and cjs_stage_regex_scan, the expected list as Python's `re` finds it, the random
patterns of the grammar of tests/host/rx_compile_check.cc and the fixed patterns of the contract.  Fixtures and the shape of a call
are search_cases'."""
import ctypes
import re

import numpy as np

import range_cases as rg
import search_cases as sc

U32, U64 = sc.U32, sc.U64
NOCASE, ALL, GUARD = sc.NOCASE, sc.ALL, sc.GUARD
E_UNSUPPORTED = -34
MAXL = 256


def bind():
    L = sc.bind()
    sig = [rg.S, rg.V, rg.u8p, ctypes.POINTER(U32), U32, U32, U64, U64, rg.V, rg.S, ctypes.POINTER(sc.Info), rg.V]
    L.cjs_bzip2_search_regex.argtypes = [rg.u8p] + sig
    L.cjs_bzip2_search_regex_device.argtypes = [rg.V] + sig
    L.cjs_regex_check.argtypes = [rg.u8p, ctypes.POINTER(U32), U32, U32, ctypes.POINTER(U32), ctypes.POINTER(U32)]
    L.cjs_stage_regex_scan.argtypes = [rg.u8p, ctypes.POINTER(U32), U32, U32, rg.u8p, rg.S, rg.V, rg.S, ctypes.POINTER(ctypes.c_size_t)]
    return L


def _pat_args(pats):
    blob, p_off = sc.pattern_arrays(pats)
    return blob, p_off, blob.ctypes.data_as(rg.u8p), p_off.ctypes.data_as(ctypes.POINTER(U32))


def check(L, pats, nocase=False):
    """cjs_regex_check -> (rc, [(states, max_len)], detail)"""
    keep, keep2, p, o = _pat_args(pats)
    st, ml = (U32 * max(len(pats), 1))(), (U32 * max(len(pats), 1))()
    rc = L.cjs_regex_check(p, o, len(pats), NOCASE if nocase else 0, st, ml)
    return rc, (list(zip(list(st), list(ml)))[:len(pats)] if rc == 0 else None), rg.detail(L)


def stage_scan(L, pats, text, nocase=False, cap=None):
    """cjs_stage_regex_scan over `text` -> (rc, [(off, pattern, length)], n_found, detail); cap=None: count first"""
    keep, keep2, p, o = _pat_args(pats)
    t = np.frombuffer(bytes(text) or b"\0", np.uint8)
    n = ctypes.c_size_t(0)
    flags = NOCASE if nocase else 0
    if cap is None:
        rc = L.cjs_stage_regex_scan(p, o, len(pats), flags, t.ctypes.data_as(rg.u8p), len(text), None, 0, ctypes.byref(n))
        if rc:
            return rc, None, 0, rg.detail(L)
        cap = n.value
    buf = np.full((cap + 2) * 16, 0xA5, np.uint8)
    rc = L.cjs_stage_regex_scan(p, o, len(pats), flags, t.ctypes.data_as(rg.u8p), len(text), ctypes.c_void_p(buf.ctypes.data + 16) if cap else None, cap, ctypes.byref(n))
    if rc:
        return rc, None, 0, rg.detail(L)
    got = min(cap, n.value)
    assert (buf[:16] == 0xA5).all() and (buf[16 * (1 + got):] == 0xA5).all()
    rec = buf[16:16 * (1 + got)].view(sc.MATCH)
    return rc, list(zip(rec["off"].tolist(), rec["pattern"].tolist(), rec["reserved"].tolist())), n.value, ""


def expected(plain, pats, off=0, ln=ALL, nocase=False, runs=None):
    """[(off, pattern, length)] sorted, by Python's re: at every start position o >= off of a run ([(lo, hi)] of decoded offsets;
    None: the whole text) the largest l <= 256 with o + l inside the window and the run and fullmatch(text, o, o + l); match()
    first, which rules most positions out at once"""
    text = bytes(plain)
    total = len(text)
    win_hi = min(off + ln, total)
    cs = [re.compile(bytes(p), re.IGNORECASE if nocase else 0) for p in pats]
    out = []
    for lo_r, hi_r in (runs if runs is not None else [(0, total)]):
        lo, end = max(lo_r, off), min(hi_r, win_hi)
        for j, c in enumerate(cs):
            for o in range(lo, end):
                hi = min(o + MAXL, end)
                m = c.match(text, o, hi)
                if m is None:
                    continue
                for e in range(hi, o, -1):
                    if e == m.end() or c.fullmatch(text, o, e):
                        out.append((o, j, e - o))
                        break
    return sorted(out)


# ---- the grammar of tests/host/rx_compile_check.cc
ALPHA = b"abBc\n"


def random_pattern(rng, depth=2):
    def byte_test():
        k = rng.randint(8)
        if k == 0:
            return b"."
        if k == 1:
            return b"\\n"
        if k == 2:
            s = b"[^" if rng.randint(3) == 0 else b"["
            for _ in range(1 + rng.randint(3)):
                r = rng.randint(20)
                s += b"a-c" if r < 5 else b"\\n" if r < 8 else ALPHA[rng.randint(4):][:1]
            return s + b"]"
        if k == 3:
            return b"\\x62"
        return ALPHA[rng.randint(4):][:1]

    def repeat(d, quantifiers):
        quantified = quantifiers and rng.randint(5) >= 3
        if d > 0 and rng.randint(3) == 0:      # (nothing is repeated inside a repeated group: `re` backtracks through those for ever)
            a = (b"(" if rng.randint(2) else b"(?:") + expr(d - 1, quantifiers and not quantified) + b")"
        else:
            a = byte_test()
        if not quantified:
            return a
        k, lo = rng.randint(7), rng.randint(3)
        q = [b"?", b"*", b"+", b"{%d}" % (1 + lo), b"{%d,}" % lo, b"{,%d}" % (1 + lo), b"{%d,%d}" % (lo, max(lo + rng.randint(3), 1))][k]
        return a + q

    def expr(d, quantifiers=True):
        return b"|".join(b"".join(repeat(d, quantifiers) for _ in range(1 + rng.randint(3))) for _ in range(2 + rng.randint(2) if rng.randint(4) == 0 else 1))
    return expr(depth)


def random_text(rng, n):
    return bytes(np.frombuffer(ALPHA, np.uint8)[rng.randint(0, 5, n)])


# ---- the fixed patterns of the contract: (pattern, letters occur)
FIXED = [(rb"\d{2}-\d", False), (rb"[a-c]+X", True), (rb"(ab|c)[^a]{1,3}\.", True), (rb"a.*b", True), (rb"[^A-C]{2}9", True), (rb"[Z-a]", True),
         (rb"\xF7[^\xF7]{254,}", False), (rb"x{256}", True), (b"\xc1[\xe1-\xe3]+|\xda\xfa", False)]


# ---- a call, both forms (search_cases._call and both_forms with the length in the record)
def _call(fn, first, n, h, pats, off, ln, flags, cap):
    blob, p_off = sc.pattern_arrays(pats)
    buf = np.full((cap + 2 * GUARD) * 16, 0xA5, np.uint8)
    info = sc.Info(7, 7, 7, 7)
    found = ctypes.c_void_p(buf.ctypes.data + 16 * GUARD) if cap else None
    rc = fn(first, n, h, blob.ctypes.data_as(rg.u8p), p_off.ctypes.data_as(ctypes.POINTER(U32)), len(pats), flags, off, ln, found, cap, ctypes.byref(info), None)
    if rc:
        assert (buf == 0xA5).all()
        return rc, None, info
    got = min(cap, info.n_matches)
    assert (buf[:16 * GUARD] == 0xA5).all() and (buf[16 * (GUARD + got):] == 0xA5).all(), "the search wrote outside its first min(cap, n_matches) records"
    rec = buf[16 * GUARD:16 * (GUARD + got)].view(sc.MATCH)
    return rc, list(zip(rec["off"].tolist(), rec["pattern"].tolist(), rec["reserved"].tolist())), info


def regex_host(L, stream, h, pats, off=0, ln=ALL, flags=0, cap=0):
    a = np.ascontiguousarray(stream, dtype=np.uint8)
    keep = a if a.size else np.zeros(1, np.uint8)
    rc, m, info = _call(L.cjs_bzip2_search_regex, keep.ctypes.data_as(rg.u8p), a.size, h, pats, off, ln, flags, cap)
    return rc, m, info, rg.detail(L)


def regex_device(L, d_in_ptr, n, h, pats, off=0, ln=ALL, flags=0, cap=0):
    rc, m, info = _call(L.cjs_bzip2_search_regex_device, d_in_ptr, n, h, pats, off, ln, flags, cap)
    return rc, m, info, rg.detail(L)


def both_forms(L, stream, h, pats, off=0, ln=ALL, flags=0, cap=None, shift_in=3):
    """The host form and the device form (the stream at an odd device address), each as a count query followed by a call with
    cap = the total (or the given cap): both must agree in everything.  -> (matches, info tuple, detail)"""
    import torch
    n = stream.size
    d_in = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    d_in[shift_in:shift_in + n] = torch.from_numpy(np.ascontiguousarray(stream)).cuda()
    torch.cuda.synchronize()
    res = []
    for form in ("host", "device"):
        def run(c):
            if form == "host":
                return regex_host(L, stream, h, pats, off, ln, flags, c)
            return regex_device(L, d_in.data_ptr() + shift_in, n, h, pats, off, ln, flags, c)
        rc, m, info, d = run(0)
        assert rc == 0 and m == [], (form, rc, d)
        total = info.n_matches
        rc, m, info2, d2 = run(total if cap is None else cap)
        assert rc == 0 and sc.info_tuple(info2) == sc.info_tuple(info) and d2 == d, (form, rc, d, d2)
        assert len(m) == min(total, total if cap is None else cap)
        res.append((m, sc.info_tuple(info), d))
    assert res[0] == res[1], "the host form and the device form differ"
    return res[0]
