"""Shared pieces of the pattern-search tests (test_search_host.py, test_gpu_search.py, test_gpu_search_js.py): the ctypes binding of
cjs_bzip2_search[_device], the expected list as plain Python finds it in the decoded text, the two fixtures of its own (S4, S5) and
the pattern sets.  The streams come from the CPU oracle and tests/golden/data (range_cases)."""
import ctypes

import numpy as np

import range_cases as rg

U32, U64 = ctypes.c_uint32, ctypes.c_uint64
NOCASE = 1
MATCH = np.dtype([("off", "<u8"), ("pattern", "<u4"), ("reserved", "<u4")])
ALL = 2 ** 64 - 1


class Match(ctypes.Structure):
    _fields_ = [("off", U64), ("pattern", U32), ("reserved", U32)]


class Info(ctypes.Structure):
    _fields_ = [("n_matches", U64), ("n_bad_blocks", U64), ("first_bad_block", U64), ("blocks_decoded", U64)]


def bind():
    L = rg.bind()
    sig = [rg.S, rg.V, rg.u8p, ctypes.POINTER(U32), U32, U32, U64, U64, rg.V, rg.S, ctypes.POINTER(Info), rg.V]
    L.cjs_bzip2_search.argtypes = [rg.u8p] + sig
    L.cjs_bzip2_search_device.argtypes = [rg.V] + sig
    return L


def pattern_arrays(pats):
    blob = np.frombuffer(b"".join(pats) or b"\0", dtype=np.uint8).copy()
    return blob, np.cumsum([0] + [len(p) for p in pats]).astype(np.uint32)


def fold(b):
    """'A'..'Z' -> 'a'..'z', nothing else (bytes.lower() does exactly this)"""
    return bytes(b).lower()


def expected(plain, pats, off=0, ln=ALL, nocase=False, runs=None):
    """[(off, pattern)] sorted: every start position o with plain[o:o + len] == pattern, o >= off, o + len <= the window's end and
    the match wholly inside one of `runs` ([(lo, hi)] of decoded offsets; None: the whole text) -- bytes.find in a loop"""
    text = bytes(plain)
    total = len(text)
    hi = min(off + ln, total)
    if nocase:
        text = fold(text)
    out = []
    for lo_r, hi_r in (runs if runs is not None else [(0, total)]):
        lo, end = max(lo_r, off), min(hi_r, hi)
        for j, p in enumerate(pats):
            p = fold(p) if nocase else bytes(p)
            at = text.find(p, lo, end) if lo < end else -1
            while at >= 0:
                out.append((at, j))
                at = text.find(p, at + 1, end)
    return sorted(out)


GUARD = 64      # canary records on either side of `found`


def _call(fn, first, n, h, pats, off, ln, flags, cap):
    """-> (rc, [(off, pattern)], info); `found` lies between canaries that must come back unchanged, as must every
    record past the first min(cap, n_matches)"""
    blob, p_off = pattern_arrays(pats)
    buf = np.full((cap + 2 * GUARD) * 16, 0xA5, np.uint8)
    info = Info(7, 7, 7, 7)
    found = ctypes.c_void_p(buf.ctypes.data + 16 * GUARD) if cap else None
    rc = fn(first, n, h, blob.ctypes.data_as(rg.u8p), p_off.ctypes.data_as(ctypes.POINTER(U32)), len(pats), flags, off, ln, found, cap, ctypes.byref(info), None)
    if rc:
        assert (buf == 0xA5).all()
        return rc, None, info
    got = min(cap, info.n_matches)
    assert (buf[:16 * GUARD] == 0xA5).all() and (buf[16 * (GUARD + got):] == 0xA5).all(), "the search wrote outside its first min(cap, n_matches) records"
    rec = buf[16 * GUARD:16 * (GUARD + got)].view(MATCH)
    assert not rec["reserved"].any()
    return rc, list(zip(rec["off"].tolist(), rec["pattern"].tolist())), info


def search_host(L, stream, h, pats, off=0, ln=ALL, flags=0, cap=0):
    a = np.ascontiguousarray(stream, dtype=np.uint8)
    keep = a if a.size else np.zeros(1, np.uint8)
    rc, m, info = _call(L.cjs_bzip2_search, keep.ctypes.data_as(rg.u8p), a.size, h, pats, off, ln, flags, cap)
    return rc, m, info, rg.detail(L)


def search_device(L, d_in_ptr, n, h, pats, off=0, ln=ALL, flags=0, cap=0):
    rc, m, info = _call(L.cjs_bzip2_search_device, d_in_ptr, n, h, pats, off, ln, flags, cap)
    return rc, m, info, rg.detail(L)


def info_tuple(info):
    return (info.n_matches, info.n_bad_blocks, info.first_bad_block, info.blocks_decoded)


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
                return search_host(L, stream, h, pats, off, ln, flags, c)
            return search_device(L, d_in.data_ptr() + shift_in, n, h, pats, off, ln, flags, c)
        rc, m, info, d = run(0)
        assert rc == 0 and m == [], (form, rc, d)
        total = info.n_matches
        rc, m, info2, d2 = run(total if cap is None else cap)
        assert rc == 0 and info_tuple(info2) == info_tuple(info) and d2 == d, (form, rc, d, d2)
        assert len(m) == min(total, total if cap is None else cap)
        res.append((m, info_tuple(info), d))
    assert res[0] == res[1], "the host form and the device form differ"
    return res[0]


# ---- fixtures
def s4(oracle):
    """80 members of 0..6 bytes over the alphabet ab, levels cycling 1..9: blocks of a few bytes, members without a block"""
    rng = np.random.RandomState(4321)
    parts, plain = [], []
    for k in range(80):
        p = rng.randint(97, 99, k % 7).astype(np.uint8)
        rc, s = oracle.bzip2_compress(p, 1 + k % 9)
        assert rc == 0
        parts.append(np.asarray(s, dtype=np.uint8)); plain.append(p)
    return np.concatenate(parts), np.concatenate(plain), 1


M37 = bytes([0xF7]) + bytes(range(1, 37))
M256 = bytes([0xF7, 0xF7]) + bytes((7 * i + 3) % 247 for i in range(254))


def s5(oracle):
    """One level-1 stream of 300 KiB: random bytes without 0xF7, and at every 1024 k + d one marker (both kinds start with 0xF7),
    d going through {-37, -36, -1, 0, 1} and the kind changing every five seams; at the multiples of 16 KiB the same by their own
    count, so that both kinds stand at every d of those too.  A marker before the seam, one ending on it, one across it, one
    starting on it and one behind it, for every power-of-two tile size >= 1 KiB.  -> (stream, plain, [positions of M37], [of M256])"""
    rng = np.random.RandomState(55)
    size = 300 * 1024
    plain = rng.randint(0, 0xF7, size).astype(np.uint8)
    ds = (-37, -36, -1, 0, 1)
    at = ([], [])
    for k in range(1, size // 1024):
        c = k // 16 if k % 16 == 0 else k
        pos, kind = 1024 * k + ds[c % 5], (c // 5) % 2
        m = (M37, M256)[kind]
        plain[pos:pos + len(m)] = np.frombuffer(m, np.uint8)
        at[kind].append(pos)
    rc, s = oracle.bzip2_compress(plain, 1)
    assert rc == 0
    return np.asarray(s, dtype=np.uint8), plain, at[0], at[1]


def seam_patterns(plain, bounds):
    """the block-seam set of F1: per inner boundary B five patterns across it, then a 1-byte pattern, a frequent 3-byte one, one
    that does not occur and one given twice"""
    pats = []
    for B in bounds:
        B = int(B)
        pats += [plain[B - 1:B + 1], plain[B - 7:B + 9], plain[B - 255:B + 1], plain[B - 1:B + 255], plain[B - 128:B + 128]]
    pats = [bytes(p) for p in pats]
    pats += [b"e", b"the", b"\x00zq\xffnot here\x01", bytes(pats[1])]
    return pats
