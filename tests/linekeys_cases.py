"""Shared pieces of the line-key tests (test_linekeys_host.py, test_gpu_linekeys.py, test_gpu_linekeys_js.py): the ctypes binding of
cjs_bzip2_line_keys / cjs_stage_line_keys / cjs_line_keys_diff, the key of a line restated with Python's big integers, the
quadratic-DP edit distance, and what applying hunks to a list of lines gives."""
import ctypes

import numpy as np

import lines_cases as lc
import range_cases as rg

U32, U64 = ctypes.c_uint32, ctypes.c_uint64
P = 2 ** 61 - 1
M64 = 2 ** 64 - 1
KEY = np.dtype([("hash", "<u8"), ("len", "<u4"), ("check", "<u4")])
HUNK = np.dtype([("a_first", "<u8"), ("a_count", "<u8"), ("b_first", "<u8"), ("b_count", "<u8")])
ONES = (M64, 2 ** 32 - 1, 2 ** 32 - 1)
MISMATCH = "line table does not match the stream at block %d"
CANARY = 0xA5


class KeysInfo(ctypes.Structure):
    _fields_ = [("n_lines", U64), ("n_bad_blocks", U64), ("first_bad_block", U64), ("blocks_decoded", U64)]


class DiffInfo(ctypes.Structure):
    _fields_ = [("n_hunks", U64), ("edits", U64), ("common", U64), ("minimal", U32), ("reserved", U32)]


def bind():
    L = lc.bind()
    V, S = rg.V, rg.S
    L.cjs_bzip2_line_keys.argtypes = [rg.u8p, S, V, V, U64, U64, U64, V, S, ctypes.POINTER(KeysInfo), V]
    L.cjs_bzip2_line_keys_device.argtypes = [V, S, V, V, U64, U64, U64, V, S, ctypes.POINTER(KeysInfo), V]
    L.cjs_stage_line_keys.argtypes = [V, S, U64, V, S, rg.PS]
    L.cjs_line_keys_diff.argtypes = [V, S, V, S, U64, V, S, ctypes.POINTER(DiffInfo)]
    return L


# ---- the key, restated
def _splitmix(state):
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return state, z ^ (z >> 31)


def bases(seed):
    s, a = _splitmix(seed & M64)
    s, b = _splitmix(s)
    return 256 + a % (P - 256), 256 + b % (P - 256)


def line_key(line, b1, b2):
    h1 = h2 = 0
    for c in bytes(line):
        h1 = (h1 * b1 + c + 1) % P
        h2 = (h2 * b2 + c + 1) % P
    return (h1, len(line) & 0xFFFFFFFF, h2 & 0xFFFFFFFF)


def split_lines(text):
    """the lines of `text` as the line table numbers them: one per newline, then the unterminated tail (which may be empty)"""
    parts = bytes(text).split(b"\n")
    return [p + b"\n" for p in parts[:-1]] + [parts[-1]]


def text_keys(text, seed):
    """-> [(hash, len, check)] of every line of text; equal lines are hashed once"""
    b1, b2 = bases(seed)
    memo = {}
    out = []
    for ln in split_lines(text):
        if ln not in memo:
            memo[ln] = line_key(ln, b1, b2)
        out.append(memo[ln])
    return out


def as_tuples(keys):
    return list(zip(keys["hash"].tolist(), keys["len"].tolist(), keys["check"].tolist()))


def key_array(tuples):
    a = np.zeros(len(tuples), dtype=KEY)
    for k, t in enumerate(tuples):
        a[k] = t
    return a


# ---- the calls
GUARD = 8


def _guarded(dtype, cap):
    buf = np.full((cap + 2 * GUARD) * dtype.itemsize, CANARY, np.uint8)
    return buf, buf.ctypes.data + GUARD * dtype.itemsize


def _unguard(buf, dtype, cap, written):
    raw = buf.view(dtype)
    assert (buf[:GUARD * dtype.itemsize] == CANARY).all(), "the call wrote in front of its array"
    assert (buf[(GUARD + written) * dtype.itemsize:] == CANARY).all(), "the call wrote past what it may write"
    return raw[GUARD:GUARD + written].copy()


def stage_keys(L, text, seed, cap=None):
    """cjs_stage_line_keys -> (rc, keys written, n_lines)"""
    a = np.frombuffer(bytes(text), dtype=np.uint8)
    keep = a if a.size else np.zeros(1, np.uint8)
    if cap is None:
        cap = bytes(text).count(b"\n") + 1
    buf, ptr = _guarded(KEY, cap)
    n = rg.S(0)
    rc = L.cjs_stage_line_keys(keep.ctypes.data, a.size, seed, ptr if cap else None, cap, ctypes.byref(n))
    return rc, _unguard(buf, KEY, cap, min(cap, n.value) if rc == 0 else 0), n.value


def _keys_call(fn, src, n, h, t, first, count, seed, cap):
    buf, ptr = _guarded(KEY, cap)
    info = KeysInfo(7, 7, 7, 7)
    rc = fn(src, n, h, t, first, count, seed, ptr if cap else None, cap, ctypes.byref(info), None)
    keys = _unguard(buf, KEY, cap, min(cap, info.n_lines) if rc == 0 else 0)
    return rc, keys, info


def keys_host(L, stream, h, t, first=0, count=M64, seed=0, cap=None):
    """cjs_bzip2_line_keys -> (rc, keys, info, detail); cap=None: the count query first, then that many"""
    a = np.ascontiguousarray(stream, dtype=np.uint8)
    keep = a if a.size else np.zeros(1, np.uint8)
    if cap is None:
        rc, _, info = _keys_call(L.cjs_bzip2_line_keys, keep.ctypes.data_as(rg.u8p), a.size, h, t, first, count, seed, 0)
        if rc:
            return rc, None, info, rg.detail(L)
        cap = info.n_lines
    rc, keys, info = _keys_call(L.cjs_bzip2_line_keys, keep.ctypes.data_as(rg.u8p), a.size, h, t, first, count, seed, cap)
    return rc, keys, info, rg.detail(L)


def keys_device(L, d_in_ptr, n, h, t, first=0, count=M64, seed=0, cap=None):
    if cap is None:
        rc, _, info = _keys_call(L.cjs_bzip2_line_keys_device, d_in_ptr, n, h, t, first, count, seed, 0)
        if rc:
            return rc, None, info, rg.detail(L)
        cap = info.n_lines
    rc, keys, info = _keys_call(L.cjs_bzip2_line_keys_device, d_in_ptr, n, h, t, first, count, seed, cap)
    return rc, keys, info, rg.detail(L)


def both_forms(L, stream, h, t, dev, **kw):
    """The host form and the device form (the stream at an odd device address): both must agree in everything.
    -> (keys as tuples, info as a tuple, detail)"""
    rc, keys, info, d = keys_host(L, stream, h, t, **kw)
    assert rc == 0, (rc, d)
    rc2, keys2, info2, d2 = keys_device(L, dev[1], np.asarray(stream).size, h, t, **kw)
    assert rc2 == 0, (rc2, d2)
    i1 = (info.n_lines, info.n_bad_blocks, info.first_bad_block, info.blocks_decoded)
    i2 = (info2.n_lines, info2.n_bad_blocks, info2.first_bad_block, info2.blocks_decoded)
    assert keys.tobytes() == keys2.tobytes() and i1 == i2 and d == d2, "the host form and the device form differ"
    return as_tuples(keys), i1, d


def diff(L, a, b, max_edits=0, cap=None):
    """cjs_line_keys_diff over two lists of key tuples -> (rc, hunks as tuples, info); cap=None: the count query, then all"""
    ka, kb = key_array(a), key_array(b)
    pa = ka.ctypes.data if len(a) else None
    pb = kb.ctypes.data if len(b) else None
    info = DiffInfo()
    if cap is None:
        rc = L.cjs_line_keys_diff(pa, len(a), pb, len(b), max_edits, None, 0, ctypes.byref(info))
        if rc:
            return rc, None, info
        cap = info.n_hunks
    buf, ptr = _guarded(HUNK, cap)
    rc = L.cjs_line_keys_diff(pa, len(a), pb, len(b), max_edits, ptr if cap else None, cap, ctypes.byref(info))
    hunks = _unguard(buf, HUNK, cap, min(cap, info.n_hunks) if rc == 0 else 0)
    return rc, [tuple(int(x) for x in h) for h in hunks.tolist()], info


# ---- what a diff must be
def edit_distance(a, b):
    """len(a) + len(b) - 2 LCS(a, b) by the quadratic DP (numpy over the rows)"""
    if not a or not b:
        return len(a) + len(b)
    ids = {}
    ia = np.array([ids.setdefault(x, len(ids)) for x in a])
    ib = np.array([ids.setdefault(x, len(ids)) for x in b])
    prev = np.zeros(len(b) + 1, dtype=np.int64)
    for x in ia:
        diag = prev[:-1] + (ib == x)
        cur = np.zeros_like(prev)
        cur[1:] = np.maximum(diag, prev[1:])
        np.maximum.accumulate(cur, out=cur)
        prev = cur
    return len(a) + len(b) - 2 * int(prev[-1])


def apply_hunks(a, b, hunks):
    """A with every hunk's lines replaced by B's"""
    out, at = [], 0
    for a_first, a_count, b_first, b_count in hunks:
        out += a[at:a_first] + b[b_first:b_first + b_count]
        at = a_first + a_count
    return out + a[at:]


def check_hunks(a, b, hunks, info):
    """the invariants of a script: ascending, non-empty, a common line between neighbours, b_first as the rule says, edits and
    common as the sums say, and applying it to A gives B"""
    shift, last_end = 0, None
    for a_first, a_count, b_first, b_count in hunks:
        assert a_count or b_count
        assert b_first == a_first + shift
        assert last_end is None or a_first > last_end, "neighbouring hunks without a common line between them"
        assert a_first + a_count <= len(a) and b_first + b_count <= len(b)
        last_end = a_first + a_count
        shift += b_count - a_count
    edits = sum(h[1] + h[3] for h in hunks)
    assert info.n_hunks == len(hunks) and info.edits == edits and info.common == (len(a) + len(b) - edits) // 2 and info.reserved == 0
    assert apply_hunks(a, b, hunks) == b
