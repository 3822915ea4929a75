"""Shared pieces of the line-table tests (test_lines_host.py, test_gpu_lines.py, test_gpu_lines_js.py): the ctypes binding of
cjs_bzip2_lines_*, the serialised table as numpy builds it, what numpy expects of start(k) and number(o), and the two fixtures of
its own (LN2, LN3).  The streams come from the CPU oracle and tests/golden/data (range_cases)."""
import ctypes

import numpy as np

import range_cases as rg

U32, U64 = ctypes.c_uint32, ctypes.c_uint64
PU32 = ctypes.POINTER(U32)
TOP = 2 ** 64 - 1
TILE, ROW = 16384, 1024
HEADER = np.dtype([("magic", "S8"), ("version", "<u4"), ("flags", "<u4"), ("blocks", "<u8"), ("total_bytes", "<u8"), ("crc_fold", "<u4"),
                   ("reserved", "<u4")])
FOREIGN = "the line table is of another index"


def bind():
    L = rg.bind()
    V, S = rg.V, rg.S
    L.cjs_bzip2_lines_build.argtypes = [rg.u8p, S, V, ctypes.POINTER(V), V]
    L.cjs_bzip2_lines_build_device.argtypes = [V, S, V, ctypes.POINTER(V), V]
    L.cjs_bzip2_lines_create.argtypes = [V, PU32, S, ctypes.POINTER(V)]
    L.cjs_bzip2_lines_save.argtypes = [V, ctypes.POINTER(rg.u8p), rg.PS]
    L.cjs_bzip2_lines_load.argtypes = [rg.u8p, S, V, ctypes.POINTER(V)]
    L.cjs_bzip2_lines_info.argtypes = [V, rg.PU, rg.PU, rg.PU]
    L.cjs_bzip2_lines_counts.argtypes = [V, PU32, ctypes.c_long]
    L.cjs_bzip2_lines_counts.restype = ctypes.c_long
    L.cjs_bzip2_lines_destroy.argtypes = [V]
    L.cjs_bzip2_lines_destroy.restype = None
    for name in ("locate", "number"):
        getattr(L, "cjs_bzip2_lines_" + name).argtypes = [rg.u8p, S, V, V, V, S, V, V, V]
        getattr(L, "cjs_bzip2_lines_" + name + "_device").argtypes = [V, S, V, V, V, S, V, V, V]
    return L


# ---- what numpy expects
def newlines(plain):
    return np.flatnonzero(np.asarray(plain) == 10)


def start(nl, total, k):
    return 0 if k == 0 else (int(nl[k - 1]) + 1 if k <= nl.size else total)


def number(nl, total, o):
    return int(np.searchsorted(nl, min(o, total), "left"))


def block_counts(plain, bounds):
    return [int((plain[int(a):int(b)] == 10).sum()) for a, b in zip(bounds[:-1], bounds[1:])]


def crc_fold(entries):
    c = 0
    for e in entries:
        c = (((c << 1) | (c >> 31)) & 0xFFFFFFFF) ^ e[3]
    return c


def image(counts, total, fold, magic=b"CJSBZLN1", version=1, flags=0, reserved=0, blocks=None):
    """the serialised table as the format says"""
    h = np.zeros(1, dtype=HEADER)
    h["magic"], h["version"], h["flags"], h["blocks"] = magic, version, flags, len(counts) if blocks is None else blocks
    h["total_bytes"], h["crc_fold"], h["reserved"] = total, fold, reserved
    return h.tobytes() + np.asarray(counts, dtype="<u4").tobytes()


# ---- the table
def create(L, h, counts):
    c = np.asarray(list(counts) or [0], dtype=np.uint32)
    t = rg.V()
    rc = L.cjs_bzip2_lines_create(h, c.ctypes.data_as(PU32), len(counts), ctypes.byref(t))
    return rc, t


def load(L, raw, h):
    a = np.frombuffer(raw, dtype=np.uint8).copy() if len(raw) else np.zeros(1, np.uint8)
    t = rg.V()
    rc = L.cjs_bzip2_lines_load(a.ctypes.data_as(rg.u8p), len(raw), h, ctypes.byref(t))
    return rc, t


def save(L, t):
    out, n = rg.u8p(), rg.S(0)
    assert L.cjs_bzip2_lines_save(t, ctypes.byref(out), ctypes.byref(n)) == 0
    raw = ctypes.string_at(out, n.value)
    L.cjs_free(out)
    return raw


def info(L, t):
    b, n, tb = U64(7), U64(7), U64(7)
    assert L.cjs_bzip2_lines_info(t, ctypes.byref(b), ctypes.byref(n), ctypes.byref(tb)) == 0
    return b.value, n.value, tb.value


def counts(L, t):
    nb = L.cjs_bzip2_lines_counts(t, None, 0)
    c = np.full(nb + 2, 0xA5A5A5A5, np.uint32)
    assert L.cjs_bzip2_lines_counts(t, c.ctypes.data_as(PU32), nb) == nb and c[nb] == 0xA5A5A5A5
    return c[:nb].tolist()


def build_host(L, stream, h):
    a = np.ascontiguousarray(stream, dtype=np.uint8)
    keep = a if a.size else np.zeros(1, np.uint8)
    t = rg.V()
    rc = L.cjs_bzip2_lines_build(keep.ctypes.data_as(rg.u8p), a.size, h, ctypes.byref(t), None)
    return rc, t, rg.detail(L)


def build_device(L, d_in_ptr, n, h):
    t = rg.V()
    rc = L.cjs_bzip2_lines_build_device(d_in_ptr, n, h, ctypes.byref(t), None)
    return rc, t, rg.detail(L)


# ---- the two questions
GUARD = 64
CANARY64, CANARY32 = 0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A


def _ask(fn, first, n, h, t, qs):
    """-> (rc, answers, status): both arrays lie between canaries that must come back unchanged"""
    count = len(qs)
    q = np.array([int(x) for x in qs] or [0], dtype=np.uint64)
    out = np.full(count + 2 * GUARD, CANARY64, np.uint64)
    st = np.full(count + 2 * GUARD, CANARY32, np.int32)
    rc = fn(first, n, h, t, q.ctypes.data, count, out.ctypes.data + 8 * GUARD, st.ctypes.data + 4 * GUARD, None)
    if rc:
        assert (out == CANARY64).all() and (st == CANARY32).all()
        return rc, None, None
    for a, c in ((out, CANARY64), (st, CANARY32)):
        assert (a[:GUARD] == c).all() and (a[GUARD + count:] == c).all(), "the call wrote outside its arrays"
    return rc, out[GUARD:GUARD + count].copy(), st[GUARD:GUARD + count].copy()


def ask_host(L, kind, stream, h, t, qs):
    """kind: "locate" or "number" -> (rc, answers, status, detail)"""
    a = np.ascontiguousarray(stream, dtype=np.uint8)
    keep = a if a.size else np.zeros(1, np.uint8)
    rc, out, st = _ask(getattr(L, "cjs_bzip2_lines_" + kind), keep.ctypes.data_as(rg.u8p), a.size, h, t, qs)
    return rc, out, st, rg.detail(L)


def ask_device(L, kind, d_in_ptr, n, h, t, qs):
    rc, out, st = _ask(getattr(L, "cjs_bzip2_lines_" + kind + "_device"), d_in_ptr, n, h, t, qs)
    return rc, out, st, rg.detail(L)


def on_device(stream, shift_in=3):
    """the stream at an odd device address -> (tensor to keep, address)"""
    import torch
    n = stream.size
    d_in = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    d_in[shift_in:shift_in + n] = torch.from_numpy(np.ascontiguousarray(stream)).cuda()
    torch.cuda.synchronize()
    return d_in, d_in.data_ptr() + shift_in


def both_forms(L, kind, stream, h, t, qs, dev=None):
    """The host form and the device form (the stream at an odd device address): both must agree in everything.
    -> (answers, status, detail) with answers and status as lists"""
    keep, ptr = dev if dev is not None else on_device(stream)
    rc, out, st, d = ask_host(L, kind, stream, h, t, qs)
    assert rc == 0, (rc, d)
    rc2, out2, st2, d2 = ask_device(L, kind, ptr, stream.size, h, t, qs)
    assert rc2 == 0, (rc2, d2)
    assert out.tolist() == out2.tolist() and st.tolist() == st2.tolist() and d == d2, "the host form and the device form differ"
    return out.tolist(), st.tolist(), d


def build_both(L, stream, h, dev=None):
    """the table of both forms (their counts must agree) -> the host form's handle"""
    keep, ptr = dev if dev is not None else on_device(stream)
    rc, t, d = build_host(L, stream, h)
    assert rc == 0, (rc, d)
    rc2, t2, d2 = build_device(L, ptr, stream.size, h)
    assert rc2 == 0, (rc2, d2)
    assert counts(L, t) == counts(L, t2) and info(L, t) == info(L, t2) and save(L, t) == save(L, t2)
    L.cjs_bzip2_lines_destroy(t2)
    return t


# ---- fixtures
def oracle_bounds(oracle, stream, multistream):
    """decoded block bounds of a stream as the CPU oracle's block table gives them"""
    rc, tab = oracle.bzip2_table(stream, multistream)
    assert rc == 0
    return np.concatenate([[0], np.cumsum([s for _, s in tab])]).astype(np.int64)


def blocks_of_line(nl, total, bounds, k):
    """blocks of non-zero size that line k overlaps"""
    a, b = start(nl, total, k), start(nl, total, k + 1)
    return sum(1 for i in range(len(bounds) - 1) if bounds[i + 1] > bounds[i] and bounds[i] < b and bounds[i + 1] > a)


LN2_SEED = 4321


def ln2(oracle):
    """80 members of 0..6 bytes over the alphabet {'a', newline}, levels cycling 1..9 (the recipe of search_cases.s4): blocks of a
    few bytes, blocks of newlines only, members without a block, lines that span several blocks -> (stream, plain, multistream)"""
    rng = np.random.RandomState(LN2_SEED)
    alphabet = np.array([97, 10], np.uint8)
    parts, plain = [], []
    for k in range(80):
        p = alphabet[rng.randint(0, 2, k % 7)]
        rc, s = oracle.bzip2_compress(p, 1 + k % 9)
        assert rc == 0
        parts.append(np.asarray(s, dtype=np.uint8)); plain.append(p)
    stream, plain = np.concatenate(parts), np.concatenate(plain)
    sizes = [p for p in (k % 7 for k in range(80)) if p]
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    nl, total = newlines(plain), plain.size
    assert max(blocks_of_line(nl, total, bounds, k) for k in range(nl.size + 1)) >= 4, "no line covers four blocks: another seed"
    assert any(c == b - a for c, a, b in zip(block_counts(plain, bounds), bounds[:-1], bounds[1:])), "no block of newlines only"
    return stream, plain, 1


LN3_SEED = 31
LN3_SIZE = 300 * 1024
LN3_QUIET = (98 * 1024 + 2048, 98 * 1024 + 2048 + 40 * 1024)      # no newline in here; one right in front and one right behind
LN3_WHITE = (200 * 1024 + 100, 200 * 1024 + 100 + 4096)          # newlines only


def _ln3_plain(seed, seams):
    rng = np.random.RandomState(seed)
    pool = np.array([b for b in range(256) if b not in (0x0A, 0x0B, 0x8A)], np.uint8)
    plain = pool[rng.randint(0, pool.size, LN3_SIZE)]
    (q0, q1), (w0, w1) = LN3_QUIET, LN3_WHITE
    free = lambda p: not (q0 - 2 <= p <= q1 + 1) and not (w0 - 2 <= p <= w1 + 1)
    for k in range(1, LN3_SIZE // 1024):
        c = k // 16 if k % 16 == 0 else k
        pos = 1024 * k + (-1, 0, 1)[c % 3]
        if free(pos):
            plain[pos] = 10
    plain[q0 - 1] = 10; plain[q1] = 10
    plain[w0:w1] = 10
    seam_bytes = {B + d for B in seams for d in (-2, -1, 0, 1)}
    spots = [int(p) for p in rng.permutation(LN3_SIZE // 8 - 2)[:600] * 8 + 3 if free(int(p)) and free(int(p) + 1) and int(p) not in seam_bytes][:400]
    pairs, highs = spots[:200], spots[200:400]
    for p in pairs:
        plain[p] = 10; plain[p + 1] = 0x0B
    for p in highs:
        plain[p] = 0x8A
    for B in seams:
        plain[B - 1] = 10; plain[B] = 10
    return plain, pairs, highs


def ln3(oracle):
    """One level-1 stream of 300 KiB (see the issue's list): -> (stream, plain, bounds, pairs, highs); every property is asserted"""
    plain, _, _ = _ln3_plain(LN3_SEED, [])
    rc, s = oracle.bzip2_compress(plain, 1)
    assert rc == 0
    first = oracle_bounds(oracle, np.asarray(s, dtype=np.uint8), 0)
    plain, pairs, highs = _ln3_plain(LN3_SEED, [int(B) for B in first[1:-1]])
    rc, s = oracle.bzip2_compress(plain, 1)
    assert rc == 0
    stream = np.asarray(s, dtype=np.uint8)
    bounds = oracle_bounds(oracle, stream, 0)
    assert bounds.tolist() == first.tolist() and len(bounds) >= 4, "the bounds moved: another seed"
    nl = newlines(plain)
    at = set(nl.tolist())
    (q0, q1), (w0, w1) = LN3_QUIET, LN3_WHITE
    assert q1 - q0 == 40 * 1024 and not (plain[q0:q1] == 10).any() and plain[q0 - 1] == 10 and plain[q1] == 10
    assert (plain[w0:w1] == 10).all() and w1 - w0 == 4096
    assert len(pairs) == 200 and len(highs) == 200 and all(plain[p] == 10 and plain[p + 1] == 0x0B for p in pairs)
    assert all(plain[p] == 0x8A for p in highs) and int((plain == 0x8A).sum()) == 200 and int((plain == 0x0B).sum()) == 200
    for seam in (1024, 16384):                              # a newline before, on and behind seams of both sizes
        assert {p - seam * round(p / seam) for p in at if abs(p - seam * round(p / seam)) <= 1 and p > 2} >= {-1, 0, 1}
    for B in bounds[1:-1]:
        assert int(B) - 1 in at and int(B) in at
    return stream, plain, bounds, pairs, highs
