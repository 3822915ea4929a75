"""Shared pieces of the indexed range-read tests (test_range_host.py, test_gpu_range.py, test_gpu_range_js.py): the ctypes
binding of the index and range entry points, the serialised index as numpy builds it, the three fixture streams and the range
list.  Streams come from the CPU oracle and tests/golden/data; the expected bytes of a range are always plain[off:off + len]."""
import ctypes
import os

import numpy as np

import support

u8p = ctypes.POINTER(ctypes.c_uint8)
S, I, V = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
U64 = ctypes.c_uint64
PU, PS, PI32 = ctypes.POINTER(U64), ctypes.POINTER(S), ctypes.POINTER(ctypes.c_int32)
E_DATA, E_NO_DEVICE, E_INVALID, E_TOO_SMALL = -5, -30, -32, -33

ENTRY = np.dtype([("bitpos", "<u8"), ("end_bit", "<u8"), ("size", "<u4"), ("crc", "<u4"), ("level", "<u4"), ("reserved", "<u4")])
HEADER = np.dtype([("magic", "S8"), ("version", "<u4"), ("flags", "<u4"), ("stream_bytes", "<u8"), ("count", "<u8")])


class Entry(ctypes.Structure):
    _fields_ = [("bitpos", U64), ("end_bit", U64), ("size", ctypes.c_uint32), ("crc", ctypes.c_uint32), ("level", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


def bind():
    L = ctypes.CDLL(os.path.join(support.PKG, "libcjs_hip.so"))
    L.cjs_bzip2_index_build.argtypes = [u8p, S, I, ctypes.POINTER(V), V]
    L.cjs_bzip2_index_create.argtypes = [ctypes.POINTER(Entry), S, U64, I, ctypes.POINTER(V)]
    L.cjs_bzip2_index_save.argtypes = [V, ctypes.POINTER(u8p), PS]
    L.cjs_bzip2_index_load.argtypes = [u8p, S, ctypes.POINTER(V)]
    L.cjs_bzip2_index_info.argtypes = [V, PU, PU, PU, ctypes.POINTER(I)]
    L.cjs_bzip2_index_entries.argtypes = [V, ctypes.POINTER(Entry), ctypes.c_long]
    L.cjs_bzip2_index_entries.restype = ctypes.c_long
    L.cjs_bzip2_index_destroy.argtypes = [V]
    L.cjs_bzip2_index_destroy.restype = None
    L.cjs_bzip2_read_ranges.argtypes = [u8p, S, V, PU, PU, S, ctypes.POINTER(u8p), PS, PS, PI32, V]
    L.cjs_bzip2_read_ranges_device.argtypes = [V, S, V, PU, PU, S, V, S, PS, PS, PI32, PS, V]
    L.cjs_bzip2_table.argtypes = [u8p, S, I, PU, ctypes.POINTER(ctypes.c_uint32), ctypes.c_long, V]
    L.cjs_bzip2_table.restype = ctypes.c_long
    L.cjs_bzip2_decompress_block.argtypes = [u8p, S, U64, ctypes.POINTER(u8p), PS, V]
    L.cjs_last_error_detail.restype = ctypes.c_char_p
    L.cjs_free.argtypes = [V]
    L.cjs_free.restype = None
    return L


def detail(L):
    return L.cjs_last_error_detail().decode()


def image(entries, stream_bytes, multistream):
    """the serialised index of `entries` (rows of bitpos, end_bit, size, crc, level, reserved) as the format says"""
    h = np.zeros(1, dtype=HEADER)
    h["magic"], h["version"], h["flags"], h["stream_bytes"], h["count"] = b"CJSBZIX1", 1, 1 if multistream else 0, stream_bytes, len(entries)
    e = np.zeros(len(entries), dtype=ENTRY)
    for k, row in enumerate(entries):
        e[k] = tuple(row)
    return h.tobytes() + e.tobytes()


def create(L, entries, stream_bytes, multistream=0):
    """cjs_bzip2_index_create -> (rc, handle)"""
    arr = (Entry * max(len(entries), 1))(*[Entry(*row) for row in entries])
    h = V()
    rc = L.cjs_bzip2_index_create(arr, len(entries), stream_bytes, multistream, ctypes.byref(h))
    return rc, h


def load(L, raw):
    a = np.frombuffer(raw, dtype=np.uint8).copy() if len(raw) else np.zeros(1, np.uint8)
    h = V()
    rc = L.cjs_bzip2_index_load(a.ctypes.data_as(u8p), len(raw), ctypes.byref(h))
    return rc, h


def save(L, h):
    out, n = u8p(), S(0)
    assert L.cjs_bzip2_index_save(h, ctypes.byref(out), ctypes.byref(n)) == 0
    raw = ctypes.string_at(out, n.value)
    L.cjs_free(out)
    return raw


def entries(L, h):
    nb = L.cjs_bzip2_index_entries(h, None, 0)
    arr = (Entry * max(nb, 1))()
    assert L.cjs_bzip2_index_entries(h, arr, nb) == nb
    return [(e.bitpos, e.end_bit, e.size, e.crc, e.level, e.reserved) for e in arr[:nb]]


def info(L, h):
    b, t, sb, m = U64(0), U64(0), U64(0), I(0)
    assert L.cjs_bzip2_index_info(h, ctypes.byref(b), ctypes.byref(t), ctypes.byref(sb), ctypes.byref(m)) == 0
    return b.value, t.value, sb.value, m.value


def build(L, data, multistream=0):
    a = np.ascontiguousarray(data, dtype=np.uint8)
    keep = a if a.size else np.zeros(1, np.uint8)
    h = V()
    rc = L.cjs_bzip2_index_build(keep.ctypes.data_as(u8p), a.size, multistream, ctypes.byref(h), None)
    return rc, h


def _arrays(ranges):
    count = len(ranges)
    off = np.array([r[0] for r in ranges] or [0], dtype=np.uint64)
    ln = np.array([r[1] for r in ranges] or [0], dtype=np.uint64)
    return count, off, ln, np.full(max(count, 1), 7, np.uint64), np.full(max(count, 1), 7, np.uint64), np.full(max(count, 1), 7, np.int32)


def read_host(L, data, h, ranges):
    """cjs_bzip2_read_ranges -> (rc, bytes of the result buffer, out_off, out_len, status, detail)"""
    a = np.ascontiguousarray(data, dtype=np.uint8)
    keep = a if a.size else np.zeros(1, np.uint8)
    count, off, ln, o_off, o_len, st = _arrays(ranges)
    out = u8p()
    rc = L.cjs_bzip2_read_ranges(keep.ctypes.data_as(u8p), a.size, h, off.ctypes.data_as(PU), ln.ctypes.data_as(PU), count, ctypes.byref(out),
                                 o_off.ctypes.data_as(PS), o_len.ctypes.data_as(PS), st.ctypes.data_as(PI32), None)
    d = detail(L)
    if rc:
        assert not out
        return rc, b"", None, None, None, d
    assert out
    buf = ctypes.string_at(out, int(o_len[:count].sum()))
    L.cjs_free(out)
    return rc, buf, o_off[:count].astype(np.int64), o_len[:count].astype(np.int64), st[:count].copy(), d


def read_device(L, d_in, n, h, ranges, d_out_ptr, out_cap):
    """cjs_bzip2_read_ranges_device -> (rc, out_off, out_len, status, need, detail)"""
    count, off, ln, o_off, o_len, st = _arrays(ranges)
    need = S(0)
    rc = L.cjs_bzip2_read_ranges_device(d_in, n, h, off.ctypes.data_as(PU), ln.ctypes.data_as(PU), count, d_out_ptr, out_cap,
                                        o_off.ctypes.data_as(PS), o_len.ctypes.data_as(PS), st.ctypes.data_as(PI32), ctypes.byref(need), None)
    return rc, o_off[:count].astype(np.int64), o_len[:count].astype(np.int64), st[:count].copy(), need.value, detail(L)


# ---- fixtures
def golden(name):
    return np.fromfile(os.path.join(support.ROOT, "tests", "golden", "data", name), dtype=np.uint8)


def f1():
    """sample4: 10 level-1 blocks, 938,848 bytes -> (stream, plain, multistream, members as (first byte, level))"""
    return golden("sample4.bz2"), golden("sample4.ref"), 0, [(0, 1)]


def f2(oracle):
    """about 40 members of 0..300 bytes under BZh1..BZh9: tiny blocks, level changes, members without any block"""
    rng = np.random.RandomState(1234)
    parts, plain, members, at = [], [], [], 0
    for k in range(40):
        size = 0 if k % 7 == 3 else int(rng.randint(1, 301))
        p = rng.randint(97, 105, size).astype(np.uint8)
        rc, s = oracle.bzip2_compress(p, 1 + k % 9)
        assert rc == 0
        parts.append(np.asarray(s, dtype=np.uint8)); plain.append(p); members.append((at, 1 + k % 9))
        at += len(s)
    return np.concatenate(parts), np.concatenate(plain), 1, members


def f3(oracle):
    """~350 kB of run-heavy bytes at level 1: the blocks of one member decode to very different sizes"""
    rng = np.random.RandomState(77)
    parts = []
    while sum(p.size for p in parts) < 350000:
        parts.append(rng.randint(0, 256, int(rng.randint(10000, 50000))).astype(np.uint8))      # decodes one to one
        left = int(rng.randint(3000, 40000))                                                     # a stretch of runs: RLE1 shrinks it
        while left > 0:
            run = min(left, int(rng.randint(5, 257)))
            parts.append(np.full(run, int(rng.randint(0, 256)), np.uint8))
            left -= run
    plain = np.concatenate(parts)
    rc, s = oracle.bzip2_compress(plain, 1)
    assert rc == 0
    return np.asarray(s, dtype=np.uint8), plain, 0, [(0, 1)]


def fixture(name, oracle):
    return {"F1": f1, "F2": lambda: f2(oracle), "F3": lambda: f3(oracle)}[name]()


def bits(stream, pos, k):
    """the k bits at bit `pos` of the stream as a number"""
    v = 0
    for b in range(pos, pos + k):
        v = (v << 1) | ((int(stream[b >> 3]) >> (7 - (b & 7))) & 1)
    return v


def set_bits(stream, pos, k, v):
    """write the number v into the k bits at bit `pos` of the stream (in place)"""
    for i, b in enumerate(range(pos, pos + k)):
        bit = (v >> (k - 1 - i)) & 1
        stream[b >> 3] = (int(stream[b >> 3]) & ~(1 << (7 - (b & 7)))) | (bit << (7 - (b & 7)))


def both_forms(L, stream, h, ranges, shift_in=3, shift_out=5):
    """One host call and one device call: -> ((buf, off, len, status, detail), (region, off, len, status, detail)) with the device
    stream and result at odd addresses, the result between two canary regions that must come back unchanged."""
    import torch
    rc, buf, off, ln, st, d = read_host(L, stream, h, ranges)
    assert rc == 0
    n = stream.size
    d_in = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    d_in[shift_in:shift_in + n] = torch.from_numpy(np.ascontiguousarray(stream)).cuda()
    rc, qoff, qln, qst, need, qd = read_device(L, d_in.data_ptr() + shift_in, n, h, ranges, None, 0)      # the size query
    assert rc == (E_TOO_SMALL if need else 0)
    guard = 4096
    d_out = torch.full((need + 2 * guard + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    base = guard + shift_out
    if need:                                                # one byte short: refused, nothing written
        rc1 = read_device(L, d_in.data_ptr() + shift_in, n, h, ranges, d_out.data_ptr() + base, need - 1)
        assert rc1[0] == E_TOO_SMALL and rc1[4] == need and bool((d_out == 0xA5).all())
    rc, doff, dln, dst, dneed, dd = read_device(L, d_in.data_ptr() + shift_in, n, h, ranges, d_out.data_ptr() + base, need)
    torch.cuda.synchronize()
    assert rc == 0 and dneed == need and doff.tolist() == qoff.tolist()
    got = d_out.cpu().numpy()
    assert (got[:base] == 0xA5).all() and (got[base + need:] == 0xA5).all(), "the device form wrote outside its region"
    return (buf, off, ln, st, d), (got[base:base + need], doff, dln, dst, dd)


def range_list(sizes, seed=5):
    """Several hundred (off, len): every block boundary from one before to one after as start and as end, lengths 0, 1, 15, 16,
    17, 31, 33, 4095..4097 at starts that walk through every residue mod 16 (and so does the packed destination), spans of 2 and
    3 blocks, the whole stream, duplicates, overlaps, a descending stretch, ranges clipped at the end, at the end and past it."""
    bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(bounds[-1])
    rng = np.random.RandomState(seed)
    r = []
    lens = [0, 1, 15, 16, 17, 31, 33, 4095, 4096, 4097]
    for i in range(160):                                    # every length at every start residue mod 16; the destination drifts with the lengths
        r.append((min(total, 1000 + 17 * i + i // 80), lens[i % len(lens)]))
    for i, ln in enumerate(lens * 2):
        r.append((int(rng.randint(0, max(total - ln, 1))) + i % 16, ln))
    edges = sorted(set(int(b) for b in bounds))
    step = max(1, len(edges) // 24)                         # (a file of tiny blocks: every few boundaries)
    for b in edges[::step] + edges[-2:]:
        for d in (-1, 0, 1):
            if 0 <= b + d <= total:
                r.append((b + d, 33))                       # starts on, before and behind the boundary
                if b + d >= 40:
                    r.append((b + d - 40, 40))              # ends there
    nz = [k for k in range(len(sizes)) if sizes[k]]
    for a in range(0, max(len(nz) - 3, 1), max(1, len(nz) // 8)):
        k = nz[a]
        r.append((int(bounds[k]) + 5, int(bounds[min(k + 2, len(sizes))] - bounds[k])))            # into the next block (or two)
        r.append((int(bounds[k + 1]) - 3, int(bounds[min(k + 3, len(sizes))] - bounds[k + 1]) + 6))  # over a whole block
        r.append((int(bounds[k]), int(sizes[k])))           # exactly a block
    r.append((0, total))
    r.append((0, total))                                    # duplicate
    r.append((7, total))                                    # clipped
    r += [(total - 1, 5), (total, 4), (total + 9, 3), (total, 0), (2 ** 63, 2 ** 62)]
    r += [(p, 300) for p in range(min(total, 9000), 0, -701)][:12]      # descending, overlapping
    return [(int(a), int(b)) for a, b in r]


def expected(plain, ranges):
    total = plain.size
    return [plain[min(a, total):min(a + b, total)].tobytes() for a, b in ranges]
