"""Shared pieces of the tally tests (test_tally_host.py, test_gpu_tally.py): the ctypes binding of cjs_keys_tally[_device] /
cjs_stage_keys_tally / cjs_bzip2_tally[_device], the restatement of a frequency table (collections.Counter over the things
themselves, ordered by the two rules), the made-up key lists of the primitive's tests, and the fixture TL1 of the stream tally with
its planted lines."""
import collections
import ctypes

import numpy as np

import linekeys_cases as lk
import range_cases as rg

U32, U64 = ctypes.c_uint32, ctypes.c_uint64
KEY = lk.KEY
TALLY = np.dtype([("hash", "<u8"), ("len", "<u4"), ("check", "<u4")] + [("first", "<u8"), ("count", "<u8")])
BY_FIRST, BY_COUNT = 0, 1
E_INVALID, E_UNSUPPORTED, E_NO_DEVICE = -32, -34, -30
ONES = lk.ONES
CANARY = lk.CANARY
MAX_KEYS = 2 ** 32 - 2


class TallyInfo(ctypes.Structure):
    _fields_ = [("n_keys", U64), ("n_bad", U64), ("n_distinct", U64), ("n_groups", U64), ("max_count", U64)]


def bind():
    L = lk.bind()
    V, S = rg.V, rg.S
    tail = [S, U32, U64, U64, V, S, ctypes.POINTER(TallyInfo)]
    L.cjs_keys_tally.argtypes = [V] + tail + [V]
    L.cjs_keys_tally_device.argtypes = [V] + tail + [V]
    L.cjs_stage_keys_tally.argtypes = [V] + tail
    return bind_stream(L)


def info_tuple(i):
    return (i.n_keys, i.n_bad, i.n_distinct, i.n_groups, i.max_count)


# ---- the restatement: groups by the things themselves (tuples of a key list, or the lines of a text), never by a hash
def tally_ref(items, order=BY_COUNT, min_count=1, max_count=0, bad=ONES):
    """-> ([(item, first, count)] in the order asked for, (n, n_bad, n_distinct, n_groups, max_count))"""
    count = collections.Counter()
    first = {}
    n_bad = 0
    for i, x in enumerate(items):
        if x == bad:
            n_bad += 1
            continue
        count[x] += 1
        first.setdefault(x, i)
    groups = [(x, first[x], c) for x, c in count.items() if c >= min_count and (max_count == 0 or c <= max_count)]
    groups.sort(key=(lambda g: (-g[2], g[1])) if order == BY_COUNT else (lambda g: g[1]))
    return groups, (len(items), n_bad, len(count), len(groups), max(count.values()) if count else 0)


def key_array(tuples):
    """[(hash, len, check)] -> a KEY array (by columns: lists of a million tuples are in the GPU tests)"""
    a = np.zeros(len(tuples), dtype=KEY)
    if len(tuples):
        cols = list(zip(*tuples))
        a["hash"], a["len"], a["check"] = np.array(cols[0], np.uint64), np.array(cols[1], np.uint32), np.array(cols[2], np.uint32)
    return a


def groups_as_tuples(groups):
    """a TALLY array -> [((hash, len, check), first, count)]"""
    return [((h, l, c), f, n) for h, l, c, f, n in groups.tolist()]


# ---- the calls
def _guarded(cap):
    buf = np.full((cap + 2) * TALLY.itemsize, CANARY, np.uint8)
    return buf, buf.ctypes.data + TALLY.itemsize


def _unguard(buf, cap, written):
    assert (buf[:TALLY.itemsize] == CANARY).all(), "the call wrote in front of its array"
    assert (buf[(1 + written) * TALLY.itemsize:] == CANARY).all(), "the call wrote past what it may write"
    return buf.view(TALLY)[1:1 + written].copy()


def _call(fn, ptr, n, order, min_count, max_count, cap, opts):
    buf, out = _guarded(cap)
    info = TallyInfo(7, 7, 7, 7, 7)
    rc = fn(ptr, n, order, min_count, max_count, out if cap else None, cap, ctypes.byref(info), *opts)
    groups = _unguard(buf, cap, min(cap, info.n_groups) if rc == 0 else 0)
    return rc, groups, info


def stage_tally(L, keys, order=BY_COUNT, min_count=1, max_count=0, cap=None):
    """cjs_stage_keys_tally over a KEY array -> (rc, groups, info); cap=None: room for every key"""
    keys = np.ascontiguousarray(keys, dtype=KEY)
    return _call(L.cjs_stage_keys_tally, keys.ctypes.data if keys.size else None, keys.size, order, min_count, max_count,
                 keys.size if cap is None else cap, ())


def host_tally(L, keys, order=BY_COUNT, min_count=1, max_count=0, cap=None):
    """cjs_keys_tally (host keys, GPU grouping) -> (rc, groups, info)"""
    keys = np.ascontiguousarray(keys, dtype=KEY)
    return _call(L.cjs_keys_tally, keys.ctypes.data if keys.size else None, keys.size, order, min_count, max_count,
                 keys.size if cap is None else cap, (None,))


def device_tally(L, torch, keys, order=BY_COUNT, min_count=1, max_count=0, cap=None, shift=0):
    """cjs_keys_tally_device: the keys at a device address `shift` bytes past a 256-byte boundary, the groups in device memory
    between canaries -> (rc, groups, info)"""
    keys = np.ascontiguousarray(keys, dtype=KEY)
    cap = keys.size if cap is None else cap
    raw = np.concatenate([np.zeros(shift, np.uint8), keys.view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])
    d_keys = torch.from_numpy(raw).cuda()
    d_out = torch.full(((cap + 2) * TALLY.itemsize,), CANARY, dtype=torch.uint8, device="cuda")
    info = TallyInfo(7, 7, 7, 7, 7)
    rc = L.cjs_keys_tally_device(d_keys.data_ptr() + shift if keys.size else None, keys.size, order, min_count, max_count,
                                 d_out.data_ptr() + TALLY.itemsize if cap else None, cap, ctypes.byref(info), None)
    torch.cuda.synchronize()
    return rc, _unguard(d_out.cpu().numpy(), cap, min(cap, info.n_groups) if rc == 0 else 0), info


# ---- made-up key lists
def random_keys(rng, n, pool, bad_share=0.0):
    """n keys drawn with skewed weights from `pool` made-up records that collide field by field (few values per field), some bad"""
    vals = [(int(rng.randint(0, 4)) << 58 | int(rng.randint(0, 3)), int(rng.randint(0, 3)), (0, 1, 1 << 31)[rng.randint(0, 3)]) for _ in range(pool)]
    w = 1.0 / np.arange(1, pool + 1)
    pick = rng.choice(pool, size=n, p=w / w.sum())
    out = [vals[i] for i in pick]
    for i in np.nonzero(rng.rand(n) < bad_share)[0]:
        out[i] = ONES
    return out


# ---- the stream tally (cjs_bzip2_tally[_device])
M64 = lk.M64
TILE = 16384
LINES, FIELDS, BYTES = 2, 0, 1          # CJS_TALLY_LINES beside CJS_CUT_FIELDS and CJS_CUT_BYTES


class StreamInfo(ctypes.Structure):
    _fields_ = [("n_lines", U64), ("n_bad_lines", U64), ("n_distinct", U64), ("n_groups", U64), ("max_count", U64), ("blocks_decoded", U64),
                ("n_bad_blocks", U64), ("first_bad_block", U64)]


def bind_stream(L):
    V, S = rg.V, rg.S
    tail = [V, V, U64, U64, U64, U32, U32, V, U32, U32, U64, U64, V, S, ctypes.POINTER(StreamInfo), V]
    L.cjs_bzip2_tally.argtypes = [rg.u8p, S] + tail
    L.cjs_bzip2_tally_device.argtypes = [V, S] + tail
    L.cjs_stage_bzip2_tally_limit.argtypes = [V, V, S, V, V, U64, U64, U64, V, S, ctypes.POINTER(StreamInfo), V]
    L.cjs_stage_text_keys_device.argtypes = [V, S, U64, V, S, rg.PS, S, V]
    return L


def stream_info_tuple(i):
    return (i.n_lines, i.n_bad_lines, i.n_distinct, i.n_groups, i.max_count, i.blocks_decoded, i.n_bad_blocks, i.first_bad_block)


def stream_tally(L, fn, src, n, h, t, first=0, count=M64, seed=0, mode=LINES, d=0, sel=(), order=BY_COUNT, min_count=1, max_count=0, cap=None):
    """cjs_bzip2_tally[_device] -> (rc, groups, info, detail); cap=None: the count query first, then exactly that many"""
    r = np.zeros(max(len(sel), 1), dtype=np.dtype([("lo", "<u4"), ("hi", "<u4")]))
    for k, x in enumerate(sel):
        r[k] = x

    def call(cap):
        buf, out = _guarded(cap)
        info = StreamInfo(*([7] * 8))
        rc = fn(src, n, h, t, first, count, seed, mode, d, r.ctypes.data if len(sel) else None, len(sel), order, min_count, max_count, out if cap else None, cap,
                ctypes.byref(info), None)
        det = rg.detail(L)
        return rc, _unguard(buf, cap, min(cap, info.n_groups) if rc == 0 else 0), info, det
    if cap is None:
        rc, _, info, det = call(0)
        if rc:
            return rc, None, info, det
        cap = info.n_groups
    return call(cap)


def both_forms(L, f, **kw):
    """The host form and the device form (the stream at an odd device address): both must agree in everything -> (groups, info)"""
    a = np.ascontiguousarray(f["stream"], dtype=np.uint8)
    rc, g1, i1, d1 = stream_tally(L, L.cjs_bzip2_tally, a.ctypes.data_as(rg.u8p), a.size, f["h"], f["t"], **kw)
    assert rc == 0, (rc, d1)
    rc, g2, i2, d2 = stream_tally(L, L.cjs_bzip2_tally_device, f["dev"][1], a.size, f["h"], f["t"], **kw)
    assert rc == 0, (rc, d2)
    assert g1.tobytes() == g2.tobytes() and stream_info_tuple(i1) == stream_info_tuple(i2) and d1 == d2, "the host form and the device form differ"
    return g1, i1


def window_lines(plain, first=0, count=None):
    """the lines of the window as the tally counts them, without their newlines: lines first .. of the table's numbering; the tail
    line, if it is inside and not empty, like any other; an empty tail is no line"""
    parts = bytes(plain).split(b"\n")
    N = len(parts) - 1
    end = N + 1 if count is None else min(first + count, N + 1)
    return [parts[k] for k in range(first, end) if k < N or parts[k]]


_key_memo = {}


def key_of(line, seed):
    """the record of `line` + newline"""
    if (line, seed) not in _key_memo:
        _key_memo[(line, seed)] = lk.line_key(line + b"\n", *lk.bases(seed))
    return _key_memo[(line, seed)]


def distinct_lines_have_distinct_records(plain, seeds):
    """what lets a table by records be compared with a table by content: no two lines of the fixture share a record"""
    lines = set(window_lines(plain))
    return all(len({key_of(x, s) for x in lines}) == len(lines) for s in seeds)


def cut_window_lines(plain, mode, d, sel, first=0, count=None):
    """the lines of the cut of the window (cut_cases.cut_ref: split, select, join), without their newlines: one per line of the
    window, the empty tail left out"""
    import cut_cases as ct
    return ct.cut_ref(plain, mode, d, sel, first=first, count=count).split(b"\n")[:-1]


def check_against_the_lines(groups, info, plain, seed=0, first=0, count=None, order=BY_COUNT, min_count=1, max_count=0, cap=None, n_bad=0, cut=None):
    """the groups are those of collections.Counter over the window's real lines (cut = (mode, d, sel): over the lines of their cut),
    in the order asked for; every group's `first` is a line of that content and its key that line's record"""
    items = window_lines(plain, first, count) if cut is None else cut_window_lines(plain, *cut, first=first, count=count)
    assert len(items) == len(window_lines(plain, first, count))
    ref, rinfo = tally_ref(items, order, min_count, max_count, bad=None)
    assert stream_info_tuple(info)[:5] == (rinfo[0], n_bad) + rinfo[2:], (stream_info_tuple(info), rinfo)
    want = ref if cap is None else ref[:cap]
    assert [(f, c) for _, f, c in groups_as_tuples(groups)] == [(first + f, c) for _, f, c in want]
    for (key, f, c), (item, _, _) in zip(groups_as_tuples(groups), want):
        assert items[f - first] == item and key == key_of(item, seed), (f, item[:60])
    if (min_count, max_count) in ((1, 0), (0, 0)) and cap is None:
        assert int(groups["count"].sum()) == info.n_lines - info.n_bad_lines


# TL1: about 300 KiB of tab-separated lines at level 1, drawn with skewed weights from a pool of 200, with planted lines.  No byte
# stands four times in a row, so the first compression stage leaves the text as it is and a block holds 99,981 bytes of it: the
# planted positions are laid out by that and asserted from the fixture's own bounds (tl1_planted).
TL1_SEED, TL1_BLOCK, TL1_BIG = 31337, 99981, 40 * 1024
TL1_SEAM, TL1_TILE_LINE = b"seam\tof\ttwo\tblocks\t0123456789abcdefghij", b"tile\tseam\tline\tABCDEFGHIJKLMNOPQRSTUVWXYZ"


def _no_runs(rng, n):
    """n lower-case letters, no two neighbours equal"""
    steps = rng.randint(1, 26, n)
    return bytes((97 + np.cumsum(steps) % 26).astype(np.uint8))


def tl1_plain():
    rng = np.random.RandomState(TL1_SEED)
    pool = [b"\t".join(_no_runs(rng, int(rng.randint(1, 9))) for _ in range(int(rng.randint(3, 6)))) for _ in range(200)]
    assert len(set(pool)) == 200
    w = 1.0 / np.arange(1, 201)
    draw = iter(rng.choice(200, size=40000, p=w / w.sum()).tolist())
    big = _no_runs(rng, TL1_BIG)
    out, pos = [], 0

    def put(line):
        nonlocal pos
        out.append(line)
        pos += len(line) + 1

    def fill_to(target):          # pool lines, then one filler line, so that the next line starts at `target`
        while pos < target - 120:
            put(pool[next(draw)])
        put((b"fg" * 60)[:target - pos - 1])
        assert pos == target

    for k in range(10):
        put(pool[next(draw)])
    put(TL1_SEAM); put(TL1_TILE_LINE); put(b""); put(b""); put(big)          # inside block 0: the twins of the planted lines
    fill_to(3 * TILE - 20); put(TL1_TILE_LINE)                                # across the seam of tiles 2 and 3 of block 0
    fill_to(TL1_BLOCK - 17); put(TL1_SEAM)                                    # across the seam of blocks 0 and 1
    for k in range(8):
        put(pool[next(draw)]); put(b""); put(b"")
    fill_to(2 * TL1_BLOCK - 1000); put(big)                                   # across the seam of blocks 1 and 2, over three tiles
    while pos < 300 * 1024:
        put(pool[next(draw)])
    return np.frombuffer(b"\n".join(out) + b"\n" + pool[0], dtype=np.uint8).copy(), pool          # an unterminated tail equal to the most frequent line


def tl1(oracle):
    plain, _ = tl1_plain()
    rc, s = oracle.bzip2_compress(plain, 1)
    assert rc == 0
    return np.asarray(s, dtype=np.uint8), plain, 0


def tl1_planted(plain, bounds):
    """where the planted lines stand, from the fixture's own bytes and bounds -> dict of line-number lists"""
    parts = bytes(plain).split(b"\n")
    starts = np.concatenate([[0], np.cumsum([len(p) + 1 for p in parts])[:-1]])
    where = lambda line: [k for k, p in enumerate(parts) if p == line]
    inside = lambda k, cuts: [c for c in cuts if starts[k] < c < starts[k] + len(parts[k]) + 1]          # cuts with bytes of line k on both sides
    tiles = [int(a) + TILE * j for a, b in zip(bounds[:-1], bounds[1:]) for j in range(1, (int(b - a) + TILE - 1) // TILE)]
    blocks = [int(b) for b in bounds[1:-1]]
    return dict(seam=[(k, bool(inside(k, blocks))) for k in where(TL1_SEAM)], tile=[(k, bool(inside(k, tiles)), bool(inside(k, blocks))) for k in where(TL1_TILE_LINE)],
                big=[(k, len(inside(k, tiles)), bool(inside(k, blocks))) for k, p in enumerate(parts) if len(p) == TL1_BIG],
                empty=where(b"")[:-1] if not parts[-1] else where(b""), tail=parts[-1], tail_twins=where(parts[-1])[:-1])


def stream_fixture(L, name, oracle):
    """TL1, or a fixture of the cut tests (CT2: 639 tiny blocks and a line over 13 of them; CT3: no block)"""
    import cut_cases as ct
    if name != "TL1":
        return ct.fixture(L, name, oracle)
    stream, plain, multi = tl1(oracle)
    rc, h = rg.build(L, stream, multi)
    assert rc == 0, (name, rc, rg.detail(L))
    e = rg.entries(L, h)
    bounds = np.concatenate([[0], np.cumsum([x[2] for x in e])]).astype(np.int64)
    import lines_cases as lc
    f = dict(name=name, stream=stream, plain=plain, text=plain.tobytes(), h=h, entries=e, bounds=bounds, nl=lc.newlines(plain), total=int(plain.size), multi=multi)
    f["dev"] = lc.on_device(stream)
    f["t"] = lc.build_both(L, stream, h, f["dev"])
    return f
