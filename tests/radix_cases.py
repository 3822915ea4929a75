"""The radix sorter on its own (cjs_stage_radix, csrc/stage_radix.hip over csrc/radix.hip): the reference that says what a call must
give, the checker that says where a result differs, and the binding.  numpy only; test_radix_cases_host.py holds the reference
and the checker against restatements and against results that are wrong on purpose, test_gpu_radix.py holds the kernels.

The rule of the sort, as the code has it: stable, on whole 8-bit digits from lo_bit up while a digit starts below hi_bit, i.e. on
sort_word() below, every segment on its own."""
import collections
import ctypes
import os

import numpy as np

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compressjs-flattened_amd")
TILE = 4096          # keys per workgroup (RS_TILE): four waves of 1024 keys each, lane l of a wave takes keys l, 64 + l, ...
DIG, SEGMENTS, FIRST_HIST, GEN = 1, 2, 4, 8
E_NO_DEVICE, E_INVALID = -30, -32
CANARY = 0x5C          # what the output arrays hold before a call

Geom = collections.namedtuple("Geom", "nseg stride n_last")


def plain(n):
    return Geom(1, n, n)


def n_of(geom):
    return (geom.nseg - 1) * geom.stride + geom.n_last


def seg_bounds(geom):
    """[(start, end)] of every segment"""
    return [(s * geom.stride, s * geom.stride + (geom.n_last if s + 1 == geom.nseg else geom.stride)) for s in range(geom.nseg)]


def tiles_per_seg(geom):
    return ((geom.stride if geom.nseg > 1 else geom.n_last) + TILE - 1) // TILE


def cap_for(geom):
    """the smallest capacity whose workspace admits the geometry: segs_for(cap) = cap / 65536 + 2 segments, and
    hist_tiles_for(cap) = ceil(cap / 4096) + cap / 65536 + 258 tiles"""
    cap = max(n_of(geom), (geom.nseg - 2) * 65536)
    while -(-cap // TILE) + cap // 65536 + 258 < geom.nseg * tiles_per_seg(geom):
        cap += 65536
    return cap


def key_dtype(key_bytes):
    return {4: np.uint32, 8: np.uint64}[key_bytes]


def sort_word(keys, key_bytes, lo, hi):
    """what the passes sort on: P = ceil((hi - lo) / 8) digits from bit lo up, clipped at the key width"""
    width = min(8 * (-(-(hi - lo) // 8)), 8 * key_bytes - lo)
    return (np.asarray(keys).astype(np.uint64) >> np.uint64(lo)) & np.uint64((1 << width) - 1)


def reference(keys, vals, geom, lo, hi):
    """the stable sort of every segment by sort_word -> (keys, vals); vals None: key-only"""
    keys = np.asarray(keys)
    key_bytes = keys.dtype.itemsize
    assert keys.size == n_of(geom)
    out_k = np.empty_like(keys)
    out_v = None if vals is None else np.empty_like(vals)
    for a, b in seg_bounds(geom):
        order = np.argsort(sort_word(keys[a:b], key_bytes, lo, hi), kind="stable")
        out_k[a:b] = keys[a:b][order]
        if vals is not None:
            out_v[a:b] = vals[a:b][order]
    return out_k, out_v


def gen_keys(text, nseg, stride, n_last):
    """the sentinel key of round 1 of the suffix sort at every position of every segment: seven 9-bit symbols byte + 1 (0 past the
    segment's end), the first on top, the segment's parity in bit 63 -> (keys u64, vals u32 = the position inside the segment)"""
    geom = Geom(nseg, stride, n_last)
    text = bytes(bytearray(np.asarray(text, dtype=np.uint8)))
    assert len(text) == n_of(geom)
    keys, vals = [], []
    for s, (a, b) in enumerate(seg_bounds(geom)):
        for p in range(a, b):
            k = 0
            for j in range(7):
                k = (k << 9) | (text[p + j] + 1 if p + j < b else 0)
            keys.append(k | ((s & 1) << 63))
            vals.append(p - a)
    return np.array(keys, dtype=np.uint64), np.array(vals, dtype=np.uint32)


def first_hist(keys, geom, lo):
    """the counts of the first digit, one row of 256 per tile, tile-major per segment (as ib_make_keys_hist of dec_ibwt.hip leaves
    them): row seg * tps + tile"""
    tps = tiles_per_seg(geom)
    out = np.zeros((geom.nseg * tps, 256), dtype=np.uint32)
    dig = ((np.asarray(keys).astype(np.uint64) >> np.uint64(lo)) & np.uint64(255)).astype(np.int64)
    for s, (a, b) in enumerate(seg_bounds(geom)):
        for t in range(tps):
            out[s * tps + t] = np.bincount(dig[min(a + t * TILE, b): min(a + (t + 1) * TILE, b)], minlength=256)
    return out


def where(slot, geom):
    """the place of a slot as the kernels see it: segment, tile of the segment, wave and lane of the tile's workgroup"""
    seg = min(slot // geom.stride, geom.nseg - 1)
    off = slot - seg * geom.stride
    return "slot %d = segment %d + %d: tile %d, wave %d, lane %d" % (slot, seg, off, off // TILE, off % TILE // 1024, off % 64)


def check(got_keys, got_vals, want_keys, want_vals, geom):
    """exact equality of keys and (unless key-only) values; the first differing slot with both records otherwise"""
    got_keys, want_keys = np.asarray(got_keys), np.asarray(want_keys)
    assert got_keys.dtype == want_keys.dtype and got_keys.shape == want_keys.shape == (n_of(geom),), (got_keys.dtype, got_keys.shape, want_keys.shape)
    assert (got_vals is None) == (want_vals is None), "values on one side only"
    diff = got_keys != want_keys
    if want_vals is not None:
        got_vals, want_vals = np.asarray(got_vals), np.asarray(want_vals)
        assert got_vals.shape == want_vals.shape == got_keys.shape, (got_vals.shape, want_vals.shape)
        diff = diff | (got_vals != want_vals)
    if not diff.any():
        return
    i = int(np.nonzero(diff)[0][0])
    rec = lambda k, v: "key %#x" % int(k[i]) + ("" if v is None else " value %d" % int(v[i]))
    raise AssertionError("%d slots differ, the first: %s: got %s, want %s" % (int(diff.sum()), where(i, geom), rec(got_keys, got_vals), rec(want_keys, want_vals)))


# ---------------------------------------------------------------- the library
def bind():
    try:
        import torch  # noqa: F401  (one HIP runtime per process: torch's copy is loaded before the library)
    except Exception:
        pass
    L = ctypes.CDLL(os.path.join(PKG, "libcjs_hip.so"))
    V, U32, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.cjs_stage_radix.argtypes = [V, I, V, V, V, U32, I, I, U32, U32, U32, ctypes.c_size_t, U32, I, V, V, ctypes.POINTER(I), ctypes.POINTER(ctypes.c_uint64), V]
    L.cjs_stage_radix.restype = I
    return L


Result = collections.namedtuple("Result", "rc keys vals cur guard_bad")
CUR_UNSET = -77


def run(L, keys, vals, geom, lo, hi, key_bytes=None, flags=0, work_cap=None, work_fill=0xA5, text=None, hist=None):
    """one call of cjs_stage_radix.  keys: u32 / u64 array (None with GEN: key_bytes 8), vals: u32 array or None (key-only).  The
    output arrays hold CANARY bytes before the call and come back as they are, whatever the return code."""
    n = n_of(geom)
    if keys is not None:
        keys = np.ascontiguousarray(keys)
        key_bytes = keys.dtype.itemsize if key_bytes is None else key_bytes
        assert keys.size == n and keys.dtype == key_dtype(key_bytes)
    if vals is not None:
        vals = np.ascontiguousarray(vals, dtype=np.uint32)
        assert vals.size == n
    if text is not None:
        text = np.ascontiguousarray(text, dtype=np.uint8)
        assert text.size == n
    if hist is not None:
        hist = np.ascontiguousarray(hist, dtype=np.uint32)
        assert hist.size == geom.nseg * tiles_per_seg(geom) * 256
    out_k = np.full(max(n, 1) * key_bytes, CANARY, dtype=np.uint8).view(key_dtype(key_bytes))
    out_v = np.full(max(n, 1) * 4, CANARY, dtype=np.uint8).view(np.uint32)
    cur, bad = ctypes.c_int(CUR_UNSET), ctypes.c_uint64(1 << 63)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = L.cjs_stage_radix(ptr(keys), key_bytes, ptr(vals), ptr(text), ptr(hist), n, lo, hi, geom.nseg, geom.stride, geom.n_last,
                           n if work_cap is None else work_cap, flags, work_fill, out_k.ctypes.data, out_v.ctypes.data, ctypes.byref(cur), ctypes.byref(bad), None)
    return Result(rc, out_k[:n], out_v[:n], cur.value, bad.value)


def untouched(res):
    """the outputs of a refused call: still the canary, cur as it was"""
    return res.cur == CUR_UNSET and bool((res.keys.view(np.uint8) == CANARY).all()) and bool((res.vals.view(np.uint8) == CANARY).all())
