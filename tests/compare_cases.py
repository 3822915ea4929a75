"""Shared pieces of the compare tests (test_compare_host.py, test_gpu_compare.py, test_gpu_compare_js.py): the ctypes binding of
cjs_bzip2_compare[_device] and cjs_bzip2_compare_streams[_device], the canary harness of `diffs`, the expected list as numpy finds
it in the decoded text (numpy.nonzero(plain != other)), and the flip sets.  The streams come from the CPU oracle and
tests/golden/data (range_cases, search_cases)."""
import ctypes

import numpy as np

import range_cases as rg

U8, U64 = ctypes.c_uint8, ctypes.c_uint64
DIFF = np.dtype([("off", "<u8"), ("a", "u1"), ("b", "u1"), ("reserved", "u1", (6,))])
ALL = 2 ** 64 - 1
NONE = 2 ** 64 - 1


class Diff(ctypes.Structure):
    _fields_ = [("off", U64), ("a", U8), ("b", U8), ("reserved", U8 * 6)]


class Info(ctypes.Structure):
    _fields_ = [("n_diffs", U64), ("first_diff", U64), ("compared", U64), ("n_bad_blocks", U64), ("first_bad_block", U64), ("blocks_decoded", U64),
                ("n_bad_blocks_b", U64), ("first_bad_block_b", U64)]


def bind():
    L = rg.bind()
    tail = [U64, U64, rg.V, rg.S, ctypes.POINTER(Info), rg.V]
    L.cjs_bzip2_compare.argtypes = [rg.u8p, rg.S, rg.V, rg.u8p, rg.S, U64] + tail
    L.cjs_bzip2_compare_device.argtypes = [rg.V, rg.S, rg.V, rg.V, rg.S, U64] + tail
    L.cjs_bzip2_compare_streams.argtypes = [rg.u8p, rg.S, rg.V, rg.u8p, rg.S, rg.V] + tail
    L.cjs_bzip2_compare_streams_device.argtypes = [rg.V, rg.S, rg.V, rg.V, rg.S, rg.V] + tail
    return L


def info_tuple(info):
    return (info.n_diffs, info.first_diff, info.compared, info.n_bad_blocks, info.first_bad_block, info.blocks_decoded, info.n_bad_blocks_b,
            info.first_bad_block_b)


ZERO_INFO = (0, NONE, 0, 0, NONE, 0, 0, NONE)


def expected(plain, other, other_off=0, off=0, ln=ALL, runs=None):
    """-> ([(off, a, b)] ascending, compared): numpy.nonzero(plain != other) over the span [max(off, other_off), min(off + ln,
    len(plain), other_off + len(other))) cut to `runs` ([(lo, hi)] of decoded offsets; None: everything)"""
    plain, other = np.asarray(plain, np.uint8), np.asarray(other, np.uint8)
    lo, hi = max(off, other_off), min(off + ln, plain.size, other_off + other.size)
    out, compared = [], 0
    for r_lo, r_hi in (runs if runs is not None else [(0, plain.size)]):
        a, b = max(lo, r_lo), min(hi, r_hi)
        if a >= b:
            continue
        x, y = plain[a:b], other[a - other_off:b - other_off]
        at = np.nonzero(x != y)[0]
        out += list(zip((at + a).tolist(), x[at].tolist(), y[at].tolist()))
        compared += b - a
    return sorted(out), compared


GUARD = 64      # canary records on either side of `diffs`


def _call(fn, head, off, ln, cap):
    """-> (rc, [(off, a, b)], info); `diffs` lies between canaries that must come back unchanged, as must every record past the
    first min(cap, n_diffs)"""
    buf = np.full((cap + 2 * GUARD) * 16, 0xA5, np.uint8)
    info = Info(7, 7, 7, 7, 7, 7, 7, 7)
    diffs = ctypes.c_void_p(buf.ctypes.data + 16 * GUARD) if cap else None
    rc = fn(*head, off, ln, diffs, cap, ctypes.byref(info), None)
    if rc:
        assert (buf == 0xA5).all()
        return rc, None, info
    got = min(cap, info.n_diffs)
    assert (buf[:16 * GUARD] == 0xA5).all() and (buf[16 * (GUARD + got):] == 0xA5).all(), "the compare wrote outside its first min(cap, n_diffs) records"
    rec = buf[16 * GUARD:16 * (GUARD + got)].view(DIFF)
    assert not rec["reserved"].any()
    return rc, list(zip(rec["off"].tolist(), rec["a"].tolist(), rec["b"].tolist())), info


def _host(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    keep = a if a.size else np.zeros(1, np.uint8)
    return keep, keep.ctypes.data_as(rg.u8p), a.size


def compare_host(L, stream, h, other, other_off=0, off=0, ln=ALL, cap=0):
    k1, p1, n1 = _host(stream)
    k2, p2, n2 = _host(other)
    rc, m, info = _call(L.cjs_bzip2_compare, (p1, n1, h, p2, n2, other_off), off, ln, cap)
    return rc, m, info, rg.detail(L)


def compare_device(L, d_in_ptr, n, h, d_other_ptr, other_n, other_off=0, off=0, ln=ALL, cap=0):
    rc, m, info = _call(L.cjs_bzip2_compare_device, (d_in_ptr, n, h, d_other_ptr, other_n, other_off), off, ln, cap)
    return rc, m, info, rg.detail(L)


def streams_host(L, a, ha, b, hb, off=0, ln=ALL, cap=0):
    k1, p1, n1 = _host(a)
    k2, p2, n2 = _host(b)
    rc, m, info = _call(L.cjs_bzip2_compare_streams, (p1, n1, ha, p2, n2, hb), off, ln, cap)
    return rc, m, info, rg.detail(L)


def streams_device(L, d_a, na, ha, d_b, nb, hb, off=0, ln=ALL, cap=0):
    rc, m, info = _call(L.cjs_bzip2_compare_streams_device, (d_a, na, ha, d_b, nb, hb), off, ln, cap)
    return rc, m, info, rg.detail(L)


def on_gpu(a, shift):
    """a's bytes in GPU memory at an address that is `shift` mod 16 -> (tensor that owns them, address)"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint8)
    t = torch.zeros(a.size + 64, dtype=torch.uint8, device="cuda")
    at = (shift - t.data_ptr()) % 16
    if a.size:
        t[at:at + a.size] = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr() + at


def _two_calls(form, run, cap):
    """a count query, then a call with cap = the total (or the given cap): the same info and detail -> (diffs, info tuple, detail)"""
    rc, m, info, d = run(0)
    assert rc == 0 and m == [], (form, rc, d)
    total = info.n_diffs
    rc, m, info2, d2 = run(total if cap is None else cap)
    assert rc == 0 and info_tuple(info2) == info_tuple(info) and d2 == d, (form, rc, d, d2)
    assert len(m) == min(total, total if cap is None else cap)
    return m, info_tuple(info), d


def both_forms(L, stream, h, other, other_off=0, off=0, ln=ALL, cap=None, shift_in=3, shift_other=5):
    """The host form and the device form (the stream and the other side at the given device addresses mod 16), each as a count
    query followed by a call with cap = the total (or the given cap): both must agree in everything.  -> (diffs, info tuple,
    detail)"""
    other = np.ascontiguousarray(other, dtype=np.uint8)
    keep1, d_in = on_gpu(stream, shift_in)
    keep2, d_other = on_gpu(other, shift_other)
    res = [_two_calls("host", lambda c: compare_host(L, stream, h, other, other_off, off, ln, c), cap),
           _two_calls("device", lambda c: compare_device(L, d_in, stream.size, h, d_other, other.size, other_off, off, ln, c), cap)]
    assert res[0] == res[1], "the host form and the device form differ"
    return res[0]


def both_forms_streams(L, a, ha, b, hb, off=0, ln=ALL, cap=None, shift_a=3, shift_b=9):
    keep1, d_a = on_gpu(a, shift_a)
    keep2, d_b = on_gpu(b, shift_b)
    res = [_two_calls("host", lambda c: streams_host(L, a, ha, b, hb, off, ln, c), cap),
           _two_calls("device", lambda c: streams_device(L, d_a, a.size, ha, d_b, b.size, hb, off, ln, c), cap)]
    assert res[0] == res[1], "the host form and the device form differ"
    return res[0]


# ---- flip sets
def flipped(plain, positions, seed=1):
    """plain with the bytes at `positions` changed (XOR with a non-zero byte: every one of them differs)"""
    other = np.array(plain, dtype=np.uint8, copy=True)
    pos = np.unique(np.asarray(list(positions), dtype=np.int64))
    other[pos] ^= np.random.RandomState(seed).randint(1, 256, pos.size).astype(np.uint8)
    return other


def seam_flips(bounds, tile=16384):
    """The flip set of the alignment sweep: the first and last byte of the text, the first and last byte of every block, the bytes
    at distance tile k - 1, tile k, tile k + 1 (k = 1, 2) from every segment start (a segment of the whole-stream compare starts
    where a block starts: every block start is taken, which covers however the blocks fall into batches) and 15 consecutive bytes
    across the seam of blocks 4 and 5"""
    bounds = [int(b) for b in bounds]
    total = bounds[-1]
    pos = {0, total - 1}
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        if hi > lo:
            pos |= {lo, hi - 1}
            for k in (1, 2):
                pos |= {lo + tile * k + d for d in (-1, 0, 1) if lo + tile * k + d < total}
    pos |= set(range(bounds[5] - 7, bounds[5] + 8))
    return sorted(pos)


def random_flips(total, count, seed):
    return sorted(set(np.random.RandomState(seed).randint(0, total, count).tolist()))
