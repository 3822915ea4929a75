"""Shared pieces of the cut tests (test_cut_host.py, test_gpu_cut.py, test_gpu_cut_js.py): the ctypes binding of cjs_bzip2_cut[_device]
/ cjs_stage_cut / cjs_cut_list_parse, output arrays between canaries on the host and on the device, a cut LIST parsed in Python,
and the restatement cut_ref: split at the newlines, split at the delimiter or index, join, the tail rule."""
import ctypes

import numpy as np

import lines_cases as lc
import range_cases as rg

U32, U64 = ctypes.c_uint32, ctypes.c_uint64
M64 = 2 ** 64 - 1
TO_END = 0xFFFFFFFF
FIELDS, BYTES = 0, 1
RANGE = np.dtype([("lo", "<u4"), ("hi", "<u4")])
MISMATCH = "line table does not match the stream at block %d"
CANARY = 0xA5
GUARD = 64


class CutInfo(ctypes.Structure):
    _fields_ = [("n_lines", U64), ("out_bytes", U64), ("blocks_decoded", U64), ("n_bad_blocks", U64), ("first_bad_block", U64)]


def bind():
    L = lc.bind()
    V, S = rg.V, rg.S
    L.cjs_bzip2_cut.argtypes = [rg.u8p, S, V, V, U64, U64, U32, U32, V, U32, ctypes.POINTER(rg.u8p), rg.PS, ctypes.POINTER(CutInfo), V]
    L.cjs_bzip2_cut_device.argtypes = [V, S, V, V, U64, U64, U32, U32, V, U32, V, S, rg.PS, ctypes.POINTER(CutInfo), V]
    L.cjs_stage_cut.argtypes = [V, S, U32, U32, V, U32, V, S, rg.PS]
    L.cjs_cut_list_parse.argtypes = [ctypes.c_char_p, V, U32, ctypes.POINTER(U32)]
    return L


# ---- the selection
def ref_list(spec):
    """a cut LIST ("1,3-5,7-", "-4") -> [(lo, hi)], parsed here in Python; hi = TO_END: to the end of the line"""
    out = []
    for item in spec.split(","):
        a, dash, b = item.partition("-")
        lo = int(a) if a else 1
        hi = (int(b) if b else TO_END) if dash else lo
        out.append((lo, hi))
    return out


def normal(sel):
    """sorted, overlapping and touching ranges merged"""
    out = []
    for lo, hi in sorted(sel):
        if out and lo <= out[-1][1] + 1:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def sel_array(sel):
    a = np.zeros(max(len(sel), 1), dtype=RANGE)
    for k, r in enumerate(sel):
        a[k] = r
    return a


def parse(L, spec, cap=64):
    """cjs_cut_list_parse -> (rc, [(lo, hi)]); the array lies between canaries"""
    buf = np.full((cap + 2 * GUARD) * 8, CANARY, np.uint8)
    n = U32(77)
    rc = L.cjs_cut_list_parse(spec.encode() if isinstance(spec, str) else spec, buf.ctypes.data + 8 * GUARD if cap else None, cap, ctypes.byref(n))
    got = n.value if rc == 0 else 0
    assert (buf[:8 * GUARD] == CANARY).all() and (buf[8 * (GUARD + cap):] == CANARY).all(), "the parser wrote outside its array"
    r = buf[8 * GUARD:8 * (GUARD + got)].view(RANGE)
    return rc, [(int(x["lo"]), int(x["hi"])) for x in r]


# ---- the restatement
def _member(sel, upto):
    """m[k] = unit k is selected, k = 0 .. upto (m[0] is False)"""
    m = np.zeros(upto + 2, dtype=bool)
    for lo, hi in sel:
        m[lo:min(hi, upto) + 1] = True
    m[0] = False
    return m


def cut_ref(text, mode, d, sel, first=0, count=None):
    """What the cut of lines [first, first + count) of `text` is: split(b"\\n"), split(d) / index, join, the tail rule."""
    lines = bytes(text).split(b"\n")                    # lines 0 .. N; the last is the unterminated tail
    N = len(lines) - 1
    end = N + 1 if count is None else min(first + count, N + 1)
    delim = bytes([d])
    out = []
    m = _member(sel, max(len(x) for x in lines) + 1)      # (a line of n bytes has at most n + 1 fields)
    for k in range(first, end):
        ln = lines[k]
        if k == N and not ln:
            break                                       # an empty tail line writes nothing
        if mode == FIELDS:
            out.append(delim.join(f for j, f in enumerate(ln.split(delim), 1) if m[j]))
        else:
            out.append(np.frombuffer(ln, dtype=np.uint8)[m[1:len(ln) + 1]].tobytes())
    return b"".join(x + b"\n" for x in out)


# ---- fixtures (streams from the CPU oracle; every property they are for is asserted by test_gpu_cut's first test)
TILE = 16384
CT1_SEED = 2718
CT1_LONG = 2 * TILE + 700                                  # bytes of the long line's middle, without a delimiter


def _ct1_plain(patch):
    rng = np.random.RandomState(CT1_SEED)
    word = lambda: bytes(rng.randint(97, 123, int(rng.randint(1, 9)) if rng.randint(0, 8) else 0).astype(np.uint8))      # one in eight is an empty field
    lines, size = [], 0
    while size < 300 * 1024:
        k = int(rng.randint(0, 13))                         # 0 fields: an empty line
        lines.append(b"\t".join(word() for _ in range(k)))
        size += len(lines[-1]) + 1
        if len(lines) == 50:
            lines.append(b"\t\t\t\t\t")                     # delimiters only
            lines.append(b"\t".join(b"f%d" % j for j in range(1, 301)))
            ends = [b"\t".join(word() or b"x" for _ in range(14))[:100] for _ in range(2)]
            lines.append(ends[0] + bytes(rng.randint(97, 123, CT1_LONG).astype(np.uint8)) + ends[1])
            size += sum(len(x) + 1 for x in lines[-3:])
    plain = np.frombuffer(b"\n".join(lines) + b"\ntail\tof\tit", dtype=np.uint8).copy()
    for p in patch:
        plain[p] = 9
    return plain


def ct1(oracle):
    """about 300 KiB of tab-separated text at level 1 -> (stream, plain, multistream): a delimiter is put on the last byte of one
    tile and on the first byte of another once the block bounds are known (they must not move)"""
    def pack(plain):
        rc, s = oracle.bzip2_compress(plain, 1)
        assert rc == 0
        s = np.asarray(s, dtype=np.uint8)
        return s, lc.oracle_bounds(oracle, s, 0)
    _, first = pack(_ct1_plain([]))
    assert len(first) >= 4
    patch = [int(first[1]) + 2 * TILE - 1, int(first[2]) + 3 * TILE]
    plain = _ct1_plain(patch)
    stream, bounds = pack(plain)
    assert bounds.tolist() == first.tolist(), "the bounds moved: another seed"
    return stream, plain, 0


CT2_SEED = 99
CT2_MEMBERS = 640


def ct2(oracle):
    """640 multistream members of 1..40 bytes over {a, b, c, tab, 0x00, newline}, levels cycling: a block and a tile each -> (stream,
    plain, multistream).  Members 100..111 hold no newline and no delimiter (a line over whole blocks), member 300 is empty, the
    stream ends in a newline."""
    rng = np.random.RandomState(CT2_SEED)
    alphabet = np.array([97, 98, 99, 97, 9, 9, 0, 10], np.uint8)
    parts, plain = [], []
    for k in range(CT2_MEMBERS):
        p = alphabet[rng.randint(0, alphabet.size, int(rng.randint(1, 41)))]
        if 100 <= k < 112:
            p = np.where((p == 10) | (p == 9) | (p == 0), 98, p).astype(np.uint8)
        if k == 300:
            p = p[:0]
        if k == CT2_MEMBERS - 1:
            p[-1] = 10
        rc, s = oracle.bzip2_compress(p, 1 + k % 9)
        assert rc == 0
        parts.append(np.asarray(s, dtype=np.uint8)); plain.append(p)
    return np.concatenate(parts), np.concatenate(plain), 1


def ct3(oracle):
    """a stream without a block"""
    rc, s = oracle.bzip2_compress(np.zeros(0, np.uint8), 9)
    assert rc == 0
    return np.asarray(s, dtype=np.uint8), np.zeros(0, np.uint8), 0


def tile_starts(bounds):
    """the decoded offset of the first byte of every tile: tiles are counted from their block's first byte"""
    return np.array([int(a) for B0, B1 in zip(bounds[:-1], bounds[1:]) for a in range(int(B0), int(B1), TILE)], dtype=np.int64)


def lines_across(plain, at):
    """the numbers of the lines that have a byte on both sides of a seam in front of a byte of `at` (a newline belongs to its line)"""
    nl, total = lc.newlines(plain), int(plain.size)
    starts = np.concatenate([[0], nl + 1]).astype(np.int64)          # start(k), k = 0 .. N
    ends = np.concatenate([nl + 1, [total]]).astype(np.int64)         # start(k + 1)
    at = np.asarray([a for a in at if 0 < a < total], dtype=np.int64)
    k = np.searchsorted(starts, at, "right") - 1
    return sorted(set(k[(starts[k] < at) & (at < ends[k])].tolist()))


def properties(plain, bounds, d=9):
    """what a fixture holds, from its own bytes and block bounds"""
    tiles = tile_starts(bounds)
    inner = np.array([a for a in tiles if a not in set(int(b) for b in bounds)], dtype=np.int64)      # seams between two tiles of one block
    lines = bytes(plain).split(b"\n")
    fields = [ln.count(bytes([d])) + 1 if ln else 0 for ln in lines[:-1]]
    return dict(
        blocks=sum(1 for a, b in zip(bounds[:-1], bounds[1:]) if b > a), tiles=int(tiles.size),
        fields=(min(fields), max(f for f in fields if f <= 12), max(fields)) if fields else (0, 0, 0),
        empty_fields=sum(1 for ln in lines if bytes([d, d]) in ln), empty_lines=sum(1 for ln in lines[:-1] if not ln),
        delimiters_only=sum(1 for ln in lines if ln and not ln.strip(bytes([d]))), longest=max(len(ln) for ln in lines), tail=len(lines[-1]),
        across_16=len(lines_across(plain, [a + 16 * j for a in tiles for j in range(1, 4)])),
        across_64=len(lines_across(plain, tiles + 64)), across_80=len(lines_across(plain, tiles + 80)),
        across_tile=len(lines_across(plain, inner)), across_block=len(lines_across(plain, bounds[1:-1])),
        delimiter_last_of_tile=int(sum(1 for a in inner if plain[a - 1] == d)), delimiter_first_of_tile=int(sum(1 for a in inner if plain[a] == d)))


def fixture(L, name, oracle):
    stream, plain, multi = {"CT1": ct1, "CT2": ct2, "CT3": ct3}[name](oracle)
    rc, h = rg.build(L, stream, multi)
    assert rc == 0, (name, rc, rg.detail(L))
    e = rg.entries(L, h)
    bounds = np.concatenate([[0], np.cumsum([x[2] for x in e])]).astype(np.int64)
    f = dict(name=name, stream=stream, plain=plain, text=plain.tobytes(), h=h, entries=e, bounds=bounds, nl=lc.newlines(plain), total=int(plain.size),
             multi=multi)
    f["dev"] = lc.on_device(stream)
    f["t"] = lc.build_both(L, stream, h, f["dev"])
    return f


# ---- the calls
def stage_cut(L, text, mode, d, sel, cap=None):
    """cjs_stage_cut -> (rc, the bytes written, out_n); cap=None: room for everything"""
    a = np.frombuffer(bytes(text), dtype=np.uint8)
    keep = a if a.size else np.zeros(1, np.uint8)
    if cap is None:
        cap = a.size + 1
    r = sel_array(sel)
    buf = np.full(cap + 2 * GUARD, CANARY, np.uint8)
    n = rg.S(0)
    rc = L.cjs_stage_cut(keep.ctypes.data, a.size, mode, d, r.ctypes.data if len(sel) else None, len(sel), buf.ctypes.data + GUARD if cap else None, cap,
                         ctypes.byref(n))
    assert (buf[:GUARD] == CANARY).all() and (buf[GUARD + cap:] == CANARY).all(), "the call wrote outside out[0 .. cap)"
    wrote = min(cap, n.value) if rc in (0, rg.E_TOO_SMALL) else 0
    assert (buf[GUARD + wrote:] == CANARY).all()
    return rc, buf[GUARD:GUARD + wrote].tobytes(), n.value


def info_tuple(info):
    return (info.n_lines, info.out_bytes, info.blocks_decoded, info.n_bad_blocks, info.first_bad_block)


def cut_host(L, stream, h, t, mode, d, sel, first=0, count=M64):
    """cjs_bzip2_cut -> (rc, bytes or None, info, detail)"""
    a = np.ascontiguousarray(stream, dtype=np.uint8)
    keep = a if a.size else np.zeros(1, np.uint8)
    r = sel_array(sel)
    out, n = rg.u8p(), rg.S(7)
    info = CutInfo(7, 7, 7, 7, 7)
    rc = L.cjs_bzip2_cut(keep.ctypes.data_as(rg.u8p), a.size, h, t, first, count, mode, d, r.ctypes.data, len(sel), ctypes.byref(out), ctypes.byref(n),
                         ctypes.byref(info), None)
    det = rg.detail(L)
    if rc:
        assert not out, "a failed call returned a buffer"
        return rc, None, info, det
    assert out, "a buffer is returned even for empty output"
    got = ctypes.string_at(out, n.value)
    L.cjs_free(out)
    return rc, got, info, det


def cut_device(L, d_in_ptr, n, h, t, mode, d, sel, first=0, count=M64, out_cap=None, shift=0):
    """cjs_bzip2_cut_device -> (rc, the bytes below min(out_cap, need), need, info, detail).  out_cap=None: the size query (d_out NULL),
    then exactly that much.  d_out stands `shift` bytes behind a 256-byte boundary between canaries that must come back unchanged."""
    import torch
    r = sel_array(sel)
    need = rg.S(7)
    info = CutInfo(7, 7, 7, 7, 7)
    call = lambda ptr, cap: L.cjs_bzip2_cut_device(d_in_ptr, n, h, t, first, count, mode, d, r.ctypes.data, len(sel), ptr, cap, ctypes.byref(need),
                                                  ctypes.byref(info), None)
    if out_cap is None:
        rc = call(None, 0)
        if rc not in (0, rg.E_TOO_SMALL):
            return rc, None, need.value, info, rg.detail(L)
        assert (rc == 0) == (need.value == 0), "the size query: too small exactly when there is output"
        out_cap = need.value
    buf = torch.full((out_cap + 2 * 256 + 16,), CANARY, dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 256 + 256 + shift
    torch.cuda.synchronize()
    rc = call(buf.data_ptr() + at if out_cap else None, out_cap)
    det = rg.detail(L)
    torch.cuda.synchronize()
    back = buf.cpu().numpy()
    assert (back[:at] == CANARY).all() and (back[at + out_cap:] == CANARY).all(), "the call wrote outside d_out[0 .. out_cap)"
    if rc not in (0, rg.E_TOO_SMALL):
        return rc, None, need.value, info, det
    return rc, back[at:at + min(out_cap, need.value)].tobytes(), need.value, info, det


def both_forms(L, stream, h, t, dev, mode, d, sel, **kw):
    """The host form and the device form (the stream at an odd device address): both must agree in everything.
    -> (bytes, info as a tuple)"""
    rc, got, info, det = cut_host(L, stream, h, t, mode, d, sel, **kw)
    assert rc == 0, (rc, det)
    rc2, got2, need, info2, det2 = cut_device(L, dev[1], np.asarray(stream).size, h, t, mode, d, sel, **kw)
    assert rc2 == 0, (rc2, det2)
    assert got == got2 and need == len(got) and info_tuple(info) == info_tuple(info2) and det == det2 == "", "the host form and the device form differ"
    assert info.out_bytes == len(got)
    return got, info_tuple(info)
