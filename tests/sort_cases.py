"""Shared pieces of the sort tests (test_sort_host.py, test_gpu_sort.py, test_gpu_sort_js.py): the ctypes binding of
cjs_text_sort[_device] / cjs_stage_text_sort / cjs_bzip2_sort[_device] / cjs_stage_bzip2_sort_limit, the restatement of the order
(Python's own sorted() over the real lines, ties by line number), the round count by the rule, and the calls between canaries."""
import ctypes

import numpy as np

import range_cases as rg
import tally_cases as tc

U32, U64 = ctypes.c_uint32, ctypes.c_uint64
REVERSE, UNIQUE = 1, 2
LINES, FIELDS, BYTES = 2, 0, 1          # CJS_SORT_LINES beside CJS_CUT_FIELDS and CJS_CUT_BYTES
E_INVALID, E_UNSUPPORTED, E_TOO_SMALL = -32, -34, -33
M64 = 2 ** 64 - 1
CANARY = 0xA5
CANARY64 = int.from_bytes(bytes([CANARY]) * 8, "little")
MAX = 2 ** 32 - 2
RANGE = np.dtype([("lo", "<u4"), ("hi", "<u4")])


class SortInfo(ctypes.Structure):
    _fields_ = [("n_lines", U64), ("n_out", U64), ("n_distinct", U64), ("text_bytes", U64), ("rounds", U64), ("blocks_decoded", U64),
                ("n_bad_blocks", U64), ("first_bad_block", U64)]


def bind():
    L = tc.bind()
    V, S, PS = rg.V, rg.S, rg.PS
    PI, PP = ctypes.POINTER(SortInfo), ctypes.POINTER(rg.u8p)
    L.cjs_text_sort.argtypes = [V, S, U32, V, V, S, PP, PS, PI, V]
    L.cjs_text_sort_device.argtypes = [V, S, U32, V, V, S, V, S, PS, PI, V]
    L.cjs_stage_text_sort.argtypes = [V, S, U32, V, V, S, PI]
    head = [V, V, U64, U64, U32, U32, V, U32, U32, V, V, S]
    L.cjs_bzip2_sort.argtypes = [rg.u8p, S] + head + [PP, PS, PI, V]
    L.cjs_bzip2_sort_device.argtypes = [V, S] + head + [V, S, PS, PI, V]
    L.cjs_stage_bzip2_sort_limit.argtypes = [V, V, S, V, V, U64, U64, U64, U64, U32, V, V, S, PI, V]
    L.cjs_free.argtypes = [V]
    L.cjs_free.restype = None
    return L


def info5(i):
    return (i.n_lines, i.n_out, i.n_distinct, i.text_bytes, i.rounds)


def info_all(i):
    return info5(i) + (i.blocks_decoded, i.n_bad_blocks, i.first_bad_block)


# ---- the restatement
def split_lines(text):
    """the lines of a text: the bytes between newlines; a tail that is not empty is a line, an empty tail is none"""
    parts = bytes(text).split(b"\n")
    if parts[-1] == b"":
        parts.pop()
    return parts


def _common(a, b):
    n = min(len(a), len(b))
    if a[:n] == b[:n]:
        return n
    lo, hi = 0, n                          # a[:lo] == b[:lo], a[:hi] != b[:hi]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if a[:mid] == b[:mid]:
            lo = mid
        else:
            hi = mid
    return lo


def rounds_by_the_rule(parts, order):
    """a group stays active behind round r iff two of its lines share their first 7 (r + 1) bytes: 1 + the largest
    floor(common prefix / 7) over neighbours of the sorted order; no lines, no round"""
    if not parts:
        return 0
    return 1 + max([_common(parts[a], parts[b]) // 7 for a, b in zip(order[:-1], order[1:])] + [0])


def sort_ref(lines, flags=0, base=0):
    """`lines`: the real lines (bytes objects) -> (line numbers, counts, (n_lines, n_out, n_distinct, text_bytes, rounds), text)
    of all n_out entries.  The order is sorted(range(L), key=lambda i: (line[i], i)), reversed run by run under REVERSE."""
    order = sorted(range(len(lines)), key=lambda i: (lines[i], i))
    runs = []
    for i in order:
        if runs and lines[runs[-1][0]] == lines[i]:
            runs[-1].append(i)
        else:
            runs.append([i])
    n_distinct = len(runs)
    if flags & REVERSE:
        runs = runs[::-1]
    if flags & UNIQUE:
        out, counts = [r[0] for r in runs], [len(r) for r in runs]
    else:
        out = [i for r in runs for i in r]
        counts = [1] * len(out)
    text = b"".join(lines[i] + b"\n" for i in out)
    return [base + i for i in out], counts, (len(lines), len(out), n_distinct, len(text), rounds_by_the_rule(lines, order)), text


# ---- the calls
def _guarded(cap):
    buf = np.full(cap + 2, CANARY64, np.uint64)
    return buf, buf.ctypes.data + 8


def _unguard(buf, written):
    assert buf[0] == CANARY64 and (buf[1 + written:] == CANARY64).all(), "the call wrote outside what it may write"
    return buf[1:1 + written].tolist()


def stage_sort(L, text, flags=0, cap=None, counts=True):
    """cjs_stage_text_sort -> (rc, lines, counts, info)"""
    raw = np.frombuffer(bytes(text), dtype=np.uint8)
    cap = raw.size if cap is None else cap
    (lb, lp), (cb, cp) = _guarded(cap), _guarded(cap)
    info = SortInfo(*([7] * 8))
    rc = L.cjs_stage_text_sort(raw.ctypes.data if raw.size else None, raw.size, flags, lp if cap else None, cp if cap and counts else None, cap, ctypes.byref(info))
    m = min(cap, info.n_out) if rc == 0 else 0
    return rc, _unguard(lb, m), _unguard(cb, m if counts else 0), info


def host_sort(L, text, flags=0, cap=None, counts=True, want_text=False):
    """cjs_text_sort -> (rc, lines, counts, info, text or None)"""
    raw = np.frombuffer(bytes(text), dtype=np.uint8)
    cap = raw.size if cap is None else cap
    (lb, lp), (cb, cp) = _guarded(cap), _guarded(cap)
    info = SortInfo(*([7] * 8))
    out, out_n = rg.u8p(), rg.S(0)
    tp = (ctypes.byref(out), ctypes.byref(out_n)) if want_text else (None, None)
    rc = L.cjs_text_sort(raw.ctypes.data if raw.size else None, raw.size, flags, lp if cap else None, cp if cap and counts else None, cap, *tp, ctypes.byref(info), None)
    m = min(cap, info.n_out) if rc == 0 else 0
    got = None
    if want_text and rc == 0:
        got = ctypes.string_at(out, out_n.value)
        L.cjs_free(out)
    return rc, _unguard(lb, m), _unguard(cb, m if counts else 0), info, got


def device_sort(L, torch, text, flags=0, cap=None, counts=True, want_text=False, text_cap=None, shift=0):
    """cjs_text_sort_device: the text at a device address = shift mod 8 in a tensor that ends with it (the allocator may
    round the tensor up, so a read past the text would not fault: that none happens rests on the kernels' code), the outputs in device memory
    between canaries -> (rc, lines, counts, info, text or None, text_n)"""
    raw = np.frombuffer(bytes(text), dtype=np.uint8)
    cap = raw.size if cap is None else cap
    d_text = torch.zeros(shift + raw.size, dtype=torch.uint8, device="cuda") if shift + raw.size else None
    if raw.size:
        d_text[shift:] = torch.from_numpy(raw.copy()).cuda()
        assert d_text.data_ptr() % 8 == 0
    d_lines = torch.from_numpy(np.full(cap + 2, CANARY64, np.uint64).view(np.int64)).cuda()
    d_counts = torch.from_numpy(np.full(cap + 2, CANARY64, np.uint64).view(np.int64)).cuda()
    text_cap = (raw.size + 1 if text_cap is None else text_cap) if want_text else 0
    d_out = torch.full((text_cap + 2 * 64,), CANARY, dtype=torch.uint8, device="cuda")
    info = SortInfo(*([7] * 8))
    tn = rg.S(0)
    rc = L.cjs_text_sort_device(d_text.data_ptr() + shift if raw.size else None, raw.size, flags, d_lines.data_ptr() + 8 if cap else None,
                                d_counts.data_ptr() + 8 if cap and counts else None, cap, d_out.data_ptr() + 64 if want_text and text_cap else None, text_cap,
                                ctypes.byref(tn) if want_text else None, ctypes.byref(info), None)
    torch.cuda.synchronize()
    m = min(cap, info.n_out) if rc in (0, E_TOO_SMALL) else 0
    lines = _unguard(d_lines.cpu().numpy().view(np.uint64), m)
    cnts = _unguard(d_counts.cpu().numpy().view(np.uint64), m if counts else 0)
    o = d_out.cpu().numpy()
    written = tn.value if rc == 0 and want_text else 0
    assert (o[:64] == CANARY).all() and (o[64 + written:] == CANARY).all(), "the call wrote text outside what it may write"
    return rc, lines, cnts, info, (o[64:64 + written].tobytes() if want_text and rc == 0 else None), tn.value


def sel_array(sel):
    r = np.zeros(max(len(sel), 1), dtype=RANGE)
    for k, x in enumerate(sel):
        r[k] = x
    return r


def stream_sort(L, f, form, first=0, count=M64, mode=LINES, d=0, sel=(), flags=0, cap=None, counts=True, want_text=False, text_cap=None, stream=None, dev=None, t=None):
    """cjs_bzip2_sort (form "host") or cjs_bzip2_sort_device over the fixture f -> (rc, lines, counts, info, text or None, text_n, detail);
    cap=None: room for every line of the table"""
    import torch
    a = np.ascontiguousarray(f["stream"] if stream is None else stream, dtype=np.uint8)
    cap = int(f["nl"].size) + 1 if cap is None else cap
    (lb, lp), (cb, cp) = _guarded(cap), _guarded(cap)
    r = sel_array(sel)
    info = SortInfo(*([7] * 8))
    head = [f["h"], f["t"] if t is None else t, first, count, mode, d, r.ctypes.data if len(sel) else None, len(sel), flags, lp if cap else None,
            cp if cap and counts else None, cap]
    tn = rg.S(0)
    got = None
    if form == "host":
        out = rg.u8p()
        tp = (ctypes.byref(out), ctypes.byref(tn)) if want_text else (None, None)
        rc = L.cjs_bzip2_sort(a.ctypes.data_as(rg.u8p), a.size, *head, *tp, ctypes.byref(info), None)
        det = rg.detail(L)
        if want_text and rc == 0:
            got = ctypes.string_at(out, tn.value)
            L.cjs_free(out)
    else:
        text_cap = (int(f["total"]) + 1 if text_cap is None else text_cap) if want_text else 0
        d_out = torch.full((text_cap + 128,), CANARY, dtype=torch.uint8, device="cuda")
        rc = L.cjs_bzip2_sort_device((f["dev"] if dev is None else dev)[1], a.size, *head, d_out.data_ptr() + 64 if want_text and text_cap else None, text_cap,
                                     ctypes.byref(tn) if want_text else None, ctypes.byref(info), None)
        det = rg.detail(L)
        torch.cuda.synchronize()
        o = d_out.cpu().numpy()
        written = tn.value if rc == 0 and want_text else 0
        assert (o[:64] == CANARY).all() and (o[64 + written:] == CANARY).all(), "the call wrote text outside what it may write"
        if want_text and rc == 0:
            got = o[64:64 + written].tobytes()
    m = min(cap, info.n_out) if rc in (0, E_TOO_SMALL) else 0
    return rc, _unguard(lb, m), _unguard(cb, m if counts else 0), info, got, tn.value, det
