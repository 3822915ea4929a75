"""The line sort on the GPU (cjs_text_sort[_device], csrc/sort.hip; cjs_bzip2_sort[_device]) against Python's own order of the real
lines, sorted(range(L), key=lambda i: (line[i], i)) (sort_cases.sort_ref): the primitive in both forms at the line counts where a
stage can break (a flag tile of 1024, a radix tile of 4096, the sorter's extra tile per 64 Ki), on the contents that tell a round
word from a plain prefix compare, under the flags, short caps between canaries, the text byte for byte, and the stream consumer over
the fixtures of the tally and the cut."""
import ctypes
import importlib
import itertools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lines_cases as lc
import range_cases as rg
import sort_cases as sc
import tally_cases as tc

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537)


@pytest.fixture(scope="module")
def L():
    return sc.bind()


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def agree(L, torch, text, flags=0, cap=None, counts=True, want_text=True, forms=("host", "device"), shift=0, want=None):
    """both GPU forms give the restatement's entries, info and text, and write nothing else -> the restatement"""
    lines, cnts, winfo, wtext = want or sc.sort_ref(sc.split_lines(text), flags)
    m = len(lines) if cap is None else min(cap, len(lines))
    parts = sc.split_lines(text)
    head_text = b"".join(parts[i] + b"\n" for i in lines[:m]) if want_text else None
    for form in forms:
        if form == "host":
            rc, got, gc, info, gtext = sc.host_sort(L, text, flags, cap, counts, want_text)
        else:
            rc, got, gc, info, gtext, tn = sc.device_sort(L, torch, text, flags, cap, counts, want_text, shift=shift)
            assert not want_text or tn == len(head_text)
        assert rc == 0, (form, rc)
        assert sc.info_all(info) == winfo + (0, 0, sc.M64), (form, flags, sc.info_all(info), winfo)
        if got != lines[:m]:
            k = next(i for i in range(m) if got[i] != lines[i])
            raise AssertionError((form, flags, cap, "entry %d" % k, got[k], lines[k]))
        assert gc == (cnts[:m] if counts else []), (form, flags)
        assert gtext == head_text, (form, flags, "text")
    return lines, cnts, winfo, wtext


def short_lines(rng, n, longest=9, alphabet=b"ab\x00\xff"):
    lens = rng.randint(0, longest + 1, n)
    body = rng.randint(0, len(alphabet), int(lens.sum()))
    a = np.frombuffer(alphabet, np.uint8)[body]
    out, at = [], 0
    for k in lens.tolist():
        out.append(a[at:at + k].tobytes())
        at += k
    return out


@pytest.mark.parametrize("n", COUNTS)
def test_primitive_line_counts(L, torch, n):
    rng = np.random.RandomState(n % 9973 + 11)
    text = b"".join(x + b"\n" for x in short_lines(rng, n))
    agree(L, torch, text, 0)
    agree(L, torch, text[:-1] if n and text[-2:-1] != b"\n" else text, sc.REVERSE | sc.UNIQUE, forms=("device",), shift=n % 8)


def test_a_million_lines_of_0_to_3_bytes(L, torch):
    rng = np.random.RandomState(7)
    text = b"".join(x + b"\n" for x in short_lines(rng, 1048577, 3, b"abc"))
    want = agree(L, torch, text, 0, forms=("device",), want_text=False)
    assert want[2][0] == 1048577 and want[2][2] == 1 + 3 + 9 + 27
    rc, got, gc, info, _, _ = sc.device_sort(L, torch, text, sc.UNIQUE, cap=64)
    parts = sc.split_lines(text)
    firsts = [next(g) for _, g in itertools.groupby(want[0], key=lambda i: parts[i])]          # the sorted order, run by run
    assert rc == 0 and info.n_distinct == 40 and sum(gc) == 1048577 and got == firsts


def _pairs():
    out = []
    for k in (1, 2, 3):
        for share in (7 * k - 1, 7 * k, 7 * k + 1):
            stem = bytes(65 + i % 26 for i in range(share))
            out += [stem + b"y" + b"tail", stem + b"x", stem]          # two that share exactly `share` bytes, and their proper prefix
    return out


def _texts():
    rng = np.random.RandomState(3)
    word = lambda n: bytes(rng.randint(97, 123, n).astype(np.uint8))
    join = lambda lines, tail=True: b"\n".join(lines) + (b"\n" if tail else b"")
    prefix = word(4096)
    big = word(40 * 1024)
    t = {
        "lines of 6 7 8 13 14 15 bytes": join([word(n)[:n - 2] + bytes([97 + k % 2]) * 2 for k, n in enumerate((6, 7, 8, 13, 14, 15) * 40)]),
        "pairs sharing 7k-1, 7k, 7k+1 bytes": join([x for i in rng.permutation(27) for x in [_pairs()[i]]]),
        "a proper prefix before the longer line": join([b"abcdefgh", b"abcdefg", b"abcdef", b"abcdefgabcdefg", b"abcdefgabcdef", b"abcdefgabcdefgh", b"abcdefg"]),
        "padding below 0x00": join([b"ab\x01", b"ab\x00\x00", b"ab", b"ab\x00", b"ab", b"ab\x00\x00\x00\x00\x00\x00", b"ab\x00\x00\x00\x00\x00"]),
        "0xFF bytes": join([b"\xff" * n for n in (9, 7, 8, 0, 1, 14, 6, 15, 7)] + [b"\xff" * 7 + b"\x00", b"\xfe" + b"\xff" * 9]),
        "only newlines": b"\n" * 1500,
        "no newline at all": b"just one line without an end",
        "a tail without a final newline": join([b"pear", b"apple", b"fig", b"apple"], tail=False),
        "a tail with a final newline": join([b"pear", b"apple", b"fig", b"apple"]),
        "carriage returns": b"b\r\na\r\n\r\na\nb\r\n",
        "all lines equal": join([b"the same line of more than seven bytes"] * 3000),
        "all distinct behind a 4 KiB prefix": join([prefix + bytes([33 + i]) for i in rng.permutation(40)]),
        "one group of 5000 across a radix tile border": join([b"%05d" % i for i in range(4000)] + [b"30005" + b"=" * 11] * 5000 + [b"%05d" % i for i in range(4000, 4200)]),
        "an active set that shrinks to one pair": join([b"shared-stem-" + word(3) for _ in range(300)] + [b"shared-stem-" + b"q" * 90 + b"1", b"shared-stem-" + b"q" * 90 + b"0"]),
    }
    t["two equal 40 KiB lines among short ones"] = join([word(5) for _ in range(50)] + [big] + [word(9) for _ in range(50)] + [big, b"zz"])
    return t


TEXTS = _texts()


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_primitive_contents(L, torch, name):
    text = TEXTS[name]
    long = name.startswith("two equal 40 KiB")
    for flags in ((0,) if long else (0, sc.REVERSE, sc.UNIQUE, sc.REVERSE | sc.UNIQUE)):
        want = agree(L, torch, text, flags, counts=bool(flags & sc.UNIQUE) or flags == 0, forms=("device",) if long else ("host", "device"), shift=3 if flags else 0)
    lines = sc.split_lines(text)
    if name.startswith("all distinct behind"):
        assert want[2][4] == 586 == (max(map(len, lines)) + 8) // 7
    if long:
        assert want[2][4] == 1 + 40 * 1024 // 7 and want[2][2] == len(lines) - 1
    if name == "all lines equal":
        assert want[2][2] == 1 and want[2][4] == 1 + len(lines[0]) // 7
    if name == "padding below 0x00":
        assert [lines[i] for i in sc.sort_ref(lines, sc.UNIQUE)[0]] == [b"ab", b"ab\x00", b"ab\x00\x00", b"ab" + b"\x00" * 5, b"ab" + b"\x00" * 6, b"ab\x01"]


def test_250000_empty_lines_and_a_long_one_in_one_gather(L, torch):
    text = b"\n" * 125000 + bytes(97 + i % 26 for i in range(40 * 1024)) + b"\n" + b"\n" * 125000
    want = agree(L, torch, text, sc.REVERSE, forms=("device",), counts=False)
    assert want[2][:3] == (250001, 250001, 2) and want[0][0] == 125000


def test_caps_between_canaries(L, torch):
    rng = np.random.RandomState(5)
    text = b"\n".join(short_lines(rng, 3000, 12)) + b"\ntail"
    for flags in (0, sc.REVERSE | sc.UNIQUE):
        want = sc.sort_ref(sc.split_lines(text), flags)
        n_out = want[2][1]
        for cap in (0, 1, n_out - 1, n_out, n_out + 5):
            agree(L, torch, text, flags, cap=cap, counts=bool(cap & 1), want=want)
    # without text, and the count query
    rc, got, gc, info, gtext = sc.host_sort(L, text, sc.UNIQUE, cap=0, counts=False, want_text=False)
    assert rc == 0 and got == [] and gtext is None and sc.info5(info) == sc.sort_ref(sc.split_lines(text), sc.UNIQUE)[2]


def test_a_text_cap_one_short_is_refused_with_the_need(L, torch):
    text = b"pear\napple\n\nfig\napple"
    want = sc.sort_ref(sc.split_lines(text))
    for cap, need in ((None, len(want[3])), (2, len(b"\napple\n"))):
        rc, got, gc, info, gtext, tn = sc.device_sort(L, torch, text, cap=cap, want_text=True, text_cap=need - 1)
        assert rc == sc.E_TOO_SMALL and tn == need and got == want[0][:cap] and sc.info5(info) == want[2]          # (device_sort has checked the canaries)
        rc, got, gc, info, gtext, tn = sc.device_sort(L, torch, text, cap=cap, want_text=True, text_cap=0)                            # the size query
        assert rc == sc.E_TOO_SMALL and tn == need
        rc, got, gc, info, gtext, tn = sc.device_sort(L, torch, text, cap=cap, want_text=True, text_cap=need)
        assert rc == 0 and tn == need and gtext == want[3][:need]


@pytest.mark.parametrize("shift", range(8))
def test_the_text_at_every_alignment_ending_its_tensor(L, torch, shift):
    rng = np.random.RandomState(40 + shift)
    for n in (1, 5, 15, 16, 17, 4090 + shift, 3 * 4096):
        lines = short_lines(rng, n, 20, b"abc")
        text = b"\n".join(lines)            # (no final newline: the last line's word ends on the text's last byte)
        agree(L, torch, text, 0, forms=("device",), shift=shift)


def test_host_pointers_are_refused_by_the_device_form(L, torch):
    text = np.frombuffer(b"b\na\n", dtype=np.uint8)
    d = torch.from_numpy(text.copy()).cuda()
    d_lines = torch.zeros(4, dtype=torch.int64, device="cuda")
    host_lines = np.zeros(4, np.uint64)
    info = sc.SortInfo()
    tn = rg.S(0)
    assert L.cjs_text_sort_device(text.ctypes.data, 4, 0, d_lines.data_ptr(), None, 4, None, 0, None, ctypes.byref(info), None) == sc.E_INVALID
    assert L.cjs_text_sort_device(d.data_ptr(), 4, 0, host_lines.ctypes.data, None, 4, None, 0, None, ctypes.byref(info), None) == sc.E_INVALID
    assert L.cjs_text_sort_device(d.data_ptr(), 4, 0, d_lines.data_ptr(), host_lines.ctypes.data, 4, None, 0, None, ctypes.byref(info), None) == sc.E_INVALID
    assert L.cjs_text_sort_device(d.data_ptr(), 4, 0, d_lines.data_ptr(), None, 4, host_lines.ctypes.data, 32, ctypes.byref(tn), ctypes.byref(info), None) == sc.E_INVALID
    assert L.cjs_text_sort_device(d.data_ptr(), 4, 0, d_lines.data_ptr(), None, 4, None, 0, None, ctypes.byref(info), None) == 0
    assert d_lines.cpu().numpy().tolist()[:2] == [1, 0]


def test_the_python_front_of_the_primitive(torch):
    pkg = importlib.import_module("compressjs-flattened_amd")
    text = TEXTS["pairs sharing 7k-1, 7k, 7k+1 bytes"] + b"AAAAAA\nAAAAAA"
    lines = sc.split_lines(text)
    for reverse in (False, True):
        for unique in (False, True):
            want = sc.sort_ref(lines, (sc.REVERSE if reverse else 0) | (sc.UNIQUE if unique else 0))
            assert pkg.sort_text(text, reverse, unique) == (want[0], want[1])
            for limit in (None, 4, 0):
                res = pkg.text_sort(text, reverse=reverse, unique=unique, limit=limit, want_text=True)
                assert (res.n_lines, res.n_out, res.n_distinct, res.text_bytes, res.rounds) == want[2]
                assert res.lines.tolist() == want[0][:limit] and res.counts.tolist() == want[1][:limit]
                assert res.text == b"".join(lines[i] + b"\n" for i in want[0][:limit])
    d = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    d_lines = torch.zeros(len(lines), dtype=torch.int64, device="cuda")
    d_out = torch.zeros(len(text) + 1, dtype=torch.uint8, device="cuda")
    res = pkg.text_sort_device(d.data_ptr(), len(text), d_lines_out_ptr=d_lines.data_ptr(), cap=len(lines), d_text_out_ptr=d_out.data_ptr(), text_cap=len(text) + 1)
    want = sc.sort_ref(lines)
    assert d_lines.cpu().numpy().tolist() == want[0] and d_out.cpu().numpy()[:res.text_n].tobytes() == want[3] and res.rounds == want[2][4]


# ---------------------------------------------------------------- the stream consumer (cjs_bzip2_sort[_device])
STREAMS = ("TL1", "CT2", "CT3")
CUTS = ((sc.FIELDS, 9, [(2, 2)]), (sc.BYTES, 0, [(1, 8)]))


@pytest.fixture(scope="module")
def fx(L, oracle):
    return {name: tc.stream_fixture(L, name, oracle) for name in STREAMS}


def window_ref(f, first, count, cut, flags):
    items = tc.window_lines(f["plain"], first, count) if cut is None else tc.cut_window_lines(f["plain"], *cut, first=first, count=count)
    return items, sc.sort_ref(items, flags, base=first)


def stream_agree(L, f, first=0, count=None, cut=None, flags=0, cap=None, counts=True, want_text=True, forms=("host", "device")):
    items, (lines, cnts, winfo, wtext) = window_ref(f, first, count, cut, flags)
    m = len(lines) if cap is None else min(cap, len(lines))
    head_text = b"".join(items[i - first] + b"\n" for i in lines[:m])
    mode, d, sel = (sc.LINES, 0, ()) if cut is None else cut
    for form in forms:
        rc, got, gc, info, gtext, tn, det = sc.stream_sort(L, f, form, first, sc.M64 if count is None else count, mode, d, sel, flags, cap, counts, want_text)
        assert rc == 0, (form, rc, det)
        assert sc.info5(info) == winfo and (info.n_bad_blocks, info.first_bad_block) == (0, sc.M64), (form, sc.info_all(info), winfo)
        assert got == lines[:m] and gc == (cnts[:m] if counts else []), (form, flags, first, count)
        if want_text:
            assert gtext == head_text and tn == len(head_text), (form, "text")
    return lines, cnts, winfo, items


def _windows(f):
    N = int(f["nl"].size)
    if f["name"] == "TL1":
        twin = min(k for k, _ in tc.tl1_planted(f["plain"], f["bounds"])["seam"])
        return [(0, None), (twin, 1), (N + 1, None), (twin + 1, None)]
    return [(0, None), (N // 3, N // 2)]


@pytest.mark.parametrize("name", STREAMS)
def test_stream_sort_against_the_lines(L, fx, name):
    f = fx[name]
    few = name == "CT2"          # (639 blocks a call)
    for first, count in _windows(f):
        stream_agree(L, f, first, count)
        if few and first:
            continue
        for cut in CUTS:          # (CT2: fields in the host form, bytes in the device form)
            stream_agree(L, f, first, count, cut=cut, flags=sc.UNIQUE if cut[0] == sc.BYTES else 0,
                         forms=(("host",) if cut[0] == sc.FIELDS else ("device",)) if few else ("host", "device"))
    if name == "CT3":
        rc, got, gc, info, gtext, tn, det = sc.stream_sort(L, f, "host", want_text=True)
        assert rc == 0 and sc.info_all(info) == (0, 0, 0, 0, 0, 0, 0, sc.M64) and gtext == b""


def test_stream_flags_limits_and_text(L, fx):
    f = fx["TL1"]
    N = int(f["nl"].size)
    lines, cnts, winfo, items = stream_agree(L, f, flags=sc.UNIQUE)
    p = tc.tl1_planted(f["plain"], f["bounds"])
    by_line = dict(zip(lines, cnts))
    assert by_line[min(k for k, _, _ in p["big"])] == 2 and by_line[p["empty"][0]] == len(p["empty"]) and by_line[p["tail_twins"][0]] == len(p["tail_twins"]) + 1
    assert winfo[4] == 1 + tc.TL1_BIG // 7          # the 40 KiB twins take the rounds of their length
    stream_agree(L, f, flags=sc.REVERSE, cap=10)
    stream_agree(L, f, flags=sc.REVERSE | sc.UNIQUE, cap=7, counts=False)
    stream_agree(L, f, 5, 1000, cap=0, want_text=False)
    stream_agree(L, f, N - 50, None, cut=CUTS[0], flags=sc.REVERSE, cap=20)
    # a device text cap one short: the cut's code, the need, nothing written
    items, want = window_ref(f, 0, 100, None, 0)
    rc, got, gc, info, gtext, tn, det = sc.stream_sort(L, f, "device", 0, 100, want_text=True, text_cap=len(want[3]) - 1)
    assert rc == sc.E_TOO_SMALL and tn == len(want[3]) and got == want[0]


def test_the_python_front_of_the_stream_sort(fx):
    pkg = importlib.import_module("compressjs-flattened_amd")
    f = fx["TL1"]
    ix = pkg.Bzip2Index.build(f["stream"])
    ln = pkg.Bzip2Lines.build(f["stream"], ix)
    items, want = window_ref(f, 0, None, None, sc.UNIQUE)
    res = ix.sort_lines(f["stream"], ln, unique=True, limit=12, want_text=True)
    dev = pkg.sort_lines_device(f["dev"][1], f["stream"].size, ix, ln, unique=True, limit=12)
    for r in (res, dev):
        assert (r.n_lines, r.n_out, r.n_distinct, r.text_bytes, r.rounds) == want[2]
        assert r.lines.tolist() == want[0][:12] and r.counts.tolist() == want[1][:12]
    head = b"".join(items[i] + b"\n" for i in want[0][:12])
    assert res.text == head and dev.text_n is None
    with pytest.raises(pkg.CjsError) as q:          # want_text without a buffer: the size query
        pkg.sort_lines_device(f["dev"][1], f["stream"].size, ix, ln, unique=True, limit=12, want_text=True)
    assert q.value.errorCode == sc.E_TOO_SMALL and q.value.need == len(head)
    # the sorted lines read back through read_lines: `sort | head`
    assert b"".join(ix.read_lines(f["stream"], ln, [(int(k), 1) for k in res.lines])) == head
    items, want = window_ref(f, 100, 2000, CUTS[0], sc.REVERSE)
    res = ix.sort_lines(f["stream"], ln, fields="2", first=100, count=2000, reverse=True, want_text=True)
    assert res.lines.tolist() == want[0] and res.text == want[3]
    import torch
    d_out = torch.zeros(64 * 1024, dtype=torch.uint8, device="cuda")
    dev = pkg.sort_lines_device(f["dev"][1], f["stream"].size, ix, ln, bytes="1-8", first=100, count=2000, d_text_out_ptr=d_out.data_ptr(), text_cap=d_out.numel())
    items, want = window_ref(f, 100, 2000, CUTS[1], 0)
    assert dev.lines.tolist() == want[0] and d_out.cpu().numpy()[:dev.text_n].tobytes() == want[3]
    with pytest.raises(pkg.CjsError) as e:
        pkg.sort_lines_device(f["dev"][1], f["stream"].size, ix, ln, first=100, count=2000, d_text_out_ptr=d_out.data_ptr(), text_cap=16)
    assert e.value.errorCode == sc.E_TOO_SMALL and e.value.need == len(window_ref(f, 100, 2000, None, 0)[1][3])


def test_a_damaged_block_fails_the_sort_as_it_fails_the_cut(L, fx):
    import cut_cases as ct
    Lc = ct.bind()                                          # (the same library, with the cut's argument types)
    f = fx["TL1"]
    e = f["entries"]
    blk = 1
    damaged = f["stream"].copy()
    bit = e[blk][0] + 48 + 32 + 1 + 23          # the lowest bit of the block's BWT start
    damaged[bit >> 3] ^= 1 << (7 - (bit & 7))
    dev = lc.on_device(damaged)
    for mode, d, sel in ((sc.BYTES, 0, [(1, ct.TO_END)]),) + CUTS:
        rc_c, _, cinfo, cdet = ct.cut_host(Lc, damaged, f["h"], f["t"], mode, d, sel)
        assert rc_c == rg.E_DATA and cdet
        for form in ("host", "device"):
            whole = mode == sc.BYTES and sel[0][1] == ct.TO_END
            rc, got, gc, info, gtext, tn, det = sc.stream_sort(L, f, form, mode=sc.LINES if whole else mode, d=d, sel=() if whole else sel, cap=8, want_text=True,
                                                               stream=damaged, dev=dev)
            assert rc == rc_c and det == cdet and got == [] and gtext is None, (rc, det, cdet)
            assert (info.n_bad_blocks, info.first_bad_block, info.blocks_decoded) == (cinfo.n_bad_blocks, cinfo.first_bad_block, cinfo.blocks_decoded) == (1, blk, 4)
    # a window in front of the block is served
    rc, got, gc, info, gtext, tn, det = sc.stream_sort(L, f, "host", 0, 50, stream=damaged, dev=dev)
    assert rc == 0 and got == window_ref(f, 0, 50, None, 0)[1][0]


def test_a_foreign_table_and_windows_above_the_limits_are_refused(L, fx):
    f, other = fx["TL1"], fx["CT2"]
    a, N = f["stream"], int(f["nl"].size)
    for form in ("host", "device"):
        rc, got, gc, info, gtext, tn, det = sc.stream_sort(L, f, form, cap=4, t=other["t"])
        assert rc == sc.E_INVALID and det == lc.FOREIGN

    def limited(form, first, count, max_bytes, max_lines, flags=0):
        info = sc.SortInfo()
        out = np.zeros(4, np.uint64)
        src = (a.ctypes.data, None) if form == "host" else (None, f["dev"][1])
        rc = L.cjs_stage_bzip2_sort_limit(src[0], src[1], a.size, f["h"], f["t"], first, count, max_bytes, max_lines, flags, out.ctypes.data, None, 4, ctypes.byref(info), None)
        return rc, info, out.tolist()
    big = 2 ** 40
    for form in ("host", "device"):
        assert limited(form, 0, sc.M64, big, 100)[0] == sc.E_UNSUPPORTED
        assert limited(form, N - 200, 101, big, 100)[0] == sc.E_UNSUPPORTED
        assert limited(form, N - 200, 100, 100, big)[0] == sc.E_UNSUPPORTED          # the touched blocks' bytes are above 100
        rc, info, out = limited(form, N - 200, 100, big, 100)
        assert rc == 0 and info.n_lines == 100 and out == window_ref(f, N - 200, 100, None, 0)[1][0][:4]
        rc, info, out = limited(form, 0, sc.M64, big, big, sc.REVERSE)          # (never above the sort's own limits)
        want = window_ref(f, 0, None, None, sc.REVERSE)[1]
        assert rc == 0 and sc.info5(info) == want[2] and out == want[0][:4]


def child(first, count, limit):
    """(the child of the test below) a window of TL1 sorted with a limit and no text under CJS_DEBUG: the [cjs sort] lines go to stderr"""
    os.environ["CJS_DEBUG"] = "1"
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy is loaded before the library)
    import support
    L = sc.bind()
    f = tc.stream_fixture(L, "TL1", support.Oracle())
    out = {}
    for form in ("host", "device"):
        rc, got, gc, info, gtext, tn, det = sc.stream_sort(L, f, form, first, count, cap=limit, want_text=False)
        assert rc == 0
        out[form] = [got, gc, list(sc.info5(info))]
    print(json.dumps(out))


SORT_LINE = r"\[cjs sort\] (host|device): lines \[(\d+), (\d+)\), .* (\d+) lines, (\d+) distinct, (\d+) out, (\d+) rounds, upload (\d+), beyond the cut: H2D (\d+) D2H (\d+)"


def test_only_the_answer_leaves_the_gpu(fx):
    """TL1, limit=10, no text: beyond the cut less than 1 KiB comes down.  The window is the 1000 lines behind the first 40 KiB line
    and in front of its twin: a round costs 8 bytes, and two equal lines of 40 KiB take 5852 of them (the worst case DESIGN states)."""
    f = fx["TL1"]
    first, count = 15, 1000
    big = [k for k, _, _ in tc.tl1_planted(f["plain"], f["bounds"])["big"]]
    assert min(big) < first and max(big) >= first + count
    penv = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", "import test_gpu_sort as t; t.child(%d, %d, 10)" % (first, count)], capture_output=True,
                         text=True, env=penv, cwd=os.path.dirname(os.path.abspath(__file__)))
    assert run.returncode == 0, run.stderr[-3000:]
    got = json.loads(run.stdout.strip().splitlines()[-1])
    want = window_ref(f, first, count, None, 0)[1]
    lines = [(m[0],) + tuple(int(x) for x in m[1:]) for m in re.findall(SORT_LINE, run.stderr)]
    assert [x[0] for x in lines] == ["host", "device"], run.stderr[-2000:]
    for form, a, b, n_lines, nd, n_out, rounds, up, h2d, d2h in lines:
        assert got[form] == [want[0][:10], want[1][:10], list(want[2])]
        assert (a, b, n_lines, nd, n_out, rounds) == (first, first + count, want[2][0], want[2][2], want[2][1], want[2][4])
        assert h2d == 0 and d2h == 16 + 16 + 8 * rounds + 16 + 2 * 8 * 10, (form, d2h)          # two scalars twice, one a round, two more, ten entries with counts
        assert d2h < 1024
