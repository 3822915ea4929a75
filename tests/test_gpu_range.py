"""Indexed range reads on the GPU (cjs_bzip2_index_build, cjs_bzip2_read_ranges[_device], Bzip2Index): the index against the
oracle's table and the stream's own bits; several hundred ranges per fixture in one host call and one device call, every offset,
length, status and byte against plain[off:off + len]; that nothing outside the touched blocks is read; a verdict per block;
several passes; the Python front.  The streams are made on the CPU (tests/range_cases.py)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import range_cases as rg

pytestmark = pytest.mark.gpu

MAGIC_BLOCK, MAGIC_END = 0x314159265359, 0x177245385090


@pytest.fixture(scope="module")
def L():
    return rg.bind()


@pytest.fixture(scope="module")
def fx(L, oracle):
    """per fixture: stream, plain, multistream flag, members, the index built on the GPU and its entries"""
    out = {}
    for name in ("F1", "F2", "F3"):
        stream, plain, multi, members = rg.fixture(name, oracle)
        rc, h = rg.build(L, stream, multi)
        assert rc == 0, (name, rc, rg.detail(L))
        out[name] = dict(stream=stream, plain=plain, multi=multi, members=members, h=h, entries=rg.entries(L, h))
    return out


def _check(res, ranges, plain, name):
    buf, off, ln, st, d = res
    want = rg.expected(plain, ranges)
    at = 0
    for k, w in enumerate(want):
        assert st[k] == 0 and off[k] == at and ln[k] == len(w), (name, k, ranges[k], int(st[k]), int(off[k]), int(ln[k]))
        assert bytes(buf[at:at + len(w)]) == w, (name, k, ranges[k])
        at += len(w)
    assert d == "" and len(buf) == at


@pytest.mark.parametrize("name", ["F1", "F2", "F3"])
def test_index_build_matches_the_oracle_and_the_stream(L, oracle, fx, name):
    f = fx[name]
    stream, e = f["stream"], f["entries"]
    rc, tab = oracle.bzip2_table(stream, f["multi"])
    assert rc == 0 and [(x[0], x[2]) for x in e] == tab and len(e) >= 3
    assert rg.info(L, f["h"]) == (len(e), f["plain"].size, stream.size, f["multi"])
    starts = [m[0] for m in f["members"]]
    for k, (bitpos, end_bit, size, crc, level, reserved) in enumerate(e):
        assert rg.bits(stream, bitpos, 48) == MAGIC_BLOCK and crc == rg.bits(stream, bitpos + 48, 32) and reserved == 0
        assert (k + 1 < len(e) and end_bit == e[k + 1][0]) or rg.bits(stream, end_bit, 48) == MAGIC_END, k
        member = max(i for i in range(len(starts)) if starts[i] * 8 <= bitpos)
        assert level == f["members"][member][1] == stream[starts[member] + 3] - 48, k
    if name == "F2":
        assert len(set(x[4] for x in e)) == 9


def test_build_on_a_damaged_stream_fails_like_table(L, fx):
    f = fx["F1"]
    for what in ("bit", "header", "cut"):
        bad = f["stream"].copy()
        if what == "bit":
            bad[(f["entries"][5][0] + f["entries"][5][1]) // 16] ^= 0x10
        elif what == "header":
            bad[3] = ord("0")
        else:
            bad = bad[:200000]
        pos, size = np.zeros(64, np.uint64), np.zeros(64, np.uint32)
        want = L.cjs_bzip2_table(bad.ctypes.data_as(rg.u8p), bad.size, 0, pos.ctypes.data_as(rg.PU), size.ctypes.data_as(rg.ctypes.POINTER(rg.ctypes.c_uint32)), 64, None)
        want_detail = rg.detail(L)
        rc, h = rg.build(L, bad, 0)
        assert want < 0 and rc == want and not h and rg.detail(L) == want_detail, what


@pytest.mark.parametrize("name", ["F1", "F2", "F3"])
def test_ranges_host_and_device(L, fx, name):
    f = fx[name]
    ranges = rg.range_list([x[2] for x in f["entries"]])
    assert len(ranges) >= 200
    host, dev = rg.both_forms(L, f["stream"], f["h"], ranges)
    _check(host, ranges, f["plain"], name + " host")
    _check(dev, ranges, f["plain"], name + " device")


def test_a_block_equals_decompress_block_and_the_dumps(L, fx):
    f = fx["F1"]
    e, stream = f["entries"], f["stream"]
    off = np.concatenate([[0], np.cumsum([x[2] for x in e])])
    for bitpos in (32, 1596228, 2342106):
        b = [x[0] for x in e].index(bitpos)
        rc, buf, o, ln, st, d = rg.read_host(L, stream, f["h"], [(int(off[b]), e[b][2])])
        out, n = rg.u8p(), rg.S(0)
        assert L.cjs_bzip2_decompress_block(stream.ctypes.data_as(rg.u8p), stream.size, bitpos, rg.ctypes.byref(out), rg.ctypes.byref(n), None) == 0
        blk = rg.ctypes.string_at(out, n.value)
        L.cjs_free(out)
        assert rc == 0 and st[0] == 0 and buf == blk == rg.golden("sample4.%d" % bitpos).tobytes()


def _runs(entries, blocks):
    return [(entries[b][0] >> 3, (entries[b][1] + 7) >> 3) for b in blocks]


def test_untouched_bytes_are_not_read(L, fx):
    """everything outside the byte runs of blocks 3 and 7 is overwritten -- header, trailer, the neighbours' magics -- and the
    ranges inside those blocks come back all the same, from both forms"""
    f = fx["F1"]
    e = f["entries"]
    off = np.concatenate([[0], np.cumsum([x[2] for x in e])])
    ranges = [(int(off[3]), e[3][2]), (int(off[7]) + 11, 5000), (int(off[8]) - 4097, 4097), (int(off[3]) + 77777, 1), (int(off[7]), e[7][2])]
    keep = np.zeros(f["stream"].size, bool)
    for lo, hi in _runs(e, (3, 7)):
        keep[lo:hi] = True
    noise = np.random.RandomState(9).randint(0, 256, f["stream"].size).astype(np.uint8)
    wrecked = np.where(keep, f["stream"], noise)
    assert not keep[:4].any() and not keep[-10:].any() and (wrecked[:4] != f["stream"][:4]).any()
    host, dev = rg.both_forms(L, wrecked, f["h"], ranges)
    _check(host, ranges, f["plain"], "wrecked host")
    _check(dev, ranges, f["plain"], "wrecked device")


def _fails(res, ranges, plain, bad, detail_re, dev):
    """ranges with an index in `bad` fail, the others deliver their bytes; host form: a failed range takes no room"""
    import re
    buf, off, ln, st, d = res
    want = rg.expected(plain, ranges)
    at = 0
    for k, w in enumerate(want):
        if k in bad:
            assert st[k] == rg.E_DATA and ln[k] == 0 and off[k] == at, (k, ranges[k])
            at += len(w) if dev else 0
            continue
        assert st[k] == 0 and off[k] == at and ln[k] == len(w) and bytes(buf[at:at + len(w)]) == w, (k, ranges[k])
        at += len(w)
    assert re.fullmatch(detail_re, d), d


def _touching(ranges, off, block, total):
    return {k for k, (a, n) in enumerate(ranges) if n and a < total and a < off[block + 1] and min(a + n, total) > off[block]}


def test_a_flipped_bit_fails_only_the_ranges_that_touch_the_block(L, fx):
    f = fx["F1"]
    e, plain = f["entries"], f["plain"]
    off = np.concatenate([[0], np.cumsum([x[2] for x in e])])
    ranges = [(10, 100), (int(off[4]) + 5, 99981 - 5), (int(off[6]) - 1, 2), (int(off[5]), 1), (int(off[4]) + 99000, 2000), (int(off[6]), 50), (0, plain.size),
              (int(off[5]) + 500, 0), (int(off[9]), 10 ** 6)]
    bad = _touching(ranges, off, 5, plain.size)
    assert bad == {2, 3, 4, 6}
    damaged = f["stream"].copy()
    damaged[(e[5][0] + e[5][1]) // 16] ^= 0x04
    # the contract's two details: only the CRC differs, or the block no longer agrees with its entry (another end, another size)
    detail = r"Bad block CRC \(got [0-9a-f]+ expected %x\)|index does not match the stream at block 5" % e[5][3]
    host, dev = rg.both_forms(L, damaged, f["h"], ranges)
    _fails(host, ranges, plain, bad, detail, False)
    _fails(dev, ranges, plain, bad, detail, True)
    assert host[4] == dev[4]
    # the detail is the lowest failing range's: block 2 damaged as well, first met by range 6 (block 5: range 2)
    damaged[(e[2][0] + e[2][1]) // 16] ^= 0x04
    host, dev = rg.both_forms(L, damaged, f["h"], ranges)
    _fails(host, ranges, plain, bad, detail, False)
    _fails(dev, ranges, plain, bad, detail, True)
    order = [ranges[6], ranges[2]]                          # the whole-stream range first: its first bad block is 2
    detail2 = r"Bad block CRC \(got [0-9a-f]+ expected %x\)|index does not match the stream at block 2" % e[2][3]
    host, dev = rg.both_forms(L, damaged, f["h"], order)
    _fails(host, order, plain, {0, 1}, detail2, False)
    _fails(dev, order, plain, {0, 1}, detail2, True)


def test_a_wrong_stored_crc_gives_the_bad_crc_detail(L, fx):
    """The one damage that is certain to leave the decode intact: the 32 stored CRC bits behind a block's magic are overwritten
    and the index is made with the same value, so the block agrees with its entry in everything and only the computed CRC
    differs -- `Bad block CRC (got <computed> expected <stored>)`, with the block's own numbers."""
    f = fx["F1"]
    e, plain = [list(x) for x in f["entries"]], f["plain"]
    off = np.concatenate([[0], np.cumsum([x[2] for x in e])])
    real = {b: e[b][3] for b in (2, 5)}
    stream = f["stream"].copy()
    for b, mask in ((5, 0x00010000), (2, 0x80000001)):
        e[b][3] = real[b] ^ mask
        rg.set_bits(stream, e[b][0] + 48, 32, e[b][3])
        assert rg.bits(stream, e[b][0] + 48, 32) == e[b][3] and rg.bits(stream, e[b][0], 48) == MAGIC_BLOCK
    rc, h = rg.create(L, [tuple(x) for x in e], stream.size, 0)
    assert rc == 0, rg.detail(L)
    # range 1 is the lowest failing one and its first bad block is 5; block 2 fails ranges 3 and 4 only
    ranges = [(10, 100), (int(off[4]) + 5, int(off[6] - off[4])), (int(off[6]), 50), (0, plain.size), (int(off[2]) + 9, 1), (int(off[5]), 1)]
    bad = _touching(ranges, off, 5, plain.size) | _touching(ranges, off, 2, plain.size)
    assert bad == {1, 3, 4, 5}
    host, dev = rg.both_forms(L, stream, h, ranges)
    for res, is_dev in ((host, False), (dev, True)):
        _fails(res, ranges, plain, bad, r".*", is_dev)
        assert res[4] == "Bad block CRC (got %x expected %x)" % (real[5], e[5][3])
    order = [ranges[3], ranges[1]]                          # the whole-stream range first: its first bad block is 2
    host, dev = rg.both_forms(L, stream, h, order)
    for res, is_dev in ((host, False), (dev, True)):
        _fails(res, order, plain, {0, 1}, r".*", is_dev)
        assert res[4] == "Bad block CRC (got %x expected %x)" % (real[2], e[2][3])
    L.cjs_bzip2_index_destroy(h)


@pytest.mark.parametrize("field", ["size", "end_bit", "crc", "bitpos"])
def test_an_altered_entry_fails_only_the_ranges_that_touch_it(L, fx, field):
    f = fx["F1"]
    e, plain = [list(x) for x in f["entries"]], f["plain"]
    off = np.concatenate([[0], np.cumsum([x[2] for x in e])])
    k = 4
    if field == "size":
        e[k][2] -= 1                                        # (the offsets behind it move by one: the expected bytes follow the index)
    elif field == "end_bit":
        e[k][1] -= 1
    elif field == "crc":
        e[k][3] ^= 1
    else:
        e[k][0] += 1
    rc, h = rg.create(L, [tuple(x) for x in e], f["stream"].size, 0)
    assert rc == 0, rg.detail(L)
    ioff = np.concatenate([[0], np.cumsum([x[2] for x in e])])
    total = int(ioff[-1])
    ranges = [(int(ioff[3]), 100), (int(ioff[4]), 1), (int(ioff[5]) - 1, 1), (int(ioff[5]), 7), (int(ioff[3]) + 99000, 1000), (0, total), (int(ioff[9]) + 3, 99)]
    bad = _touching(ranges, ioff, k, total)
    assert bad == {1, 2, 4, 5}
    shift = int(off[-1]) - total                            # blocks behind k sit one byte further in the real plaintext
    want_plain = plain if not shift else np.concatenate([plain[:int(ioff[k + 1])], plain[int(ioff[k + 1]) + shift:]])
    host, dev = rg.both_forms(L, f["stream"], h, ranges)
    _fails(host, ranges, want_plain, bad, "index does not match the stream at block 4", False)
    _fails(dev, ranges, want_plain, bad, "index does not match the stream at block 4", True)
    L.cjs_bzip2_index_destroy(h)


def test_the_index_of_another_stream_fails_every_range(L, oracle, fx):
    f = fx["F1"]
    rc, other = oracle.bzip2_compress(f["plain"][:600000][::-1].copy(), 1)
    assert rc == 0 and other.size < f["stream"].size
    padded = np.concatenate([other, np.zeros(f["stream"].size - other.size, np.uint8)])      # (bytes behind the end of a single stream are ignored)
    rc, h = rg.build(L, padded, 0)
    assert rc == 0 and rg.info(L, h)[2] == f["stream"].size
    ranges = [(0, 10), (250000, 4096), (5, 0), (599990, 100), (600000, 1)]
    host, dev = rg.both_forms(L, f["stream"], h, ranges)
    for buf, off, ln, st, d in (host, dev):
        assert st.tolist() == [rg.E_DATA, rg.E_DATA, 0, rg.E_DATA, 0] and ln.tolist() == [0] * 5
        assert d == "index does not match the stream at block 0"
    L.cjs_bzip2_index_destroy(h)


def _digest(res):
    buf, off, ln, st, d = res
    return [hashlib.sha256(bytes(buf)).hexdigest(), [int(x) for x in off], [int(x) for x in ln], [int(x) for x in st], d]


def child_passes():
    """(the child of test_several_passes) F1 and F2 under CJS_RANGE_PASS_BLOCKS = 1 and 3: the digests of both forms"""
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy is loaded before the library)
    import support
    L, oracle, out = rg.bind(), support.Oracle(), {}
    for name in ("F1", "F2"):
        stream, plain, multi, members = rg.fixture(name, oracle)
        rc, h = rg.build(L, stream, multi)
        assert rc == 0
        ranges = rg.range_list([x[2] for x in rg.entries(L, h)])
        for cap in ("1", "3"):
            os.environ["CJS_RANGE_PASS_BLOCKS"] = cap       # (read at every call)
            host, dev = rg.both_forms(L, stream, h, ranges)
            out[name + "/" + cap] = [_digest(host), _digest(dev)]
    print(json.dumps(out))


def test_several_passes_give_the_single_pass_result(L, fx):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    code = "import test_gpu_range as t; t.child_passes()"
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", code], capture_output=True, text=True, env=env,
                         cwd=os.path.dirname(os.path.abspath(__file__)))
    assert run.returncode == 0, run.stderr[-3000:]
    got = json.loads(run.stdout.strip().splitlines()[-1])
    for name in ("F1", "F2"):
        f = fx[name]
        ranges = rg.range_list([x[2] for x in f["entries"]])
        host, dev = rg.both_forms(L, f["stream"], f["h"], ranges)
        _check(host, ranges, f["plain"], name)
        for cap in ("1", "3"):
            assert got[name + "/" + cap] == [_digest(host), _digest(dev)], (name, cap)


def _flipped_bit_case(f):
    """F1 with a bit of block 5 flipped (test_a_flipped_bit...): -> (stream, ranges)"""
    e = f["entries"]
    off = np.concatenate([[0], np.cumsum([x[2] for x in e])])
    ranges = [(10, 100), (int(off[4]) + 5, 99981 - 5), (int(off[6]) - 1, 2), (int(off[5]), 1), (int(off[4]) + 99000, 2000), (int(off[6]), 50), (0, f["plain"].size),
              (int(off[5]) + 500, 0), (int(off[9]), 10 ** 6)]
    damaged = f["stream"].copy()
    damaged[(e[5][0] + e[5][1]) // 16] ^= 0x04
    return damaged, ranges


def _wrong_crc_case(L, f):
    """F1 with the stored CRC of block 5 overwritten in the stream and in the index (test_a_wrong_stored_crc...):
    -> (stream, handle, ranges, the detail)"""
    e = [list(x) for x in f["entries"]]
    off = np.concatenate([[0], np.cumsum([x[2] for x in e])])
    real = e[5][3]
    e[5][3] = real ^ 0x00010000
    stream = f["stream"].copy()
    rg.set_bits(stream, e[5][0] + 48, 32, e[5][3])
    rc, h = rg.create(L, [tuple(x) for x in e], stream.size, 0)
    assert rc == 0, rg.detail(L)
    ranges = [(10, 100), (int(off[4]) + 5, int(off[6] - off[4])), (int(off[6]), 50), (0, f["plain"].size), (int(off[2]) + 9, 1), (int(off[5]), 1)]
    return stream, h, ranges, "Bad block CRC (got %x expected %x)" % (real, e[5][3])


def _batch_runs(L, name, f):
    """The calls of test_several_batches on fixture `name`: the full range list; F1: block 5 -- the second block of the third
    inverse-BWT batch when a batch holds two -- with a flipped bit and with a wrong stored CRC.  -> case -> [host, device]"""
    ranges = rg.range_list([x[2] for x in f["entries"]])
    res = {"all": rg.both_forms(L, f["stream"], f["h"], ranges)}
    if name == "F1":
        damaged, ranges = _flipped_bit_case(f)
        res["bit"] = rg.both_forms(L, damaged, f["h"], ranges)
        stream, h, ranges, detail = _wrong_crc_case(L, f)
        res["crc"] = rg.both_forms(L, stream, h, ranges)
        L.cjs_bzip2_index_destroy(h)
        assert res["crc"][0][4] == res["crc"][1][4] == detail
    return res


def child_batches(name, elems):
    """(the child of test_several_batches) fixture `name` with at most `elems` BWT bytes to an inverse-BWT batch: the digests of
    _batch_runs; the [cjs range] lines go to stderr"""
    os.environ["CJS_DEC_BATCH_ELEMS"] = elems               # (read once, at the first batch of the process)
    os.environ["CJS_DEBUG"] = "1"
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy is loaded before the library)
    import support
    L, oracle = rg.bind(), support.Oracle()
    stream, plain, multi, members = rg.fixture(name, oracle)
    rc, h = rg.build(L, stream, multi)
    assert rc == 0
    f = dict(stream=stream, plain=plain, h=h, entries=rg.entries(L, h))
    print(json.dumps({k: [_digest(v[0]), _digest(v[1])] for k, v in _batch_runs(L, name, f).items()}))


@pytest.mark.parametrize("name,elems", [("F1", "250000"), ("F2", "1000")])
def test_several_batches_in_a_pass_give_the_same(L, fx, name, elems):
    """Several inverse-BWT batches inside one pass (CJS_DEC_BATCH_ELEMS shrunk; F1: 10 blocks of <= 100,000 BWT bytes, two to a
    batch): bytes, offsets, statuses and detail of both forms as in this process, also with a bad block in a later batch."""
    import re
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    code = "import test_gpu_range as t; t.child_batches(%r, %r)" % (name, elems)
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", code], capture_output=True, text=True, env=env,
                         cwd=os.path.dirname(os.path.abspath(__file__)))
    assert run.returncode == 0, run.stderr[-3000:]
    got = json.loads(run.stdout.strip().splitlines()[-1])
    f = fx[name]
    here = _batch_runs(L, name, f)
    _check(here["all"][0], rg.range_list([x[2] for x in f["entries"]]), f["plain"], name)
    assert sorted(got) == sorted(here)
    for case, (host, dev) in here.items():
        assert got[case] == [_digest(host), _digest(dev)], (name, case)
    if name == "F1":                                        # not vacuous: the full list went through >= 4 batches in one pass, in both forms
        nranges = len(rg.range_list([x[2] for x in f["entries"]]))
        lines = re.findall(r"\[cjs range\] (host|device): (\d+) ranges, .*? (\d+) passes \((\d+) row batches, (\d+) inverse-BWT batches\)", run.stderr)
        full = [(form, int(p), int(b)) for form, n, p, a, b in lines if int(n) == nranges]
        assert sorted(x[0] for x in full) == ["device", "host"], lines
        for form, passes, batches in full:
            assert passes == 1 and batches >= 4, (form, passes, batches)
        assert len(lines) == 6 and all(int(b) > int(p) for form, n, p, a, b in lines), lines


def test_python_front(fx):
    import importlib
    import torch
    pkg = importlib.import_module("compressjs-flattened_amd")
    f = fx["F1"]
    stream, plain = f["stream"], f["plain"]
    ix = pkg.Bzip2Index.build(stream)
    assert ix.blocks == 10 and ix.total == plain.size and ix.entries() == [x[:5] for x in f["entries"]]
    assert pkg.Bzip2Index.load(ix.save()).entries() == ix.entries()
    assert ix.read(stream, 99975, 20) == plain[99975:99995].tobytes() and ix.read(stream, plain.size - 3, 100) == plain[-3:].tobytes()
    ranges = [(5, 10), (plain.size, 4), (300000, 70000), (5, 10)]
    assert ix.read_ranges(stream, ranges) == rg.expected(plain, ranges)
    d_in = torch.from_numpy(stream).cuda()
    d_out = torch.zeros(70020, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                # (the caller has finished writing both buffers: the memory rules of the device forms)
    off, ln, st, d = pkg.read_ranges_device(d_in.data_ptr(), stream.size, ix, ranges, d_out.data_ptr(), d_out.numel())
    assert off.tolist() == [0, 10, 10, 70010] and ln.tolist() == [10, 0, 70000, 10] and not st.any() and d == ""
    assert d_out.cpu().numpy().tobytes() == b"".join(rg.expected(plain, ranges))
    with pytest.raises(pkg.CjsError) as err:
        pkg.read_ranges_device(d_in.data_ptr(), stream.size, ix, ranges, None, 0)
    assert err.value.errorCode == rg.E_TOO_SMALL and err.value.need == 70020
    damaged = stream.copy()
    damaged[(f["entries"][5][0] + f["entries"][5][1]) // 16] ^= 0x04
    res = ix.read_ranges(damaged, [(0, 5), (550000, 5), (560000, 5)])
    assert res[0] == plain[:5].tobytes() and isinstance(res[1], pkg.CjsError) and isinstance(res[2], pkg.CjsError) and res[1].errorCode == rg.E_DATA
    assert "block" in str(res[1]).lower() and ":" not in str(res[2]).split("(code")[0]
    with pytest.raises(pkg.CjsError):
        ix.read(damaged, 550000, 5)
