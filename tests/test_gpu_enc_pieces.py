"""The compress pipeline in pieces (csrc/pipeline.hip, blocks_through_tables): from 400 MB of blocks on a call cuts its blocks into
four runs and overlaps the suffix sort of one with MTF / RLE2 and the Huffman tables of the one before.  CJS_ENC_PIECE_BYTES=1
takes every entry point down that path at a few hundred kilobytes: 1..13 blocks, every one of another kind than its neighbours
(enc_pieces_cases.py), in pieces of (1) .. (4,4,4,1).  Every call runs with the variable set and unset; both must give the
oracle's bits.  One child process under CJS_DEBUG shows from the library's "[cjs pieces]" lines that the calls did go in the pieces
the rule (csrc/enc_pieces.h) gives, and in one piece without the variable."""
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import enc_pieces_cases as ec

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_refs = {}


def _pkg():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("compressjs-flattened_amd")


@pytest.fixture(scope="module")
def pkg():
    return _pkg()


def ref(oracle, name):
    """per input, made once and never changed: the input, its level, the oracle's stream and block count"""
    if name not in _refs:
        data, level = ec.data(name), ec.level(name)
        rc, stream = oracle.bzip2_compress(data, level)
        assert rc == 0
        rc, _, _, total, _ = oracle.bzip2_compress_range(data, level, 0, 0)
        assert rc == 0
        _refs[name] = dict(data=data, level=level, stream=stream, nb=int(total))
    return _refs[name]


# ---------------------------------------------------------------------------------------------------- the inputs, on the CPU
def test_enc_pieces_cases_are_what_they_say(oracle):
    """no GPU: every input has the block count it is named after, its blocks begin where its stretches do, and neighbouring blocks
    differ in alphabet size (so does every block from the one a piece further on that could be read in its place)"""
    for name in ec.ALL:
        data, level = ec.data(name), ec.level(name)
        rc, _, bits, total, crcs = oracle.bzip2_compress_range(data, level, 0, 0)
        assert rc == 0 and bits == 0 and total == ec.NBLOCKS[name] and crcs.size == total, name
        blocks = oracle.rle1_blocks(data, level)
        assert len(blocks) == total, name
        assert [b[2] for b in blocks] + [blocks[-1][3]] == ec.stretch_bounds(name), name
        asz = [int(np.unique(b[0]).size) for b in blocks]
        assert all(a != b for a, b in zip(asz, asz[1:])), (name, asz)
        cap = level * 100000 - 19
        assert all(b[0].size == cap for b in blocks[:-1]), name
    # the last blocks the issue names: one byte, exactly cap bytes, something between
    last = {name: int(oracle.rle1_blocks(ec.data(name), ec.level(name))[-1][0].size) for name in ec.LEVEL1}
    assert last["b3"] == 1 and last["b7"] == 1 and last["b2"] == last["b4"] == last["b9"] == ec.CAP1 and 1 < last["b13"] < ec.CAP1
    assert sorted(ec.NBLOCKS[n] for n in ec.LEVEL1) == [1, 2, 3, 4, 5, 7, 9, 10, 13] and ec.NBLOCKS["l9b5"] == 5
    # the rule restated here gives the piece lists the issue names
    want = {1: [1], 2: [1, 1], 3: [1, 1, 1], 4: [1, 1, 1, 1], 5: [2, 2, 1], 6: [2, 2, 2], 7: [2, 2, 2, 1], 8: [2, 2, 2, 2], 9: [3, 3, 3],
            10: [3, 3, 3, 1], 13: [4, 4, 4, 1]}
    for cnt, sizes in want.items():
        assert ec.piece_sizes(cnt, True) == sizes and ec.piece_sizes(cnt, False) == [cnt]


# ---------------------------------------------------------------------------------------------------- helpers of the GPU tests
class Dev:
    """an input on the device, a context for it and an output buffer pre-filled with 0xA5"""

    def __init__(self, pkg, R, max_range_blocks=0, out_cap=None):
        import torch
        self.torch, self.R = torch, R
        self.n = int(R["data"].size)
        self.d_in = torch.from_numpy(np.array(R["data"])).to("cuda:0")
        self.cap = out_cap if out_cap is not None else (self.n + self.n // 4 + 4096) & ~3
        self.ctx = pkg.DeviceContext(0, self.n, R["level"], max_range_blocks)
        self.fresh()

    def fresh(self):
        self.d_out = self.torch.full((self.cap + 64,), 0xA5, dtype=self.torch.uint8, device="cuda:0")

    def out(self):
        return self.d_out.cpu().numpy()

    def close(self):
        self.ctx.close()


ZEROED = 16


def _stream_and_rest(back, n, want, what):
    """the n bytes at the front of `back` are the stream `want`; the packer zeroes up to ZEROED bytes behind a stream (it stores
    whole words and ORs boundary words: csrc/huff_rules.h, stream_zeroed_bytes), behind those every byte is still 0xA5"""
    assert n == want.size and np.array_equal(back[:n], want), what
    assert (back[n + ZEROED:] == 0xA5).all() and not (back[n: n + ZEROED] & ~np.uint8(0xA5)).any(), what


def _bits_equal(got, want, bits):
    """the first `bits` bits of two byte arrays"""
    full = bits // 8
    if not np.array_equal(got[:full], want[:full]):
        return False
    if bits % 8:
        mask = (0xFF00 >> (bits % 8)) & 0xFF
        return (int(got[full]) & mask) == (int(want[full]) & mask)
    return True


# ---------------------------------------------------------------------------------------------------- a. DeviceContext.compress
@gpu
@pytest.mark.parametrize("name", ec.ALL)
def test_compress_over_every_input(pkg, oracle, name):
    R = ref(oracle, name)
    D = Dev(pkg, R)
    try:
        for on in (True, False):
            pieces = len(ec.piece_sizes(R["nb"], on))
            with ec.knob(on):
                # no stats
                D.fresh()
                n = D.ctx.compress(D.d_in.data_ptr(), D.n, D.d_out.data_ptr(), D.cap)
                _stream_and_rest(D.out(), n, R["stream"], (name, on, "no stats"))
                # stats, events only: the path of bench.py's timed loop, in pieces under the knob
                D.fresh()
                D.ctx.set_stage_times(False)
                st = pkg.Stats()
                n = D.ctx.compress(D.d_in.data_ptr(), D.n, D.d_out.data_ptr(), D.cap, st)
                _stream_and_rest(D.out(), n, R["stream"], (name, on, "events only"))
                assert st.blocks == R["nb"] and st.ms_total > 0 and st.bwt_dominant_launches >= pieces, (name, on, st.as_dict())
                assert st.bytes_in == D.n and st.bytes_out == n and st.ms_bwt == 0, (name, on, st.as_dict())
                # stats with per-stage times: one piece whatever the knob says
                D.fresh()
                D.ctx.set_stage_times(True)
                st = pkg.Stats()
                n = D.ctx.compress(D.d_in.data_ptr(), D.n, D.d_out.data_ptr(), D.cap, st)
                _stream_and_rest(D.out(), n, R["stream"], (name, on, "stage times"))
                assert st.blocks == R["nb"] and st.ms_total > 0, (name, on, st.as_dict())
                assert min(st.ms_rle1, st.ms_bwt, st.ms_mtf, st.ms_huff, st.ms_pack) > 0, (name, on, st.as_dict())
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------- b. compress_range
def _ranges(nb):
    return [(0, nb), (2, nb - 2), (1, 5), (nb - 1, 1), (3, 0)]


@gpu
@pytest.mark.parametrize("name", ["b9", "b13"])
@pytest.mark.parametrize("max_range_blocks", [0, 5])
def test_compress_range(pkg, oracle, name, max_range_blocks):
    R = ref(oracle, name)
    nb = R["nb"]
    want = {r: oracle.bzip2_compress_range(R["data"], R["level"], r[0], r[1]) for r in _ranges(nb)}
    D = Dev(pkg, R, max_range_blocks)
    try:
        for on in (True, False):
            with ec.knob(on):
                for first, count in _ranges(nb):
                    D.fresh()
                    what = (name, max_range_blocks, on, first, count)
                    if max_range_blocks and count > max_range_blocks:
                        with pytest.raises(pkg.CjsError) as e:
                            D.ctx.compress_range(D.d_in.data_ptr(), D.n, first, count, D.d_out.data_ptr(), D.cap)
                        assert e.value.errorCode == -32, what
                        assert (D.out() == 0xA5).all(), what
                        continue
                    rc, wbytes, wbits, wtotal, wcrcs = want[(first, count)]
                    assert rc == 0 and wtotal == nb
                    bits, total, crcs = D.ctx.compress_range(D.d_in.data_ptr(), D.n, first, count, D.d_out.data_ptr(), D.cap)
                    assert bits == wbits and total == nb and crcs.size == nb, what
                    assert np.array_equal(crcs[first: first + count], wcrcs[first: first + count]), what      # (a call makes the CRCs of its own blocks)
                    back = D.out()
                    assert _bits_equal(back, wbytes, bits), what
                    assert (back[(bits + 7) // 8 + ZEROED:] == 0xA5).all(), what
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------- c. compress_indexed
def _tables_ref(pkg, oracle, name):
    """the dictionary test_gpu_enc_index.check_tables compares with: the parent route's tables of the oracle's stream"""
    R = ref(oracle, name)
    if "ix_raw" not in R:
        rc, table = oracle.bzip2_table(R["stream"])
        assert rc == 0
        ix = pkg.Bzip2Index.build(R["stream"])
        ln = pkg.Bzip2Lines.build(R["stream"], ix)
        R.update(table=table, ix_raw=ix.save(), ln_raw=ln.save(), nl=np.flatnonzero(R["data"] == 10).astype(np.int64))
    return R


@gpu
@pytest.mark.parametrize("name", ["b7", "b10"])
def test_compress_indexed(pkg, oracle, name):
    from test_gpu_enc_index import check_tables
    R = _tables_ref(pkg, oracle, name)
    D = Dev(pkg, R)
    try:
        for on in (True, False):
            with ec.knob(on):
                D.fresh()
                out_n, index, lines = D.ctx.compress_indexed(D.d_in.data_ptr(), D.n, D.d_out.data_ptr(), D.cap)
                back = D.out()
                _stream_and_rest(back, out_n, R["stream"], (name, on))
                assert index.blocks == R["nb"]
                check_tables(R, back[:out_n].copy(), index, lines, "indexed %s knob %s" % (name, on))
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------- d. the shard phases
@gpu
@pytest.mark.parametrize("name", ["b9", "l9b5"])
@pytest.mark.parametrize("world", [2, 3])
def test_shard_phases(pkg, oracle, name, world):
    import torch
    from test_gpu_shards import _run_phases
    R = ref(oracle, name)
    ndev = max(1, pkg.load_library().cjs_device_count())
    for on in (True, False):
        with ec.knob(on):
            stream, metas = _run_phases(pkg, torch, np.array(R["data"]), R["level"], world, ndev)
        assert stream.size == R["stream"].size and np.array_equal(stream, R["stream"]), (name, world, on, [m.blocks for m in metas])
        share = -(-R["nb"] // world)
        assert [(m.first_block, m.blocks) for m in metas] == [(min(r * share, R["nb"]), min(share, R["nb"] - min(r * share, R["nb"]))) for r in range(world)]


# ---------------------------------------------------------------------------------------------------- e. the streaming encoder
def _encode(pkg, data, level, chunk, piece, index):
    parts = []
    with pkg.Bzip2Encoder(level, chunk, index=index, lines=index) as enc:
        for pos in range(0, int(data.size), piece):
            enc.write(data[pos: pos + piece])
            while enc.pending:
                parts.append(enc.read())
        enc.finish()
        tables = enc.index() if index else (None, None)
        while enc.pending:
            parts.append(enc.read())
    return np.concatenate(parts), tables[0], tables[1]


@gpu
def test_encoder_steps(pkg, oracle):
    """chunks of 700,000 bytes written in pieces of 250,000: a step holds several blocks, all but the last go through the tables
    (cnt = nb - 1, first block 0) and the last is carried into the next step"""
    from test_gpu_enc_index import check_tables
    R = _tables_ref(pkg, oracle, "b13")
    for on in (True, False):
        with ec.knob(on):                                     # (set before the encoder's worker thread starts, unset behind its end)
            stream, _, _ = _encode(pkg, R["data"], 1, 700000, 250000, False)
            assert stream.size == R["stream"].size and np.array_equal(stream, R["stream"]), on
            stream, index, lines = _encode(pkg, R["data"], 1, 700000, 250000, True)
            check_tables(R, stream, index, lines, "encoder b13 knob %s" % on)


# ---------------------------------------------------------------------------------------------------- f. the host entry point
@gpu
@pytest.mark.parametrize("name", ["b5", "b9"])
def test_host_compress_on_the_cached_context(hip, oracle, name):
    R = ref(oracle, name)
    for on in (True, False, True):
        with ec.knob(on):
            rc, out = hip.bzip2_compress(R["data"], R["level"])
        assert rc == 0 and out.size == R["stream"].size and np.array_equal(out, R["stream"]), (name, on)


# ---------------------------------------------------------------------------------------------------- g. one context, a sequence
@gpu
@pytest.mark.parametrize("knobs", [(True, True, True, True), (False, False, False, False), (True, False, True, False), (False, True, False, True)],
                         ids=["split", "unsplit", "split-first", "unsplit-first"])
def test_one_context_through_a_sequence(pkg, oracle, knobs):
    """13 blocks, 1 block, 9 blocks into half the room (CJS_E_OUTPUT_TOO_SMALL, nothing written), 9 blocks with room"""
    import torch
    R13, R1, R9 = ref(oracle, "b13"), ref(oracle, "b1"), ref(oracle, "b9")
    ctx = pkg.DeviceContext(0, int(R13["data"].size), 1)
    d_in = {k: torch.from_numpy(np.array(R["data"])).to("cuda:0") for k, R in (("b13", R13), ("b1", R1), ("b9", R9))}
    room = (int(R13["data"].size) * 5 // 4 + 4096) & ~3
    half = (R9["stream"].size // 2) & ~3
    try:
        for step, (key, R, cap, on) in enumerate([("b13", R13, room, knobs[0]), ("b1", R1, room, knobs[1]), ("b9", R9, half, knobs[2]),
                                                  ("b9", R9, room, knobs[3])]):
            d_out = torch.full((room + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
            with ec.knob(on):
                if cap == half:
                    with pytest.raises(pkg.CjsError) as e:
                        ctx.compress(d_in[key].data_ptr(), int(R["data"].size), d_out.data_ptr(), cap)
                    assert e.value.errorCode == -33, (knobs, step)
                    assert (d_out.cpu().numpy() == 0xA5).all(), (knobs, step)
                else:
                    n = ctx.compress(d_in[key].data_ptr(), int(R["data"].size), d_out.data_ptr(), cap)
                    _stream_and_rest(d_out.cpu().numpy(), n, R["stream"], (knobs, step))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------- h. bwt_rounds
@gpu
def test_split_call_reports_the_most_rounds_of_its_pieces(pkg, oracle, capsys):
    """b10 goes in pieces of 3, 3, 3 and 1 blocks: the first holds the "ab" block, the last is 40,000 bytes of text.  Each piece
    alone (compress_range over its blocks, knob off: the same arguments reach bwt_run) tells its rounds; the split call over all
    blocks reports the most of them, not the last piece's."""
    R = ref(oracle, "b10")
    D = Dev(pkg, R)
    try:
        alone = []
        with ec.knob(False):
            for k0, kc in ec.piece_ranges(R["nb"], True):
                st = pkg.Stats()
                D.ctx.compress_range(D.d_in.data_ptr(), D.n, k0, kc, D.d_out.data_ptr(), D.cap, st)
                assert st.blocks == kc
                alone.append(int(st.bwt_rounds))
        assert len(alone) == 4 and alone[0] == max(alone) and alone[-1] < max(alone), alone      # (else the test could not tell the two)
        D.ctx.set_stage_times(False)
        with ec.knob(True):
            st = pkg.Stats()
            D.fresh()
            n = D.ctx.compress(D.d_in.data_ptr(), D.n, D.d_out.data_ptr(), D.cap, st)
        _stream_and_rest(D.out(), n, R["stream"], "b10 split, stats")
        with capsys.disabled():
            print("\n[bwt_rounds] b10 pieces alone %r, split call %d" % (alone, st.bwt_rounds))
        assert st.bwt_rounds == max(alone), (alone, st.bwt_rounds)
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------- not vacuous: the pieces ran
PIECES_LINE = re.compile(r"\[cjs pieces\] blocks \[(\d+), (\d+)\) of (\d+): (\d+) pieces of up to (\d+) blocks")


def child():
    """(the child of the test below) a sample of the calls above under CJS_DEBUG, with the knob and without; a "[case] tag" line on
    stderr in front of every call, the library's [cjs pieces] lines behind it; {tag: the call gave the oracle's bits} on stdout"""
    os.environ["CJS_DEBUG"] = "1"
    import torch
    import support
    from test_gpu_shards import _run_phases
    pkg, oracle, hip, out = _pkg(), support.Oracle(), support.HipLib(), {}

    def mark(tag):
        sys.stderr.flush()
        os.write(2, ("[case] %s\n" % tag).encode())

    for on in (True, False):
        k = "on" if on else "off"
        with ec.knob(on):
            for name in ec.ALL:
                R = ref(oracle, name)
                D = Dev(pkg, R)
                mark("compress/%s/%s" % (name, k))
                n = D.ctx.compress(D.d_in.data_ptr(), D.n, D.d_out.data_ptr(), D.cap)
                out["compress/%s/%s" % (name, k)] = bool(n == R["stream"].size and np.array_equal(D.out()[:n], R["stream"]))
                if name == "b13":
                    D.ctx.set_stage_times(False)
                    for stage_times in (False, True):
                        tag = "stats%d/b13/%s" % (stage_times, k)
                        D.ctx.set_stage_times(stage_times)
                        mark(tag)
                        st = pkg.Stats()
                        n = D.ctx.compress(D.d_in.data_ptr(), D.n, D.d_out.data_ptr(), D.cap, st)
                        out[tag] = bool(np.array_equal(D.out()[:n], R["stream"]))
                    for first, count in ((2, 11), (1, 5), (12, 1)):
                        tag = "range%d+%d/b13/%s" % (first, count, k)
                        mark(tag)
                        rc, wbytes, wbits, _, _ = oracle.bzip2_compress_range(R["data"], 1, first, count)
                        bits, _, _ = D.ctx.compress_range(D.d_in.data_ptr(), D.n, first, count, D.d_out.data_ptr(), D.cap)
                        out[tag] = bool(rc == 0 and bits == wbits and _bits_equal(D.out(), wbytes, bits))
                if name == "b7":
                    mark("indexed/b7/%s" % k)
                    n, index, lines = D.ctx.compress_indexed(D.d_in.data_ptr(), D.n, D.d_out.data_ptr(), D.cap)
                    out["indexed/b7/%s" % k] = bool(np.array_equal(D.out()[:n], R["stream"]) and index.blocks == 7)
                D.close()
            R = ref(oracle, "b9")
            mark("shards2/b9/%s" % k)
            stream, _ = _run_phases(pkg, torch, np.array(R["data"]), 1, 2, 1)
            out["shards2/b9/%s" % k] = bool(np.array_equal(stream, R["stream"]))
            mark("host/b5/%s" % k)
            rc, got = hip.bzip2_compress(ref(oracle, "b5")["data"], 1)
            out["host/b5/%s" % k] = bool(rc == 0 and np.array_equal(got, ref(oracle, "b5")["stream"]))
            R = ref(oracle, "b13")
            mark("encoder/b13/%s" % k)
            stream, _, _ = _encode(pkg, R["data"], 1, 700000, 250000, False)
            out["encoder/b13/%s" % k] = bool(np.array_equal(stream, R["stream"]))
            mark("end/%s" % k)
    print(json.dumps(out))


def _run_child():
    penv = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    penv.pop("CJS_ENC_PIECE_BYTES", None)
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", "import test_gpu_enc_pieces as t; t.child()"], capture_output=True, text=True,
                         env=penv, cwd=os.path.dirname(os.path.abspath(__file__)))
    assert run.returncode == 0, run.stderr[-3000:]
    lines, tag = {}, None
    for ln in run.stderr.splitlines():
        if ln.startswith("[case] "):
            tag = ln[7:].strip()
            lines[tag] = []
        m = PIECES_LINE.search(ln)
        if m and tag is not None:
            lines[tag].append(tuple(int(x) for x in m.groups()))
    return json.loads(run.stdout.strip().splitlines()[-1]), lines


def _line(f, cnt, nb, split):
    """the [cjs pieces] line of a call over blocks [f, f + cnt) of nb"""
    sizes = ec.piece_sizes(cnt, split)
    return (f, f + cnt, nb, len(sizes), sizes[0])


@gpu
def test_the_calls_ran_in_the_pieces_of_the_rule(capsys):
    ok, lines = _run_child()
    assert ok and all(ok.values()), [t for t, v in ok.items() if not v]
    seen = set()
    for on in (True, False):
        k = "on" if on else "off"
        for name in ec.ALL:
            nb = ec.NBLOCKS[name]
            assert lines["compress/%s/%s" % (name, k)] == [_line(0, nb, nb, on)], (name, k)
        assert lines["stats0/b13/%s" % k] == [_line(0, 13, 13, on)]
        assert lines["stats1/b13/%s" % k] == [_line(0, 13, 13, False)]                 # per-stage times: one piece, knob or not
        for first, count in ((2, 11), (1, 5), (12, 1)):
            assert lines["range%d+%d/b13/%s" % (first, count, k)] == [_line(first, count, 13, on)]
        assert lines["indexed/b7/%s" % k] == [_line(0, 7, 7, on)]
        assert lines["shards2/b9/%s" % k] == [_line(0, 5, 9, on), _line(5, 4, 9, on)]
        assert lines["host/b5/%s" % k] and sum(e - f for f, e, nb, p, per in lines["host/b5/%s" % k]) == 5
        # the encoder: steps of several blocks, all from block 0 on, every non-final one short of its carried last block
        steps = lines["encoder/b13/%s" % k]
        assert len(steps) >= 3 and sum(e - f for f, e, nb, p, per in steps) == 13
        assert all(f == 0 for f, e, nb, p, per in steps) and all(e == nb - 1 for f, e, nb, p, per in steps[:-1]) and steps[-1][1] == steps[-1][2]
        assert max(e for f, e, nb, p, per in steps) >= 5
        for tag, got in lines.items():
            if tag.endswith("/" + k):
                for f, e, nb, p, per in got:                                           # every call of the child, whatever made it
                    assert (f, e, nb, p, per) == _line(f, e - f, nb, on and not tag.startswith("stats1/")), (tag, got)
                    if on:
                        seen.add(tuple(ec.piece_sizes(e - f, not tag.startswith("stats1/"))))
    need = {(1,), (1, 1), (1, 1, 1), (1, 1, 1, 1), (2, 2, 1), (2, 2, 2, 1), (3, 3, 3), (3, 3, 3, 1), (4, 4, 4, 1)}
    with capsys.disabled():
        print("\n[cjs pieces] piece lists seen under the knob: %s" % sorted(seen))
    assert need <= seen, sorted(need - seen)
