"""Bzip2 recovery on the GPU (cjs_bzip2_recover, cjs_bzip2_recover_device): the intact blocks of damaged .bz2 data as bytes and as
a repaired stream, host and device form, held to the contract of include/cjs_hip.h: what the inputs of tests/recover_cases.py were
built to give (checked there against the oracle on the CPU), the existing decoder on undamaged input, the numpy model of both
result forms, and -- for every stream form produced -- the oracle's and the library's own decoder."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bzblocks
import recover_cases as rc_

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = ctypes.c_size_t


def _pkg():
    import importlib
    sys.path.insert(0, ROOT)
    return importlib.import_module("compressjs-flattened_amd")


@pytest.fixture(scope="module")
def L():
    return rc_.bind(_pkg().LIB_PATH)


def check(L, oracle, hip, buf, positions=None, data=None, stream=None, device=True):
    """Both forms, host and device, of one input, against what is expected of it (None: not stated) and against each other; the
    report against the magics numpy finds; the stream form through both decoders.  -> (data, stream, found of the bytes form)"""
    buf = rc_.u8(buf)
    rc, got, found = rc_.recover_host(L, buf, 0)
    assert rc == 0
    assert [f[0] for f in found] == rc_.magics(buf)
    rec = [f for f in found if f[4] == 0]
    if positions is not None:
        assert [f[0] for f in rec] == positions
    if data is not None:
        assert got == data, bzblocks.first_difference(got, data)
    assert sum(f[3] for f in rec) == len(got)
    assert [f[2] for f in rec] == np.concatenate([[0], np.cumsum([f[3] for f in rec])])[:-1].astype(np.int64).tolist()       # out_off: the prefix sums
    last = 0
    for p, end, off, size, status, crc in found:
        assert status != 0 or (end > p >= last and end < 8 * buf.size)
        assert (status == rc_.SHADOWED) == (p < last)
        if status == 0:
            last = end
        else:
            assert off == 0 and size == 0
    rc, sgot, sfound = rc_.recover_host(L, buf, 1)
    assert rc == 0
    assert [(f[0], f[1], f[3], f[4], f[5]) for f in sfound] == [(f[0], f[1], f[3], f[4], f[5]) for f in found]
    at = 32
    for p, end, off, size, status, crc in sfound:                            # out_off: where the block's magic stands in the new stream
        if status == 0:
            assert off == at
            at += end - p
    assert len(sgot) == (at + 80 + 7) // 8 and sgot[:4] == b"BZh9"
    if stream is not None:
        assert sgot == stream
    rc, back = oracle.bzip2_decompress(rc_.u8(sgot), 0)                      # the repaired stream decodes, by both decoders, to the bytes form
    assert rc == 0 and back.tobytes() == got
    rc, back = hip.bzip2_decompress(rc_.u8(sgot), 0)
    assert rc == 0 and back.tobytes() == got
    if device:
        assert rc_.recover_device(L, buf, 0) == (0, got, found, len(got))
        assert rc_.recover_device(L, buf, 1) == (0, sgot, sfound, len(sgot))
    return got, sgot, found


def check_model(L, oracle, hip, buf, **kw):
    m = rc_.model(oracle, buf)
    return check(L, oracle, hip, buf, positions=[r[0] for r in m.recovered], data=m.data, stream=m.stream, **kw), m


# ---------------------------------------------------------------- 1. undamaged input equals decompress
def _table(L, buf, multi):
    a = rc_.u8(buf)
    pos, size = np.zeros(4096, np.uint64), np.zeros(4096, np.uint32)
    n = L.cjs_bzip2_table(a.ctypes.data_as(rc_.u8p), a.size, multi, pos.ctypes.data, size.ctypes.data, 4096, None)
    assert 0 <= n <= 4096
    return list(zip(pos[:n].tolist(), size[:n].tolist()))


def test_undamaged_level1_stream(L, oracle, hip):
    s = rc_.stream250(oracle)
    rc, want = hip.bzip2_decompress(s, 1)
    assert rc == 0
    want9 = s.copy(); want9[3] = ord("9")
    data, stream, found = check(L, oracle, hip, s, positions=[p for p, _ in rc_.BLOCKS250], data=want.tobytes(), stream=want9.tobytes())
    assert [(f[0], f[3]) for f in found] == _table(L, s, 1) == rc_.BLOCKS250
    assert [f[1] for f in found] == [299452, 604689, rc_.EOS250]             # inside a member end_bit[k] == bitpos[k + 1]
    assert all(f[4] == 0 for f in found)


def test_undamaged_level9_stream_is_its_own_repair(L, oracle, hip):
    s = rc_.stream250_l9(oracle)
    check(L, oracle, hip, s, positions=[32], data=rc_.text250().tobytes(), stream=s.tobytes())


def test_empty_stream(L, oracle, hip):
    data, stream, found = check(L, oracle, hip, rc_.EMPTY_STREAM, positions=[], data=b"", stream=rc_.EMPTY_STREAM)
    assert found == []


def test_three_members_become_one_stream(L, oracle, hip):
    s, payload = rc_.members(oracle)
    rc, want = hip.bzip2_decompress(s, 1)
    assert rc == 0 and want.tobytes() == payload
    (data, stream, found), m = check_model(L, oracle, hip, s)
    assert data == payload and [(f[0], f[3]) for f in found if f[4] == 0] == _table(L, s, 1)
    rc, first = oracle.bzip2_decompress(s, 0)
    assert rc == 0 and first.size < len(payload)                            # (the reference stops behind the first member)


# ---------------------------------------------------------------- 2. damage behind which decompress returns nothing
def test_flipped_bit_in_block_1(L, oracle, hip):
    t = rc_.text250().tobytes()
    bad = rc_.damage_a(oracle)
    assert hip.bzip2_decompress(bad, 1)[0] != 0
    data, stream, found = check(L, oracle, hip, bad, positions=[32, 604689], data=t[:99898] + t[99898 + 99897:])
    assert found[1][0] == 299452 and found[1][4] not in (0, rc_.SHADOWED)


def test_flipped_stored_crc_is_decodable_and_lost(L, oracle, hip):
    t = rc_.text250().tobytes()
    data, stream, found = check(L, oracle, hip, rc_.damage_b(oracle), positions=[32, 604689], data=t[:99898] + t[99898 + 99897:])
    assert found[1][:2] == (299452, 604689) and found[1][4] == -5


def test_deleted_byte_no_header_cut_tail(L, oracle, hip):
    t = rc_.text250().tobytes()
    bad = rc_.damage_c(oracle)
    assert hip.bzip2_decompress(bad, 1)[0] == -2
    check(L, oracle, hip, bad, positions=[299444], data=t[99898: 99898 + 99897])


def test_garbage_between_streams(L, oracle, hip):
    t = rc_.text250().tobytes()
    bad = rc_.damage_d(oracle)
    assert hip.bzip2_decompress(bad, 1)[0] == -2
    check(L, oracle, hip, bad, positions=[32, 299452, 604689, 768960], data=t + t[:1000])


def test_every_bit_shift(L, oracle, hip):
    """the file k bits later for k = 0 .. 31: every relative shift of the gather against the same destination"""
    t = rc_.text250().tobytes()
    base = None
    for k in range(32):
        buf = rc_.shifted(oracle, k)
        rc, stream, found = rc_.recover_host(L, buf, 1)
        assert rc == 0 and [f[0] for f in found if f[4] == 0] == [p + k for p, _ in rc_.BLOCKS250], k
        base = stream if base is None else base
        assert stream == base, k
        assert rc_.recover_device(L, buf, 1, in_shift=k % 5) == (0, stream, found, len(stream)), k
        rc, data, _ = rc_.recover_host(L, buf, 0)
        assert rc == 0 and data == t, k
    want9 = rc_.stream250(oracle).copy(); want9[3] = ord("9")
    assert base == want9.tobytes()


# ---------------------------------------------------------------- 3. odd sizes and alignments
@pytest.mark.parametrize("which", sorted(rc_.FORTY_DAMAGE))
def test_forty_small_blocks(L, oracle, hip, which):
    s, want, tab = rc_.forty(oracle)
    bad, keep = rc_.forty_damaged(oracle, which)
    (data, stream, found), m = check_model(L, oracle, hip, bad)
    assert data == keep and len(found) == 40
    assert [f[4] for f in found] == [-5 if k in rc_.FORTY_DAMAGE[which] else 0 for k in range(40)]
    if which == "all":
        assert stream == rc_.EMPTY_STREAM
    if which == "none":
        assert stream == s.tobytes()


# ---------------------------------------------------------------- 4. shadowing
def test_false_magic_inside_a_block_is_shadowed(L, oracle, hip):
    s, payload = rc_.magic_in_map(oracle)
    data, stream, found = check(L, oracle, hip, s, positions=[32], data=payload, stream=s.tobytes())
    assert [(f[0], f[4]) for f in found] == [(32, 0), (137, rc_.SHADOWED)]


def test_a_lost_block_shadows_nothing(L, oracle, hip):
    s, _ = rc_.magic_in_map(oracle)
    data, stream, found = check(L, oracle, hip, rc_.flip(s, 32 + 53), positions=[], data=b"", stream=rc_.EMPTY_STREAM)
    assert [f[0] for f in found] == [32, 137] and found[0][4] == -5 and found[0][1] > 137
    assert found[1][4] < 0                                                   # its own code (the oracle: -7), not "shadowed"


# ---------------------------------------------------------------- 5. level limit
def test_blocks_are_decoded_with_the_level_9_limit(L, oracle, hip):
    s, payload = rc_.level_limit(oracle)
    assert hip.bzip2_decompress(s, 0)[0] == -5
    check(L, oracle, hip, s, positions=[32], data=payload)


# ---------------------------------------------------------------- 6. batches
@pytest.mark.parametrize("rows, elems", [(14 * 900000, 1000000), (14 * 900000, 150000)])
def test_shrunk_batches_give_the_same(L, oracle, rows, elems):
    """cases 1-3 in a child process whose row and inverse-BWT batches are small (the budgets are read once per process)"""
    env = dict(os.environ, CJS_DEC_ROW_BYTES=str(rows), CJS_DEC_BATCH_ELEMS=str(elems))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "recover_cases.py")], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    theirs = json.loads(out.stdout.strip().splitlines()[-1])
    ours = rc_.digest(L, oracle, True)
    assert sorted(theirs) == sorted(ours) and len(ours) == 4 * 14
    assert [k for k in sorted(ours) if theirs[k] != ours[k]] == []


# ---------------------------------------------------------------- 7. device form
def test_device_capacity_rules(L, oracle):
    import torch
    bad = rc_.damage_a(oracle)
    for as_stream in (0, 1):
        rc, want, found = rc_.recover_host(L, bad, as_stream)
        assert rc == 0 and len(want) > 1000
        assert rc_.recover_device(L, bad, as_stream, cap_bytes=len(want)) == (0, want, found, len(want))           # exact
        rc, _, dfound, need = rc_.recover_device(L, bad, as_stream, cap_bytes=len(want) - 1)
        assert (rc, need, dfound) == (-33, len(want), found)
        rc, _, dfound, need = rc_.recover_device(L, bad, as_stream, cap_bytes=0)                                  # the size query
        assert (rc, need, dfound) == (-33, len(want), found)
    rc, _, _, need = rc_.recover_device(L, rc_.EMPTY_STREAM, 1, cap_bytes=13)
    assert (rc, need) == (-33, 14)
    assert rc_.recover_device(L, rc_.EMPTY_STREAM, 0, cap_bytes=0) == (0, b"", [], 0)                             # nothing recovered fits in nothing
    host_in = rc_.u8(bad)
    dst = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    n, nf = S(0), ctypes.c_long(0)
    assert L.cjs_bzip2_recover_device(host_in.ctypes.data, host_in.size, 0, dst.data_ptr(), dst.numel(), ctypes.byref(n), None, 0, ctypes.byref(nf), None) == -32
    src = torch.from_numpy(host_in).cuda()
    host_out = np.zeros(1 << 20, np.uint8)
    assert L.cjs_bzip2_recover_device(src.data_ptr(), host_in.size, 0, host_out.ctypes.data, host_out.size, ctypes.byref(n), None, 0, ctypes.byref(nf), None) == -32
    assert not host_out.any()


def test_python_front(L, oracle):
    import torch
    pkg = _pkg()
    bad = rc_.damage_a(oracle)
    for as_stream in (False, True):
        rc, want, found = rc_.recover_host(L, bad, int(as_stream))
        data, pfound = pkg.Bzip2.recoverFile(bad, None, as_stream)
        assert data.tobytes() == want and pfound == found
        src = torch.from_numpy(bad).cuda()
        dst = torch.zeros(len(want), dtype=torch.uint8, device="cuda")
        assert pkg.recover_device(src.data_ptr(), bad.size, dst.data_ptr(), dst.numel(), as_stream) == (len(want), found)
        assert dst.cpu().numpy().tobytes() == want
        with pytest.raises(pkg.CjsError) as e:
            pkg.recover_device(src.data_ptr(), bad.size, dst.data_ptr(), dst.numel() - 1, as_stream)
        assert e.value.errorCode == -33 and e.value.need == len(want) and e.value.found == found
    data, pfound = pkg.Bzip2.recoverFile(b"abc")
    assert data.size == 0 and pfound == []


# ---------------------------------------------------------------- 8. seeded random damage against the model
@pytest.mark.parametrize("seed", rc_.SEEDS)
def test_random_damage_matches_the_model(L, oracle, hip, seed):
    check_model(L, oracle, hip, rc_.random_damage(oracle, seed))
