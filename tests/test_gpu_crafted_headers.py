"""-m gpu: blocks whose HEADERS no compressor emits (bzcraft_cases.py), decoded by the HIP path and by the oracle.

The decoder's first phase rebuilds the reference's sequential header reader (J/Bzip2_joined_.js:1440-1596) and the walk over the
groups of 50 codes as wave-parallel code (csrc/bz_stage2.h: dec_prologue, bz_chain): selector values read as lane words of a
2048-bit stretch with a run of ones carried from lane to lane, the move-to-front as composed nibble permutations, code lengths
whose bits mean control or direction by the parity of the ones in front, three forms of every canonical table, later groups
placed by the shortest codes of the tables in front of them.  Every case here reaches one of those seams -- test_bzcraft_host.py
proves that from the writer's bit offsets, and that the model decoder the block CRCs come from agrees with the oracle -- and the
HIP decoder must give the oracle's status and bytes, alone and as an item of one batch call.
"""
import ctypes

import numpy as np
import pytest

import bzblocks
import bzcraft
import bzcraft_cases as cc

pytestmark = pytest.mark.gpu
u8p = ctypes.POINTER(ctypes.c_uint8)
CJS_E_HIP = -31               # include/cjs_hip.h: the HIP runtime reported an error

_streams = {}


def stream_of(name):
    if name not in _streams:
        _streams[name] = cc.BY_NAME[name].stream()
    return _streams[name]


def check(hip, oracle, name, rc_h, out_h):
    case = cc.BY_NAME[name]
    if rc_h == CJS_E_HIP:                            # nothing more is to be launched on a device that has reported an error
        pytest.exit("HIP error in %s: %s" % (name, hip.last_error_detail()), returncode=3)
    rc_o, out_o = oracle.bzip2_decompress(stream_of(name))
    assert rc_h == rc_o, (name, rc_h, rc_o, hip.last_error_detail())
    assert rc_o == (0 if case.expect == "ok" else bzcraft.OBSOLETE_INPUT if case.expect.startswith("randomised") else bzcraft.DATA_ERROR), (name, rc_o)
    if rc_o == 0:
        assert len(out_h) == out_o.size and bytes(out_h) == out_o.tobytes(), (name, bzblocks.first_difference(out_h, out_o))


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_crafted_header(hip, oracle, name):
    rc_h, out_h = hip.bzip2_decompress(stream_of(name))
    check(hip, oracle, name, rc_h, out_h if rc_h == 0 else b"")


def decompress_batch(hip, inputs):
    """cjs_bzip2_decompress_batch -> (rc, [(status, bytes)])"""
    f = hip.L.cjs_bzip2_decompress_batch
    S = ctypes.c_size_t
    f.argtypes = [ctypes.POINTER(u8p), ctypes.POINTER(S), S, ctypes.c_int, ctypes.POINTER(u8p), ctypes.POINTER(S), ctypes.POINTER(S),
                  ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p]
    f.restype = ctypes.c_int
    arrs = [np.ascontiguousarray(x, dtype=np.uint8) for x in inputs]
    cnt = len(arrs)
    ptrs = (u8p * cnt)(*[a.ctypes.data_as(u8p) for a in arrs])
    lens = (S * cnt)(*[a.size for a in arrs])
    off, ln, st = (S * cnt)(), (S * cnt)(), (ctypes.c_int32 * cnt)()
    out = u8p()
    rc = f(ptrs, lens, cnt, 0, ctypes.byref(out), off, ln, st, None)
    res = []
    if rc == 0:
        for k in range(cnt):
            res.append((st[k], ctypes.string_at(ctypes.addressof(out.contents) + off[k], ln[k]) if ln[k] else b""))
        hip.L.cjs_free(out)
    return rc, res


def test_all_cases_as_one_batch(hip, oracle):
    # the _batch instantiations of the same kernels read every item up to its OWN end and hold it to its OWN level's limits: the
    # level pairs (100000 and 100001 bytes under BZh1 and under BZh9) sit in the same batch as everything else
    names = [c.name for c in cc.CASES]
    assert {"B-level1-100000-bytes", "B-level1-100001-bytes", "B-level9-100000-bytes", "B-level9-100001-bytes"} <= set(names)
    rc, res = decompress_batch(hip, [stream_of(n) for n in names])
    if rc == CJS_E_HIP:
        pytest.exit("HIP error in the batch call: %s" % hip.last_error_detail(), returncode=3)
    assert rc == 0, (rc, hip.last_error_detail())
    singles = [hip.bzip2_decompress(stream_of(n)) for n in names]
    for name, (st, out), (rc_s, out_s) in zip(names, res, singles):
        assert st == rc_s, (name, st, rc_s)
        assert out == (out_s.tobytes() if rc_s == 0 else b""), (name, bzblocks.first_difference(out, out_s if rc_s == 0 else b""))
        check(hip, oracle, name, st, out)
    by = dict(zip(names, res))
    assert by["B-level1-100000-bytes"][0] == 0 and by["B-level9-100001-bytes"][0] == 0 and by["B-level1-100001-bytes"][0] == bzcraft.DATA_ERROR


@pytest.mark.parametrize("family", "USLTCM")
def test_family_in_reverse_order_as_a_batch(hip, oracle, family):
    # the same items in another order and company: a row's scratch (selector values, tables, chain arrays) is whatever the item in
    # front of it in the batch left behind
    names = [c.name for c in cc.CASES if c.family == family][::-1]
    rc, res = decompress_batch(hip, [stream_of(n) for n in names])
    assert rc == 0, (rc, hip.last_error_detail())
    for name, (st, out) in zip(names, res):
        check(hip, oracle, name, st, out)
