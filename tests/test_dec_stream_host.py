"""Streaming Bzip2 decoder (cjs_bzip2_dec_*), the part that needs no GPU: the argument checks and the state machine of the C
ABI, the header verdicts (decided on the host from the first four bytes), and the plan itself -- decode, from the bytes of a
sliding window alone, every block that ends inside the window, carry the rest -- as a pure-Python model over the oracle's
single-block decoder, against the oracle's one-shot result."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

import recipes
import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NOT_BZIP, E_NO_DEVICE, E_INVALID_ARG = -2, -30, -32
NAMES = ("create", "write", "finish", "read", "done", "destroy")


def _lib():
    L = ctypes.CDLL(os.path.join(support.PKG, "libcjs_hip.so"))
    S, I, V = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    L.cjs_bzip2_dec_create.argtypes = [ctypes.POINTER(V), I, S, S, V]
    L.cjs_bzip2_dec_write.argtypes = [V, V, S, ctypes.POINTER(S)]
    L.cjs_bzip2_dec_finish.argtypes = [V]
    L.cjs_bzip2_dec_read.argtypes = [V, V, S, ctypes.POINTER(S)]
    L.cjs_bzip2_dec_done.argtypes = [V]
    L.cjs_bzip2_dec_destroy.argtypes = [V]
    L.cjs_bzip2_dec_destroy.restype = None
    L.cjs_device_count.restype = I
    L.cjs_last_error_detail.restype = ctypes.c_char_p
    return L


def _create(L, multi=0, chunk=0, out_bytes=0):
    h = ctypes.c_void_p()
    rc = L.cjs_bzip2_dec_create(ctypes.byref(h), multi, chunk, out_bytes, None)
    assert rc == 0 and h.value
    return h


def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cjs_hip.h")).read()
    L = _lib()
    for name in NAMES:
        assert "cjs_bzip2_dec_%s(" % name in hdr
        assert hasattr(L, "cjs_bzip2_dec_" + name)
    assert "PROGRESS" in hdr                                          # the progress contract is stated where callers read


def test_null_arguments_before_the_device_and_the_decoder_stays_failed():
    L = _lib()
    buf = (ctypes.c_uint8 * 16)(*b"BZh9")
    taken, got = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert L.cjs_bzip2_dec_create(None, 0, 0, 0, None) == E_INVALID_ARG
    assert L.cjs_bzip2_dec_write(None, buf, 4, ctypes.byref(taken)) == E_INVALID_ARG and taken.value == 0
    assert L.cjs_bzip2_dec_finish(None) == E_INVALID_ARG
    assert L.cjs_bzip2_dec_read(None, buf, 16, ctypes.byref(got)) == E_INVALID_ARG and got.value == 0
    assert L.cjs_bzip2_dec_done(None) == 0
    L.cjs_bzip2_dec_destroy(None)
    bad_calls = [
        lambda h: L.cjs_bzip2_dec_write(h, None, 3, ctypes.byref(taken)),      # in NULL with n > 0
        lambda h: L.cjs_bzip2_dec_write(h, buf, 4, None),                       # taken NULL
        lambda h: L.cjs_bzip2_dec_read(h, buf, 16, None),                       # got NULL
        lambda h: L.cjs_bzip2_dec_read(h, None, 16, ctypes.byref(got)),         # out NULL with cap > 0
    ]
    for bad in bad_calls:
        h = _create(L)
        assert L.cjs_bzip2_dec_write(h, None, 0, ctypes.byref(taken)) == 0      # a zero-length write is a write
        assert L.cjs_bzip2_dec_read(h, None, 0, ctypes.byref(got)) == 0 and got.value == 0
        assert bad(h) == E_INVALID_ARG
        # ... and the decoder stays failed with that code
        assert L.cjs_bzip2_dec_write(h, buf, 4, ctypes.byref(taken)) == E_INVALID_ARG and taken.value == 0
        assert L.cjs_bzip2_dec_finish(h) == E_INVALID_ARG
        assert L.cjs_bzip2_dec_read(h, buf, 16, ctypes.byref(got)) == E_INVALID_ARG and got.value == 0
        assert L.cjs_bzip2_dec_done(h) == 0
        L.cjs_bzip2_dec_destroy(h)


def test_write_after_finish():
    L = _lib()
    buf = (ctypes.c_uint8 * 4)(*b"BZh9")
    taken = ctypes.c_size_t(0)
    h = _create(L)
    assert L.cjs_bzip2_dec_write(h, buf, 2, ctypes.byref(taken)) == 0 and taken.value == 2
    assert L.cjs_bzip2_dec_finish(h) == 0
    assert L.cjs_bzip2_dec_write(h, buf, 2, ctypes.byref(taken)) == E_INVALID_ARG and taken.value == 0
    assert L.cjs_bzip2_dec_finish(h) == E_INVALID_ARG
    L.cjs_bzip2_dec_destroy(h)


def test_write_reports_what_the_window_took():
    # the window is chunk_bytes (clamped up to 64 KiB) plus one level-9 block's extent: writes never start GPU work, so this runs
    # without a device
    L = _lib()
    h = _create(L, 0, 1)
    data = np.zeros(4 << 20, np.uint8)
    data[:4] = np.frombuffer(b"BZh9", np.uint8)
    taken = ctypes.c_size_t(0)
    assert L.cjs_bzip2_dec_write(h, data.ctypes.data, data.size, ctypes.byref(taken)) == 0
    assert taken.value == 65536 + 900000 * 5 // 2 + 65536
    assert L.cjs_bzip2_dec_write(h, data.ctypes.data, 100, ctypes.byref(taken)) == 0 and taken.value == 0
    L.cjs_bzip2_dec_destroy(h)


@pytest.mark.parametrize("written,detail", [(b"BZx9" + bytes(40), "bad magic"), (b"BZh0" + bytes(40), "level out of range"),
                                            (b"BZh:" + bytes(40), "level out of range"), (b"", "bad magic"), (b"BZh", "bad magic")],
                         ids=["BZx9", "BZh0", "BZh_colon", "nothing", "three_bytes"])
@pytest.mark.parametrize("multi", [0, 1])
def test_header_verdicts_come_from_the_host(written, detail, multi):
    L = _lib()
    h = _create(L, multi)
    taken, got = ctypes.c_size_t(0), ctypes.c_size_t(0)
    out = (ctypes.c_uint8 * 64)()
    if written:
        arr = (ctypes.c_uint8 * len(written))(*written)
        assert L.cjs_bzip2_dec_write(h, arr, len(written), ctypes.byref(taken)) == 0 and taken.value == len(written)
    if len(written) < 4:                                               # fewer than four bytes decide nothing before finish
        assert L.cjs_bzip2_dec_read(h, out, 64, ctypes.byref(got)) == 0 and got.value == 0
    assert L.cjs_bzip2_dec_finish(h) == 0
    assert L.cjs_bzip2_dec_read(h, out, 64, ctypes.byref(got)) == E_NOT_BZIP and got.value == 0      # -2 and not -30: no device was asked
    assert L.cjs_last_error_detail().decode() == detail
    assert L.cjs_bzip2_dec_read(h, out, 64, ctypes.byref(got)) == E_NOT_BZIP
    assert L.cjs_last_error_detail().decode() == detail
    assert L.cjs_bzip2_dec_finish(h) == E_NOT_BZIP and L.cjs_bzip2_dec_done(h) == 0
    L.cjs_bzip2_dec_destroy(h)


def test_without_a_device_the_first_step_fails_loudly_and_for_good(oracle):
    L = _lib()
    if L.cjs_device_count() > 0:
        pytest.skip("a device is present")
    rc, stream = oracle.bzip2_compress(b"hello, world\n" * 50, 9)
    assert rc == 0
    h = _create(L)
    taken, got = ctypes.c_size_t(0), ctypes.c_size_t(0)
    out = (ctypes.c_uint8 * 64)()
    assert L.cjs_bzip2_dec_write(h, stream.ctypes.data, stream.size, ctypes.byref(taken)) == 0 and taken.value == stream.size
    assert L.cjs_bzip2_dec_read(h, out, 64, ctypes.byref(got)) == 0 and got.value == 0      # less than a chunk: no step is due
    assert L.cjs_bzip2_dec_finish(h) == 0
    assert L.cjs_bzip2_dec_read(h, out, 64, ctypes.byref(got)) == E_NO_DEVICE               # no CPU fallback
    assert L.cjs_bzip2_dec_read(h, out, 64, ctypes.byref(got)) == E_NO_DEVICE
    assert L.cjs_bzip2_dec_finish(h) == E_NO_DEVICE
    L.cjs_bzip2_dec_destroy(h)


def test_python_front_surface():
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("compressjs-flattened_amd")
    with pkg.Bzip2Decoder(False, 1 << 20) as dec:
        assert dec.write(b"BZ") == 2 and not dec.done
        assert dec.read(10).size == 0
        assert dec.write(b"x9") == 2
        dec.finish()
        with pytest.raises(pkg.CjsError) as e:
            dec.read(10)
        assert e.value.errorCode == E_NOT_BZIP and str(e.value).startswith("Not bzip data: bad magic")
        assert not dec.done
    gen = pkg.Bzip2.decompressStream([b"BZ", b"", b"h0", bytes(9)], multistream=True)
    with pytest.raises(pkg.CjsError) as e:
        list(gen)
    assert e.value.errorCode == E_NOT_BZIP and "level out of range" in str(e.value)


# ---------------------------------------------------------------------------------------------- the plan, on the oracle alone
def _bits_at(stream, bit, k):
    v = 0
    for i in range(k):
        b = bit + i
        v = (v << 1) | ((int(stream[b >> 3]) >> (7 - (b & 7))) & 1)
    return v


def model_decode(orc, stream, level, cuts):
    """The decoder's plan over the oracle's single-block decoder.  Every cut is the end of a non-final step's window, the stream's
    end is the final step.  A block is decided in a step when its 48 magic bits and its end lie inside the window (the final step:
    whatever is there); it is decoded from the WINDOW'S bytes alone -- the bytes from the carry point to the cut behind a stream
    header -- so a decoder that read anything behind a block's end-of-block code would fail here.  Returns (bytes, blocks decoded
    per step)."""
    stream = support.as_u8(stream)
    rc, table = orc.bzip2_table(stream)
    assert rc == 0
    starts = [b for b, _ in table]
    eos = next(b for b in range(stream.size * 8 - 87, stream.size * 8 - 79) if _bits_at(stream, b, 48) == 0x177245385090)
    ends = starts[1:] + [eos]
    head = np.frombuffer(b"BZh" + bytes([48 + level]), np.uint8)
    out, per_step, k, carry = [], [], 0, starts[0] // 8
    for cut in list(cuts) + [stream.size]:
        final = cut == stream.size
        win = stream[carry:cut]
        done = 0
        while k < len(starts):
            if starts[k] + 48 > cut * 8:                               # the block magic is not all in the window
                break
            if not final and ends[k] >= cut * 8:                       # the block does not end inside the window
                break
            rc, blk = orc.bzip2_decompress_block(np.concatenate([head, win]), 32 + starts[k] - carry * 8)
            assert rc == 0 and blk.size == table[k][1], (k, cut, rc)
            out.append(blk)
            k += 1
            done += 1
        per_step.append(done)
        carry = (starts[k] if k < len(starts) else eos) // 8           # the carry begins at the walk position's byte
        assert carry <= cut
    assert k == len(starts)
    return np.concatenate(out), per_step


@pytest.fixture(scope="module")
def text_stream(oracle):
    data = recipes.textgen(1200000, 5)
    rc, stream = oracle.bzip2_compress(data, 1)
    assert rc == 0
    return data, stream


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_plan_equals_the_one_shot_result(oracle, text_stream, seed):
    data, stream = text_stream
    rc, want = oracle.bzip2_decompress(stream)
    assert rc == 0 and np.array_equal(want, data)
    rng = np.random.default_rng(seed)
    cuts = sorted(set(int(c) for c in rng.integers(5, stream.size, 9)))
    got, per_step = model_decode(oracle, stream, 1, cuts)
    assert np.array_equal(got, want)
    assert sum(per_step) >= 12 and sum(1 for d in per_step if d) >= 4      # the 12 or so blocks were spread over the steps


def test_plan_with_cuts_at_the_block_boundaries(oracle, text_stream):
    # windows that end exactly at, one byte before and one byte behind a block's last byte
    data, stream = text_stream
    rc, table = oracle.bzip2_table(stream)
    assert rc == 0
    cuts = sorted(set(max(5, b // 8 + d) for (b, _), d in zip(table[1:], [-1, 0, 1, 2] * 4)))
    got, per_step = model_decode(oracle, stream, 1, cuts)
    assert np.array_equal(got, data)
