"""Several host threads in the C ABI at once (the reference's concurrency contract, J/README.md:11): 4 threads, each on an
input of its own, compress, decompress and batch-compress through the host-buffer entry points and free the results, three
times over.  Every result must equal the one the same call gave on a single thread.  Results of 1 MiB and more come from
the pinned result pool, so this runs cjs_free and the pool's take / give from several threads at once.  A pass does not
prove that no race is left; it is the contract under load."""
import ctypes
import threading

import numpy as np
import pytest

import recipes
import support

pytestmark = pytest.mark.gpu

THREADS = 4
REPEATS = 3
INPUT_BYTES = 6_000_000                 # level-9 stream of textgen text: well over 1 MiB (pinned result path)
BATCH_SIZES = (1, 300, 70_000, 250_000)


def _lib():
    h = support.HipLib()
    L = h.L
    S = ctypes.c_size_t
    L.cjs_bzip2_compress_batch.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(S), S, ctypes.c_int,
                                           ctypes.POINTER(support.u8p), ctypes.POINTER(S), ctypes.POINTER(S), ctypes.c_void_p]
    L.cjs_bzip2_compress_batch.restype = ctypes.c_int
    return h


def _batch(h, inputs):
    """cjs_bzip2_compress_batch of `inputs` -> (rc, [stream bytes])"""
    count = len(inputs)
    ptrs = (ctypes.c_void_p * count)(*[x.ctypes.data for x in inputs])
    ns = (ctypes.c_size_t * count)(*[x.size for x in inputs])
    off = (ctypes.c_size_t * count)()
    ln = (ctypes.c_size_t * count)()
    out = support.u8p()
    rc = h.L.cjs_bzip2_compress_batch(ptrs, ns, count, 9, ctypes.byref(out), off, ln, None)
    if rc:
        return rc, None
    end = max(off[k] + ln[k] for k in range(count))
    buf = np.ctypeslib.as_array(out, shape=(max(end, 1),))
    streams = [buf[off[k]: off[k] + ln[k]].tobytes() for k in range(count)]
    h.L.cjs_free(out)
    return 0, streams


def _work(h, data, small):
    """one round of the calls a thread makes: (compressed, decompressed, batch streams)"""
    rc, comp = h.bzip2_compress(data, 9)
    assert rc == 0, h.L.cjs_strerror(rc)
    rc, back = h.bzip2_decompress(comp)
    assert rc == 0, h.L.cjs_strerror(rc)
    rc, streams = _batch(h, small)
    assert rc == 0, h.L.cjs_strerror(rc)
    return comp.tobytes(), back.tobytes(), streams


def test_host_abi_from_several_threads():
    h = _lib()
    inputs = [recipes.textgen(INPUT_BYTES, 500 + t) for t in range(THREADS)]
    smalls = [[recipes.textgen(n, 900 + 10 * t + i) for i, n in enumerate(BATCH_SIZES)] for t in range(THREADS)]
    want = [_work(h, inputs[t], smalls[t]) for t in range(THREADS)]        # single thread first
    for t in range(THREADS):
        assert len(want[t][0]) >= 1 << 20
        assert want[t][1] == inputs[t].tobytes()

    got = [[] for _ in range(THREADS)]
    errors = []

    def run(t):
        try:
            for _ in range(REPEATS):
                got[t].append(_work(h, inputs[t], smalls[t]))
        except BaseException as e:      # reported by the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(THREADS):
        assert len(got[t]) == REPEATS
        for r in range(REPEATS):
            comp, back, streams = got[t][r]
            assert comp == want[t][0], "thread %d round %d: compressed stream differs" % (t, r)
            assert back == want[t][1], "thread %d round %d: decompressed bytes differ" % (t, r)
            assert streams == want[t][2], "thread %d round %d: batch streams differ" % (t, r)
