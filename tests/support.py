"""ctypes bindings used by the tests: the oracle (checker) and the HIP C-ABI library (product)."""
import ctypes
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PKG = os.path.join(ROOT, "compressjs-flattened_amd")

u8p = ctypes.POINTER(ctypes.c_uint8)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def as_u8(x):
    if isinstance(x, (bytes, bytearray)):
        return np.frombuffer(bytes(x), dtype=np.uint8)
    return np.ascontiguousarray(x, dtype=np.uint8)


class _StreamLib:
    """shared helper: functions of the form f(in, n, [args...], &out, &out_n) -> rc"""

    def _call_stream(self, fn, free, data, *mid, tail=()):
        data = as_u8(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        out = u8p()
        out_n = ctypes.c_size_t(0)
        rc = fn(keep.ctypes.data_as(u8p), data.size, *mid, ctypes.byref(out), ctypes.byref(out_n), *tail)
        if rc != 0:
            return rc, None
        res = np.ctypeslib.as_array(out, shape=(max(out_n.value, 1),))[: out_n.value].copy() if out_n.value else np.empty(0, np.uint8)
        free(out)
        return 0, res


class Oracle(_StreamLib):
    def __init__(self):
        path = os.path.join(ROOT, "oracle", "libcjs_oracle.so")
        if not os.path.exists(path):
            raise RuntimeError("oracle/libcjs_oracle.so missing: run `make oracle`")
        L = self.L = ctypes.CDLL(path)
        S, I, V = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
        L.cjs_oracle_bzip2_compress.argtypes = [u8p, S, I, ctypes.POINTER(u8p), ctypes.POINTER(S)]
        L.cjs_oracle_bzip2_decompress.argtypes = [u8p, S, I, ctypes.POINTER(u8p), ctypes.POINTER(S)]
        L.cjs_oracle_bwtc_compress.argtypes = [u8p, S, I, ctypes.POINTER(u8p), ctypes.POINTER(S)]
        L.cjs_oracle_bwtc_decompress.argtypes = [u8p, S, ctypes.POINTER(u8p), ctypes.POINTER(S)]
        L.cjs_oracle_bzip2_decompress_block.argtypes = [u8p, S, ctypes.c_uint64, ctypes.POINTER(u8p), ctypes.POINTER(S)]
        L.cjs_oracle_bzip2_table.argtypes = [u8p, S, I, V, V, ctypes.c_long]
        L.cjs_oracle_bzip2_table.restype = ctypes.c_long
        L.cjs_oracle_free.argtypes = [V]
        L.cjs_oracle_crc32.argtypes = [V, S]
        L.cjs_oracle_crc32.restype = ctypes.c_uint32
        L.cjs_oracle_suffix_array.argtypes = [V, I, V]
        L.cjs_oracle_bwt_cyclic.argtypes = [V, I, V]
        L.cjs_oracle_bwt_sentinel.argtypes = [V, I, V]
        L.cjs_oracle_huff_alloc.argtypes = [V, I, I]
        L.cjs_oracle_huff_lengths.argtypes = [V, I, V]
        L.cjs_oracle_rle1_block.argtypes = [V, S, ctypes.POINTER(S), V, I, ctypes.POINTER(ctypes.c_uint32)]
        L.cjs_oracle_mtf_rle2.argtypes = [V, V, I, V, V, ctypes.POINTER(I)]
        L.cjs_oracle_huff_groups.argtypes = [V, I, I, V, V]
        L.cjs_oracle_bzip2_block_bits.argtypes = [V, I, I, V, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(u8p),
                                                  ctypes.POINTER(ctypes.c_uint64)]
        L.cjs_oracle_bzip2_compress_range.argtypes = [u8p, S, I, ctypes.c_long, ctypes.c_long, ctypes.POINTER(u8p),
                                                      ctypes.POINTER(ctypes.c_uint64), V, ctypes.c_long, ctypes.POINTER(ctypes.c_long)]
        L.cjs_oracle_bwtc_model_steps.argtypes = [V, S, I, I, V, V, S, V]
        L.cjs_oracle_bwtc_model_steps.restype = ctypes.c_long
        L.cjs_oracle_bwtc_stream_steps.argtypes = [u8p, S, I, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint64)), ctypes.POINTER(S),
                                                   ctypes.POINTER(S), ctypes.POINTER(I), V, V, ctypes.c_long]
        L.cjs_oracle_bwtc_stream_steps.restype = ctypes.c_long
        L.cjs_oracle_rc_encode_steps.argtypes = [I, V, S, ctypes.POINTER(u8p), ctypes.POINTER(S), V]

    def _free(self, p):
        self.L.cjs_oracle_free(p)

    def bzip2_compress(self, data, level=9):
        return self._call_stream(self.L.cjs_oracle_bzip2_compress, self._free, data, level)

    def bzip2_decompress(self, data, multistream=0):
        return self._call_stream(self.L.cjs_oracle_bzip2_decompress, self._free, data, multistream)

    def bzip2_compress_range(self, data, level, first, count, crc_cap=1 << 16):
        """bare bit string of blocks [first, first+count): (bytes, nbits, total_blocks, all block crcs)"""
        data = as_u8(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        out, bits, tot = u8p(), ctypes.c_uint64(0), ctypes.c_long(0)
        crcs = np.zeros(crc_cap, dtype=np.uint32)
        rc = self.L.cjs_oracle_bzip2_compress_range(keep.ctypes.data_as(u8p), data.size, level, first, count, ctypes.byref(out),
                                                    ctypes.byref(bits), crcs.ctypes.data, crc_cap, ctypes.byref(tot))
        if rc:
            return rc, None, 0, 0, None
        nb = (bits.value + 7) // 8
        arr = np.ctypeslib.as_array(out, shape=(max(nb, 1),))[:nb].copy()
        self.L.cjs_oracle_free(out)
        return 0, arr, bits.value, tot.value, crcs[: tot.value].copy()

    def bwtc_compress(self, data, level=9):
        return self._call_stream(self.L.cjs_oracle_bwtc_compress, self._free, data, level)

    def bwtc_decompress(self, data):
        return self._call_stream(self.L.cjs_oracle_bwtc_decompress, self._free, data)

    def bzip2_decompress_block(self, data, bitpos):
        return self._call_stream(self.L.cjs_oracle_bzip2_decompress_block, self._free, data, ctypes.c_uint64(bitpos))

    # event counters of bwtc_model_steps (oracle/cjs_oracle.h, CJSO_FEN_* / CJSO_DSM_*)
    FEN_EVENTS = ("rescale", "escape", "last_escape", "decay", "esc_zeroed", "esc_reinstated", "rescale_between")
    DSM_EVENTS = ("fold", "refused_cap", "refused_thresh", "escape")

    def bwtc_model_steps(self, A, asz, fast):
        """one block's model section: (steps u64, symbol position of each step u32, {event: count})"""
        A = np.ascontiguousarray(A, dtype=np.uint16)
        cap = 2 * A.size + 1
        steps = np.zeros(cap, dtype=np.uint64)
        pos = np.zeros(cap, dtype=np.uint32)
        ev = np.zeros(8, dtype=np.uint64)
        n = self.L.cjs_oracle_bwtc_model_steps(A.ctypes.data, A.size, asz, 1 if fast else 0, steps.ctypes.data, pos.ctypes.data, cap,
                                               ev.ctypes.data)
        assert 0 <= n < cap, "cjs_oracle_bwtc_model_steps: %d" % n
        names = self.DSM_EVENTS if fast else self.FEN_EVENTS
        return steps[:n], pos[:n], {k: int(ev[i]) for i, k in enumerate(names)}

    def bwtc_stream_steps(self, data, level, cap=4096):
        """every coder call of bwtc_compress(data, level): (rc, steps u64, prefix_n, first_byte, [(lo, hi) of each block's model
        section])"""
        data = as_u8(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        p, n, pre, fb = ctypes.POINTER(ctypes.c_uint64)(), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int(0)
        lo = np.zeros(cap, dtype=np.uint64)
        hi = np.zeros(cap, dtype=np.uint64)
        nb = self.L.cjs_oracle_bwtc_stream_steps(keep.ctypes.data_as(u8p), data.size, level, ctypes.byref(p), ctypes.byref(n),
                                                 ctypes.byref(pre), ctypes.byref(fb), lo.ctypes.data, hi.ctypes.data, cap)
        if nb < 0:
            return nb, None, 0, 0, None
        steps = np.ctypeslib.as_array(p, shape=(max(n.value, 1),))[: n.value].copy()
        self.L.cjs_oracle_free(p)
        return 0, steps, pre.value, fb.value, [(int(lo[k]), int(hi[k])) for k in range(min(nb, cap))]

    def rc_encode_steps(self, first_byte, steps):
        """(rc, coder bytes, {max_help, carries, max_shifts, finish_carry})"""
        steps = np.ascontiguousarray(steps, dtype=np.uint64)
        keep = steps if steps.size else np.zeros(1, dtype=np.uint64)
        out, out_n = u8p(), ctypes.c_size_t(0)
        st = np.zeros(4, dtype=np.uint32)
        rc = self.L.cjs_oracle_rc_encode_steps(first_byte, keep.ctypes.data, steps.size, ctypes.byref(out), ctypes.byref(out_n),
                                               st.ctypes.data)
        if rc:
            return rc, None, None
        res = np.ctypeslib.as_array(out, shape=(max(out_n.value, 1),))[: out_n.value].copy()
        self.L.cjs_oracle_free(out)
        return 0, res, dict(zip(("max_help", "carries", "max_shifts", "finish_carry"), (int(v) for v in st)))

    def bzip2_table(self, data, multistream=0, cap=100000):
        data = as_u8(data)
        pos = np.zeros(cap, dtype=np.uint64)
        size = np.zeros(cap, dtype=np.uint32)
        n = self.L.cjs_oracle_bzip2_table(data.ctypes.data_as(u8p), data.size, multistream, pos.ctypes.data, size.ctypes.data, cap)
        if n < 0:
            return n, None
        return 0, list(zip(pos[:n].tolist(), size[:n].tolist()))

    def crc32(self, data):
        data = as_u8(data)
        keep = data if data.size else np.zeros(1, np.uint8)
        return self.L.cjs_oracle_crc32(keep.ctypes.data, data.size)

    def bwt_cyclic(self, data):
        data = as_u8(data)
        U = np.empty(max(data.size, 1), dtype=np.uint8)
        pidx = self.L.cjs_oracle_bwt_cyclic(data.ctypes.data, data.size, U.ctypes.data)
        return U[: data.size], pidx

    def bwt_sentinel(self, data):
        data = as_u8(data)
        U = np.empty(max(data.size, 1), dtype=np.uint8)
        pidx = self.L.cjs_oracle_bwt_sentinel(data.ctypes.data, data.size, U.ctypes.data)
        return U[: data.size], pidx

    def suffix_array(self, data):
        data = as_u8(data)
        SA = np.empty(max(data.size, 1), dtype=np.int32)
        self.L.cjs_oracle_suffix_array(data.ctypes.data, data.size, SA.ctypes.data)
        return SA[: data.size]

    def huff_alloc(self, sorted_freq, maxlen):
        a = np.array(sorted_freq, dtype=np.int32)
        self.L.cjs_oracle_huff_alloc(a.ctypes.data, a.size, maxlen)
        return a.tolist()

    def huff_lengths(self, freq):
        f = np.array(freq, dtype=np.uint32)
        out = np.zeros(f.size, dtype=np.uint8)
        self.L.cjs_oracle_huff_lengths(f.ctypes.data, f.size, out.ctypes.data)
        return out

    def rle1_blocks(self, data, level):
        """all RLE1 blocks of a stream: list of (block bytes, crc, consumed_start, consumed_end)"""
        return self.rle1_blocks_cap(data, level * 100000 - 19)

    def rle1_len(self, data):
        """RLE1 length of the whole input as ONE block (no capacity in the way)"""
        data = as_u8(data)
        res = self.rle1_blocks_cap(data, 2 * data.size + 16)
        assert len(res) <= 1
        return res[0][0].size if res else 0

    def rle1_blocks_cap(self, data, cap):
        """the same with any block capacity cap >= 1"""
        data = as_u8(data)
        cur = ctypes.c_size_t(0)
        res = []
        keep = data if data.size else np.zeros(1, np.uint8)
        blk = np.empty(cap, dtype=np.uint8)                   # (a small cap makes thousands of blocks: one buffer, addresses taken once)
        crc = ctypes.c_uint32(0)
        p_in, p_blk, p_cur, p_crc, fn = keep.ctypes.data, blk.ctypes.data, ctypes.byref(cur), ctypes.byref(crc), self.L.cjs_oracle_rle1_block
        while True:
            start = cur.value
            n = fn(p_in, data.size, p_cur, p_blk, cap, p_crc)
            if n > 0:
                res.append((blk[:n].copy(), crc.value, start, cur.value))
            if n != cap:
                break
        return res

    def mtf_rle2(self, U, block):
        U = as_u8(U)
        block = as_u8(block)
        A = np.empty(U.size + 1, dtype=np.uint16)
        freq = np.zeros(258, dtype=np.uint32)
        asz = ctypes.c_int(0)
        pos = self.L.cjs_oracle_mtf_rle2(U.ctypes.data, block.ctypes.data, U.size, A.ctypes.data, freq.ctypes.data, ctypes.byref(asz))
        return A[:pos].copy(), freq[: asz.value + 2].copy(), asz.value

    def huff_groups(self, A, alphabet_size):
        A = np.ascontiguousarray(A, dtype=np.uint16)
        nsel = (A.size + 49) // 50
        sel = np.zeros(max(nsel, 1), dtype=np.uint8)
        lens = np.zeros(6 * 258, dtype=np.uint8)
        ng = self.L.cjs_oracle_huff_groups(A.ctypes.data, A.size, alphabet_size, sel.ctypes.data, lens.ctypes.data)
        return ng, sel[:nsel].copy(), lens.reshape(6, 258)[:ng, : alphabet_size + 2].copy()

    def bzip2_block_bits(self, A, alphabet_size, used_bytes, crc, pidx):
        """one block's bare bit string from its MTF/RLE2 symbols (magic .. data): (rc, bytes, nbits); used_bytes = the byte
        values present (ascending list or array)"""
        A = np.ascontiguousarray(A, dtype=np.uint16)
        used = np.zeros(256, dtype=np.uint8)
        used[np.asarray(used_bytes, dtype=np.int64)] = 1
        out, bits = u8p(), ctypes.c_uint64(0)
        rc = self.L.cjs_oracle_bzip2_block_bits(A.ctypes.data, A.size, alphabet_size, used.ctypes.data, crc, pidx,
                                                ctypes.byref(out), ctypes.byref(bits))
        if rc:
            return rc, None, 0
        nb = (bits.value + 7) // 8
        arr = np.ctypeslib.as_array(out, shape=(max(nb, 1),))[:nb].copy()
        self.L.cjs_oracle_free(out)
        return 0, arr, bits.value


class HipLib(_StreamLib):
    """The product: compressjs-flattened_amd/libcjs_hip.so through its C ABI (include/cjs_hip.h)."""

    def __init__(self):
        path = os.path.join(PKG, "libcjs_hip.so")
        if not os.path.exists(path):
            raise RuntimeError("libcjs_hip.so missing: run `make hip` (python __graft_entry__.py)")
        L = self.L = ctypes.CDLL(path)
        S, I, V = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
        PS = ctypes.POINTER(S)
        PP = ctypes.POINTER(u8p)
        sigs = {
            "cjs_bzip2_compress": [u8p, S, I, PP, PS, V],
            "cjs_bwtc_compress": [u8p, S, I, PP, PS, V],
            "cjs_bzip2_decompress": [u8p, S, I, PP, PS, V],
            "cjs_bwtc_decompress": [u8p, S, PP, PS, V],
            "cjs_free": [V],
            "cjs_strerror": [I],
            "cjs_device_count": [],
            "cjs_bzip2_decompress_block": [u8p, S, ctypes.c_uint64, PP, PS, V],
            "cjs_bzip2_table": [u8p, S, I, V, V, ctypes.c_long, V],
            "cjs_stage_bwt": [V, S, I, I, V, V, V],
            "cjs_stage_bwt_var": [V, ctypes.c_uint32, ctypes.c_uint32, V, V, V, V],
            "cjs_stage_rle1": [V, S, I, V, S, V, V, V, ctypes.c_long, ctypes.POINTER(ctypes.c_long), V],
            "cjs_stage_rle1_cap": [V, S, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, I, V, S, V, V, V, V, ctypes.c_long,
                                   ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_uint32), V],
            "cjs_stage_rle1_batch": [V, S, V, ctypes.c_uint32, ctypes.c_uint32, I, V, V, V, ctypes.c_uint32, ctypes.c_uint32, V, V, V, V,
                                     V, V, V, ctypes.c_uint32, ctypes.c_uint32, V, V, V],
            "cjs_stage_mtf": [V, V, S, I, V, V, V, V, V],
            "cjs_stage_mtf_var": [V, ctypes.c_uint32, ctypes.c_uint32, V, I, V, V, V, V, V, V, V],
            "cjs_stage_huff": [V, ctypes.c_uint32, ctypes.c_uint32, V, V, V, V],
            "cjs_stage_huff_blocks": [V, S, ctypes.c_uint32, V, V, V, V, V, I, V, V, V, V, S, V, V],
            "cjs_stage_bwtc_entropy_decode": [u8p, S, PP, PS, V, V, ctypes.c_long, ctypes.POINTER(I)],
            "cjs_stage_bwtc_model": [V, S, ctypes.c_uint32, V, V, I, V, S, V, V],
            "cjs_stage_bwtc_code": [V, S, I, I, PP, PS],
            "cjs_last_error_detail": [],
        }
        self.missing = []
        for name, args in sigs.items():
            fn = getattr(L, name, None)
            if fn is None:      # symbol missing from the C ABI (tests/test_abi.py fails on this)
                self.missing.append(name)
                continue
            fn.argtypes = args
            fn.restype = I
        L.cjs_strerror.restype = ctypes.c_char_p
        L.cjs_version.restype = ctypes.c_char_p
        if hasattr(L, "cjs_last_error_detail"):
            L.cjs_last_error_detail.restype = ctypes.c_char_p
        if hasattr(L, "cjs_stage_bwtc_entropy_decode"):
            L.cjs_stage_bwtc_entropy_decode.restype = ctypes.c_long
        L.cjs_free.restype = None
        L.cjs_trim.argtypes = []
        L.cjs_trim.restype = None
        if hasattr(L, "cjs_bzip2_table"):
            L.cjs_bzip2_table.restype = ctypes.c_long

    def _free(self, p):
        self.L.cjs_free(p)

    def bzip2_compress(self, data, level=9):
        return self._call_stream(self.L.cjs_bzip2_compress, self._free, data, level, tail=(None,))

    def bwtc_compress(self, data, level=9):
        return self._call_stream(self.L.cjs_bwtc_compress, self._free, data, level, tail=(None,))

    def bzip2_decompress(self, data, multistream=0):
        return self._call_stream(self.L.cjs_bzip2_decompress, self._free, data, multistream, tail=(None,))

    def bwtc_decompress(self, data):
        return self._call_stream(self.L.cjs_bwtc_decompress, self._free, data, tail=(None,))

    def bzip2_decompress_block(self, data, bitpos):
        return self._call_stream(self.L.cjs_bzip2_decompress_block, self._free, data, ctypes.c_uint64(bitpos), tail=(None,))

    def bzip2_table(self, data, multistream=0, cap=100000):
        data = as_u8(data)
        pos = np.zeros(cap, dtype=np.uint64)
        size = np.zeros(cap, dtype=np.uint32)
        n = self.L.cjs_bzip2_table(data.ctypes.data_as(u8p), data.size, multistream, pos.ctypes.data, size.ctypes.data, cap, None)
        if n < 0:
            return n, None
        return 0, list(zip(pos[:n].tolist(), size[:n].tolist()))

    def last_error_detail(self):
        return self.L.cjs_last_error_detail().decode()

    def stage_bwtc_entropy_decode(self, data, cap=1 << 16):
        """(rc or number of blocks, level, [(BWT column bytes, pidx)])  -- host logic, runs without a GPU"""
        data = as_u8(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        cols, cols_n, level = u8p(), ctypes.c_size_t(0), ctypes.c_int(0)
        lens = np.zeros(cap, dtype=np.uint32)
        pidx = np.zeros(cap, dtype=np.uint32)
        nb = self.L.cjs_stage_bwtc_entropy_decode(keep.ctypes.data_as(u8p), data.size, ctypes.byref(cols), ctypes.byref(cols_n),
                                                  lens.ctypes.data, pidx.ctypes.data, cap, ctypes.byref(level))
        if nb < 0:
            return nb, 0, None
        flat = np.ctypeslib.as_array(cols, shape=(max(cols_n.value, 1),))[: cols_n.value].copy() if cols_n.value else np.empty(0, np.uint8)
        self.L.cjs_free(cols)
        out, off = [], 0
        for k in range(min(nb, cap)):
            out.append((flat[off: off + int(lens[k])], int(pidx[k])))
            off += int(lens[k])
        return nb, level.value, out

    def stage_bwtc_model(self, blocks, level):
        """the model kernel of `level` on many blocks in one launch (cjs_stage_bwtc_model).  blocks: list of (A u16 symbols,
        asz).  Returns (rc, [steps u64 of each block])"""
        nb = len(blocks)
        a_stride = max(1, max(len(a) for a, _ in blocks))
        A = np.zeros((nb, a_stride), dtype=np.uint16)
        nsym = np.zeros(nb, dtype=np.uint32)
        asz = np.zeros(nb, dtype=np.uint32)
        for k, (a, z) in enumerate(blocks):
            A[k, : len(a)] = a
            nsym[k], asz[k] = len(a), z
        step_stride = 2 * a_stride
        steps = np.zeros((nb, step_stride), dtype=np.uint64)
        nsteps = np.zeros(nb, dtype=np.uint32)
        rc = self.L.cjs_stage_bwtc_model(A.ctypes.data, a_stride, nb, nsym.ctypes.data, asz.ctypes.data, level, steps.ctypes.data,
                                         step_stride, nsteps.ctypes.data, None)
        if rc:
            return rc, None
        return 0, [steps[k, : min(int(nsteps[k]), step_stride)] if nsteps[k] <= step_stride else None for k in range(nb)]

    def stage_bwtc_code(self, steps, first_byte, mode):
        """the host range coder over a step list (cjs_stage_bwtc_code; mode 0 one thread, 1 split): (rc, bytes).  No GPU"""
        steps = np.ascontiguousarray(steps, dtype=np.uint64)
        keep = steps if steps.size else np.zeros(1, dtype=np.uint64)
        out, out_n = u8p(), ctypes.c_size_t(0)
        rc = self.L.cjs_stage_bwtc_code(keep.ctypes.data, steps.size, first_byte, mode, ctypes.byref(out), ctypes.byref(out_n))
        if rc:
            return rc, None
        res = np.ctypeslib.as_array(out, shape=(max(out_n.value, 1),))[: out_n.value].copy() if out_n.value else np.empty(0, np.uint8)
        self.L.cjs_free(out)
        return 0, res

    def stage_bwt(self, data, block_len, cyclic):
        data = as_u8(data)
        nb = max(1, -(-data.size // block_len))
        U = np.zeros(max(data.size, 1), dtype=np.uint8)
        pidx = np.zeros(nb, dtype=np.int32)
        rc = self.L.cjs_stage_bwt(data.ctypes.data, data.size, block_len, 1 if cyclic else 0, U.ctypes.data, pidx.ctypes.data, None)
        return rc, U[: data.size], pidx

    def stage_bwt_var(self, blocks, stride, hole_fill=0):
        """the cyclic BWT of blocks of different lengths, block k in slot k of `stride` bytes (cjs_stage_bwt_var); the holes
        behind the blocks are filled with `hole_fill`.  Returns (rc, [U_k, len(blocks[k]) bytes each], pidx)"""
        blocks = [as_u8(b) for b in blocks]
        nb = len(blocks)
        lens = np.array([b.size for b in blocks], dtype=np.uint32)
        slots = np.full((max(nb, 1), stride), hole_fill, dtype=np.uint8)
        for k, b in enumerate(blocks):
            slots[k, : min(b.size, stride)] = b[:stride]        # (a block longer than its slot: the entry point refuses the call)
        U = np.zeros((max(nb, 1), stride), dtype=np.uint8)
        pidx = np.zeros(max(nb, 1), dtype=np.int32)
        keep = lens if nb else np.zeros(1, dtype=np.uint32)
        rc = self.L.cjs_stage_bwt_var(slots.ctypes.data, nb, stride, keep.ctypes.data, U.ctypes.data, pidx.ctypes.data, None)
        if rc:
            return rc, None, None
        return 0, [U[k, : blocks[k].size] for k in range(nb)], pidx[:nb]

    def stage_rle1(self, data, level):
        data = as_u8(data)
        cap = level * 100000 - 19
        maxb = data.size // (cap * 4 // 5) + 2
        blocks = np.zeros(maxb * cap, dtype=np.uint8)
        blen = np.zeros(maxb, dtype=np.uint32)
        bcrc = np.zeros(maxb, dtype=np.uint32)
        bstart = np.zeros(maxb + 1, dtype=np.uint64)
        nb = ctypes.c_long(0)
        keep = data if data.size else np.zeros(1, np.uint8)
        rc = self.L.cjs_stage_rle1(keep.ctypes.data, data.size, level, blocks.ctypes.data, blocks.size, blen.ctypes.data,
                                   bcrc.ctypes.data, bstart.ctypes.data, maxb, ctypes.byref(nb), None)
        if rc:
            return rc, None
        n = nb.value
        return 0, [(blocks[k * cap: k * cap + int(blen[k])].copy(), int(bcrc[k]), int(bstart[k])) for k in range(n)]

    def stage_rle1_cap(self, data, cap, world=1, range_blocks=0, work_fill=0):
        """stage 0 with a block capacity of the caller's choice (cjs_stage_rle1_cap): (rc, [(block bytes, crc, input start, input
        end)], last_len).  The host rows are pre-filled with 0xA5, so bytes the stage never wrote do not pass for zeros."""
        data = as_u8(data)
        maxb = data.size // max(cap * 4 // 5, 1) + 2
        blocks = np.full(maxb * max(cap, 1), 0xA5, dtype=np.uint8)
        blen = np.zeros(maxb, dtype=np.uint32)
        bcrc = np.zeros(maxb, dtype=np.uint32)
        bstart = np.zeros(maxb, dtype=np.uint64)
        bend = np.zeros(maxb, dtype=np.uint64)
        nb, last = ctypes.c_long(0), ctypes.c_uint32(0)
        keep = data if data.size else np.zeros(1, np.uint8)
        rc = self.L.cjs_stage_rle1_cap(keep.ctypes.data, data.size, cap, world, range_blocks, work_fill, blocks.ctypes.data, blocks.size,
                                       blen.ctypes.data, bcrc.ctypes.data, bstart.ctypes.data, bend.ctypes.data, maxb, ctypes.byref(nb),
                                       ctypes.byref(last), None)
        if rc:
            return rc, None, None
        return 0, [(blocks[k * cap: k * cap + int(blen[k])], int(bcrc[k]), int(bstart[k]), int(bend[k])) for k in range(nb.value)], last.value

    def stage_rle1_batch(self, buf, se, cap, item=(), tbase=(0,), table_slots=None, mat=(), stride=16, work_fill=0):
        """the three batch kernels of stage 0, each with the caller's arrays (cjs_stage_rle1_batch).  se: [(start, end)] in buf;
        item / tbase: the walk's inputs and slot grants; mat: [(s, e, len)] of the blocks to materialise into rows of `stride`.
        Returns (rc, len2[count], (walk_s, walk_e, walk_len)[table_slots], nblk[nitem], rows[nmat][stride], crc[nmat])"""
        buf = as_u8(buf)
        keep = buf if buf.size else np.zeros(1, np.uint8)
        count, nitem, nmat = len(se), len(item), len(mat)
        se_a = np.array([x for p in se for x in p], dtype=np.uint64).reshape(-1)
        item_a = np.array(list(item) + [0], dtype=np.uint32)
        tbase_a = np.array(list(tbase), dtype=np.uint32)
        assert tbase_a.size == nitem + 1
        slots = int(tbase_a[-1]) if table_slots is None else table_slots
        len2 = np.zeros(max(count, 1), dtype=np.uint64)
        ws, we = np.zeros(max(slots, 1), dtype=np.uint64), np.zeros(max(slots, 1), dtype=np.uint64)
        wl = np.zeros(max(slots, 1), dtype=np.uint32)
        nblk = np.zeros(max(nitem, 1), dtype=np.uint32)
        ms = np.array([m[0] for m in mat] + [0], dtype=np.uint64)
        me = np.array([m[1] for m in mat] + [0], dtype=np.uint64)
        ml = np.array([m[2] for m in mat] + [0], dtype=np.uint32)
        rows = np.zeros((max(nmat, 1), stride), dtype=np.uint8)
        crc = np.zeros(max(nmat, 1), dtype=np.uint32)
        keep_se = se_a if se_a.size else np.zeros(2, dtype=np.uint64)
        rc = self.L.cjs_stage_rle1_batch(keep.ctypes.data, buf.size, keep_se.ctypes.data, count, cap, work_fill, len2.ctypes.data,
                                         item_a.ctypes.data, tbase_a.ctypes.data, nitem, slots, ws.ctypes.data, we.ctypes.data,
                                         wl.ctypes.data, nblk.ctypes.data, ms.ctypes.data, me.ctypes.data, ml.ctypes.data, nmat, stride,
                                         rows.ctypes.data, crc.ctypes.data, None)
        if rc:
            return rc, None, None, None, None, None
        return 0, len2[:count], (ws[:slots], we[:slots], wl[:slots]), nblk[:nitem], rows[:nmat], crc[:nmat]

    def stage_mtf(self, U, blocks, block_len):
        U = as_u8(U)
        blocks = as_u8(blocks)
        nb = max(1, -(-U.size // block_len))
        A = np.zeros(nb * (block_len + 1), dtype=np.uint16)
        npos = np.zeros(nb, dtype=np.uint32)
        freq = np.zeros(nb * 258, dtype=np.uint32)
        asz = np.zeros(nb, dtype=np.uint32)
        rc = self.L.cjs_stage_mtf(U.ctypes.data, blocks.ctypes.data, U.size, block_len, A.ctypes.data, npos.ctypes.data,
                                  freq.ctypes.data, asz.ctypes.data, None)
        return rc, A.reshape(nb, block_len + 1), npos, freq.reshape(nb, 258), asz

    def stage_mtf_var(self, blocks, stride, hole_fill=0, work_fill=0):
        """MTF + RLE2 of blocks of different lengths, block k in slot k of `stride` bytes (cjs_stage_mtf_var).  hole_fill: one byte
        for every hole, or one per block (the hole behind block k); the workspace is filled with `work_fill` before the run.
        Returns (rc, A[nb][stride + 1], npos, freq[nb][258], asz, alist[nb][256], nheads)"""
        blocks = [as_u8(b) for b in blocks]
        nb = len(blocks)
        lens = np.array([b.size for b in blocks], dtype=np.uint32)
        slots = np.zeros((max(nb, 1), stride), dtype=np.uint8)
        slots[:] = np.asarray(hole_fill, dtype=np.uint8).reshape(-1, 1)
        for k, b in enumerate(blocks):
            slots[k, : min(b.size, stride)] = b[:stride]        # (a block longer than its slot: the entry point refuses the call)
        m = max(nb, 1)
        A = np.zeros((m, stride + 1), dtype=np.uint16)
        npos, asz, nheads = (np.zeros(m, dtype=np.uint32) for _ in range(3))
        freq = np.zeros((m, 258), dtype=np.uint32)
        alist = np.zeros((m, 256), dtype=np.uint8)
        keep = lens if nb else np.zeros(1, dtype=np.uint32)
        rc = self.L.cjs_stage_mtf_var(slots.ctypes.data, nb, stride, keep.ctypes.data, work_fill, A.ctypes.data, npos.ctypes.data,
                                      freq.ctypes.data, asz.ctypes.data, alist.ctypes.data, nheads.ctypes.data, None)
        if rc:
            return rc, None, None, None, None, None, None
        return 0, A[:nb], npos[:nb], freq[:nb], asz[:nb], alist[:nb], nheads[:nb]

    def stage_huff(self, A, alphabet):
        A = np.ascontiguousarray(A, dtype=np.uint16)
        nsel = (A.size + 49) // 50
        sel = np.zeros(max(nsel, 1), dtype=np.uint8)
        lens = np.zeros(6 * 258, dtype=np.uint8)
        ng = ctypes.c_uint32(0)
        rc = self.L.cjs_stage_huff(A.ctypes.data, A.size, alphabet, sel.ctypes.data, lens.ctypes.data, ctypes.byref(ng), None)
        return rc, ng.value, sel[:nsel], lens.reshape(6, 258)[: ng.value, : alphabet + 2]

    def stage_huff_blocks(self, blocks, path):
        """Huffman tables + bare bit packing of several blocks in one call (cjs_stage_huff_blocks).  blocks: list of dicts with
        A (u16 symbols, EOB last), asz, used (ascending byte values), crc, pidx.  path 0 = the compressors' rule, 1 = one
        workgroup per block, 2 = the chain of kernels.  Returns (rc, [(ngroups, selectors, lengths[ng][asz+2], bytes, nbits)])"""
        nb = len(blocks)
        a_stride = max(b["A"].size for b in blocks)
        A = np.zeros(nb * a_stride, dtype=np.uint16)
        npos = np.zeros(nb, dtype=np.uint32)
        asz = np.zeros(nb, dtype=np.uint32)
        used = np.zeros(nb * 256, dtype=np.uint8)
        crc = np.zeros(nb, dtype=np.uint32)
        pidx = np.zeros(nb, dtype=np.uint32)
        for k, b in enumerate(blocks):
            a = np.asarray(b["A"], dtype=np.uint16)
            A[k * a_stride: k * a_stride + a.size] = a
            npos[k], asz[k], crc[k], pidx[k] = a.size, b["asz"], b["crc"], b["pidx"]
            u = np.asarray(b["used"], dtype=np.uint8)
            used[k * 256: k * 256 + u.size] = u
        hsel = (a_stride + 49) // 50
        ng = np.zeros(nb, dtype=np.uint32)
        sel = np.zeros(nb * hsel, dtype=np.uint8)
        lens = np.zeros(nb * 6 * 258, dtype=np.uint8)
        bits_stride = ((a_stride * 20 + 6 * 258 * 41 + 6 * hsel + 512) // 8 + 7) & ~7     # > any block's bit string
        bits = np.zeros(nb * bits_stride, dtype=np.uint8)
        nbits = np.zeros(nb, dtype=np.uint64)
        rc = self.L.cjs_stage_huff_blocks(A.ctypes.data, a_stride, nb, npos.ctypes.data, asz.ctypes.data, used.ctypes.data,
                                          crc.ctypes.data, pidx.ctypes.data, path, ng.ctypes.data, sel.ctypes.data,
                                          lens.ctypes.data, bits.ctypes.data, bits_stride, nbits.ctypes.data, None)
        if rc:
            return rc, None
        out = []
        for k in range(nb):
            g, n, b = int(ng[k]), int(nbits[k]), k * bits_stride
            out.append((g, sel[k * hsel: k * hsel + (int(npos[k]) + 49) // 50].copy(),
                        lens.reshape(nb, 6, 258)[k, :g, : int(asz[k]) + 2].copy(), bits[b: b + (n + 7) // 8].copy(), n))
        return 0, out
