"""compressjs-flattened_amd — MI355X-native block-sorting core behind the compressjs Bzip2/BWTC API.

The product is the HIP library `libcjs_hip.so` (C ABI: include/cjs_hip.h) plus the JavaScript fronts
under js/ (Node + N-API).  This Python module is plumbing for tests and bench.py: a ctypes binding of
the same C ABI and `Bzip2` / `BWTC` objects that mirror the reference's method names
(`compressFile`, `decompressFile`; J/Bzip2_joined_.js:2198-2253, J/BWTC_joined_.js:1696-1698,1827).
There is no CPU fallback: if the library or a GPU is missing every call raises.
"""
import ctypes
import os
import weakref

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CJS_HIP_LIB") or os.path.join(PKG_DIR, "libcjs_hip.so")   # same override as the N-API addon
u8p = ctypes.POINTER(ctypes.c_uint8)


class CjsError(Exception):
    def __init__(self, code, msg):
        super().__init__("%s (code %d)" % (msg, code))
        self.errorCode = code


class Stats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_rle1", ctypes.c_double), ("ms_bwt", ctypes.c_double),
                ("ms_mtf", ctypes.c_double), ("ms_huff", ctypes.c_double), ("ms_pack", ctypes.c_double),
                ("ms_bwt_dominant", ctypes.c_double), ("bwt_dominant_launches", ctypes.c_uint64),
                ("bwt_dominant_bytes", ctypes.c_uint64), ("blocks", ctypes.c_uint64), ("bytes_in", ctypes.c_uint64),
                ("bytes_out", ctypes.c_uint64), ("bwt_rounds", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ShardMeta(ctypes.Structure):
    """cjs_shard_meta: what the ranks of a multi-GPU job exchange between the block phase and the pack phase (32 bytes)."""
    _fields_ = [("bits", ctypes.c_uint64), ("total_blocks", ctypes.c_uint64), ("first_block", ctypes.c_uint64),
                ("blocks", ctypes.c_uint32), ("crc_fold", ctypes.c_uint32)]


class Found(ctypes.Structure):
    """cjs_bz_found: one block candidate of a recovery (40 bytes)."""
    _fields_ = [("bitpos", ctypes.c_uint64), ("end_bit", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("size", ctypes.c_uint32),
                ("status", ctypes.c_int32), ("crc", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


REC_SHADOWED = 1      # CJS_REC_SHADOWED


class IndexEntry(ctypes.Structure):
    """cjs_bz_index_entry: one block of a block index (32 bytes, also its serialised form)."""
    _fields_ = [("bitpos", ctypes.c_uint64), ("end_bit", ctypes.c_uint64), ("size", ctypes.c_uint32), ("crc", ctypes.c_uint32),
                ("level", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class Match(ctypes.Structure):
    """cjs_bz_match: one match of a search (16 bytes)."""
    _fields_ = [("off", ctypes.c_uint64), ("pattern", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class SearchInfo(ctypes.Structure):
    """cjs_bz_search_info (32 bytes)."""
    _fields_ = [("n_matches", ctypes.c_uint64), ("n_bad_blocks", ctypes.c_uint64), ("first_bad_block", ctypes.c_uint64),
                ("blocks_decoded", ctypes.c_uint64)]


SEARCH_NOCASE = 1     # CJS_SEARCH_NOCASE


class Diff(ctypes.Structure):
    """cjs_bz_diff: one differing byte of a compare (16 bytes)."""
    _fields_ = [("off", ctypes.c_uint64), ("a", ctypes.c_uint8), ("b", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 6)]


class CompareInfo(ctypes.Structure):
    """cjs_bz_cmp_info (64 bytes)."""
    _fields_ = [("n_diffs", ctypes.c_uint64), ("first_diff", ctypes.c_uint64), ("compared", ctypes.c_uint64), ("n_bad_blocks", ctypes.c_uint64),
                ("first_bad_block", ctypes.c_uint64), ("blocks_decoded", ctypes.c_uint64), ("n_bad_blocks_b", ctypes.c_uint64),
                ("first_bad_block_b", ctypes.c_uint64)]


class LineKey(ctypes.Structure):
    """cjs_bz_linekey: the key of one line (16 bytes); all three fields all-ones: the line touches a bad block."""
    _fields_ = [("hash", ctypes.c_uint64), ("len", ctypes.c_uint32), ("check", ctypes.c_uint32)]


class LineKeysInfo(ctypes.Structure):
    """cjs_bz_linekeys_info (32 bytes)."""
    _fields_ = [("n_lines", ctypes.c_uint64), ("n_bad_blocks", ctypes.c_uint64), ("first_bad_block", ctypes.c_uint64),
                ("blocks_decoded", ctypes.c_uint64)]


class Hunk(ctypes.Structure):
    """cjs_bz_hunk: lines [a_first, +a_count) of A replaced by [b_first, +b_count) of B (32 bytes)."""
    _fields_ = [("a_first", ctypes.c_uint64), ("a_count", ctypes.c_uint64), ("b_first", ctypes.c_uint64), ("b_count", ctypes.c_uint64)]


class LineDiffInfo(ctypes.Structure):
    """cjs_bz_ldiff_info (32 bytes)."""
    _fields_ = [("n_hunks", ctypes.c_uint64), ("edits", ctypes.c_uint64), ("common", ctypes.c_uint64), ("minimal", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class CutInfo(ctypes.Structure):
    """cjs_bz_cut_info (40 bytes)."""
    _fields_ = [("n_lines", ctypes.c_uint64), ("out_bytes", ctypes.c_uint64), ("blocks_decoded", ctypes.c_uint64),
                ("n_bad_blocks", ctypes.c_uint64), ("first_bad_block", ctypes.c_uint64)]


class TallyInfo(ctypes.Structure):
    """cjs_tally_info (40 bytes)."""
    _fields_ = [("n_keys", ctypes.c_uint64), ("n_bad", ctypes.c_uint64), ("n_distinct", ctypes.c_uint64), ("n_groups", ctypes.c_uint64),
                ("max_count", ctypes.c_uint64)]


class StreamTallyInfo(ctypes.Structure):
    """cjs_bz_tally_info (64 bytes)."""
    _fields_ = [("n_lines", ctypes.c_uint64), ("n_bad_lines", ctypes.c_uint64), ("n_distinct", ctypes.c_uint64), ("n_groups", ctypes.c_uint64),
                ("max_count", ctypes.c_uint64), ("blocks_decoded", ctypes.c_uint64), ("n_bad_blocks", ctypes.c_uint64), ("first_bad_block", ctypes.c_uint64)]


class SortInfo(ctypes.Structure):
    """cjs_bz_sort_info (64 bytes)."""
    _fields_ = [("n_lines", ctypes.c_uint64), ("n_out", ctypes.c_uint64), ("n_distinct", ctypes.c_uint64), ("text_bytes", ctypes.c_uint64),
                ("rounds", ctypes.c_uint64), ("blocks_decoded", ctypes.c_uint64), ("n_bad_blocks", ctypes.c_uint64), ("first_bad_block", ctypes.c_uint64)]


LINE_KEY_DTYPE = np.dtype([("hash", "<u8"), ("len", "<u4"), ("check", "<u4")])
TALLY_DTYPE = np.dtype([("hash", "<u8"), ("len", "<u4"), ("check", "<u4"), ("first", "<u8"), ("count", "<u8")])      # cjs_bz_tally (32 bytes)
TALLY_BY_FIRST, TALLY_BY_COUNT, TALLY_LINES = 0, 1, 2
SORT_REVERSE, SORT_UNIQUE, SORT_LINES = 1, 2, 2
CUT_RANGE_DTYPE = np.dtype([("lo", "<u4"), ("hi", "<u4")])
CUT_FIELDS, CUT_BYTES, CUT_TO_END = 0, 1, 0xFFFFFFFF

_lib = None


def load_library():
    """dlopen the HIP C-ABI library; raises if it has not been built (`python __graft_entry__.py`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libcjs_hip.so not built: run `make hip` / `python __graft_entry__.py` (no CPU fallback exists)")
    try:
        # torch wheels bundle their own libamdhip64: load it first so that both share ONE HIP runtime in this
        # process (two copies of the runtime cannot both own the device)
        import torch  # noqa: F401
    except Exception:
        pass
    L = ctypes.CDLL(LIB_PATH)
    S, I, V = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    PS, PP = ctypes.POINTER(S), ctypes.POINTER(u8p)
    L.cjs_bzip2_compress.argtypes = [u8p, S, I, PP, PS, V]
    L.cjs_bwtc_compress.argtypes = [u8p, S, I, PP, PS, V]
    L.cjs_bzip2_decompress.argtypes = [u8p, S, I, PP, PS, V]
    L.cjs_bwtc_decompress.argtypes = [u8p, S, PP, PS, V]
    L.cjs_free.argtypes = [V]
    L.cjs_free.restype = None
    L.cjs_trim.argtypes = []
    L.cjs_trim.restype = None
    L.cjs_strerror.argtypes = [I]
    L.cjs_strerror.restype = ctypes.c_char_p
    L.cjs_version.restype = ctypes.c_char_p
    L.cjs_last_error_detail.restype = ctypes.c_char_p
    L.cjs_device_count.restype = I
    L.cjs_ctx_create.argtypes = [ctypes.POINTER(V), I, S, I]
    L.cjs_ctx_create_sharded.argtypes = [ctypes.POINTER(V), I, S, ctypes.c_long, I]
    L.cjs_ctx_destroy.argtypes = [V]
    L.cjs_ctx_destroy.restype = None
    L.cjs_ctx_set_stage_times.argtypes = [V, I]
    L.cjs_ctx_set_stage_times.restype = None
    L.cjs_bzip2_compress_device.argtypes = [V, V, S, I, V, S, PS, ctypes.POINTER(Stats)]
    L.cjs_bzip2_compress_device_range.argtypes = [V, V, S, I, ctypes.c_long, ctypes.c_long, V, S, ctypes.POINTER(ctypes.c_uint64),
                                                  V, ctypes.c_long, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(Stats)]
    L.cjs_bzip2_compress_batch.argtypes = [ctypes.POINTER(u8p), PS, S, I, PP, PS, PS, V]
    L.cjs_ctx_create_batch.argtypes = [ctypes.POINTER(V), I, S, S, I]
    L.cjs_bzip2_decompress_batch.argtypes = [ctypes.POINTER(u8p), PS, S, I, PP, PS, PS, ctypes.POINTER(ctypes.c_int32), V]
    L.cjs_bzip2_compress_batch_device.argtypes = [V, V, PS, S, I, V, S, PS, PS]
    L.cjs_bzip2_decompress_device.argtypes = [V, S, I, V, S, PS, V]
    L.cjs_bzip2_decompress_batch_device.argtypes = [V, PS, S, I, V, S, PS, PS, ctypes.POINTER(ctypes.c_int32), PS, V]
    L.cjs_bzip2_shard_share_bytes.argtypes = [S, I]
    L.cjs_bzip2_shard_share_bytes.restype = S
    L.cjs_bzip2_shard_tiles.argtypes = [V, V, S, I, I, V]
    L.cjs_bzip2_shard_blocks.argtypes = [V, V, S, I, I, I, V, ctypes.POINTER(ShardMeta), ctypes.POINTER(Stats)]
    L.cjs_bzip2_shard_pack.argtypes = [V, I, I, I, ctypes.POINTER(ShardMeta), V, S, PS, PS, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.cjs_bzip2_recover.argtypes = [u8p, S, I, PP, PS, ctypes.POINTER(Found), ctypes.c_long, ctypes.POINTER(ctypes.c_long), V]
    L.cjs_bzip2_recover_device.argtypes = [V, S, I, V, S, PS, ctypes.POINTER(Found), ctypes.c_long, ctypes.POINTER(ctypes.c_long), V]
    PE, PU = ctypes.POINTER(IndexEntry), ctypes.POINTER(ctypes.c_uint64)
    L.cjs_bzip2_index_build.argtypes = [u8p, S, I, ctypes.POINTER(V), V]
    L.cjs_bzip2_index_create.argtypes = [PE, S, ctypes.c_uint64, I, ctypes.POINTER(V)]
    L.cjs_bzip2_index_save.argtypes = [V, PP, PS]
    L.cjs_bzip2_index_load.argtypes = [u8p, S, ctypes.POINTER(V)]
    L.cjs_bzip2_index_info.argtypes = [V, PU, PU, PU, ctypes.POINTER(I)]
    L.cjs_bzip2_index_entries.argtypes = [V, PE, ctypes.c_long]
    L.cjs_bzip2_index_entries.restype = ctypes.c_long
    L.cjs_bzip2_index_destroy.argtypes = [V]
    L.cjs_bzip2_index_destroy.restype = None
    L.cjs_bzip2_read_ranges.argtypes = [u8p, S, V, PU, PU, S, PP, PS, PS, ctypes.POINTER(ctypes.c_int32), V]
    L.cjs_bzip2_read_ranges_device.argtypes = [V, S, V, PU, PU, S, V, S, PS, PS, ctypes.POINTER(ctypes.c_int32), PS, V]
    U32, U64 = ctypes.c_uint32, ctypes.c_uint64
    L.cjs_bzip2_search.argtypes = [u8p, S, V, u8p, ctypes.POINTER(U32), U32, U32, U64, U64, ctypes.POINTER(Match), S, ctypes.POINTER(SearchInfo), V]
    L.cjs_bzip2_search_device.argtypes = [V, S, V, u8p, ctypes.POINTER(U32), U32, U32, U64, U64, ctypes.POINTER(Match), S, ctypes.POINTER(SearchInfo), V]
    L.cjs_bzip2_search_regex.argtypes = L.cjs_bzip2_search.argtypes
    L.cjs_bzip2_search_regex_device.argtypes = L.cjs_bzip2_search_device.argtypes
    L.cjs_regex_check.argtypes = [u8p, ctypes.POINTER(U32), U32, U32, ctypes.POINTER(U32), ctypes.POINTER(U32)]
    cmp_tail = [U64, U64, ctypes.POINTER(Diff), S, ctypes.POINTER(CompareInfo), V]
    L.cjs_bzip2_compare.argtypes = [u8p, S, V, u8p, S, U64] + cmp_tail
    L.cjs_bzip2_compare_device.argtypes = [V, S, V, V, S, U64] + cmp_tail
    L.cjs_bzip2_compare_streams.argtypes = [u8p, S, V, u8p, S, V] + cmp_tail
    L.cjs_bzip2_compare_streams_device.argtypes = [V, S, V, V, S, V] + cmp_tail
    PU32, PI32 = ctypes.POINTER(U32), ctypes.POINTER(ctypes.c_int32)
    L.cjs_bzip2_lines_build.argtypes = [u8p, S, V, ctypes.POINTER(V), V]
    L.cjs_bzip2_lines_build_device.argtypes = [V, S, V, ctypes.POINTER(V), V]
    L.cjs_bzip2_lines_create.argtypes = [V, PU32, S, ctypes.POINTER(V)]
    L.cjs_bzip2_lines_save.argtypes = [V, PP, PS]
    L.cjs_bzip2_lines_load.argtypes = [u8p, S, V, ctypes.POINTER(V)]
    L.cjs_bzip2_lines_info.argtypes = [V, PU, PU, PU]
    L.cjs_bzip2_lines_counts.argtypes = [V, PU32, ctypes.c_long]
    L.cjs_bzip2_lines_counts.restype = ctypes.c_long
    L.cjs_bzip2_lines_destroy.argtypes = [V]
    L.cjs_bzip2_lines_destroy.restype = None
    L.cjs_bzip2_lines_locate.argtypes = [u8p, S, V, V, PU, S, PU, PI32, V]
    L.cjs_bzip2_lines_locate_device.argtypes = [V, S, V, V, PU, S, PU, PI32, V]
    L.cjs_bzip2_lines_number.argtypes = [u8p, S, V, V, PU, S, PU, PI32, V]
    L.cjs_bzip2_lines_number_device.argtypes = [V, S, V, V, PU, S, PU, PI32, V]
    keys_tail = [V, V, U64, U64, U64, V, S, ctypes.POINTER(LineKeysInfo), V]
    L.cjs_bzip2_line_keys.argtypes = [u8p, S] + keys_tail
    L.cjs_bzip2_line_keys_device.argtypes = [V, S] + keys_tail
    L.cjs_line_keys_diff.argtypes = [V, S, V, S, U64, ctypes.POINTER(Hunk), S, ctypes.POINTER(LineDiffInfo)]
    tally_tail = [S, U32, U64, U64, V, S, ctypes.POINTER(TallyInfo)]
    L.cjs_keys_tally.argtypes = [V] + tally_tail + [V]
    L.cjs_keys_tally_device.argtypes = [V] + tally_tail + [V]
    L.cjs_stage_keys_tally.argtypes = [V] + tally_tail
    stream_tally_tail = [V, V, U64, U64, U64, U32, U32, V, U32, U32, U64, U64, V, S, ctypes.POINTER(StreamTallyInfo), V]
    L.cjs_bzip2_tally.argtypes = [u8p, S] + stream_tally_tail
    L.cjs_bzip2_tally_device.argtypes = [V, S] + stream_tally_tail
    PSI = ctypes.POINTER(SortInfo)
    L.cjs_text_sort.argtypes = [V, S, U32, V, V, S, PP, PS, PSI, V]
    L.cjs_text_sort_device.argtypes = [V, S, U32, V, V, S, V, S, PS, PSI, V]
    L.cjs_stage_text_sort.argtypes = [V, S, U32, V, V, S, PSI]
    sort_head = [V, V, U64, U64, U32, U32, V, U32, U32, V, V, S]
    L.cjs_bzip2_sort.argtypes = [u8p, S] + sort_head + [PP, PS, PSI, V]
    L.cjs_bzip2_sort_device.argtypes = [V, S] + sort_head + [V, S, PS, PSI, V]
    L.cjs_stage_bzip2_sort_limit.argtypes = [u8p, V, S, V, V, U64, U64, U64, U64, U32, V, V, S, PSI, V]
    cut_head = [V, V, U64, U64, U32, U32, V, U32]
    L.cjs_bzip2_cut.argtypes = [u8p, S] + cut_head + [PP, PS, ctypes.POINTER(CutInfo), V]
    L.cjs_bzip2_cut_device.argtypes = [V, S] + cut_head + [V, S, PS, ctypes.POINTER(CutInfo), V]
    L.cjs_stage_cut.argtypes = [V, S, U32, U32, V, U32, V, S, PS]
    L.cjs_cut_list_parse.argtypes = [ctypes.c_char_p, V, U32, PU32]
    L.cjs_bzip2_enc_create.argtypes = [ctypes.POINTER(V), I, S, V]
    L.cjs_bzip2_enc_write.argtypes = [V, V, S]
    L.cjs_bzip2_enc_finish.argtypes = [V]
    L.cjs_bzip2_enc_pending.argtypes = [V]
    L.cjs_bzip2_enc_pending.restype = S
    L.cjs_bzip2_enc_read.argtypes = [V, V, S, PS]
    L.cjs_bzip2_enc_destroy.argtypes = [V]
    L.cjs_bzip2_enc_destroy.restype = None
    L.cjs_bzip2_enc_index.argtypes = [V, ctypes.POINTER(V), ctypes.POINTER(V)]
    L.cjs_bzip2_compress_indexed.argtypes = [u8p, S, I, PP, PS, ctypes.POINTER(V), ctypes.POINTER(V), V]
    L.cjs_bzip2_compress_device_indexed.argtypes = [V, V, S, I, V, S, PS, ctypes.POINTER(V), ctypes.POINTER(V), ctypes.POINTER(Stats)]
    L.cjs_bzip2_dec_create.argtypes = [ctypes.POINTER(V), I, S, S, V]
    L.cjs_bzip2_dec_write.argtypes = [V, V, S, PS]
    L.cjs_bzip2_dec_finish.argtypes = [V]
    L.cjs_bzip2_dec_read.argtypes = [V, V, S, PS]
    L.cjs_bzip2_dec_done.argtypes = [V]
    L.cjs_bzip2_dec_destroy.argtypes = [V]
    L.cjs_bzip2_dec_destroy.restype = None
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        L = load_library()
        detail = L.cjs_last_error_detail().decode()          # the reference's optDetail (J/Bzip2_joined_.js:1385-1391)
        raise CjsError(rc, L.cjs_strerror(rc).decode() + (": " + detail if detail else ""))


def _coerce_input(data):
    # Util.coerceInputStream (J/Bzip2_joined_.js:178-220): anything indexable with a length
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(data), dtype=np.uint8)
    return np.ascontiguousarray(data, dtype=np.uint8)


def _adopt(out, n):
    """the library's malloc'd result as a uint8 ndarray without a copy; cjs_free runs when the array is collected
    (what the N-API addon does with an external ArrayBuffer and a finalizer)"""
    L = load_library()
    if not n:
        L.cjs_free(out)
        return np.empty(0, np.uint8)
    addr = ctypes.cast(out, ctypes.c_void_p).value
    buf = (ctypes.c_uint8 * n).from_address(addr)
    weakref.finalize(buf, L.cjs_free, ctypes.c_void_p(addr))
    return np.frombuffer(buf, dtype=np.uint8)


def _stream_call(fn, data, *mid):
    data = _coerce_input(data)
    keep = data if data.size else np.zeros(1, dtype=np.uint8)
    out, out_n = u8p(), ctypes.c_size_t(0)
    _check(fn(keep.ctypes.data_as(u8p), data.size, *mid, ctypes.byref(out), ctypes.byref(out_n), None))
    return _adopt(out, out_n.value)


def _bzip2_level(props):
    # Q17: typeof props === 'number' -> the level, anything else -> 9 (5.0 is the number 5 in JavaScript)
    level = props if isinstance(props, (int, float)) and not isinstance(props, bool) else 9
    if isinstance(level, float) and level == int(level):
        level = int(level)
    if level < 1 or level > 9 or not isinstance(level, int):      # (a fractional level is meaningless; the reference does not guard it)
        raise CjsError(-20, "Invalid block size multiplier")
    return level


class Bzip2:
    """Same surface as the reference's `Bzip2` object for the hot path (returns a uint8 ndarray)."""

    @staticmethod
    def compressFile(input, output=None, props=None):
        res = _stream_call(load_library().cjs_bzip2_compress, input, _bzip2_level(props))
        return _deliver(res, output)

    @staticmethod
    def compressIndexed(input, props=None, lines=True, n_devices=0):
        """compressFile that also hands out the tables of its stream (cjs_bzip2_compress_indexed): (stream, Bzip2Index,
        Bzip2Lines or None).  The stream is compressFile's; the tables are what Bzip2Index.build / Bzip2Lines.build give on it,
        without their table pass and full decode.  n_devices: cjs_opts.n_devices (0: one GPU, or CJS_DEVICES)."""
        L = load_library()
        level = _bzip2_level(props)
        data = _coerce_input(input)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        out, out_n = u8p(), ctypes.c_size_t(0)
        hi, hl = ctypes.c_void_p(), ctypes.c_void_p()
        opts = _Opts(ctypes.sizeof(_Opts), -1, n_devices, 0, None)
        _check(L.cjs_bzip2_compress_indexed(keep.ctypes.data_as(u8p), data.size, level, ctypes.byref(out), ctypes.byref(out_n), ctypes.byref(hi),
                                            ctypes.byref(hl) if lines else None, ctypes.byref(opts)))
        return _adopt(out, out_n.value), Bzip2Index(hi), Bzip2Lines(hl) if lines else None

    @staticmethod
    def compressFiles(inputs, props=None):
        """compressFile over a batch: one uint8 ndarray (a .bz2 stream) per input, in input order, all inputs in one pass
        per stage on the GPU (cjs_bzip2_compress_batch).  The streams are views of one result buffer."""
        level = _bzip2_level(props)
        arrs = [_coerce_input(x) for x in inputs]
        L = load_library()
        count = len(arrs)
        ptrs = (u8p * max(count, 1))(*[a.ctypes.data_as(u8p) for a in arrs])
        lens = (ctypes.c_size_t * max(count, 1))(*[a.size for a in arrs])
        off = (ctypes.c_size_t * max(count, 1))()
        ln = (ctypes.c_size_t * max(count, 1))()
        out = u8p()
        _check(L.cjs_bzip2_compress_batch(ptrs, lens, count, level, ctypes.byref(out), off, ln, None))
        if not count:
            return []
        total = max(off[k] + ln[k] for k in range(count))
        buf = _adopt(out, total)
        return [buf[off[k]: off[k] + ln[k]] for k in range(count)]

    @staticmethod
    def compressStream(chunks, props=None, chunk_bytes=0):
        """compressFile over an iterable of byte chunks, in bounded memory: a generator of uint8 ndarrays, the pieces of the
        .bz2 stream as they become ready; joined they are compressFile(all chunks joined, None, props)."""
        level = _bzip2_level(props)

        def gen():
            with Bzip2Encoder(level, chunk_bytes) as enc:
                for c in chunks:
                    enc.write(c)
                    if enc.pending:
                        yield enc.read()
                enc.finish()
                if enc.pending:
                    yield enc.read()
        return gen()

    @staticmethod
    def decompressFile(input, output=None, multistream=False):
        res = _stream_call(load_library().cjs_bzip2_decompress, input, 1 if multistream else 0)
        return _deliver(res, output)

    @staticmethod
    def decompressStream(chunks, multistream=False, chunk_bytes=0, out_bytes=0):
        """decompressFile over an iterable of pieces of a .bz2 stream, in bounded memory: a generator of uint8 ndarrays, the
        decoded bytes as they become ready; joined they are decompressFile(all chunks joined, None, multistream).  A stream
        that fails raises decompressFile's error once every block in front of the failure has been yielded."""
        def gen():
            with Bzip2Decoder(multistream, chunk_bytes, out_bytes) as dec:
                def drain():
                    while True:
                        piece = dec.read(_DEC_READ_BYTES)
                        if not piece.size:
                            return
                        yield piece
                for c in chunks:
                    a = _coerce_input(c)
                    while a.size:
                        took = dec.write(a)
                        a = a[took:]
                        if a.size:                  # the window is full: after a drain the next write takes at least a byte
                            yield from drain()
                    yield from drain()
                dec.finish()
                yield from drain()
        return gen()

    @staticmethod
    def decompressFiles(inputs, multistream=False):
        """decompressFile over a batch: one uint8 ndarray per input, in input order, decoded in shared GPU passes
        (cjs_bzip2_decompress_batch); views of one result buffer.  If an input fails, CjsError for the lowest-index one,
        with decompressFile's message for it and the attribute `index`."""
        arrs = [_coerce_input(x) for x in inputs]
        L = load_library()
        count = len(arrs)
        if not count:
            return []
        ptrs = (u8p * count)(*[a.ctypes.data_as(u8p) for a in arrs])
        lens = (ctypes.c_size_t * count)(*[a.size for a in arrs])
        off = (ctypes.c_size_t * count)()
        ln = (ctypes.c_size_t * count)()
        status = (ctypes.c_int32 * count)()
        out = u8p()
        _check(L.cjs_bzip2_decompress_batch(ptrs, lens, count, 1 if multistream else 0, ctypes.byref(out), off, ln, status, None))
        total = max(off[k] + ln[k] for k in range(count))
        buf = _adopt(out, total)
        for k in range(count):
            if status[k]:
                detail = L.cjs_last_error_detail().decode()
                e = CjsError(status[k], L.cjs_strerror(status[k]).decode() + (": " + detail if detail else ""))
                e.index = k
                raise e
        return [buf[off[k]: off[k] + ln[k]] for k in range(count)]


    @staticmethod
    def recoverFile(input, output=None, as_stream=False):
        """What bzip2recover is for (cjs_bzip2_recover): the intact blocks of damaged .bz2 data -- any bytes, no header needed --
        as their decoded bytes, or with as_stream as a repaired single-stream .bz2.  Returns (data, found): found has one
        (bitpos, end_bit, out_off, size, status, crc) per block magic in the input, ascending; status 0 = recovered,
        REC_SHADOWED = a false magic inside a recovered block, else the block's error code."""
        L = load_library()
        data = _coerce_input(input)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)

        def call(cap):
            out, out_n, nf = u8p(), ctypes.c_size_t(0), ctypes.c_long(0)
            found = (Found * cap)()
            _check(L.cjs_bzip2_recover(keep.ctypes.data_as(u8p), data.size, 1 if as_stream else 0, ctypes.byref(out), ctypes.byref(out_n),
                                       found, cap, ctypes.byref(nf), None))
            return _adopt(out, out_n.value), found, nf.value
        return _deliver_found(call, data.size, output)


class Bzip2Encoder:
    """Streaming Bzip2.compressFile (cjs_bzip2_enc_*): write() input in pieces of any size, read() the stream in pieces; after
    finish() the bytes read are those of compressFile over everything written.  The device and pinned memory it holds depend
    on chunk_bytes (0: the library's default) and level, not on the bytes written.  One worker thread runs the GPU steps.
    index / lines: the encoder keeps the block index (and the line table) of the stream it writes, 36 bytes of host memory per
    block; index() hands them out after finish()."""

    ENC_INDEX, ENC_LINES = 4, 8          # CJS_FLAG_ENC_INDEX, CJS_FLAG_ENC_LINES

    def __init__(self, level=9, chunk_bytes=0, device=-1, index=False, lines=False):
        self.L = load_library()
        self.h = ctypes.c_void_p()
        self._lines = bool(lines)
        flags = (self.ENC_INDEX if index or lines else 0) | (self.ENC_LINES if lines else 0)
        opts = _Opts(ctypes.sizeof(_Opts), device, 0, flags, None)
        _check(self.L.cjs_bzip2_enc_create(ctypes.byref(self.h), level, chunk_bytes, ctypes.byref(opts)))

    def index(self):
        """(Bzip2Index, Bzip2Lines or None) of the finished stream (cjs_bzip2_enc_index)"""
        hi, hl = ctypes.c_void_p(), ctypes.c_void_p()
        _check(self.L.cjs_bzip2_enc_index(self.h, ctypes.byref(hi), ctypes.byref(hl) if self._lines else None))
        return Bzip2Index(hi), Bzip2Lines(hl) if self._lines else None

    def write(self, data):
        a = _coerce_input(data)
        _check(self.L.cjs_bzip2_enc_write(self.h, a.ctypes.data if a.size else None, a.size))

    def finish(self):
        _check(self.L.cjs_bzip2_enc_finish(self.h))

    @property
    def pending(self):
        """output bytes read() can hand out now"""
        return self.L.cjs_bzip2_enc_pending(self.h)

    def read(self, max_bytes=None):
        n = self.pending if max_bytes is None else min(int(max_bytes), self.pending)
        out = np.empty(n, dtype=np.uint8)
        got = ctypes.c_size_t(0)
        _check(self.L.cjs_bzip2_enc_read(self.h, out.ctypes.data if n else None, n, ctypes.byref(got)))
        return out[: got.value]

    def close(self):
        if self.h:
            self.L.cjs_bzip2_enc_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_DEC_READ_BYTES = 16 << 20      # piece size of decompressStream


class Bzip2Decoder:
    """Streaming Bzip2.decompressFile (cjs_bzip2_dec_*), a pull model: write() takes as much of a piece of the .bz2 stream as
    the input window has room for and returns the count; read(max_bytes) hands out decoded bytes and is what runs the GPU steps.
    An empty read means "write more, or finish()"; after finish() it means the stream has ended (`done`).  After a write that
    took less than it was given, reading until an empty read guarantees that the next write takes at least a byte.  The bytes
    read are those of decompressFile over everything written, and a stream that fails raises the same error from read() once
    the blocks in front of the failure have been read.  The memory held depends on chunk_bytes and out_bytes (0: the library's
    defaults), not on the bytes written or produced."""

    def __init__(self, multistream=False, chunk_bytes=0, out_bytes=0, device=-1):
        self.L = load_library()
        self.h = ctypes.c_void_p()
        opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
        _check(self.L.cjs_bzip2_dec_create(ctypes.byref(self.h), 1 if multistream else 0, chunk_bytes, out_bytes, ctypes.byref(opts)))

    def write(self, data):
        a = _coerce_input(data)
        taken = ctypes.c_size_t(0)
        _check(self.L.cjs_bzip2_dec_write(self.h, a.ctypes.data if a.size else None, a.size, ctypes.byref(taken)))
        return taken.value

    def finish(self):
        _check(self.L.cjs_bzip2_dec_finish(self.h))

    def read(self, max_bytes):
        n = int(max_bytes)
        out = np.empty(n, dtype=np.uint8)
        got = ctypes.c_size_t(0)
        _check(self.L.cjs_bzip2_dec_read(self.h, out.ctypes.data if n else None, n, ctypes.byref(got)))
        return out[: got.value]

    @property
    def done(self):
        """the stream has ended and every byte has been read"""
        return bool(self.h) and self.L.cjs_bzip2_dec_done(self.h) == 1

    def close(self):
        if self.h:
            self.L.cjs_bzip2_dec_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BWTC:
    MAGIC = "bwtc"

    @staticmethod
    def compressFile(input, output=None, props=None):
        level = int(props) if isinstance(props, (int, float)) and not isinstance(props, bool) and 1 <= props <= 9 and props == int(props) else 9   # W2
        return _deliver(_stream_call(load_library().cjs_bwtc_compress, input, level), output)

    @staticmethod
    def decompressFile(input, output=None):
        L = load_library()
        data = _coerce_input(input)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        out, out_n = u8p(), ctypes.c_size_t(0)
        _check(L.cjs_bwtc_decompress(keep.ctypes.data_as(u8p), data.size, ctypes.byref(out), ctypes.byref(out_n), None))
        return _deliver(_adopt(out, out_n.value), output)


def _deliver(res, output):
    # Util.coerceOutputStream (J/Bzip2_joined_.js:254-272)
    if output is None:
        return res
    if isinstance(output, int):
        if output != res.size:
            raise TypeError("outputsize does not match decoded input")
        return res
    if hasattr(output, "writeByte"):
        for b in res.tolist():
            output.writeByte(b)
        return output
    if len(output) != res.size:
        raise TypeError("outputsize does not match decoded input")
    output[:] = res
    return output


class DeviceContext:
    """Per-GPU workspace + stream for the device-resident pipeline (what bench.py times)."""

    def __init__(self, device, max_input, level, max_range_blocks=0):
        self.L = load_library()
        self.h = ctypes.c_void_p()
        self.level = level
        _check(self.L.cjs_ctx_create_sharded(ctypes.byref(self.h), device, max_input, max_range_blocks, level))

    def set_stage_times(self, on):
        """stats of later calls: per-stage times (a stream synchronisation per stage) or events only"""
        self.L.cjs_ctx_set_stage_times(self.h, 1 if on else 0)

    @classmethod
    def batch(cls, device, max_input, max_items, level):
        """context of the batch path (compress_batch): batches of up to max_input bytes and max_items inputs per pass"""
        self = cls.__new__(cls)
        self.L = load_library()
        self.h = ctypes.c_void_p()
        self.level = level
        _check(self.L.cjs_ctx_create_batch(ctypes.byref(self.h), device, max_input, max_items, level))
        return self

    def compress_batch(self, d_in_ptr, in_off, d_out_ptr, out_cap):
        """input k = d_in[in_off[k] .. in_off[k+1]) (device memory; in_off on the host) -> (out_off, out_len) uint64 arrays:
        stream k is left at d_out + out_off[k], out_len[k] bytes"""
        o = np.ascontiguousarray(in_off, dtype=np.uint64)
        count = max(o.size - 1, 0)
        off = np.zeros(max(count, 1), dtype=np.uint64)
        ln = np.zeros(max(count, 1), dtype=np.uint64)
        PS = ctypes.POINTER(ctypes.c_size_t)
        keep = o if o.size else np.zeros(1, dtype=np.uint64)
        _check(self.L.cjs_bzip2_compress_batch_device(self.h, d_in_ptr, keep.ctypes.data_as(PS), count, self.level, d_out_ptr, out_cap,
                                                      off.ctypes.data_as(PS), ln.ctypes.data_as(PS)))
        return off[:count], ln[:count]

    def close(self):
        if self.h:
            self.L.cjs_ctx_destroy(self.h)
            self.h = ctypes.c_void_p()

    def compress(self, d_in_ptr, n, d_out_ptr, out_cap, stats=None):
        out_n = ctypes.c_size_t(0)
        _check(self.L.cjs_bzip2_compress_device(self.h, d_in_ptr, n, self.level, d_out_ptr, out_cap, ctypes.byref(out_n),
                                                ctypes.byref(stats) if stats is not None else None))
        return out_n.value

    def compress_indexed(self, d_in_ptr, n, d_out_ptr, out_cap, lines=True, stats=None):
        """compress, and the tables of the stream it left at d_out (cjs_bzip2_compress_device_indexed): (out_n, Bzip2Index,
        Bzip2Lines or None)"""
        out_n = ctypes.c_size_t(0)
        hi, hl = ctypes.c_void_p(), ctypes.c_void_p()
        _check(self.L.cjs_bzip2_compress_device_indexed(self.h, d_in_ptr, n, self.level, d_out_ptr, out_cap, ctypes.byref(out_n), ctypes.byref(hi),
                                                        ctypes.byref(hl) if lines else None, ctypes.byref(stats) if stats is not None else None))
        return out_n.value, Bzip2Index(hi), Bzip2Lines(hl) if lines else None

    def compress_range(self, d_in_ptr, n, first, count, d_out_ptr, out_cap, stats=None, crc_cap=1 << 16):
        bits = ctypes.c_uint64(0)
        total = ctypes.c_long(0)
        crcs = np.zeros(crc_cap, dtype=np.uint32)
        _check(self.L.cjs_bzip2_compress_device_range(self.h, d_in_ptr, n, self.level, first, count, d_out_ptr, out_cap,
                                                      ctypes.byref(bits), crcs.ctypes.data, crc_cap, ctypes.byref(total),
                                                      ctypes.byref(stats) if stats is not None else None))
        return bits.value, total.value, crcs[: total.value]


    # ---- the three phases of a one-process-per-GPU job (include/cjs_hip.h); the caller owns the exchange between them
    def share_bytes(self, n, world):
        return self.L.cjs_bzip2_shard_share_bytes(n, world)

    def shard_tiles(self, d_in_ptr, n, rank, world, d_share_ptr):
        _check(self.L.cjs_bzip2_shard_tiles(self.h, d_in_ptr, n, rank, world, d_share_ptr))

    def shard_blocks(self, d_in_ptr, n, rank, world, d_shares_ptr, stats=None):
        meta = ShardMeta()
        _check(self.L.cjs_bzip2_shard_blocks(self.h, d_in_ptr, n, self.level, rank, world, d_shares_ptr, ctypes.byref(meta),
                                             ctypes.byref(stats) if stats is not None else None))
        return meta

    def shard_pack(self, rank, metas, d_out_ptr, out_cap):
        """-> (frag_off, frag_len, stream_off, stream_len): bytes [frag_off, +frag_len) of d_out are stream bytes [stream_off, +frag_len)"""
        arr = (ShardMeta * len(metas))(*metas)
        fo, fl = ctypes.c_size_t(0), ctypes.c_size_t(0)
        so, sl = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(self.L.cjs_bzip2_shard_pack(self.h, self.level, rank, len(metas), arr, d_out_ptr, out_cap, ctypes.byref(fo), ctypes.byref(fl),
                                           ctypes.byref(so), ctypes.byref(sl)))
        return fo.value, fl.value, so.value, sl.value


class _Opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("device", ctypes.c_int32), ("n_devices", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("stats", ctypes.c_void_p)]


def decompress_device(d_in_ptr, n, d_out_ptr, out_cap, multistream=False, device=-1):
    """Bzip2.decompressFile with the stream and the result in GPU memory (cjs_bzip2_decompress_device): d_in_ptr / d_out_ptr are
    device addresses (e.g. tensor.data_ptr()) on `device` (-1: the current one).  Returns the bytes written.  Raises CjsError with
    decompressFile's message; on CJS_E_OUTPUT_TOO_SMALL (-33) the error carries `need`, the bytes the result takes."""
    L = load_library()
    out_n = ctypes.c_size_t(0)
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    rc = L.cjs_bzip2_decompress_device(d_in_ptr, n, 1 if multistream else 0, d_out_ptr, out_cap, ctypes.byref(out_n), ctypes.byref(opts))
    if rc == -33:
        e = CjsError(rc, L.cjs_strerror(rc).decode())
        e.need = out_n.value
        raise e
    _check(rc)
    return out_n.value


def _found_cap(n):
    return n // 64 + 1024      # (a block takes a few dozen bytes at least; more magics than that: one more call)


def _found_list(found, count):
    return [(f.bitpos, f.end_bit, f.out_off, f.size, f.status, f.crc) for f in found[:count]]


def _deliver_found(call, n, output):
    res, found, nf = call(_found_cap(n))
    if nf > len(found):
        res, found, nf = call(nf)
    return _deliver(res, output), _found_list(found, nf)


def recover_device(d_in_ptr, n, d_out_ptr, out_cap, as_stream=False, device=-1):
    """Bzip2.recoverFile with the damaged data and the result in GPU memory (cjs_bzip2_recover_device; the memory rules of
    decompress_device).  Returns (out_n, found).  On CJS_E_OUTPUT_TOO_SMALL (-33) the CjsError carries `need`, the bytes the
    result takes, and `found`; out_cap = 0 with d_out_ptr = None is the size query."""
    L = load_library()
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    cap = _found_cap(n)
    while True:
        out_n, nf = ctypes.c_size_t(0), ctypes.c_long(0)
        found = (Found * cap)()
        rc = L.cjs_bzip2_recover_device(d_in_ptr, n, 1 if as_stream else 0, d_out_ptr, out_cap, ctypes.byref(out_n), found, cap,
                                        ctypes.byref(nf), ctypes.byref(opts))
        if rc in (0, -33) and nf.value > cap:
            cap = nf.value
            continue
        break
    if rc == -33:
        e = CjsError(rc, L.cjs_strerror(rc).decode())
        e.need = out_n.value
        e.found = _found_list(found, nf.value)
        raise e
    _check(rc)
    return out_n.value, _found_list(found, nf.value)


def decompress_batch_device(d_in_ptr, in_off, d_out_ptr, out_cap, multistream=False, device=-1):
    """decompressFiles with the inputs and the result in GPU memory (cjs_bzip2_decompress_batch_device): input k is
    d_in[in_off[k] .. in_off[k+1]) (in_off on the host).  -> (out_off, out_len, status, detail): uint64 / int32 arrays (input k's
    bytes at d_out + out_off[k]) and the lowest-index failing input's detail ("" if none).  Per-input failures are in status;
    CjsError for a failure of the call, with `need` on CJS_E_OUTPUT_TOO_SMALL (-33)."""
    L = load_library()
    o = np.ascontiguousarray(in_off, dtype=np.uint64)
    count = max(o.size - 1, 0)
    PS = ctypes.POINTER(ctypes.c_size_t)
    keep = o if o.size else np.zeros(1, dtype=np.uint64)
    off = np.zeros(max(count, 1), dtype=np.uint64)
    ln = np.zeros(max(count, 1), dtype=np.uint64)
    st = np.zeros(max(count, 1), dtype=np.int32)
    need = ctypes.c_size_t(0)
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    rc = L.cjs_bzip2_decompress_batch_device(d_in_ptr, keep.ctypes.data_as(PS), count, 1 if multistream else 0, d_out_ptr, out_cap,
                                             off.ctypes.data_as(PS), ln.ctypes.data_as(PS), st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                             ctypes.byref(need), ctypes.byref(opts))
    if rc == -33:
        e = CjsError(rc, L.cjs_strerror(rc).decode())
        e.need = need.value
        raise e
    _check(rc)
    detail = L.cjs_last_error_detail().decode() if st[:count].any() else ""
    return off[:count], ln[:count], st[:count], detail


def _range_arrays(ranges):
    r = np.asarray(list(ranges), dtype=np.uint64).reshape(-1, 2)
    count = r.shape[0]
    off = np.ascontiguousarray(r[:, 0]) if count else np.zeros(1, dtype=np.uint64)
    ln = np.ascontiguousarray(r[:, 1]) if count else np.zeros(1, dtype=np.uint64)
    return count, off, ln, np.zeros(max(count, 1), dtype=np.uint64), np.zeros(max(count, 1), dtype=np.uint64), np.zeros(max(count, 1), dtype=np.int32)


class Bzip2Index:
    """The block index of a .bz2 stream (cjs_bz_index) and the range reads over it: bytes [off, off + length) of what
    Bzip2.decompressFile(data, multistream) returns, decoding only the blocks they touch (cjs_bzip2_read_ranges).  Made by
    build() (one table pass on the GPU), load() (the serialised form save() returns) or create() (a caller's entries)."""

    def __init__(self, handle):
        self._h = handle
        self._fin = weakref.finalize(self, load_library().cjs_bzip2_index_destroy, handle)

    @staticmethod
    def build(data, multistream=False):
        L = load_library()
        data = _coerce_input(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        h = ctypes.c_void_p()
        _check(L.cjs_bzip2_index_build(keep.ctypes.data_as(u8p), data.size, 1 if multistream else 0, ctypes.byref(h), None))
        return Bzip2Index(h)

    @staticmethod
    def load(raw):
        L = load_library()
        raw = _coerce_input(raw)
        keep = raw if raw.size else np.zeros(1, dtype=np.uint8)
        h = ctypes.c_void_p()
        _check(L.cjs_bzip2_index_load(keep.ctypes.data_as(u8p), raw.size, ctypes.byref(h)))
        return Bzip2Index(h)

    @staticmethod
    def create(entries, stream_bytes, multistream=False):
        """entries: (bitpos, end_bit, size, crc, level[, reserved]) per block, in stream order"""
        L = load_library()
        entries = list(entries)
        arr = (IndexEntry * max(len(entries), 1))()
        for k, e in enumerate(entries):
            arr[k] = IndexEntry(*e)
        h = ctypes.c_void_p()
        _check(L.cjs_bzip2_index_create(arr, len(entries), stream_bytes, 1 if multistream else 0, ctypes.byref(h)))
        return Bzip2Index(h)

    def save(self):
        L = load_library()
        out, out_n = u8p(), ctypes.c_size_t(0)
        _check(L.cjs_bzip2_index_save(self._h, ctypes.byref(out), ctypes.byref(out_n)))
        raw = ctypes.string_at(out, out_n.value)
        L.cjs_free(out)
        return raw

    def _info(self):
        b, t, sb, m = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
        _check(load_library().cjs_bzip2_index_info(self._h, ctypes.byref(b), ctypes.byref(t), ctypes.byref(sb), ctypes.byref(m)))
        return b.value, t.value, sb.value, bool(m.value)

    blocks = property(lambda self: self._info()[0])
    total = property(lambda self: self._info()[1])
    stream_bytes = property(lambda self: self._info()[2])
    multistream = property(lambda self: self._info()[3])

    def entries(self):
        """[(bitpos, end_bit, size, crc, level)] per block"""
        nb = self.blocks
        arr = (IndexEntry * max(nb, 1))()
        load_library().cjs_bzip2_index_entries(self._h, arr, nb)
        return [(e.bitpos, e.end_bit, e.size, e.crc, e.level) for e in arr[:nb]]

    def read_ranges_raw(self, data, ranges):
        """cjs_bzip2_read_ranges as it is: (buffer, out_off, out_len, status, detail) for ranges = [(off, length)]"""
        L = load_library()
        data = _coerce_input(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        count, off, ln, o_off, o_len, st = _range_arrays(ranges)
        PU, PS = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t)
        out = u8p()
        _check(L.cjs_bzip2_read_ranges(keep.ctypes.data_as(u8p), data.size, self._h, off.ctypes.data_as(PU), ln.ctypes.data_as(PU), count,
                                       ctypes.byref(out), o_off.ctypes.data_as(PS), o_len.ctypes.data_as(PS),
                                       st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None))
        detail = L.cjs_last_error_detail().decode() if st[:count].any() else ""
        return _adopt(out, int(o_len[:count].sum())), o_off[:count], o_len[:count], st[:count], detail

    def read_ranges(self, data, ranges):
        """-> per range its bytes, or a CjsError (the lowest-index failing range's carries the detail)"""
        L = load_library()
        buf, o_off, o_len, st, detail = self.read_ranges_raw(data, ranges)
        res = []
        for k in range(len(st)):
            if st[k]:
                msg = L.cjs_strerror(int(st[k])).decode()
                res.append(CjsError(int(st[k]), msg + (": " + detail if detail else "")))
                detail = ""
            else:
                res.append(buf[int(o_off[k]):int(o_off[k] + o_len[k])].tobytes())
        return res

    def read(self, data, off, length):
        r = self.read_ranges(data, [(off, length)])[0]
        if isinstance(r, CjsError):
            raise r
        return r

    def search(self, data, patterns, off=0, length=None, nocase=False, limit=None):
        """Where `patterns` (bytes-likes or str) occur in [off, off + length) of the decoded bytes, found on the GPU
        (cjs_bzip2_search): -> SearchResult.  limit=None counts first and then fetches every match."""
        L = load_library()
        data = _coerce_input(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        return _search(lambda *a: L.cjs_bzip2_search(keep.ctypes.data_as(u8p), data.size, self._h, *a, None), patterns, off, length, nocase, limit)

    def search_regex(self, data, patterns, off=0, length=None, nocase=False, limit=None):
        """search with patterns that are bounded regular expressions (cjs_bzip2_search_regex: the dialect and the 256-byte clamp
        are described there): -> SearchResult whose matches are (off, pattern, length) triples, length the longest match there."""
        L = load_library()
        data = _coerce_input(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        return _search(lambda *a: L.cjs_bzip2_search_regex(keep.ctypes.data_as(u8p), data.size, self._h, *a, None), patterns, off, length, nocase, limit, lengths=True)

    def grep(self, data, patterns, before=0, after=0, regex=False, **kw):
        """search, then one read_ranges of [o - before, o + len(pattern) + after) per match: -> [(off, pattern, bytes)] (a
        CjsError in place of the bytes of a context that touches a bad block).  regex=True: search_regex, and the match's own
        length in the pattern's place."""
        if regex:
            res = self.search_regex(data, patterns, **kw)
            ranges = [(max(o - before, 0), min(o, before) + n + after) for o, j, n in res.matches]
            ctx = self.read_ranges(data, ranges) if ranges else []
            return [(o, j, c) for (o, j, n), c in zip(res.matches, ctx)]
        pats = _pattern_arrays(patterns)[0]
        res = self.search(data, patterns, **kw)
        ranges = [(max(o - before, 0), min(o, before) + len(pats[j]) + after) for o, j in res.matches]
        ctx = self.read_ranges(data, ranges) if ranges else []
        return [(o, j, c) for (o, j), c in zip(res.matches, ctx)]

    def compare(self, data, other, off=0, length=None, other_off=0, limit=64):
        """cmp on the GPU (cjs_bzip2_compare): other[k] against decoded byte other_off + k, inside [off, off + length): ->
        CompareResult with at most `limit` differences.  limit=None counts first and then fetches every difference."""
        L = load_library()
        data, other = _coerce_input(data), _coerce_input(other)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        keep2 = other if other.size else np.zeros(1, dtype=np.uint8)
        return _compare(lambda *a: L.cjs_bzip2_compare(keep.ctypes.data_as(u8p), data.size, self._h, keep2.ctypes.data_as(u8p), other.size, int(other_off), *a, None),
                        off, length, limit, self.total, int(other_off) + other.size)

    def compare_stream(self, data, other_data, other_index, off=0, length=None, limit=64):
        """bzcmp on the GPU (cjs_bzip2_compare_streams): this stream against the stream `other_data` of `other_index`"""
        L = load_library()
        data, other = _coerce_input(data), _coerce_input(other_data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        keep2 = other if other.size else np.zeros(1, dtype=np.uint8)
        return _compare(lambda *a: L.cjs_bzip2_compare_streams(keep.ctypes.data_as(u8p), data.size, self._h, keep2.ctypes.data_as(u8p), other.size, other_index._h, *a, None),
                        off, length, limit, self.total, other_index.total)

    def line_starts(self, data, lines, line_numbers):
        """start(k) of every line number (cjs_bzip2_lines_locate): -> (starts, status, detail), uint64 / int32 arrays"""
        L = load_library()
        data = _coerce_input(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        return _lines_ask(lambda *a: L.cjs_bzip2_lines_locate(keep.ctypes.data_as(u8p), data.size, self._h, lines._h, *a, None), line_numbers)

    def line_numbers(self, data, lines, offsets):
        """number(o) of every decoded offset (cjs_bzip2_lines_number): -> (numbers, status, detail)"""
        L = load_library()
        data = _coerce_input(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        return _lines_ask(lambda *a: L.cjs_bzip2_lines_number(keep.ctypes.data_as(u8p), data.size, self._h, lines._h, *a, None), offsets)

    def read_lines(self, data, lines, spans):
        """spans = [(first, count)]: lines first .. first + count - 1, newlines included -- one locate of 2 * len(spans)
        questions, then one read_ranges.  -> per span its bytes, or a CjsError for a span that touches a bad block"""
        L = load_library()
        spans = [(int(a), int(c)) for a, c in spans]
        if not spans:
            return []
        ask = [min(x, 2 ** 64 - 1) for a, c in spans for x in (a, a + c)]
        at, st, detail = self.line_starts(data, lines, ask)
        res = [None] * len(spans)
        ranges, where = [], []
        for k in range(len(spans)):
            bad = int(st[2 * k]) or int(st[2 * k + 1])
            if bad:
                res[k] = CjsError(bad, L.cjs_strerror(bad).decode() + (": " + detail if detail else ""))
                detail = ""
            else:
                ranges.append((int(at[2 * k]), int(at[2 * k + 1]) - int(at[2 * k])))
                where.append(k)
        for k, r in zip(where, self.read_ranges(data, ranges) if ranges else []):
            res[k] = r
        return res

    def line_keys(self, data, lines, first=0, count=None, seed=0):
        """The keys of lines [first, first + count) (count=None: to the last), hashed on the GPU (cjs_bzip2_line_keys): ->
        (keys, info): a structured array of (hash, len, check) per line, all-ones for a line that touches a bad block, and a
        LineKeysResult.  The bases follow from `seed` alone: against crafted input pass a seed of your own."""
        L = load_library()
        data = _coerce_input(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        return _line_keys(lambda *a: L.cjs_bzip2_line_keys(keep.ctypes.data_as(u8p), data.size, self._h, lines._h, *a, None), first, count, seed)

    def cut_lines(self, data, lines, fields=None, bytes=None, delimiter=b"\t", first=0, count=None):
        """`bzcat | cut -f LIST -d D` / `cut -b LIST` over lines [first, first + count) (count=None: to the last), selected and
        packed on the GPU (cjs_bzip2_cut) -> bytes.  Exactly one of fields / bytes: a cut-style string ("1,3-5,7-"), or a list of
        ints and (lo, hi) pairs (hi=None: to the end of the line).  A line without the delimiter is a line of one field (GNU cut
        prints it whole).  A bad block inside the window: CjsError(CJS_E_DATA_ERROR)."""
        L = load_library()
        mode, d, sel = _cut_args(fields, bytes, delimiter)
        data = _coerce_input(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        out, out_n, info = u8p(), ctypes.c_size_t(0), CutInfo()
        _check(L.cjs_bzip2_cut(keep.ctypes.data_as(u8p), data.size, self._h, lines._h, int(first), 2 ** 64 - 1 if count is None else int(count), mode, d,
                               sel.ctypes.data, sel.size, ctypes.byref(out), ctypes.byref(out_n), ctypes.byref(info), None))
        return _adopt(out, out_n.value).tobytes()

    def tally_lines(self, data, lines, fields=None, bytes=None, delimiter=b"\t", first=0, count=None, seed=0, order="count", min_count=1, max_count=0,
                    limit=None):
        """`bzcat | sort | uniq -c | sort -rn | head` over lines [first, first + count) (count=None: to the last): the lines' keys
        are made and grouped on the GPU (cjs_bzip2_tally), only the groups come down -> TallyResult.  order="count": descending
        count, ties by first occurrence; "first": by first occurrence.  min_count=2 is `uniq -d`, max_count=1 is `uniq -u`;
        limit: the first so many groups (None: all).  A group's `first` is the number of its first line.  A tail line without a
        newline counts as if it had one; an empty tail is no line.  Lines that touch a bad block are counted in n_bad_lines and
        grouped nowhere.  fields / bytes (one of them, with delimiter, as in cut_lines): the tally of that cut, "which values of
        column 3 occur how often" -- the key of a line is that of its cut_lines output line; a bad block inside the window then
        fails the call as it fails cut_lines."""
        L = load_library()
        data = _coerce_input(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        return _tally_lines(lambda *a: L.cjs_bzip2_tally(keep.ctypes.data_as(u8p), data.size, self._h, lines._h, *a, None), lines, fields, bytes, delimiter, first, count,
                            seed, order, min_count, max_count, limit)

    def sort_lines(self, data, lines, fields=None, bytes=None, delimiter=b"\t", first=0, count=None, reverse=False, unique=False, limit=None, want_text=False):
        """`bzcat | sort` over lines [first, first + count) (count=None: to the last), ordered by content on the GPU
        (cjs_bzip2_sort) -> SortResult: the absolute numbers of the lines in LC_ALL=C order (bytes as Python orders them; equal
        lines by ascending number).  reverse: descending content (`sort -r`, equal lines still ascending); unique: one entry per
        run of equal lines, its lowest number, with the run's size in .counts (`sort -u`, `sort | uniq -c`); limit: the first so
        many entries (`sort | head`; None: all); want_text: the text of the returned entries, each with a newline, in .text.  A
        tail without a newline is a line, an empty tail is none.  fields / bytes (one of them, with delimiter, as in cut_lines):
        the cut of each line is what is compared and what .text holds; the numbers are still those of whole lines (`sort -s -k`).
        A bad block inside the window fails the call as it fails cut_lines."""
        L = load_library()
        data = _coerce_input(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        out, out_n = u8p(), ctypes.c_size_t(0)
        text = (ctypes.byref(out), ctypes.byref(out_n)) if want_text else (None, None)
        res = _sort_lines(lambda *a: L.cjs_bzip2_sort(keep.ctypes.data_as(u8p), data.size, self._h, lines._h, *a[:-1], *text, a[-1], None), lines, fields, bytes,
                          delimiter, first, count, reverse, unique, limit)
        res.text = _adopt(out, out_n.value).tobytes() if want_text else None
        return res

    def diff_stream(self, data, lines, other_data, other_index, other_lines, max_edits=0, seed=0):
        """bzdiff on the GPU: the line diff of this stream (A) against the stream `other_data` of `other_index` (B) -> LineDiff.
        Both streams' lines are hashed where they stand decoded (line_keys); the diff runs on the host over 16 bytes per line
        (diff_keys).  An empty final line (the text ends in a newline) is dropped from either side first, as `diff` does.  A bad
        block on either side: CjsError(CJS_E_DATA_ERROR) with its detail."""
        sides = []
        for ix, d, ln in ((self, data, lines), (other_index, other_data, other_lines)):
            keys, info = ix.line_keys(d, ln, seed=seed)
            if info.bad_blocks:
                raise CjsError(-5, load_library().cjs_strerror(-5).decode() + (": " + info.detail if info.detail else ""))
            ends_in_newline = keys.size > 0 and keys[-1].tolist() == (0, 0, 0)
            sides.append((keys[:-1] if ends_in_newline else keys, ends_in_newline or ix.total == 0))
        (ka, a_nl), (kb, b_nl) = sides
        res = diff_keys(ka, kb, max_edits)
        res.a_lines, res.b_lines, res.a_final_newline, res.b_final_newline = int(ka.size), int(kb.size), a_nl, b_nl
        return res

    def grep_lines(self, data, lines, patterns, regex=False, **search_kw):
        """bzgrep -n: search, then number of the match offsets, then locate of each distinct line and its successor, then one
        read_ranges.  -> [(line_no, line_bytes, [(off, pattern), ...])] ascending, each line once (a match that spans lines
        belongs to the line its first byte is in; a CjsError in place of the bytes of a line that touches a bad block).
        regex=True is bzgrep -n -E: search_regex, the matches (off, pattern, length) triples."""
        res = self.search_regex(data, patterns, **search_kw) if regex else self.search(data, patterns, **search_kw)
        if not res.matches:
            return []
        numbers, st, _ = self.line_numbers(data, lines, [m[0] for m in res.matches])
        by_line = {}
        for m, no, s in zip(res.matches, numbers.tolist(), st.tolist()):
            if not s:
                by_line.setdefault(no, []).append(m)
        order = sorted(by_line)
        text = self.read_lines(data, lines, [(no, 1) for no in order])
        return [(no, t, by_line[no]) for no, t in zip(order, text)]


class Bzip2Lines:
    """The line table of an indexed .bz2 stream (cjs_bz_lines): the newlines of every block of one Bzip2Index.  Made by build()
    (one counting pass on the GPU), load() (the serialised form save() returns) or create() (a caller's counts)."""

    def __init__(self, handle):
        self._h = handle
        self._fin = weakref.finalize(self, load_library().cjs_bzip2_lines_destroy, handle)

    @staticmethod
    def build(data, index):
        L = load_library()
        data = _coerce_input(data)
        keep = data if data.size else np.zeros(1, dtype=np.uint8)
        h = ctypes.c_void_p()
        _check(L.cjs_bzip2_lines_build(keep.ctypes.data_as(u8p), data.size, index._h, ctypes.byref(h), None))
        return Bzip2Lines(h)

    @staticmethod
    def load(raw, index):
        L = load_library()
        raw = _coerce_input(raw)
        keep = raw if raw.size else np.zeros(1, dtype=np.uint8)
        h = ctypes.c_void_p()
        _check(L.cjs_bzip2_lines_load(keep.ctypes.data_as(u8p), raw.size, index._h, ctypes.byref(h)))
        return Bzip2Lines(h)

    @staticmethod
    def create(index, counts):
        L = load_library()
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        keep = c if c.size else np.zeros(1, dtype=np.uint32)
        h = ctypes.c_void_p()
        _check(L.cjs_bzip2_lines_create(index._h, keep.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), c.size, ctypes.byref(h)))
        return Bzip2Lines(h)

    def save(self):
        L = load_library()
        out, out_n = u8p(), ctypes.c_size_t(0)
        _check(L.cjs_bzip2_lines_save(self._h, ctypes.byref(out), ctypes.byref(out_n)))
        raw = ctypes.string_at(out, out_n.value)
        L.cjs_free(out)
        return raw

    def _info(self):
        b, nl, t = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(load_library().cjs_bzip2_lines_info(self._h, ctypes.byref(b), ctypes.byref(nl), ctypes.byref(t)))
        return b.value, nl.value, t.value

    blocks = property(lambda self: self._info()[0])
    newlines = property(lambda self: self._info()[1])
    total = property(lambda self: self._info()[2])

    def counts(self):
        """the newlines of every block, a uint32 array"""
        c = np.zeros(max(self.blocks, 1), dtype=np.uint32)
        nb = load_library().cjs_bzip2_lines_counts(self._h, c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), c.size)
        return c[:nb]

    def close(self):
        self._fin()


def _lines_ask(call, questions):
    """call(q, count, out, status) -> rc: the answers, the statuses and the lowest-index failing question's detail"""
    q = np.ascontiguousarray(np.asarray(list(questions), dtype=np.uint64).reshape(-1))
    count = q.size
    keep = q if count else np.zeros(1, dtype=np.uint64)
    out, st = np.zeros(max(count, 1), dtype=np.uint64), np.zeros(max(count, 1), dtype=np.int32)
    PU = ctypes.POINTER(ctypes.c_uint64)
    _check(call(keep.ctypes.data_as(PU), count, out.ctypes.data_as(PU), st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    detail = load_library().cjs_last_error_detail().decode() if st[:count].any() else ""
    return out[:count], st[:count], detail


def lines_build_device(d_in_ptr, n, index, device=-1):
    """Bzip2Lines.build with the stream in GPU memory (cjs_bzip2_lines_build_device; the memory rules of decompress_device)"""
    L = load_library()
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    h = ctypes.c_void_p()
    _check(L.cjs_bzip2_lines_build_device(d_in_ptr, n, index._h, ctypes.byref(h), ctypes.byref(opts)))
    return Bzip2Lines(h)


def line_starts_device(d_in_ptr, n, index, lines, line_numbers, device=-1):
    """Bzip2Index.line_starts with the stream in GPU memory (cjs_bzip2_lines_locate_device).  The result is host memory."""
    L = load_library()
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    return _lines_ask(lambda *a: L.cjs_bzip2_lines_locate_device(d_in_ptr, n, index._h, lines._h, *a, ctypes.byref(opts)), line_numbers)


def line_numbers_device(d_in_ptr, n, index, lines, offsets, device=-1):
    """Bzip2Index.line_numbers with the stream in GPU memory (cjs_bzip2_lines_number_device).  The result is host memory."""
    L = load_library()
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    return _lines_ask(lambda *a: L.cjs_bzip2_lines_number_device(d_in_ptr, n, index._h, lines._h, *a, ctypes.byref(opts)), offsets)


class LineKeysResult:
    """What came with the keys: n_lines = the lines of the window; bad_blocks / first_bad_block (None if none) / detail = the
    touched blocks that were not good."""

    def __init__(self, info, detail):
        self.n_lines = int(info.n_lines)
        self.bad_blocks = int(info.n_bad_blocks)
        self.first_bad_block = int(info.first_bad_block) if info.n_bad_blocks else None
        self.blocks_decoded = int(info.blocks_decoded)
        self.detail = detail


def _line_keys(call, first, count, seed):
    """call(first, count, seed, keys, cap, info) -> rc: the count query (the table alone), then every key of the window"""
    L = load_library()
    first, cnt = int(first), 2 ** 64 - 1 if count is None else int(count)
    info = LineKeysInfo()
    _check(call(first, cnt, int(seed), None, 0, ctypes.byref(info)))
    keys = np.zeros(int(info.n_lines), dtype=LINE_KEY_DTYPE)
    if keys.size:
        _check(call(first, cnt, int(seed), keys.ctypes.data, keys.size, ctypes.byref(info)))
    detail = L.cjs_last_error_detail().decode() if info.n_bad_blocks else ""
    return keys, LineKeysResult(info, detail)


def line_keys_device(d_in_ptr, n, index, lines, first=0, count=None, seed=0, device=-1):
    """Bzip2Index.line_keys with the stream in GPU memory (cjs_bzip2_line_keys_device; the memory rules of decompress_device).
    The result is host memory."""
    L = load_library()
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    return _line_keys(lambda *a: L.cjs_bzip2_line_keys_device(d_in_ptr, n, index._h, lines._h, *a, ctypes.byref(opts)), first, count, seed)


def cut_list(spec):
    """A cut-style LIST ("1,3-5,7-", "-4") -> [(lo, hi)] as written (cjs_cut_list_parse; no device); hi = CUT_TO_END: to the end
    of the line.  CjsError(CJS_E_INVALID_ARG) for what is no list."""
    L = load_library()
    sel = np.zeros(64, dtype=CUT_RANGE_DTYPE)
    n = ctypes.c_uint32(0)
    _check(L.cjs_cut_list_parse(spec.encode() if isinstance(spec, str) else bytes(spec), sel.ctypes.data, 64, ctypes.byref(n)))
    return [(int(r["lo"]), int(r["hi"])) for r in sel[:n.value]]


def _cut_args(fields, bytes_, delimiter):
    """-> (mode, delimiter byte, the ranges as an array): exactly one of fields / bytes_, each a LIST string or ints and pairs"""
    if (fields is None) == (bytes_ is None):
        raise ValueError("exactly one of fields and bytes must be given")
    spec = fields if bytes_ is None else bytes_
    if isinstance(spec, (str, bytes)):
        pairs = cut_list(spec)
    else:
        pairs = [(int(x), int(x)) if not isinstance(x, (tuple, list)) else (int(x[0]), CUT_TO_END if x[1] is None else int(x[1])) for x in spec]
    if any(not 0 <= v <= CUT_TO_END for p in pairs for v in p):
        raise ValueError("a unit number does not fit 32 bits")
    raw = delimiter.encode("latin-1") if isinstance(delimiter, str) else bytes([delimiter]) if isinstance(delimiter, int) else bytes(delimiter)
    if len(raw) != 1:
        raise ValueError("the delimiter is one byte")
    d = raw[0]
    sel = np.zeros(max(len(pairs), 1), dtype=CUT_RANGE_DTYPE)
    for k, p in enumerate(pairs):
        sel[k] = p
    return (CUT_FIELDS if bytes_ is None else CUT_BYTES), d, sel[:len(pairs)]


def cut_text(text, fields=None, bytes=None, delimiter=b"\t"):
    """The cut of a plain host buffer by the library's scalar walk (cjs_stage_cut; no device): what Bzip2Index.cut_lines gives for
    the whole of a stream that decodes to `text`."""
    L = load_library()
    mode, d, sel = _cut_args(fields, bytes, delimiter)
    text = _coerce_input(text)
    keep = text if text.size else np.zeros(1, dtype=np.uint8)
    out = np.zeros(text.size + 1, dtype=np.uint8)
    n = ctypes.c_size_t(0)
    _check(L.cjs_stage_cut(keep.ctypes.data, text.size, mode, d, sel.ctypes.data, sel.size, out.ctypes.data, out.size, ctypes.byref(n)))
    return out[:n.value].tobytes()


def cut_lines_device(d_in_ptr, n, index, lines, fields=None, bytes=None, delimiter=b"\t", first=0, count=None, d_out_ptr=None, out_cap=0, device=-1):
    """Bzip2Index.cut_lines with the stream and the result in GPU memory (cjs_bzip2_cut_device; the memory rules of
    decompress_device) -> the bytes written at d_out_ptr.  Output above out_cap: CjsError(CJS_E_OUTPUT_TOO_SMALL) whose `need` is
    the full size (d_out_ptr=None, out_cap=0: the size query); nothing at or past out_cap is written."""
    L = load_library()
    mode, d, sel = _cut_args(fields, bytes, delimiter)
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    need, info = ctypes.c_size_t(0), CutInfo()
    rc = L.cjs_bzip2_cut_device(d_in_ptr, n, index._h, lines._h, int(first), 2 ** 64 - 1 if count is None else int(count), mode, d, sel.ctypes.data,
                                sel.size, d_out_ptr, out_cap, ctypes.byref(need), ctypes.byref(info), ctypes.byref(opts))
    try:
        _check(rc)
    except CjsError as e:
        e.need = need.value if rc == -33 else None
        raise
    return need.value


class LineDiff:
    """A line diff: hunks = [(a_first, a_count, b_first, b_count)] ascending, each replacing lines [a_first, +a_count) of A by
    [b_first, +b_count) of B; edits = the lines deleted plus the lines inserted; common = the lines kept; minimal = the script is
    a shortest one (False: max_edits was below the minimum and everything between the common ends is one hunk)."""

    def __init__(self, hunks, info):
        self.hunks = hunks
        self.edits, self.common, self.minimal = int(info.edits), int(info.common), bool(info.minimal)
        self.a_lines = self.b_lines = None                           # (diff_stream: the lines of either side ...
        self.a_final_newline = self.b_final_newline = True           # ... and whether its last one ends in a newline)

    @property
    def equal(self):
        return not self.hunks      # (a last line with and without its newline are two keys)

    def normal_text(self, index, data, lines, other_index, other_data, other_lines):
        """What `diff` prints in its normal format: NaM, N,MdK and N,McK,L commands, "< " and "> " lines, "---" between the two
        sides of a change and "\\ No newline at end of file" behind a side's last line when that has none.  Only the hunks' lines
        are read, through read_lines (one call per side); a hunk that touches a bad block raises its CjsError."""
        def side(ix, d, ln, spans):
            got = ix.read_lines(d, ln, spans) if spans else []
            for g in got:
                if isinstance(g, CjsError):
                    raise g
            return [g.split(b"\n") for g in got]

        def numbers(first, count):
            return "%d" % (first + (1 if count else 0)) if count <= 1 else "%d,%d" % (first + 1, first + count)

        a_text = side(index, data, lines, [(h[0], h[1]) for h in self.hunks])
        b_text = side(other_index, other_data, other_lines, [(h[2], h[3]) for h in self.hunks])
        out = []
        for (a0, an, b0, bn), ta, tb in zip(self.hunks, a_text, b_text):
            out.append((numbers(a0, an) + ("a" if not an else "d" if not bn else "c") + numbers(b0, bn)).encode() + b"\n")
            for mark, parts, n, last, final in ((b"< ", ta, an, a0 + an == self.a_lines, self.a_final_newline),
                                                (b"> ", tb, bn, b0 + bn == self.b_lines, self.b_final_newline)):
                if mark == b"> " and an and bn:
                    out.append(b"---\n")
                for k in range(n):
                    out.append(mark + parts[k] + b"\n")
                    if k == n - 1 and last and not final:
                        out.append(b"\\ No newline at end of file\n")
        return b"".join(out)


def diff_keys(a, b, max_edits=0):
    """The line diff of two key arrays (Bzip2Index.line_keys) on the host (cjs_line_keys_diff; no device) -> LineDiff.  With at
    most max_edits edits (0: 16,384) in the shortest script the result is one; else everything between the common ends is one
    hunk.  All-ones keys equal nothing."""
    L = load_library()
    a = np.ascontiguousarray(a, dtype=LINE_KEY_DTYPE)
    b = np.ascontiguousarray(b, dtype=LINE_KEY_DTYPE)
    pa, pb = (a.ctypes.data if a.size else None), (b.ctypes.data if b.size else None)
    info = LineDiffInfo()
    _check(L.cjs_line_keys_diff(pa, a.size, pb, b.size, int(max_edits), None, 0, ctypes.byref(info)))
    hunks = (Hunk * max(int(info.n_hunks), 1))()
    if info.n_hunks:
        _check(L.cjs_line_keys_diff(pa, a.size, pb, b.size, int(max_edits), hunks, int(info.n_hunks), ctypes.byref(info)))
    return LineDiff([(h.a_first, h.a_count, h.b_first, h.b_count) for h in hunks[:int(info.n_hunks)]], info)


class TallyResult:
    """A frequency table: groups = a structured array of (hash, len, check, first, count) per returned group, in the order asked
    for and at most `limit` of them; n_lines = the keys tallied; n_bad_lines = those that were all-ones (grouped nowhere);
    n_distinct = all groups; n_groups = the groups that pass the filter; max_count = the size of the largest group."""

    def __init__(self, groups, info, detail="", cut=None):
        self.groups = groups
        self.cut = cut          # of a tally of a cut: the fields / bytes / delimiter it was made with
        if isinstance(info, TallyInfo):
            self.n_lines, self.n_bad_lines = int(info.n_keys), int(info.n_bad)
        else:      # of a stream: the touched blocks that were not good beside it, as in LineKeysResult
            self.n_lines, self.n_bad_lines = int(info.n_lines), int(info.n_bad_lines)
            self.bad_blocks, self.blocks_decoded = int(info.n_bad_blocks), int(info.blocks_decoded)
            self.first_bad_block = int(info.first_bad_block) if info.n_bad_blocks else None
            self.detail = detail
        self.n_distinct, self.n_groups, self.max_count = int(info.n_distinct), int(info.n_groups), int(info.max_count)

    def text(self, index, data, lines):
        """`uniq -c` style lines ("%7d %s") of the returned groups of Bzip2Index.tally_lines (or of tally_keys over the keys of
        the stream's lines from line 0 on): each group's representative line is read through read_lines, all in one call, and
        for the tally of a cut passed through cut_text.  A line that touches a bad block raises its CjsError."""
        got = index.read_lines(data, lines, [(int(f), 1) for f in self.groups["first"]])
        out = []
        for g, c in zip(got, self.groups["count"].tolist()):
            if isinstance(g, CjsError):
                raise g
            if self.cut:
                g = cut_text(g, **self.cut)          # the group's key is that of the cut line
            out.append(b"%7d " % c + (g if g.endswith(b"\n") else g + b"\n"))
        return b"".join(out)


def _tally_args(order, min_count, max_count, limit):
    orders = {"first": TALLY_BY_FIRST, "count": TALLY_BY_COUNT}
    if order not in orders:
        raise ValueError("order is 'count' or 'first'")
    min_count, max_count = int(min_count), int(max_count)
    if min_count < 0 or max_count < 0 or (max_count and max_count < min_count):
        raise ValueError("0 <= min_count, and max_count is 0 (no bound) or at least min_count")
    if limit is not None and int(limit) < 0:
        raise ValueError("limit is None or a count")
    return orders[order], min_count, max_count, None if limit is None else int(limit)


def _tally(call, limit, most, info=None, cut=None):
    """call(out, cap, info) -> rc, once: with room for `limit` groups, or without a limit for `most`, which bounds their number"""
    info = TallyInfo() if info is None else info
    cap = int(most) if limit is None else min(limit, int(most))
    groups = np.zeros(cap, dtype=TALLY_DTYPE)
    _check(call(groups.ctypes.data if cap else None, cap, ctypes.byref(info)))      # (no room: the count query)
    detail = load_library().cjs_last_error_detail().decode() if getattr(info, "n_bad_blocks", 0) else ""
    return TallyResult(groups[:min(cap, int(info.n_groups))].copy(), info, detail, cut)


def tally_keys(keys, order="count", min_count=1, max_count=0, limit=None, device=-1):
    """`sort | uniq -c` over a key array (Bzip2Index.line_keys), grouped on the GPU (cjs_keys_tally) -> TallyResult.  Two keys are
    one group iff all three fields are equal; all-ones keys are grouped nowhere.  order="count": descending count, ties by first
    occurrence; "first": by first occurrence.  min_count=2 is `uniq -d`, max_count=1 is `uniq -u`; limit: the first so many groups
    (None: all).  A group's `first` is the index of its first key."""
    L = load_library()
    order, min_count, max_count, limit = _tally_args(order, min_count, max_count, limit)
    keys = np.ascontiguousarray(keys, dtype=LINE_KEY_DTYPE)
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    ptr = keys.ctypes.data if keys.size else None
    return _tally(lambda *a: L.cjs_keys_tally(ptr, keys.size, order, min_count, max_count, *a, ctypes.byref(opts)), limit, keys.size)


def _tally_lines(call, lines, fields, bytes_, delimiter, first, count, seed, order, min_count, max_count, limit):
    """call(first, count, seed, mode, delim, sel, nsel, order, min_count, max_count, out, cap, info) -> rc"""
    order, min_count, max_count, limit = _tally_args(order, min_count, max_count, limit)
    if fields is None and bytes_ is None:
        mode, d, sel, cut = TALLY_LINES, 0, np.zeros(0, dtype=CUT_RANGE_DTYPE), None
    else:
        mode, d, sel = _cut_args(fields, bytes_, delimiter)
        cut = dict(fields=fields, bytes=bytes_, delimiter=delimiter)
    first, cnt = int(first), 2 ** 64 - 1 if count is None else int(count)
    window = max(min(first + cnt, lines.newlines + 1) - first, 0)          # the window's lines by the table: no more groups than that
    head = (first, cnt, int(seed), mode, d, sel.ctypes.data if sel.size else None, sel.size, order, min_count, max_count)
    return _tally(lambda *a: call(*head, *a), limit, window, StreamTallyInfo(), cut)


def tally_lines_device(d_in_ptr, n, index, lines, fields=None, bytes=None, delimiter=b"\t", first=0, count=None, seed=0, order="count", min_count=1,
                       max_count=0, limit=None, device=-1):
    """Bzip2Index.tally_lines with the stream in GPU memory (cjs_bzip2_tally_device; the memory rules of decompress_device).  The
    result is host memory."""
    L = load_library()
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    return _tally_lines(lambda *a: L.cjs_bzip2_tally_device(d_in_ptr, n, index._h, lines._h, *a, ctypes.byref(opts)), lines, fields, bytes, delimiter, first,
                        count, seed, order, min_count, max_count, limit)


class SortResult:
    """A sort: lines = the line numbers (uint64) in the order asked for, at most `limit` of them; counts = the size of each
    entry's run of equal lines (all ones without unique); text = the returned entries' lines, each with a newline (None unless
    asked for; the device forms give its size in text_n instead); n_lines = the lines sorted; n_distinct = the runs of equal lines;
    n_out = the entries the flags select; text_bytes = the size of the text of all n_out entries; rounds = the sort rounds run."""

    def __init__(self, lines, counts, info, text=None, text_n=None):
        self.lines, self.counts, self.text, self.text_n = lines, counts, text, text_n
        self.n_lines, self.n_out, self.n_distinct = int(info.n_lines), int(info.n_out), int(info.n_distinct)
        self.text_bytes, self.rounds = int(info.text_bytes), int(info.rounds)
        self.blocks_decoded = int(info.blocks_decoded)


def sort_text(text, reverse=False, unique=False):
    """The rule of the line sort restated in Python (no library call) -> (lines, counts): the text's lines (a tail that is not
    empty is one, an empty tail is none) ordered as Python orders bytes, equal lines by ascending number; reverse: descending
    content, equal lines still ascending; unique: the first line of every run of equal lines, with the run's size."""
    body = bytes(_coerce_input(text).tobytes())
    parts = body.split(b"\n")
    if parts[-1] == b"":
        parts.pop()
    runs = []                                                   # [[line numbers]] per distinct content, ascending content
    for i in sorted(range(len(parts)), key=lambda i: (parts[i], i)):
        if runs and parts[runs[-1][0]] == parts[i]:
            runs[-1].append(i)
        else:
            runs.append([i])
    if reverse:
        runs.reverse()
    if unique:
        return [r[0] for r in runs], [len(r) for r in runs]
    return [i for r in runs for i in r], [1] * len(parts)


def _sort_flags(reverse, unique, limit):
    if limit is not None and int(limit) < 0:
        raise ValueError("limit is None or a count")
    return (SORT_REVERSE if reverse else 0) | (SORT_UNIQUE if unique else 0), None if limit is None else int(limit)


def _sort(call, limit, most, text_n=None):
    """call(lines_out, counts_out, cap, info) -> rc, once: with room for `limit` entries, or without a limit for `most`"""
    info = SortInfo()
    cap = int(most) if limit is None else min(limit, int(most))
    lines_out, counts = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
    rc = call(lines_out.ctypes.data if cap else None, counts.ctypes.data if cap else None, cap, ctypes.byref(info))
    try:
        _check(rc)
    except CjsError as e:
        e.need = text_n.value if rc == -33 and text_n is not None else None
        raise
    m = min(cap, int(info.n_out))
    return SortResult(lines_out[:m].copy(), counts[:m].copy(), info, None, None if text_n is None else text_n.value)


def text_sort(text, reverse=False, unique=False, limit=None, want_text=False, device=-1):
    """`sort` over the lines of a plain host buffer, ordered on the GPU (cjs_text_sort) -> SortResult; the arguments are those of
    Bzip2Index.sort_lines, the line numbers count from 0."""
    L = load_library()
    flags, limit = _sort_flags(reverse, unique, limit)
    text = _coerce_input(text)
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    out, out_n = u8p(), ctypes.c_size_t(0)
    tp = (ctypes.byref(out), ctypes.byref(out_n)) if want_text else (None, None)
    ptr = text.ctypes.data if text.size else None
    res = _sort(lambda lo, co, cap, info: L.cjs_text_sort(ptr, text.size, flags, lo, co, cap, *tp, info, ctypes.byref(opts)), limit,
                int(np.count_nonzero(text == 10)) + 1)          # (the lines are the newlines and at most a tail)
    res.text = _adopt(out, out_n.value).tobytes() if want_text else None
    return res


def _sort_lines(call, lines, fields, bytes_, delimiter, first, count, reverse, unique, limit, text_n=None):
    """call(first, count, mode, delim, sel, nsel, flags, lines_out, counts_out, cap, info) -> rc"""
    flags, limit = _sort_flags(reverse, unique, limit)
    if fields is None and bytes_ is None:
        mode, d, sel = SORT_LINES, 0, np.zeros(0, dtype=CUT_RANGE_DTYPE)
    else:
        mode, d, sel = _cut_args(fields, bytes_, delimiter)
    first, cnt = int(first), 2 ** 64 - 1 if count is None else int(count)
    window = max(min(first + cnt, lines.newlines + 1) - first, 0)          # the window's lines by the table: no more entries than that
    head = (first, cnt, mode, d, sel.ctypes.data if sel.size else None, sel.size, flags)
    return _sort(lambda *a: call(*head, *a), limit, window, text_n)


def sort_lines_device(d_in_ptr, n, index, lines, fields=None, bytes=None, delimiter=b"\t", first=0, count=None, reverse=False, unique=False, limit=None,
                      d_text_out_ptr=None, text_cap=0, want_text=None, device=-1):
    """Bzip2Index.sort_lines with the stream in GPU memory and, when asked for, the text written to GPU memory
    (cjs_bzip2_sort_device; the memory rules of decompress_device).  Line numbers and counts are host memory.  Text is wanted
    when d_text_out_ptr is given or want_text is true (want_text alone: the size query); its size comes back as .text_n; a text
    above text_cap: CjsError(CJS_E_OUTPUT_TOO_SMALL) whose `need` is the full size, and nothing is written."""
    L = load_library()
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    wanted = d_text_out_ptr is not None or bool(want_text)
    text_n = ctypes.c_size_t(0) if wanted else None
    tn = ctypes.byref(text_n) if wanted else None
    return _sort_lines(lambda *a: L.cjs_bzip2_sort_device(d_in_ptr, n, index._h, lines._h, *a[:-1], d_text_out_ptr, text_cap, tn, a[-1], ctypes.byref(opts)),
                       lines, fields, bytes, delimiter, first, count, reverse, unique, limit, text_n)


def text_sort_device(d_text_ptr, n, reverse=False, unique=False, d_lines_out_ptr=None, d_counts_out_ptr=None, cap=0, d_text_out_ptr=None, text_cap=0,
                     want_text=None, device=-1):
    """text_sort with everything in GPU memory (cjs_text_sort_device) -> SortResult without arrays: the first min(cap, n_out)
    line numbers and counts stand at d_lines_out_ptr / d_counts_out_ptr (uint64), the text at d_text_out_ptr, .text_n its size."""
    L = load_library()
    flags, _ = _sort_flags(reverse, unique, None)
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    wanted = d_text_out_ptr is not None or bool(want_text)
    text_n, info = ctypes.c_size_t(0), SortInfo()
    rc = L.cjs_text_sort_device(d_text_ptr, n, flags, d_lines_out_ptr, d_counts_out_ptr, cap, d_text_out_ptr, text_cap, ctypes.byref(text_n) if wanted else None,
                                ctypes.byref(info), ctypes.byref(opts))
    try:
        _check(rc)
    except CjsError as e:
        e.need = text_n.value if rc == -33 else None
        raise
    return SortResult(None, None, info, None, text_n.value if wanted else None)


class SearchResult:
    """What a search found: matches = [(off, pattern)] sorted by (off, pattern), at most `limit` of them; total = all matches of
    the window; bad_blocks / first_bad_block (None if none) / detail = the touched blocks that were not good."""

    def __init__(self, matches, info, detail):
        self.matches, self.total = matches, int(info.n_matches)
        self.bad_blocks = int(info.n_bad_blocks)
        self.first_bad_block = int(info.first_bad_block) if info.n_bad_blocks else None
        self.blocks_decoded = int(info.blocks_decoded)
        self.detail = detail


def _pattern_arrays(patterns):
    pats = [bytes(_coerce_input(p.encode() if isinstance(p, str) else p)) for p in patterns]
    blob = np.frombuffer(b"".join(pats) or b"\0", dtype=np.uint8).copy()
    return pats, blob, np.cumsum([0] + [len(p) for p in pats]).astype(np.uint32)


def _search(call, patterns, off, length, nocase, limit, lengths=False):
    """call(pat, pat_off, npat, flags, off, len, found, cap, info) -> rc; limit=None: the count query, then all; lengths: the
    matches are (off, pattern, length) triples (the regex search)"""
    L = load_library()
    pats, blob, p_off = _pattern_arrays(patterns)
    ln = 2 ** 64 - 1 if length is None else int(length)

    def once(cap):
        found = (Match * max(cap, 1))()
        info = SearchInfo()
        _check(call(blob.ctypes.data_as(u8p), p_off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(pats), SEARCH_NOCASE if nocase else 0,
                    int(off), ln, found if cap else None, cap, ctypes.byref(info)))
        detail = L.cjs_last_error_detail().decode() if info.n_bad_blocks else ""
        got = min(cap, info.n_matches)
        raw = np.frombuffer(found, dtype=[("off", "<u8"), ("pattern", "<u4"), ("reserved", "<u4")], count=got)
        cols = (raw["off"].tolist(), raw["pattern"].tolist()) + ((raw["reserved"].tolist(),) if lengths else ())
        return SearchResult(list(zip(*cols)), info, detail)

    if limit is not None:
        return once(int(limit))
    res = once(0)
    return once(res.total) if res.total else res


def search_device(d_in_ptr, n, index, patterns, off=0, length=None, nocase=False, limit=None, device=-1):
    """Bzip2Index.search with the stream in GPU memory (cjs_bzip2_search_device; the memory rules of decompress_device).  The
    result is host memory."""
    L = load_library()
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    return _search(lambda *a: L.cjs_bzip2_search_device(d_in_ptr, n, index._h, *a, ctypes.byref(opts)), patterns, off, length, nocase, limit)


def search_regex_device(d_in_ptr, n, index, patterns, off=0, length=None, nocase=False, limit=None, device=-1):
    """Bzip2Index.search_regex with the stream in GPU memory (cjs_bzip2_search_regex_device).  The result is host memory."""
    L = load_library()
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    return _search(lambda *a: L.cjs_bzip2_search_regex_device(d_in_ptr, n, index._h, *a, ctypes.byref(opts)), patterns, off, length, nocase, limit, lengths=True)


def regex_check(patterns, nocase=False):
    """Compile `patterns` as Bzip2Index.search_regex would, without a device (cjs_regex_check): -> [(states, max_len)] per pattern;
    a CjsError with the detail text ("pattern J, byte P: ...") for a pattern the dialect refuses."""
    L = load_library()
    pats, blob, p_off = _pattern_arrays(patterns)
    states, max_len = (ctypes.c_uint32 * max(len(pats), 1))(), (ctypes.c_uint32 * max(len(pats), 1))()
    _check(L.cjs_regex_check(blob.ctypes.data_as(u8p), p_off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(pats), SEARCH_NOCASE if nocase else 0, states, max_len))
    return list(zip(list(states), list(max_len)))[:len(pats)]


class CompareResult:
    """What a compare found: diffs = [(off, a, b)] ascending, at most `limit` of them (a: the stream's byte, b: the other side's);
    total = all differences of the span; first_diff (None if none); compared = the bytes actually
    compared; len_a / len_b = the decoded bytes of the stream / where the other side ends; bad_blocks / first_bad_block /
    bad_blocks_b / first_bad_block_b / detail = the touched blocks that were not good."""

    def __init__(self, diffs, info, detail, len_a, len_b):
        self.diffs, self.total = diffs, int(info.n_diffs)
        self.first_diff = int(info.first_diff) if info.n_diffs else None
        self.compared = int(info.compared)
        self.len_a, self.len_b = int(len_a), int(len_b)
        self.bad_blocks, self.bad_blocks_b = int(info.n_bad_blocks), int(info.n_bad_blocks_b)
        self.first_bad_block = int(info.first_bad_block) if info.n_bad_blocks else None
        self.first_bad_block_b = int(info.first_bad_block_b) if info.n_bad_blocks_b else None
        self.blocks_decoded = int(info.blocks_decoded)
        self.detail = detail

    @property
    def whole(self):
        """the whole of both sides was compared"""
        return self.len_a == self.len_b and self.compared == self.len_a

    @property
    def equal(self):
        return self.total == 0 and self.bad_blocks == 0 and self.bad_blocks_b == 0 and self.whole

    def cmp_text(self, index=None, data=None, lines=None):
        """What `cmp` prints: "" when equal, "differ: byte N[, line M]" (both 1-based; the line needs the stream's index, its
        bytes and its Bzip2Lines: one line_numbers question), "EOF on a" / "EOF on b" when one side is a proper prefix of the
        other.  The common prefix must have been compared whole (CjsError otherwise: bad blocks, or a narrower window)."""
        if self.total:
            text = "differ: byte %d" % (self.first_diff + 1)
            if lines is not None:
                numbers, st, detail = index.line_numbers(data, lines, [self.first_diff])
                _check(int(st[0]))
                text += ", line %d" % (int(numbers[0]) + 1)
            return text
        if self.bad_blocks or self.bad_blocks_b or self.compared != min(self.len_a, self.len_b):
            raise CjsError(-5, "compare: not every byte of the common prefix was compared" + (": " + self.detail if self.detail else ""))
        if self.len_a == self.len_b:
            return ""
        return "EOF on a" if self.len_a < self.len_b else "EOF on b"


def _compare(call, off, length, limit, len_a, len_b):
    """call(off, len, diffs, cap, info) -> rc; limit=None: the count query, then all"""
    L = load_library()
    ln = 2 ** 64 - 1 if length is None else int(length)

    def once(cap):
        diffs = (Diff * max(cap, 1))()
        info = CompareInfo()
        _check(call(int(off), ln, diffs if cap else None, cap, ctypes.byref(info)))
        detail = L.cjs_last_error_detail().decode() if info.n_bad_blocks or info.n_bad_blocks_b else ""
        got = min(cap, info.n_diffs)
        raw = np.frombuffer(diffs, dtype=[("off", "<u8"), ("a", "u1"), ("b", "u1"), ("reserved", "u1", (6,))], count=got)
        return CompareResult(list(zip(raw["off"].tolist(), raw["a"].tolist(), raw["b"].tolist())), info, detail, len_a, len_b)

    if limit is not None:
        return once(int(limit))
    res = once(0)
    return once(res.total) if res.total else res


def compare_device(d_in_ptr, n, index, d_other_ptr, other_n, off=0, length=None, other_off=0, limit=64, device=-1):
    """Bzip2Index.compare with the stream and the other side in GPU memory (cjs_bzip2_compare_device; the memory rules of
    decompress_device).  The result is host memory."""
    L = load_library()
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    return _compare(lambda *a: L.cjs_bzip2_compare_device(d_in_ptr, n, index._h, d_other_ptr, other_n, int(other_off), *a, ctypes.byref(opts)),
                    off, length, limit, index.total, int(other_off) + int(other_n))


def compare_streams_device(d_a_ptr, na, index_a, d_b_ptr, nb, index_b, off=0, length=None, limit=64, device=-1):
    """Bzip2Index.compare_stream with both streams in GPU memory (cjs_bzip2_compare_streams_device)."""
    L = load_library()
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    return _compare(lambda *a: L.cjs_bzip2_compare_streams_device(d_a_ptr, na, index_a._h, d_b_ptr, nb, index_b._h, *a, ctypes.byref(opts)),
                    off, length, limit, index_a.total, index_b.total)


def read_ranges_device(d_in_ptr, n, index, ranges, d_out_ptr, out_cap, device=-1):
    """Bzip2Index.read_ranges with the stream and the result in GPU memory (cjs_bzip2_read_ranges_device; the memory rules of
    decompress_device).  -> (out_off, out_len, status, detail): range k's bytes at d_out + out_off[k]; a failed range keeps its
    region.  CjsError for a failure of the call, with `need` on CJS_E_OUTPUT_TOO_SMALL (-33); out_cap = 0 with d_out_ptr = None
    is the size query."""
    L = load_library()
    count, off, ln, o_off, o_len, st = _range_arrays(ranges)
    PU, PS = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t)
    need = ctypes.c_size_t(0)
    opts = _Opts(ctypes.sizeof(_Opts), device, 0, 0, None)
    rc = L.cjs_bzip2_read_ranges_device(d_in_ptr, n, index._h, off.ctypes.data_as(PU), ln.ctypes.data_as(PU), count, d_out_ptr, out_cap,
                                        o_off.ctypes.data_as(PS), o_len.ctypes.data_as(PS), st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                        ctypes.byref(need), ctypes.byref(opts))
    if rc == -33:
        e = CjsError(rc, L.cjs_strerror(rc).decode())
        e.need = need.value
        raise e
    _check(rc)
    detail = L.cjs_last_error_detail().decode() if st[:count].any() else ""
    return o_off[:count], o_len[:count], st[:count], detail


def trim():
    """Give the workspace that cjs_bzip2_compress keeps per device between calls back to the driver."""
    load_library().cjs_trim()
