/* cjs_hip.h — C ABI of the MI355X-native block-sorting core (libcjs_hip.so).
 *
 * This is the drop-in boundary for the compressjs Bzip2 / BWTC hot path: exactly what an FFI
 * binding of the reference's per-algorithm `compressFile` / `decompressFile` would call
 * (N-API shim: compressjs-flattened_amd/js/cjs_napi.cc; ctypes: tests/support.py).
 * Plain pointers and sizes only.  Functions never throw; they return 0 or a negative code.
 * Every entry point needs a HIP device: without one the call fails with CJS_E_NO_DEVICE
 * (there is NO CPU fallback in this library).
 *
 * J/ = /root/reference/ (reference source, cited for parity checks).
 */
#ifndef CJS_HIP_H
#define CJS_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes.  -1..-8 keep the reference's Err table (J/Bzip2_joined_.js:1365-1375) */
#define CJS_OK 0
#define CJS_E_NOT_BZIP_DATA (-2)   /* TypeError "Not bzip data[: bad magic|level out of range]" */
#define CJS_E_DATA_ERROR (-5)      /* TypeError "Data error[: Bad block CRC ...]" */
#define CJS_E_OUT_OF_MEMORY (-6)
#define CJS_E_OBSOLETE_INPUT (-7)  /* randomised blocks */
#define CJS_E_BAD_LEVEL (-20)      /* Error('Invalid block size multiplier') J/Bzip2_joined_.js:2208 */
#define CJS_E_BAD_MAGIC (-21)      /* Error("Bad magic") J/BWTC_joined_.js:559-565 */
#define CJS_E_NO_DEVICE (-30)      /* no HIP device / HIP runtime error */
#define CJS_E_HIP (-31)
#define CJS_E_INVALID_ARG (-32)
#define CJS_E_OUTPUT_TOO_SMALL (-33)
#define CJS_E_UNSUPPORTED (-34)

/* ---- options (all optional; pass NULL for defaults) */
typedef struct cjs_stats {
  double ms_total;        /* device time of the whole call (hipEvents on the work stream) */
  double ms_rle1;         /* RLE1 + CRC + block boundaries */
  double ms_bwt;          /* suffix sort + BWT emit */
  double ms_mtf;          /* MTF + RLE2 + histogram */
  double ms_huff;         /* Huffman table construction / optimisation */
  double ms_pack;         /* bit packing + stream assembly */
  double ms_bwt_dominant; /* average launch duration of the dominant kernel (radix scatter) */
  uint64_t bwt_dominant_launches;
  uint64_t bwt_dominant_bytes;   /* algorithmic bytes moved by those launches */
  uint64_t blocks;
  uint64_t bytes_in, bytes_out;
  uint32_t bwt_rounds;
  uint32_t reserved;      /* written as 0 */
} cjs_stats;               /* OUT only: cleared and filled by the call, never read */
/* cjs_bwtc_compress fills the same struct with wall-clock times of its two halves: ms_total = whole call, ms_bwt =
 * longest GPU batch (workspace + H2D + BWT + MTF + model), ms_mtf = time until the first step list reached the host,
 * ms_pack = serial range coder over the step lists (host), ms_rle1 = time the coder spent waiting for the GPU. */

typedef struct cjs_opts {
  uint32_t struct_size;   /* sizeof(cjs_opts) */
  int32_t device;         /* HIP device ordinal; -1 = current device */
  uint32_t n_devices;     /* host-buffer entry points: shard blocks over this many GPUs (0/1 = one) */
  uint32_t flags;         /* CJS_FLAG_* */
  cjs_stats *stats;       /* optional out */
} cjs_opts;
/* cjs_bwtc_compress: the input came from a stream without a known size, so the header carries varint(0) instead of
 * varint(size+1) (Util.compressFileHelper, J/BWTC_joined_.js:529-543) */
#define CJS_FLAG_SIZE_UNKNOWN 1u
/* cjs_bzip2_compress with opts->stats: no stream synchronisation between the stages -- ms_rle1 / ms_bwt / ms_mtf / ms_huff /
 * ms_pack stay 0, the rest is filled (whole-call events, dominant-kernel events, counts).  Device-resident entry points:
 * cjs_ctx_set_stage_times(ctx, 0). */
#define CJS_FLAG_NO_STAGE_TIMES 2u

/* ---- host-buffer entry points (what the JS fronts bind).
 * cjs_bzip2_compress   replaces Bzip2.compressFile    J/Bzip2_joined_.js:2199-2249
 * cjs_bzip2_decompress replaces Bzip2.decompressFile  J/Bzip2_joined_.js:1769-1796
 * cjs_bwtc_compress    replaces BWTC.compressFile     J/BWTC_joined_.js:1698-1825
 * cjs_bwtc_decompress  replaces BWTC.decompressFile   J/BWTC_joined_.js:1827-1920
 * `*out` is allocated by the library (plain malloc, or for results of 1 MiB and more a cached pinned host buffer: see
 * cjs_trim); release it with cjs_free and with nothing else.  level: 1..9 (bzip2: else
 * CJS_E_BAD_LEVEL; bwtc: else 9, J/BWTC_joined_.js:1702-1705). */
int cjs_bzip2_compress(const uint8_t *in, size_t n, int level, uint8_t **out, size_t *out_n, const cjs_opts *opts);
int cjs_bzip2_decompress(const uint8_t *in, size_t n, int multistream, uint8_t **out, size_t *out_n, const cjs_opts *opts);
int cjs_bwtc_compress(const uint8_t *in, size_t n, int level, uint8_t **out, size_t *out_n, const cjs_opts *opts);
int cjs_bwtc_decompress(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n, const cjs_opts *opts);
/* Bzip2.compressFile over a batch: `count` independent inputs (in[k], n[k] bytes; n[k] may be 0) at one level, one .bz2 stream
 * per input, stream k byte-identical to cjs_bzip2_compress(in[k], n[k], level).  The library allocates ONE result buffer
 * (*out, released with cjs_free): stream k is bytes [off[k], off[k] + len[k]) of it (4-byte-aligned offsets; off / len have
 * `count` entries).  level outside 1..9: CJS_E_BAD_LEVEL before the device is touched; count == 0: success, *out = NULL.
 * Inputs are uploaded in groups of up to 256 MiB; an input larger than that goes through cjs_bzip2_compress in the same call.
 * The batch context of each device is kept between calls (cjs_trim gives it back). */
int cjs_bzip2_compress_batch(const uint8_t *const *in, const size_t *n, size_t count, int level, uint8_t **out, size_t *off,
                             size_t *len, const cjs_opts *opts);
/* Bzip2.table (J/Bzip2_joined_.js:1823-1863): fills (bit position, uncompressed size) of up to `cap` blocks,
 * returns the number of blocks or a negative code.  Bzip2.decompressBlock (:1797-1818): the single block
 * whose 48-bit magic starts at bit `bitpos`. */
long cjs_bzip2_table(const uint8_t *in, size_t n, int multistream, uint64_t *bitpos, uint32_t *size, long cap, const cjs_opts *opts);
int cjs_bzip2_decompress_block(const uint8_t *in, size_t n, uint64_t bitpos, uint8_t **out, size_t *out_n, const cjs_opts *opts);
/* Bzip2.decompressFile over a batch: `count` independent inputs (in[k], n[k] bytes; n[k] may be 0, in[k] may then be NULL),
 * each decoded exactly as cjs_bzip2_decompress(in[k], n[k], multistream) would decode it, in shared GPU passes.  Returns 0 when
 * every input got its own verdict: status[k] = 0 or the code cjs_bzip2_decompress gives for input k (CJS_E_NOT_BZIP_DATA,
 * CJS_E_DATA_ERROR, CJS_E_OBSOLETE_INPUT, CJS_E_UNSUPPORTED).  One result buffer (*out, release with cjs_free): input k's bytes are
 * [off[k], off[k] + len[k]), offsets ascend in input order, a failed input has len[k] = 0.  When some status[k] != 0,
 * cjs_last_error_detail() returns the detail of the LOWEST-index failing input, as cjs_bzip2_decompress of that input alone
 * would leave it -- the one case where the detail belongs to a call that returned 0.  A negative return is a failure of the
 * call itself (CJS_E_INVALID_ARG, CJS_E_NO_DEVICE, CJS_E_HIP, CJS_E_OUT_OF_MEMORY); *out is then NULL.  count == 0: success,
 * *out = NULL.  NULL out / off / len / status / in / n with count > 0, or n[k] > 0 with in[k] == NULL: CJS_E_INVALID_ARG before the
 * device is touched.  opts->device is honoured; opts->n_devices and opts->stats are ignored. */
int cjs_bzip2_decompress_batch(const uint8_t *const *in, const size_t *n, size_t count, int multistream, uint8_t **out, size_t *off,
                               size_t *len, int32_t *status, const cjs_opts *opts);
/* cjs_bzip2_decompress with the stream and the result in GPU memory: d_in (n bytes) and d_out (out_cap bytes) are device memory
 * of the GPU opts->device names (-1: the current one), any byte alignment; bytes past d_in + n are never read.  The caller has
 * finished writing d_in (e.g. synchronised its stream); synchronous on return.  Return code, bytes and cjs_last_error_detail() are
 * what cjs_bzip2_decompress gives for the same bytes on the host; on success *out_n = the decoded size.  A decoded size above
 * out_cap: CJS_E_OUTPUT_TOO_SMALL with *out_n = the bytes needed and d_out untouched (out_cap = 0, d_out = NULL: the size query).
 * No byte at or past min(out_cap, decoded size) is written, and every failure but a bad block CRC leaves d_out untouched.
 * Before any launch d_in (n > 0) and d_out (out_cap > 0) must be device memory of that GPU (hipPointerGetAttributes), else
 * CJS_E_INVALID_ARG, as for out_n NULL, d_in NULL with n > 0 or d_out NULL with out_cap > 0 (checked before the device is
 * touched).  opts->n_devices and opts->stats are ignored. */
int cjs_bzip2_decompress_device(const uint8_t *d_in, size_t n, int multistream, uint8_t *d_out, size_t out_cap, size_t *out_n,
                                const cjs_opts *opts);
/* cjs_bzip2_decompress_batch with the inputs and the result in GPU memory (the memory rules of cjs_bzip2_decompress_device): input k
 * is d_in[in_off[k] .. in_off[k+1]) (in_off: HOST array of count + 1 ascending offsets).  status[k], out_off[k], out_len[k] (from
 * d_out), the bytes and the lowest-index detail are what cjs_bzip2_decompress_batch gives for the same inputs; the same groups
 * (CJS_DEC_GROUP_BYTES), a larger input through the single device path.  On success *out_need = the end of the last input's
 * region.  A layout larger than out_cap: CJS_E_OUTPUT_TOO_SMALL with *out_need = the bytes needed, d_out untouched and the other
 * out arrays not meaningful.  No byte at or past min(out_cap, out_need) is written; a failed input's region holds unspecified
 * bytes.  count == 0: 0 with *out_need = 0.  CJS_E_INVALID_ARG before the device is touched for in_off / out_off / out_len /
 * status / out_need NULL, in_off not ascending, d_in NULL with input bytes, d_out NULL with out_cap > 0; and before any launch
 * for memory that is not the GPU's. */
int cjs_bzip2_decompress_batch_device(const uint8_t *d_in, const size_t *in_off, size_t count, int multistream, uint8_t *d_out,
                                      size_t out_cap, size_t *out_off, size_t *out_len, int32_t *status, size_t *out_need,
                                      const cjs_opts *opts);
/* Recovery of damaged .bz2 data (what bzip2recover is for): the blocks that are still intact, as their decoded bytes
 * (as_stream == 0) or as a repaired single-stream .bz2 (as_stream != 0).  The input is any n bytes: no header is needed and
 * none is checked.  A CANDIDATE is every bit position at which the 48-bit block magic 0x314159265359 starts (end-of-stream
 * magics are ignored).  It is DECODABLE if the block decoder accepts it under the level-9 limits, whatever any header says
 * (at most 900000 BWT bytes, origPtr below their count, not randomised -- bzip2recover's re-wrapping as 'BZh9'), and its
 * end-of-block code ends strictly inside the input (end_bit < 8 n: a block that touches the end counts as cut off); INTACT if
 * the CRC of its decoded bytes is the stored one.  The candidates are walked in ascending bit position with last_end = 0: one
 * that starts below last_end is SHADOWED (a false magic inside a block already accepted); otherwise an intact one is RECOVERED
 * and sets last_end to its end_bit; otherwise it is lost.  Only a recovered block shadows anything.
 * Bytes form: the decoded bytes of the recovered blocks in order.  Stream form: 'BZh9', the bit strings [bitpos, end_bit) of the
 * recovered blocks back to back from bit 32, the end-of-stream magic, the combined CRC (c = rol1(c) ^ stored crc, from 0), zero
 * bits to a whole byte; with nothing recovered the 14-byte empty stream.  For input that cjs_bzip2_decompress(.., 1) accepts the
 * bytes form is that call's output and the recovered (bitpos, size) are cjs_bzip2_table(.., 1)'s; the stream form always decodes
 * to the bytes form of the same input.
 * Returns 0 whenever the call itself worked, also when nothing was recovered; a negative code is a failure of the call
 * (CJS_E_INVALID_ARG, CJS_E_NO_DEVICE, CJS_E_HIP, CJS_E_OUT_OF_MEMORY, CJS_E_OUTPUT_TOO_SMALL).  *n_found = the number of
 * candidates; found (may be NULL with cap == 0) gets the first cap of them, ascending.  *out: the rules of cjs_bzip2_decompress
 * (cjs_free).  NULL out / out_n / n_found, NULL in with n > 0, NULL found with cap > 0: CJS_E_INVALID_ARG before the device is
 * touched; n < 6 (no magic fits): success with nothing found, also before the device is touched (the stream form is then the
 * empty stream).  opts->device is honoured, n_devices and stats are ignored.
 * _device: the memory rules of cjs_bzip2_decompress_device for d_in / d_out (any alignment, checked before any launch); found
 * and n_found are host memory.  A result above out_cap: CJS_E_OUTPUT_TOO_SMALL with *out_n = the bytes needed (out_cap = 0,
 * d_out = NULL: the size query; *n_found and found are filled all the same).  No byte at or past out_cap is ever written; the
 * contents of d_out are unspecified after CJS_E_OUTPUT_TOO_SMALL, and in [*out_n, out_cap) on success. */
#define CJS_REC_SHADOWED 1
typedef struct cjs_bz_found {
  uint64_t bitpos;    /* where the candidate's magic starts in the input */
  uint64_t end_bit;   /* first bit behind its end-of-block code; 0 if not decodable */
  uint64_t out_off;   /* recovered: byte offset in the bytes form / bit position of its magic in the stream form */
  uint32_t size;      /* recovered: decoded bytes */
  int32_t  status;    /* 0 recovered, CJS_REC_SHADOWED, else the block's code: CJS_E_DATA_ERROR, CJS_E_OBSOLETE_INPUT */
  uint32_t crc;       /* stored block CRC; 0 if the header could not be read */
  uint32_t reserved;  /* 0 */
} cjs_bz_found;
int cjs_bzip2_recover(const uint8_t *in, size_t n, int as_stream, uint8_t **out, size_t *out_n,
                      cjs_bz_found *found, long cap, long *n_found, const cjs_opts *opts);
int cjs_bzip2_recover_device(const uint8_t *d_in, size_t n, int as_stream, uint8_t *d_out, size_t out_cap, size_t *out_n,
                             cjs_bz_found *found, long cap, long *n_found, const cjs_opts *opts);
/* Indexed range reads: bytes [off, off + len) of what cjs_bzip2_decompress would return, decoding only the blocks they touch.
 * A cjs_bz_index holds one entry per block of a stream, in stream order, with the stream's size in bytes and the multistream
 * flag it was made with.  Decoded offsets are the prefix sums of `size`; their total is total_bytes.  Host logic only, except
 * _build, which is one table pass (cjs_bzip2_table's: the same verdicts, codes and details on the same bytes, opts->n_devices
 * honoured as there) that also hands out every block's end bit, stored CRC and the level of its member stream.
 * _create takes a caller's entries (another tool's, or cjs_bzip2_table's plus the caller's own knowledge); _save gives the
 * serialised form (*bytes: malloc'd, cjs_free), _load reads it:
 *   32-byte header: the 8 bytes "CJSBZIX1", u32 version = 1, u32 flags (bit 0 = multistream), u64 stream_bytes, u64 count;
 *   then `count` entries of 32 bytes, the struct below; everything little-endian.
 * _create and _load refuse with CJS_E_INVALID_ARG and a detail text, before any device is touched: wrong magic, version or
 * length; bitpos < 32; bitpos[k] < end_bit[k-1]; end_bit <= bitpos + 48 + 32; end_bit > 8 * stream_bytes; level outside 1..9;
 * size > 52 * 100000 * level; reserved != 0; undefined flag bits.  NULL arguments: CJS_E_INVALID_ARG.
 * _info: any out pointer may be NULL.  _entries copies the first min(cap, blocks) entries and returns the number of blocks.
 * An index is immutable once made: any number of threads may read ranges through one index. */
typedef struct cjs_bz_index_entry {   /* 32 bytes, also the serialised entry (little-endian) */
  uint64_t bitpos;    /* where the block's 48-bit magic starts */
  uint64_t end_bit;   /* first bit behind its end-of-block code */
  uint32_t size;      /* decoded bytes */
  uint32_t crc;       /* stored block CRC */
  uint32_t level;     /* 1..9: level of the member stream the block belongs to */
  uint32_t reserved;  /* 0 */
} cjs_bz_index_entry;
typedef struct cjs_bz_index cjs_bz_index;
int cjs_bzip2_index_build(const uint8_t *in, size_t n, int multistream, cjs_bz_index **idx, const cjs_opts *opts);
int cjs_bzip2_index_create(const cjs_bz_index_entry *entries, size_t count, uint64_t stream_bytes, int multistream, cjs_bz_index **idx);
int cjs_bzip2_index_save(const cjs_bz_index *idx, uint8_t **bytes, size_t *nbytes);
int cjs_bzip2_index_load(const uint8_t *bytes, size_t nbytes, cjs_bz_index **idx);
int cjs_bzip2_index_info(const cjs_bz_index *idx, uint64_t *blocks, uint64_t *total_bytes, uint64_t *stream_bytes, int *multistream);
long cjs_bzip2_index_entries(const cjs_bz_index *idx, cjs_bz_index_entry *entries, long cap);
void cjs_bzip2_index_destroy(cjs_bz_index *idx);
/* cjs_bzip2_read_ranges: `count` ranges of the address space [0, total_bytes) = the output of cjs_bzip2_decompress(in, n,
 * the index's multistream flag).  Range k is [off[k], off[k] + len[k]) clipped to total_bytes, like pread: out_len[k] is what is
 * delivered; a range that starts at or past the end, or has len[k] == 0, has out_len 0 and status 0.  Ranges may overlap, repeat
 * and come in any order.  The results are packed back to back in range order: out_off[k] = the sum of the out_len in front.
 * The TOUCHED blocks are those of non-zero size that overlap a clipped range.  Each is decoded once, however many ranges want it,
 * and nothing else of the stream is read: not the other blocks' bytes, not a stream header, not a stream CRC; there is no magic
 * scan.  What is uploaded (host form: staged in one pinned buffer, one copy per pass; device form: gathered on the device by one
 * launch per pass) is the byte runs [bitpos >> 3, (end_bit + 7) >> 3) of the touched blocks, neighbours merged.  A touched block
 * is GOOD only if the block magic stands at its bitpos, it decodes under its entry's level, ends at the entry's end_bit, decodes
 * to the entry's size, and the CRC of its bytes equals the stored one, which equals the entry's.  A range that touches a bad block
 * gets status[k] = CJS_E_DATA_ERROR and out_len[k] = 0; other ranges are unaffected, and the call returns 0.
 * cjs_last_error_detail() is then the detail of the lowest-index failing range's first bad block: "Bad block CRC (got .. expected
 * ..)" when everything but the computed CRC agrees, otherwise "index does not match the stream at block <k>".
 * The touched blocks go through the decoder in ascending passes bounded by the batch decoder's group size (CJS_DEC_GROUP_BYTES of
 * upload), the inverse-BWT batch and the row budget of the block decode: device memory depends on a pass, never on the stream.
 * CJS_RANGE_PASS_BLOCKS (read at every call; for tests) caps the touched blocks of a pass.  A slice-gather kernel copies every
 * piece of every range from a pass's expanded blocks to its place, one launch per slab of pieces.
 * Host form: *out is allocated by the library (the rules of cjs_bzip2_decompress; cjs_free), the layout is made after the
 * verdicts (a failed range takes no room).  Device form (the memory rules of cjs_bzip2_decompress_device for d_in / d_out): the
 * layout comes from the index alone, so a failed range keeps its region, which holds unspecified bytes; a layout above out_cap:
 * CJS_E_OUTPUT_TOO_SMALL with *out_need set, before any launch (out_cap = 0, d_out = NULL: the size query); no byte of d_out at
 * or past min(out_cap, *out_need) is ever written.  On success *out_need = the end of the last region.
 * Negative returns are failures of the call: CJS_E_INVALID_ARG before the device is touched for NULL idx, NULL arrays with
 * count > 0 (out / out_need always), NULL in with n > 0, n != the index's stream_bytes and off[k] + len[k] overflowing; before any
 * launch for memory that is not the GPU's; CJS_E_NO_DEVICE, CJS_E_HIP, CJS_E_OUT_OF_MEMORY.  count == 0, or no touched block:
 * success without touching the device (host form: *out is a buffer all the same).  opts->device is honoured, n_devices and stats
 * are ignored.  CJS_DEBUG: one "[cjs range]" line per call on stderr (blocks, passes, H2D and D2H bytes). */
int cjs_bzip2_read_ranges(const uint8_t *in, size_t n, const cjs_bz_index *idx, const uint64_t *off, const uint64_t *len, size_t count,
                          uint8_t **out, size_t *out_off, size_t *out_len, int32_t *status, const cjs_opts *opts);
int cjs_bzip2_read_ranges_device(const uint8_t *d_in, size_t n, const cjs_bz_index *idx, const uint64_t *off, const uint64_t *len,
                                 size_t count, uint8_t *d_out, size_t out_cap, size_t *out_off, size_t *out_len, int32_t *status,
                                 size_t *out_need, const cjs_opts *opts);
/* cjs_bzip2_search: where `npat` byte patterns occur in a window of the address space of cjs_bzip2_read_ranges ([0, total_bytes)
 * of the index), found on the GPU: the decoded bytes never leave it, 16 bytes per match do.  Pattern j is pat[pat_off[j] ..
 * pat_off[j+1]) (pat_off: npat + 1 ascending offsets, pat_off[0] == 0; 1..CJS_SEARCH_MAX_PATTERNS patterns of
 * 1..CJS_SEARCH_MAX_PATTERN_BYTES bytes).  The window is [off, min(off + len, total_bytes)); the add saturates, so len =
 * UINT64_MAX means "to the end".  A match (o, j) exists iff pattern j's bytes stand at decoded offset o, o >= off and o + its
 * length <= the window's end.  Every start position counts: overlapping matches, matches of several patterns at one offset and
 * the matches of equal patterns are all reported.  With CJS_SEARCH_NOCASE the ASCII letters 'A'..'Z' equal 'a'..'z', in the
 * patterns and in the text; no other byte is folded.  The matches are sorted by (off, pattern); `found` gets the first
 * min(cap, n_matches) of them and nothing past those is written, info->n_matches counts them all (cap = 0, found = NULL: the count
 * query).  The list does not depend on how the blocks fall into passes and batches.
 * The TOUCHED blocks are those of non-zero size that overlap the window; each is decoded once and judged as cjs_bzip2_read_ranges
 * judges it, by the same passes (CJS_RANGE_PASS_BLOCKS, CJS_DEC_GROUP_BYTES, CJS_DEC_BATCH_ELEMS and CJS_DEC_ROW_BYTES act as
 * there).  A bad block does not fail the call: it returns 0, info->n_bad_blocks / first_bad_block say what was bad,
 * cjs_last_error_detail() is the first bad block's detail (read_ranges' two texts), and the matches are those that lie wholly
 * inside runs of consecutive GOOD blocks (blocks of size zero are transparent): nothing matches across a bad block.
 * Per decoded inverse-BWT batch two kernels run over 16 KiB tiles of the good runs -- one counts the matches of every tile, the
 * other, behind a scan of the counts, writes them at their rank -- so there is no atomic on the list and no sort.  The last
 * (longest pattern - 1) bytes of a batch's last run wait in a small buffer of the call until the next batch shows whether the run
 * goes on.  Device memory held: a pass's (as for cjs_bzip2_read_ranges), 8 bytes per tile, and 16 bytes per match delivered from
 * one batch.  A batch's matches reach `found` in one copy.
 * CJS_E_INVALID_ARG before the device is touched: NULL idx, info, pat or pat_off; NULL in with n > 0; NULL found with cap > 0;
 * n != the index's stream_bytes; npat outside 1..64; a pattern length outside 1..256; pat_off[0] != 0; undefined flag bits.
 * A window without a touched block: success without touching the device.  Device form: d_in is memory of the GPU (the memory
 * rules of cjs_bzip2_decompress_device; CJS_E_INVALID_ARG before any launch otherwise); found and info are HOST memory.
 * opts->device is honoured, n_devices and stats are ignored.  CJS_DEBUG: one "[cjs search]" line per call on stderr (blocks,
 * passes, upload, H2D and D2H bytes, matches). */
#define CJS_SEARCH_NOCASE 1u
#define CJS_SEARCH_MAX_PATTERNS 64
#define CJS_SEARCH_MAX_PATTERN_BYTES 256
typedef struct cjs_bz_match {
  uint64_t off;        /* decoded offset of the match's first byte */
  uint32_t pattern;    /* which pattern */
  uint32_t reserved;   /* 0 from cjs_bzip2_search; the match's length from cjs_bzip2_search_regex */
} cjs_bz_match;
typedef struct cjs_bz_search_info {
  uint64_t n_matches;       /* all matches of the window, also when more than cap */
  uint64_t n_bad_blocks;    /* touched blocks that were not GOOD */
  uint64_t first_bad_block; /* index of the first of them; ~0 if none */
  uint64_t blocks_decoded;  /* touched blocks */
} cjs_bz_search_info;
int cjs_bzip2_search(const uint8_t *in, size_t n, const cjs_bz_index *idx, const uint8_t *pat, const uint32_t *pat_off, uint32_t npat,
                     uint32_t flags, uint64_t off, uint64_t len, cjs_bz_match *found, size_t cap, cjs_bz_search_info *info,
                     const cjs_opts *opts);
int cjs_bzip2_search_device(const uint8_t *d_in, size_t n, const cjs_bz_index *idx, const uint8_t *pat, const uint32_t *pat_off,
                            uint32_t npat, uint32_t flags, uint64_t off, uint64_t len, cjs_bz_match *found, size_t cap,
                            cjs_bz_search_info *info, const cjs_opts *opts);
/* cjs_bzip2_search_regex: cjs_bzip2_search with patterns that are bounded regular expressions.  The arguments are those of
 * cjs_bzip2_search; pattern j is the TEXT pat[pat_off[j] .. pat_off[j+1]) of 1..1024 bytes, flags are CJS_SEARCH_NOCASE or 0.
 * A match (o, j, L) exists iff some string of 1..256 bytes matched by pattern j stands at decoded offset o, with o >= off, the
 * string inside the window, and the string inside one run of consecutive GOOD blocks (blocks of size zero are transparent).
 * L is the LONGEST such length, bounded by 256, by the window's end and by the run's end.  Matches longer than 256 bytes are not
 * seen.  A start position is still reported if a shorter match starts there.  `a.*b` finds every `a` with a `b` within the next
 * 255 bytes of its line, with L reaching to the last such `b`.  A record's `reserved` holds L.
 * No state is carried from byte to byte across tiles, batches or passes: every start position is judged on its own, by walking an
 * anchored automaton over at most 256 bytes in front of it, so segments, carry, tiles, the count-then-emit round and the bad-block
 * rules are those of cjs_bzip2_search, and so are these: every start position counts (overlapping matches, several patterns at
 * one offset); the list is sorted by (off, pattern); `found` gets the first min(cap, n_matches) and nothing past them is written;
 * cap = 0 with found = NULL is the count query; a bad block is reported in info and the detail text, the call returns 0 and
 * nothing matches across it; a window without a touched block succeeds without touching the device; the list does not depend on
 * CJS_RANGE_PASS_BLOCKS, CJS_DEC_GROUP_BYTES, CJS_DEC_BATCH_ELEMS or CJS_DEC_ROW_BYTES.
 * The dialect: patterns are byte strings, and where both Python's `re` on a bytes pattern (no flags, or re.IGNORECASE) and this
 * dialect accept a pattern they mean the same.  Accepted: literal bytes (bytes >= 0x80 are literals); \ before punctuation;
 * \n \r \t \f \v \xHH; \d \w \s \D \W \S (ASCII); `.` = any byte but 0x0A; bracket classes with ranges, negation and the
 * escapes above ([^a] matches 0x0A); ( ) and (?: ), both plain grouping; |; ? * + {m} {m,} {,n} {m,n} with bounds <= 256.  With
 * CJS_SEARCH_NOCASE 'A'..'Z' equal 'a'..'z' in pattern and text, classes included ([Z-a] matches z Z [ ` a A, [^A-C] neither b nor
 * B); no other byte folds.
 * Refusals, all before the device is touched, each with a detail text "pattern J, byte P: ...".  CJS_E_INVALID_ARG: the argument
 * errors of cjs_bzip2_search; npat outside 1..64; a pattern text outside 1..1024 bytes; a syntax error (unbalanced ( or [, a
 * quantifier with nothing to repeat or behind another, {m,n} with n < m or a bound above 256, a bad \x, an unescaped { that is no
 * quantifier); a pattern that matches the empty string.  CJS_E_UNSUPPORTED: what `re` has and this dialect does not (^ $ \b \B
 * \A \Z, backreferences, lookaround, lazy or possessive quantifiers, named groups, inline flags, any other escaped letter or
 * digit); a pattern whose minimised automaton has more than 255 states that a transition enters (the start state takes none of the
 * 255 when nothing leads back to it: x{256} is accepted); patterns whose tables together exceed CJS_REGEX_MAX_TABLE_BYTES.
 * Anchors are left out on purpose: a start position does not know the byte in front of it; lines are the line table's business.
 * CJS_DEBUG: one "[cjs regex]" line per call on stderr.
 * cjs_regex_check compiles only, without a device: per pattern the number of states of its automaton (the dead one not counted)
 * and the longest possible match, clamped to 256 (the largest of these sizes the halo and the carry); either array may be NULL.
 * cjs_stage_regex_scan EXISTS FOR TESTS; no product path calls it: it runs the compiled tables over the plain host buffer
 * text[0 .. n) with the per-position walk of the kernels; found gets the first min(cap, *n_found) of every (o, j, L) of the buffer
 * in (off, pattern) order, *n_found counts them all. */
#define CJS_REGEX_MAX_PATTERN_TEXT 1024
#define CJS_REGEX_MAX_TABLE_BYTES 32768
int cjs_bzip2_search_regex(const uint8_t *in, size_t n, const cjs_bz_index *idx, const uint8_t *pat, const uint32_t *pat_off,
                           uint32_t npat, uint32_t flags, uint64_t off, uint64_t len, cjs_bz_match *found, size_t cap,
                           cjs_bz_search_info *info, const cjs_opts *opts);
int cjs_bzip2_search_regex_device(const uint8_t *d_in, size_t n, const cjs_bz_index *idx, const uint8_t *pat, const uint32_t *pat_off,
                                  uint32_t npat, uint32_t flags, uint64_t off, uint64_t len, cjs_bz_match *found, size_t cap,
                                  cjs_bz_search_info *info, const cjs_opts *opts);
int cjs_regex_check(const uint8_t *pat, const uint32_t *pat_off, uint32_t npat, uint32_t flags, uint32_t *states, uint32_t *max_len);
int cjs_stage_regex_scan(const uint8_t *pat, const uint32_t *pat_off, uint32_t npat, uint32_t flags, const uint8_t *text, size_t n,
                         cjs_bz_match *found, size_t cap, size_t *n_found);
/* The line table of an indexed stream: seek by line, number offsets (`wc -l`, `sed -n 'a,bp'`, `bzgrep -n` over a .bz2 stream).
 * A NEWLINE is the byte 0x0A and no other (CR does not count).  With off[b] the decoded offset of block b of `idx`, total =
 * total_bytes, nl[b] the newlines among block b's decoded bytes, cum[b] the sum of nl[0..b) and N their total:
 *   lines are numbered from 0; start(0) = 0; for 1 <= k <= N start(k) = the decoded offset of the k-th newline (1-based) + 1;
 *   for k > N start(k) = total.  Line k is the bytes [start(k), start(k+1)), its newline included; line N is the unterminated
 *   tail and may be empty.  number(o) = the newlines in decoded bytes [0, min(o, total)): the line that byte o belongs to.
 * A cjs_bz_lines holds nl[] for one index; it is immutable once made and shared between threads like an index.
 * _build (and _build_device: d_in under the memory rules of cjs_bzip2_decompress_device) counts the newlines on the GPU in one
 * pass of the range engine over every block of non-zero size; four bytes per block come back.  A touched block that is not GOOD
 * by cjs_bzip2_read_ranges' rules fails the call: CJS_E_DATA_ERROR with that block's detail (the lowest such block), no table.
 * An index without a block of non-zero size: success without touching the device.  _create takes a caller's counts[count];
 * _save gives the serialised form (*bytes: malloc'd, cjs_free), _load reads it:
 *   40-byte header: the 8 bytes "CJSBZLN1", u32 version = 1, u32 flags = 0, u64 blocks, u64 total_bytes, u32 crc_fold (the
 *   index entries' stored CRCs folded from 0 as c = rol1(c) ^ crc, the stream-CRC rule), u32 reserved = 0; then `blocks` u32
 *   counts; everything little-endian.
 * _create and _load refuse with CJS_E_INVALID_ARG and a detail text, before any device is touched: wrong magic, version or
 * length; flag or reserved bits set; blocks, total_bytes or crc_fold not those of idx; counts[b] > size[b].  NULL arguments:
 * CJS_E_INVALID_ARG.  _info: any out pointer may be NULL.  _counts copies the first min(cap, blocks) counts and returns the
 * number of blocks.  A table belongs to one index: every call that takes both compares blocks, total_bytes and crc_fold again
 * and refuses with CJS_E_INVALID_ARG, "the line table is of another index".
 * _locate: start[k] = start(line[k]).  _number: line[k] = number(off[k]).  Queries may repeat and come in any order; count == 0
 * is a success.  The table alone answers line[k] == 0, line[k] > N, off[k] at a block's first byte and off[k] >= total: such a
 * query touches no block, and a call in which no query needs a block does not touch the device.  Else the TOUCHED block of a
 * locate query is the one block b with cum[b] < line[k] <= cum[b+1], of a number query the block that holds off[k].  Each is
 * decoded once, however many queries want it, judged as cjs_bzip2_read_ranges judges it and by the same passes
 * (CJS_RANGE_PASS_BLOCKS, CJS_DEC_GROUP_BYTES, CJS_DEC_BATCH_ELEMS and CJS_DEC_ROW_BYTES act as there).  A query whose block is
 * bad gets status[k] = CJS_E_DATA_ERROR and start / line 0; other queries are unaffected and the call returns 0;
 * cjs_last_error_detail() is then the detail of the lowest-index failing query's block.  Every tile of a touched block is
 * counted anyway, so a GOOD block whose newline count is not the table's fails its queries the same way, with the detail
 * "line table does not match the stream at block <b>".
 * Per decoded inverse-BWT batch, over 16 KiB tiles of the blocks (a tile never spans two blocks): one kernel counts the newlines
 * of every tile, one scans the counts per block, and one wave per query finds the r-th newline of its block (locate) or counts
 * those in front of its offset (number).  No atomics; the answers do not depend on how the blocks fall into passes and batches.
 * Eight bytes per query and four per touched block leave the GPU.  Device memory held: a pass's (as for cjs_bzip2_read_ranges),
 * 4 bytes per tile of the batch, and 16 bytes per query of the batch: never proportional to the stream.
 * CJS_E_INVALID_ARG before the device is touched: NULL idx or lines; NULL arrays with count > 0; NULL in with n > 0; n != the
 * index's stream_bytes; a foreign table.  All arrays are HOST memory in both forms.  opts->device is honoured, n_devices and
 * stats are ignored.  CJS_DEBUG: one "[cjs lines]" line per call on stderr (form, build / locate / number, queries, blocks
 * touched, passes, inverse-BWT batches, H2D and D2H bytes). */
typedef struct cjs_bz_lines cjs_bz_lines;
int cjs_bzip2_lines_build(const uint8_t *in, size_t n, const cjs_bz_index *idx, cjs_bz_lines **lines, const cjs_opts *opts);
int cjs_bzip2_lines_build_device(const uint8_t *d_in, size_t n, const cjs_bz_index *idx, cjs_bz_lines **lines, const cjs_opts *opts);
int cjs_bzip2_lines_create(const cjs_bz_index *idx, const uint32_t *counts, size_t count, cjs_bz_lines **lines);
int cjs_bzip2_lines_save(const cjs_bz_lines *lines, uint8_t **bytes, size_t *nbytes);
int cjs_bzip2_lines_load(const uint8_t *bytes, size_t nbytes, const cjs_bz_index *idx, cjs_bz_lines **lines);
int cjs_bzip2_lines_info(const cjs_bz_lines *lines, uint64_t *blocks, uint64_t *newlines, uint64_t *total_bytes);
long cjs_bzip2_lines_counts(const cjs_bz_lines *lines, uint32_t *counts, long cap);
void cjs_bzip2_lines_destroy(cjs_bz_lines *lines);
int cjs_bzip2_lines_locate(const uint8_t *in, size_t n, const cjs_bz_index *idx, const cjs_bz_lines *lines, const uint64_t *line,
                           size_t count, uint64_t *start, int32_t *status, const cjs_opts *opts);
int cjs_bzip2_lines_locate_device(const uint8_t *d_in, size_t n, const cjs_bz_index *idx, const cjs_bz_lines *lines,
                                  const uint64_t *line, size_t count, uint64_t *start, int32_t *status, const cjs_opts *opts);
int cjs_bzip2_lines_number(const uint8_t *in, size_t n, const cjs_bz_index *idx, const cjs_bz_lines *lines, const uint64_t *off,
                           size_t count, uint64_t *line, int32_t *status, const cjs_opts *opts);
int cjs_bzip2_lines_number_device(const uint8_t *d_in, size_t n, const cjs_bz_index *idx, const cjs_bz_lines *lines,
                                  const uint64_t *off, size_t count, uint64_t *line, int32_t *status, const cjs_opts *opts);
/* cjs_bzip2_line_keys: a fixed-size key per line of an indexed stream, hashed on the GPU while the blocks stand decoded there
 * (the primitive under `bzdiff`: a line diff of two streams is a host algorithm over 16 bytes per line instead of the text).
 * Lines are the line table's: line k is the bytes [start(k), start(k+1)), its newline included; line N is the unterminated tail.
 * With P = 2^61 - 1 and B1, B2 = 256 + (s mod (P - 256)), s the first and the second output of splitmix64 started at `seed`
 * (constants 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB; shifts 30, 27, 31), and for bytes b_0 .. b_{m-1}
 * H_B = sum (b_i + 1) * B^(m-1-i) mod P (the empty string: 0), a line's key is hash = H_B1 (always below 2^61), len = the low 32
 * bits of m, check = the low 32 bits of H_B2.  Two lines are taken as equal iff their records are equal: equality of lines up to
 * a collision (about 93 bits of hash, plus the length).  The bases are PUBLIC for a given seed, so a caller who faces crafted
 * input passes a seed of its own.  All three fields all-ones: "this line touches a bad block"; no key has that value.
 * The WINDOW is lines [first, min(first + count, N + 1)); the add saturates.  `keys` gets the first min(cap, lines in the window)
 * records and nothing past them is written; info->n_lines counts the window's lines (cap = 0, keys = NULL: the count query, which
 * the table alone answers without a device; so does every empty window).
 * The TOUCHED blocks come from the table alone: from the block that holds newline number `first` (1-based; block 0 when first is
 * 0) through the block that holds newline number first + count (the last block when there is no such newline), blocks of size
 * zero left out.  Each is decoded once and judged as cjs_bzip2_read_ranges judges it, by the same passes; the records do not
 * depend on CJS_RANGE_PASS_BLOCKS, CJS_DEC_GROUP_BYTES, CJS_DEC_BATCH_ELEMS or CJS_DEC_ROW_BYTES.
 * Per decoded inverse-BWT batch, over 16 KiB tiles of the blocks (a tile never spans two blocks): one kernel counts the newlines
 * of every tile and hashes the fragment behind its last newline, one per block scans the counts and chains those fragments
 * into every tile's carry-in, and -- once the host has seen that every GOOD block has the newlines the table says -- one writes
 * a record per newline at its rank (the fragment from the block's previous newline, or from its first byte) and, per block, the
 * fragment behind its last newline.  No atomics.  16 bytes per newline and 32 per block leave the GPU; the fragments of a line
 * that spans blocks, batches or passes are joined on the host (H is linear in the string), so no state stays on the device
 * between batches.  Device memory held: a pass's, 32 bytes per tile and 16 bytes per newline of the batch.
 * A GOOD block whose counted newlines differ from the table's fails the call: CJS_E_DATA_ERROR, "line table does not match the
 * stream at block <b>"; nothing is written at the table's ranks for it.  A bad block does not fail the call: it returns 0, info
 * and cjs_last_error_detail() follow cjs_bzip2_search's rules, and every line that by the table's account may have a byte in bad
 * block b gets the all-ones record: lines cum[b] .. cum[b+1].  (The last of them is included although it has no byte there when
 * the block's last byte is a newline: only the block's bytes could tell.)
 * CJS_E_INVALID_ARG before the device is touched: the argument errors of cjs_bzip2_lines_locate (NULL idx or lines; NULL in with
 * n > 0; n != the index's stream_bytes; a foreign table), NULL keys with cap > 0, NULL info.  keys and info are HOST memory in
 * both forms (d_in: the memory rules of cjs_bzip2_decompress_device).  opts->device is honoured.  CJS_DEBUG: one "[cjs linekeys]"
 * line per call on stderr (form, window, lines, blocks touched and bad, passes, batches, tiles, H2D and D2H bytes).
 * cjs_stage_line_keys EXISTS FOR TESTS; no product path calls it: the keys of the lines of the plain host buffer text[0 .. n),
 * by the same functions (csrc/line_key.h), without a device; *n_lines = newlines + 1.
 * cjs_line_keys_diff: the line diff of two key lists, on the host (no device).  Hunks are ascending; each replaces lines
 * [a_first, +a_count) of A by [b_first, +b_count) of B; at least one count is non-zero; neighbouring hunks are separated by at
 * least one common line; b_first = a_first - (earlier a_counts) + (earlier b_counts).  info->edits = sum (a_count + b_count),
 * common = (na + nb - edits) / 2.  The common prefix and suffix are trimmed, the rest goes through Myers' O(ND) search with the
 * linear-space middle-snake recursion: memory O(na + nb + max_edits), no stored trace.  If the shortest script has at most
 * max_edits edits (0: 16,384), edits is that minimum, na + nb - 2 LCS, and minimal = 1; otherwise everything between the common
 * prefix and suffix is one hunk and minimal = 0: still a valid, deterministic script.  `hunks` gets the first min(cap, n_hunks)
 * and nothing past them is written (cap = 0, hunks = NULL: the count query).  All-ones records never equal anything.
 * CJS_E_INVALID_ARG: NULL info; NULL a / b / hunks with na / nb / cap > 0. */
typedef struct cjs_bz_linekey {
  uint64_t hash;   /* H_B1, below 2^61 */
  uint32_t len;    /* the line's length in bytes, newline included (low 32 bits) */
  uint32_t check;  /* the low 32 bits of H_B2 */
} cjs_bz_linekey;
typedef struct cjs_bz_linekeys_info {
  uint64_t n_lines;         /* lines of the window, also when more than cap */
  uint64_t n_bad_blocks;    /* touched blocks that were not GOOD */
  uint64_t first_bad_block; /* index of the first of them; ~0 if none */
  uint64_t blocks_decoded;  /* touched blocks */
} cjs_bz_linekeys_info;
typedef struct cjs_bz_hunk {
  uint64_t a_first, a_count, b_first, b_count;
} cjs_bz_hunk;
typedef struct cjs_bz_ldiff_info {
  uint64_t n_hunks, edits, common;
  uint32_t minimal, reserved;
} cjs_bz_ldiff_info;
int cjs_bzip2_line_keys(const uint8_t *in, size_t n, const cjs_bz_index *idx, const cjs_bz_lines *lines, uint64_t first, uint64_t count,
                        uint64_t seed, cjs_bz_linekey *keys, size_t cap, cjs_bz_linekeys_info *info, const cjs_opts *opts);
int cjs_bzip2_line_keys_device(const uint8_t *d_in, size_t n, const cjs_bz_index *idx, const cjs_bz_lines *lines, uint64_t first,
                               uint64_t count, uint64_t seed, cjs_bz_linekey *keys, size_t cap, cjs_bz_linekeys_info *info,
                               const cjs_opts *opts);
int cjs_stage_line_keys(const uint8_t *text, size_t n, uint64_t seed, cjs_bz_linekey *keys, size_t cap, size_t *n_lines);
int cjs_line_keys_diff(const cjs_bz_linekey *a, size_t na, const cjs_bz_linekey *b, size_t nb, uint64_t max_edits, cjs_bz_hunk *hunks,
                       size_t cap, cjs_bz_ldiff_info *info);
/* cjs_keys_tally: the frequency table of a list of line keys (`... | sort | uniq -c | sort -rn | head` over keys), grouped on the
 * GPU: only the groups asked for leave it.
 * GROUPS: two records are one group iff all three fields are equal, the equality cjs_line_keys_diff uses.  An all-ones record
 * belongs to no group; info->n_bad counts them.  A group's `first` is the lowest index of a member in keys, `count` its size,
 * `key` the record.  info->n_keys = n, n_distinct = all groups, max_count = the size of the largest of them, n_groups = the groups
 * with min_count <= count and (max_count == 0 or count <= max_count): `uniq -d` is min_count = 2, `uniq -u` is max_count = 1.
 * ORDER of those groups: CJS_TALLY_BY_FIRST, ascending first occurrence, or CJS_TALLY_BY_COUNT, descending count with ties by
 * ascending first occurrence.  Both are total, so the output is fully determined: `out` gets the first min(cap, n_groups) groups
 * and nothing past them is written (cap = 0, out = NULL: the count query, which runs everything and writes nothing).  The order
 * of `sort` itself, by content, is NOT offered: keys do not order as lines do.
 * n == 0 is answered without a device.  n > 2^32 - 2: CJS_E_UNSUPPORTED (the sorter's indices are 32 bits).
 * On the device: a sort word len << 32 | check per record with its index as the value, a stable LSD radix sort over it, the hashes
 * gathered through that permutation and a second stable sort over them -- together the sort by the whole record with ties in input
 * order, the bad records last; a head flag per record from a compare of the whole record with its predecessor's, a scan, every
 * group's head position (count = the distance to the next head, first = the index at the head), the filter as a compaction by
 * scan, a sort of the kept groups by the order word and an emit of the first cap of them.  No atomic decides an order.  Besides
 * the groups the host reads four scalars.  Device memory: 37 bytes per key, the sorter's histograms and, in the host form, the
 * keys (16 bytes each) and the groups written.
 * cjs_keys_tally: keys and out are host memory.  cjs_keys_tally_device: both are memory of the GPU; d_keys must be 8-byte aligned
 * (a record array at an address that is no multiple of 16 is served) and d_out 16-byte aligned, anything else is refused.
 * CJS_E_INVALID_ARG before the device is touched: NULL info, NULL keys with n > 0, NULL out with cap > 0, an unknown order,
 * max_count != 0 below min_count, a misaligned pointer of the device form; before any launch: a pointer of the device form that is
 * not memory of the GPU.  opts->device is honoured.  info is host memory.
 * cjs_stage_keys_tally EXISTS FOR TESTS; no product path calls it: the same rule on the host with std::stable_sort
 * (csrc/tally_plan.h), without a device. */
typedef struct { cjs_bz_linekey key; uint64_t first; uint64_t count; } cjs_bz_tally;   /* 32 bytes */
typedef struct { uint64_t n_keys, n_bad, n_distinct, n_groups, max_count; } cjs_tally_info;
#define CJS_TALLY_BY_FIRST 0u   /* ascending first occurrence */
#define CJS_TALLY_BY_COUNT 1u   /* descending count, ties by ascending first occurrence */
int cjs_keys_tally(const cjs_bz_linekey *keys, size_t n, uint32_t order, uint64_t min_count, uint64_t max_count, cjs_bz_tally *out,
                   size_t cap, cjs_tally_info *info, const cjs_opts *opts);
int cjs_keys_tally_device(const cjs_bz_linekey *d_keys, size_t n, uint32_t order, uint64_t min_count, uint64_t max_count,
                          cjs_bz_tally *d_out, size_t cap, cjs_tally_info *info, const cjs_opts *opts);
int cjs_stage_keys_tally(const cjs_bz_linekey *keys, size_t n, uint32_t order, uint64_t min_count, uint64_t max_count,
                         cjs_bz_tally *out, size_t cap, cjs_tally_info *info);
/* cjs_bzip2_cut: fields or byte columns of the lines of an indexed stream (`bzcat x.bz2 | cut -f LIST` / `cut -b LIST`), selected
 * and packed on the GPU while the blocks stand decoded there: only the selected bytes leave it.
 * The WINDOW is lines [first, min(first + count, N + 1)) as the line table numbers them, as in cjs_bzip2_line_keys: line N is the
 * unterminated tail, the add saturates, info->n_lines is the clipped count.  A window starts at a line start.
 * The OUTPUT of one line (its bytes without the newline):
 *   CJS_CUT_FIELDS, delimiter d (any byte value but 0x0A): the fields are the line split at every d, numbered from 1; the
 *     selected fields that are present, in input order, joined by d, then "\n".  Per byte: a field byte is written iff its field
 *     is selected; the delimiter that opens field k iff k is selected and the selection holds a field below k; a newline always.
 *   CJS_CUT_BYTES: the bytes at the selected 1-based positions of the line, then "\n" (delim is ignored).
 *   The tail line, if it is inside the window and not empty, is written like any line with a "\n" appended; an empty tail line
 *   writes nothing.
 * The output of the call is the concatenation: what `cut -d d -f LIST` / `cut -b LIST` writes under LC_ALL=C, with ONE
 * DIFFERENCE: a line WITHOUT the delimiter is a line of one field here (GNU cut prints such a line whole whatever the list says).
 * -s, --complement and --output-delimiter are not offered.
 * The SELECTION: 1 .. 64 ranges, 1-based and closed, 1 <= lo <= hi, hi == 0xFFFFFFFF: to the end of the line; they may overlap
 * and come in any order (the library sorts and merges them).  The unit counter of a line (delimiters, or bytes) is 32 bits and
 * saturates at 0xFFFFFFFE: every further unit of such a line keeps the last number, nothing wraps.
 * The TOUCHED blocks are those of cjs_bzip2_line_keys, by the same passes.  The output has no place for a hole: a touched block
 * that is not GOOD fails the call with CJS_E_DATA_ERROR, cjs_last_error_detail() being the text cjs_bzip2_read_ranges gives for
 * that block, info->n_bad_blocks / first_bad_block filled (host form: no buffer; device form: unspecified bytes below out_cap).
 * A block whose newlines differ from the table's: CJS_E_DATA_ERROR, "line table does not match the stream at block <k>".
 * Per decoded inverse-BWT batch, over 16 KiB tiles of the blocks: a summary per tile (newlines, units behind the last newline), one
 * workgroup chains the summaries across the tiles and blocks of the batch from the state the previous batch left (line number,
 * unit counter, open line: carried ON THE DEVICE side of the call, a few words per batch come back), a count per tile, a scan, and
 * an emit that packs the tile's selected bytes in LDS and stores them at the scanned offset.  No atomics decide an order.  The
 * result does not depend on CJS_RANGE_PASS_BLOCKS, CJS_DEC_GROUP_BYTES, CJS_DEC_BATCH_ELEMS or CJS_DEC_ROW_BYTES.
 * Host form: *out is allocated by the library (cjs_free) and grows batch by batch; a buffer is returned even for empty output.
 * Device form: no byte of d_out at or past out_cap is ever written; output above out_cap: the remaining passes still run to count
 * and the call returns CJS_E_OUTPUT_TOO_SMALL with *out_need = the full size (d_out = NULL, out_cap = 0: the size query, on the
 * same path).  On success *out_need = the bytes written.  The window's bytes + 1 are always room enough.
 * CJS_E_INVALID_ARG before the device is touched: nsel == 0 or > 64, NULL sel, lo == 0, lo > hi, delim > 255, delim == 0x0A in
 * fields mode, an unknown mode, NULL idx / lines / info / out / out_n / out_need, NULL in with n > 0, NULL d_out with out_cap > 0,
 * n != the index's stream_bytes, a foreign table.  CJS_DEBUG: one "[cjs cut]" line per call on stderr.
 * cjs_stage_cut EXISTS FOR TESTS; no product path calls it: the same rule walked byte by byte over the plain host buffer
 * text[0 .. n) (csrc/cut_plan.h), without a device.  *out_n = the full size; above cap: CJS_E_OUTPUT_TOO_SMALL, out[0 .. cap) written.
 * cjs_cut_list_parse: a cut-style LIST ("1,3-5,7-", "-4") as ranges; CJS_E_INVALID_ARG for an empty list or item, a zero, a
 * decreasing range, a "-" alone, any other character, a number above 0xFFFFFFFE, more than `cap` items. */
typedef struct { uint32_t lo, hi; } cjs_cut_range;   /* 1-based, closed; hi == 0xFFFFFFFF: to the end of the line */
typedef struct { uint64_t n_lines, out_bytes, blocks_decoded, n_bad_blocks, first_bad_block; } cjs_bz_cut_info;
#define CJS_CUT_FIELDS 0u
#define CJS_CUT_BYTES  1u
int cjs_bzip2_cut(const uint8_t *in, size_t n, const cjs_bz_index *idx, const cjs_bz_lines *lines, uint64_t first, uint64_t count,
                  uint32_t mode, uint32_t delim, const cjs_cut_range *sel, uint32_t nsel, uint8_t **out, size_t *out_n,
                  cjs_bz_cut_info *info, const cjs_opts *opts);
int cjs_bzip2_cut_device(const uint8_t *d_in, size_t n, const cjs_bz_index *idx, const cjs_bz_lines *lines, uint64_t first,
                         uint64_t count, uint32_t mode, uint32_t delim, const cjs_cut_range *sel, uint32_t nsel, uint8_t *d_out,
                         size_t out_cap, size_t *out_need, cjs_bz_cut_info *info, const cjs_opts *opts);
int cjs_stage_cut(const uint8_t *text, size_t n, uint32_t mode, uint32_t delim, const cjs_cut_range *sel, uint32_t nsel,
                  uint8_t *out, size_t cap, size_t *out_n);
int cjs_cut_list_parse(const char *list, cjs_cut_range *sel, uint32_t cap, uint32_t *nsel);
/* cjs_bzip2_tally: the frequency table of the lines of an indexed stream (`bzcat x.bz2 | sort | uniq -c | sort -rn | head`): the
 * keys of cjs_bzip2_line_keys, made by the same passes over the same touched blocks of the same window, stay in GPU memory and are
 * grouped there as by cjs_keys_tally; the first min(cap, n_groups) groups come down, `first` being an absolute line number of the
 * table (the window's first + the index in the window).  out and info are HOST memory in both forms.
 * mode CJS_TALLY_LINES: the key of a line is its cjs_bzip2_line_keys record, newline included, with one rule for the tail: a tail
 * line that is not empty is keyed as if it ended in a newline (so it groups with the earlier lines of its content), an empty tail
 * is no line (info->n_lines does not count it), as in cjs_bzip2_cut.  delim, sel and nsel are ignored.
 * modes CJS_CUT_FIELDS / CJS_CUT_BYTES ("which values of column 3 occur how often"): the key of a line is the key of its
 * cjs_bzip2_cut output line, the selected bytes plus "\n"; cut's stated difference from GNU cut holds here too.  A composition:
 * cjs_bzip2_cut_device into a pooled device buffer of the touched blocks' bytes + 1 (the host form uploads the stream first), the
 * keys of that text's lines by the kernels of cjs_bzip2_line_keys over pieces of at most 900,000 bytes, which they see as they
 * see a block (a piece's record count comes down before its records are written at their ranks; the pieces are joined on the host
 * as blocks are), then the grouping.  A bad block in the window fails the call exactly as cjs_bzip2_cut fails, with its code,
 * detail and info->n_bad_blocks / first_bad_block; the selection's argument checks are cut's.  Device memory on top of the
 * figures below: the stream (host form), the touched blocks' bytes + 1, and about 100 bytes per 16 KiB of them.
 * The rest of this comment is the whole-line mode's.
 * A line that may touch a bad block (an all-ones record of cjs_bzip2_line_keys) is grouped nowhere and counted in
 * info->n_bad_lines; the call does not fail, info->n_bad_blocks / first_bad_block and cjs_last_error_detail() follow
 * cjs_bzip2_line_keys.  The sum of the counts of all groups is n_lines - n_bad_lines.  A block whose newlines differ from the
 * table's: CJS_E_DATA_ERROR as there.  cap = 0, out = NULL: the count query, which runs everything.  An empty window, and a
 * stream without a block, are answered without a device.
 * The records do not cross the bus: a block's whole-line records go to their ranks in a device array of the window's lines by
 * device-to-device copies, 16 bytes per touched block come down beside its tail fragment, the host joins the lines that span
 * blocks as cjs_bzip2_line_keys does, and those records (at most one per touched block, and the tail) go up as patches at the
 * end, the lines of bad blocks as fills.  Device memory beyond a pass's: 53 bytes per line of the window (16 for its record, 37
 * for the grouping), the sorter's histograms, 24 bytes per touched block and 32 bytes per group that can come down (min(cap,
 * the window's lines)), all sized from the table and taken before the first pass (failure: CJS_E_OUT_OF_MEMORY).  A window of
 * more than 2^32 - 2 lines: CJS_E_UNSUPPORTED, checked before the device is touched, in every mode.
 * CJS_E_INVALID_ARG before the device is touched: the argument errors of cjs_bzip2_line_keys (out for keys), an unknown order,
 * max_count != 0 below min_count, an unknown mode, the selection errors of cjs_bzip2_cut.  opts->device is honoured.  CJS_DEBUG:
 * one "[cjs tally]" line per call (form, window, mode, ..., H2D and D2H bytes).
 * cjs_stage_bzip2_tally_limit and cjs_stage_text_keys_device EXIST FOR TESTS; no product path calls them.  The first is the
 * whole-line tally by count with the limit on the window's lines as an argument (exactly one of in / d_in).  The second is the
 * middle step of the tally of a cut: the keys of the lines of plain text in GPU memory, one per newline and one for the tail
 * whatever it is (what cjs_stage_line_keys gives), brought down to keys (host); piece_bytes 0: 900,000. */
typedef struct { uint64_t n_lines, n_bad_lines, n_distinct, n_groups, max_count, blocks_decoded, n_bad_blocks, first_bad_block; } cjs_bz_tally_info;
#define CJS_TALLY_LINES 2u   /* beside CJS_CUT_FIELDS 0u and CJS_CUT_BYTES 1u */
int cjs_bzip2_tally(const uint8_t *in, size_t n, const cjs_bz_index *idx, const cjs_bz_lines *lines, uint64_t first, uint64_t count,
                    uint64_t seed, uint32_t mode, uint32_t delim, const cjs_cut_range *sel, uint32_t nsel, uint32_t order,
                    uint64_t min_count, uint64_t max_count, cjs_bz_tally *out, size_t cap, cjs_bz_tally_info *info, const cjs_opts *opts);
int cjs_bzip2_tally_device(const uint8_t *d_in, size_t n, const cjs_bz_index *idx, const cjs_bz_lines *lines, uint64_t first,
                           uint64_t count, uint64_t seed, uint32_t mode, uint32_t delim, const cjs_cut_range *sel, uint32_t nsel,
                           uint32_t order, uint64_t min_count, uint64_t max_count, cjs_bz_tally *out, size_t cap,
                           cjs_bz_tally_info *info, const cjs_opts *opts);
int cjs_stage_bzip2_tally_limit(const uint8_t *in, const uint8_t *d_in, size_t n, const cjs_bz_index *idx, const cjs_bz_lines *lines,
                                uint64_t first, uint64_t count, uint64_t max_lines, cjs_bz_tally *out, size_t cap,
                                cjs_bz_tally_info *info, const cjs_opts *opts);
int cjs_stage_text_keys_device(const uint8_t *d_text, size_t n, uint64_t seed, cjs_bz_linekey *keys, size_t cap, size_t *n_lines,
                               size_t piece_bytes, const cjs_opts *opts);
/* cjs_text_sort / cjs_bzip2_sort: the lines of a text, or of a window of an indexed stream (`bzcat x.bz2 | sort`, `| sort | head`,
 * `| sort -u`, `| cut .. | sort`), ordered by content on the GPU: only line numbers, counts and, when asked for, the sorted text
 * leave it (the rule is csrc/sort_plan.h).
 * A LINE is the bytes between newlines without the newline; a tail that is not empty is a line, an empty tail is none (the tail rule
 * of cjs_bzip2_cut).  Lines are numbered from 0.  The ORDER is bytewise as memcmp, a proper prefix before the longer line
 * (LC_ALL=C sort); equal lines go by ascending line number.  CJS_SORT_REVERSE: descending content, equal lines still by ascending
 * line number.  CJS_SORT_UNIQUE: one entry per run of equal lines, its lowest line number, the run's size as its count.  Both
 * orders are total: the output is fully determined.
 * lines_out gets the first min(cap, info->n_out) line numbers in that order, counts_out (may be NULL) their counts (without
 * CJS_SORT_UNIQUE all ones); nothing past those is written.  info->n_lines = the lines, n_distinct = the runs of equal lines, n_out
 * = what the flags select of them, rounds = the sort rounds run (at most (longest line + 8) / 7).  cap = 0 without text: the count
 * query, which runs everything.
 * TEXT is optional (text_out and text_n both NULL: none): the emitted lines, i.e. the first min(cap, n_out), each followed by
 * "\n".  info->text_bytes is the size that text has for all n_out lines, whatever cap is.  Host forms: *text_out is allocated by
 * the library (cjs_free), also for empty output.  Device forms: d_text_out of text_cap bytes; a text above text_cap returns
 * CJS_E_OUTPUT_TOO_SMALL with *text_n = the need and writes no byte of d_text_out (d_text_out = NULL, text_cap = 0 with text_n
 * given: the size query); lines_out and counts_out are complete then.
 * cjs_text_sort: everything is host memory; n == 0 needs no device.  cjs_text_sort_device: d_text, d_lines_out, d_counts_out and
 * d_text_out are memory of the GPU (host pointers: CJS_E_INVALID_ARG); d_text at any alignment, and no byte outside
 * [d_text, d_text + n) is read; the two output arrays 8-byte aligned; info and text_n are host memory.  More than 2^32 - 2 bytes
 * or lines: CJS_E_UNSUPPORTED.  CJS_E_INVALID_ARG: NULL text with n > 0, NULL lines_out with cap > 0, one of text_out / text_n
 * without the other, NULL info, an unknown flag.
 * How: newline counts per 4 KiB tile and a scan give every line's start; round r keys every line of an active group by its ROUND
 * WORD at depth 7 r (bytes [7 r, 7 r + 7) big-endian, zero-padded, << 8 | min(7, max(0, len - 7 r)): padding sorts below 0x00),
 * two stable runs of the radix sorter order the active lines by (group, word), head flags and a scan split the groups, and the
 * host reads one scalar per round: the lines still active.  A group is done with one member or a word that has ended.  Two equal
 * lines of L bytes cost L / 7 rounds.  No atomics.  What comes down beyond the entries and the text asked for is 48 bytes of
 * scalars (56 with text) and 8 bytes PER ROUND: under 1 KiB for ten entries while the rounds stay below a hundred, about 46 KB
 * where two equal lines of 40 KiB take 5,852 rounds.
 * cjs_bzip2_sort / cjs_bzip2_sort_device: the window is lines [first, min(first + count, N + 1)) of the table as in cjs_bzip2_cut.
 * mode CJS_SORT_LINES: whole lines (the cut with bytes 1-).  modes CJS_CUT_FIELDS / CJS_CUT_BYTES: the cut of each line is what
 * is sorted and what the text holds (`bzcat | cut .. | sort`); the cut writes one line per input line, so the line numbers are
 * those of whole lines, `sort -s -t D -k ..` over them.  Line numbers are absolute: window line k is first + k.  A composition:
 * cjs_bzip2_cut_device into a pooled device buffer of the touched blocks' bytes + 1 (the host form uploads the stream first),
 * then the primitive.  lines_out, counts_out, info and text_n are HOST memory in both forms; the device form takes the stream and
 * gives the text in GPU memory.  The argument checks are those of cjs_bzip2_cut (out / out_n for lines_out / text) and of the
 * primitive, before the device is touched.  A bad block in the window fails the call as it fails cjs_bzip2_cut: code, detail,
 * info->n_bad_blocks / first_bad_block.  Touched blocks above 2^32 - 2 bytes or a window above 2^32 - 2 lines:
 * CJS_E_UNSUPPORTED.  All device memory (the text, 90 bytes per line of the window, 8 bytes per 4 KiB of text, the sorter's
 * histograms, the outputs) is sized from the tables and taken before the cut runs (failure: CJS_E_OUT_OF_MEMORY).  An empty
 * window needs no device.  CJS_DEBUG: one "[cjs sort]" line per call (lines, rounds, H2D and D2H bytes beyond the cut).
 * cjs_stage_text_sort and cjs_stage_bzip2_sort_limit EXIST FOR TESTS; no product path calls them.  The first is the same rounds
 * on the host (csrc/sort_plan.h), without a device.  The second is the whole-line stream sort with the limits on the touched
 * blocks' bytes and the window's lines as arguments (exactly one of in / d_in; no text). */
typedef struct { uint64_t n_lines, n_out, n_distinct, text_bytes, rounds, blocks_decoded, n_bad_blocks, first_bad_block; } cjs_bz_sort_info;   /* 64 bytes */
#define CJS_SORT_REVERSE 1u
#define CJS_SORT_UNIQUE  2u
#define CJS_SORT_LINES   2u   /* mode, beside CJS_CUT_FIELDS 0u and CJS_CUT_BYTES 1u, as CJS_TALLY_LINES */
int cjs_text_sort(const uint8_t *text, size_t n, uint32_t flags, uint64_t *lines_out, uint64_t *counts_out, size_t cap,
                  uint8_t **text_out, size_t *text_n, cjs_bz_sort_info *info, const cjs_opts *opts);
int cjs_text_sort_device(const uint8_t *d_text, size_t n, uint32_t flags, uint64_t *d_lines_out, uint64_t *d_counts_out, size_t cap,
                         uint8_t *d_text_out, size_t text_cap, size_t *text_n, cjs_bz_sort_info *info, const cjs_opts *opts);
int cjs_bzip2_sort(const uint8_t *in, size_t n, const cjs_bz_index *idx, const cjs_bz_lines *lines, uint64_t first, uint64_t count,
                   uint32_t mode, uint32_t delim, const cjs_cut_range *sel, uint32_t nsel, uint32_t flags, uint64_t *lines_out,
                   uint64_t *counts_out, size_t cap, uint8_t **text_out, size_t *text_n, cjs_bz_sort_info *info, const cjs_opts *opts);
int cjs_bzip2_sort_device(const uint8_t *d_in, size_t n, const cjs_bz_index *idx, const cjs_bz_lines *lines, uint64_t first,
                          uint64_t count, uint32_t mode, uint32_t delim, const cjs_cut_range *sel, uint32_t nsel, uint32_t flags,
                          uint64_t *lines_out, uint64_t *counts_out, size_t cap, uint8_t *d_text_out, size_t text_cap, size_t *text_n,
                          cjs_bz_sort_info *info, const cjs_opts *opts);
int cjs_stage_text_sort(const uint8_t *text, size_t n, uint32_t flags, uint64_t *lines_out, uint64_t *counts_out, size_t cap,
                        cjs_bz_sort_info *info);
int cjs_stage_bzip2_sort_limit(const uint8_t *in, const uint8_t *d_in, size_t n, const cjs_bz_index *idx, const cjs_bz_lines *lines,
                               uint64_t first, uint64_t count, uint64_t max_bytes, uint64_t max_lines, uint32_t flags,
                               uint64_t *lines_out, uint64_t *counts_out, size_t cap, cjs_bz_sort_info *info, const cjs_opts *opts);
/* cjs_bzip2_compare: `cmp` over the address space of cjs_bzip2_read_ranges ([0, total_bytes) of the index), done on the GPU: is
 * the decoded stream equal to `other`, and if not, where and with which bytes?  The decoded bytes never leave the GPU, 16 bytes
 * per reported difference do.  other[k] is compared with decoded byte other_off + k.  The COMPARED SPAN is
 * [max(off, other_off), min(off + len, total_bytes, other_off + other_n)) minus the bad blocks; off + len saturates, so len =
 * UINT64_MAX means "to the end".  A difference is one byte position of the span where the two sides differ: `a` is the stream's
 * byte, `b` the other side's.  `diffs` gets the first min(cap, n_diffs) differences in ascending offset and nothing past those is
 * written; info->n_diffs counts them all, info->first_diff is the lowest offset (~0: none), info->compared the bytes actually
 * compared (cap = 0, diffs = NULL: the count query).  The list does not depend on how the blocks fall into passes, batches and
 * tiles.  Lengths are not judged: total_bytes is in the index and other_n is the caller's, who turns the two into "equal" or
 * "EOF on ..".
 * The TOUCHED blocks are those of non-zero size that overlap the span without the bad blocks taken out; each is decoded once and
 * judged as cjs_bzip2_read_ranges judges it, by the same passes (CJS_RANGE_PASS_BLOCKS, CJS_DEC_GROUP_BYTES, CJS_DEC_BATCH_ELEMS
 * and CJS_DEC_ROW_BYTES act as there).  A bad block does not fail the call: it returns 0, info->n_bad_blocks / first_bad_block
 * say what was bad, cjs_last_error_detail() is the first bad block's detail (read_ranges' two texts), and its bytes are neither
 * compared nor counted in `compared`.
 * Per decoded inverse-BWT batch two kernels run over 16 KiB tiles of the good runs -- one counts the differing bytes of every
 * tile in one pass over its bytes (16 bytes per lane and step, aligned vector loads of both sides bounded to their sources, the
 * other side brought into phase by a byte funnel shift), the other, behind a scan of the counts and only when there is something
 * to deliver, writes the differences at their rank -- so there is no atomic on the list and no sort.  Device memory held: a
 * pass's (as for cjs_bzip2_read_ranges), 16 bytes per tile, 16 bytes per difference delivered from one batch; host form: the
 * bytes of `other` under the batch's good blocks (the only part of `other` that is uploaded).
 * cjs_bzip2_compare_streams: the other side is a second indexed stream B.  The span is [off, min(off + len, total_bytes of A,
 * total_bytes of B)); it is walked in windows of CJS_COMPARE_WINDOW_BYTES decoded bytes (read at every call; default 64 MiB):
 * B's window is read into one device buffer by the range reads' core, one range per touched block of B, so that a bad block of
 * B costs only its own bytes (reported in n_bad_blocks_b / first_bad_block_b, not compared); then A's blocks of the window are
 * compared against it.  A block that straddles a window edge is decoded once per window it touches.  Device memory: one window
 * plus a pass's, whatever the streams' sizes.  The detail is that of A's first bad block, or of B's if A has none.
 * CJS_E_INVALID_ARG before the device is touched: NULL idx or info; NULL in with n > 0; NULL other with other_n > 0; NULL diffs
 * with cap > 0; n != the index's stream_bytes (for either stream).  An empty span: success with zeros without touching the device.
 * Device forms: d_in and d_other (d_a and d_b) are memory of the GPU (the memory rules of cjs_bzip2_decompress_device;
 * CJS_E_INVALID_ARG before any launch otherwise); diffs and info are HOST memory.  opts->device is honoured, n_devices and stats
 * are ignored.  CJS_DEBUG: one "[cjs compare]" line per call on stderr (form, window, blocks touched and bad, passes and batches,
 * windows, tiles, H2D and D2H bytes, n_diffs, compared). */
typedef struct cjs_bz_diff {
  uint64_t off;        /* decoded offset of the differing byte */
  uint8_t a, b;        /* the stream's byte, the other side's */
  uint8_t reserved[6]; /* 0 */
} cjs_bz_diff;
typedef struct cjs_bz_cmp_info {
  uint64_t n_diffs;           /* all differences of the span, also when more than cap */
  uint64_t first_diff;        /* the lowest differing offset; ~0 if none */
  uint64_t compared;          /* bytes actually compared */
  uint64_t n_bad_blocks;      /* touched blocks (of the stream `idx` / `idx_a` is of) that were not GOOD */
  uint64_t first_bad_block;   /* index of the first of them; ~0 if none */
  uint64_t blocks_decoded;    /* touched blocks of that stream */
  uint64_t n_bad_blocks_b;    /* two-stream forms: the same for stream B; else 0 */
  uint64_t first_bad_block_b; /* ~0 if none */
} cjs_bz_cmp_info;
int cjs_bzip2_compare(const uint8_t *in, size_t n, const cjs_bz_index *idx, const uint8_t *other, size_t other_n, uint64_t other_off,
                      uint64_t off, uint64_t len, cjs_bz_diff *diffs, size_t cap, cjs_bz_cmp_info *info, const cjs_opts *opts);
int cjs_bzip2_compare_device(const uint8_t *d_in, size_t n, const cjs_bz_index *idx, const uint8_t *d_other, size_t other_n,
                             uint64_t other_off, uint64_t off, uint64_t len, cjs_bz_diff *diffs, size_t cap, cjs_bz_cmp_info *info,
                             const cjs_opts *opts);
int cjs_bzip2_compare_streams(const uint8_t *a, size_t na, const cjs_bz_index *idx_a, const uint8_t *b, size_t nb,
                              const cjs_bz_index *idx_b, uint64_t off, uint64_t len, cjs_bz_diff *diffs, size_t cap,
                              cjs_bz_cmp_info *info, const cjs_opts *opts);
int cjs_bzip2_compare_streams_device(const uint8_t *d_a, size_t na, const cjs_bz_index *idx_a, const uint8_t *d_b, size_t nb,
                                     const cjs_bz_index *idx_b, uint64_t off, uint64_t len, cjs_bz_diff *diffs, size_t cap,
                                     cjs_bz_cmp_info *info, const cjs_opts *opts);
/* Streaming form of cjs_bzip2_compress: the input is written in pieces of any size (zero included), the .bz2 stream is read in
 * pieces of any size, and the bytes read, in order, once cjs_bzip2_enc_finish has returned, are exactly what
 * cjs_bzip2_compress(all written bytes, level) returns -- for every level, every split of the input, every chunk_bytes and every
 * pattern of reads; no input at all gives the 14-byte stream 'BZh<level>', end-of-stream magic, CRC 0.
 * The encoder works in steps of up to chunk_bytes new input bytes (0 = the default, 64 MiB; clamped to 64 KiB .. 1 GiB).  The
 * device and pinned host memory it holds depend on chunk_bytes and level, never on the total written: two pinned and two device
 * staging chunks, the device input buffer (chunk_bytes + the carried block's input; it grows when a step finds no complete block,
 * up to ~51 x level x 100000 bytes of runs), two packed-output buffers and a workspace of ~70 B per byte of chunk_bytes.
 * _write takes all n bytes; it blocks only while both staging chunks wait for the device.  One worker thread per encoder runs the
 * steps beside the caller.  Output not yet read is kept in host memory; _pending is the number of bytes _read can hand out now.
 * The worker hands a step's output over only when all earlier output has been read, or while the caller waits for it inside
 * _write or _finish: a caller that drains after each write of at most chunk_bytes never holds more than one step's output, and
 * one that never reads is never held up.  _read copies up to cap bytes and never blocks.
 * _finish says that no more input follows and returns when the whole stream is ready to be read (after a drain that is the
 * output of at most four steps: those still under way and the final one); a second _finish is harmless.
 * The memory is given back by _destroy (or by the failure that ended the worker), not by _finish.
 * level outside 1..9: CJS_E_BAD_LEVEL; NULL e, NULL in with n > 0, NULL out with cap > 0, NULL got: CJS_E_INVALID_ARG; both before
 * the device is touched (the device is first touched by the first write of n > 0 bytes).  _write after _finish:
 * CJS_E_INVALID_ARG.  After any failing call the encoder stays failed: every later call returns the same code (and _pending 0);
 * _destroy is always safe.  opts->device is honoured, n_devices and stats are ignored.  Encoders are independent of each other
 * and of the contexts cjs_bzip2_compress keeps; one encoder is driven by one thread at a time. */
typedef struct cjs_bz_enc cjs_bz_enc;
int cjs_bzip2_enc_create(cjs_bz_enc **e, int level, size_t chunk_bytes, const cjs_opts *opts);
int cjs_bzip2_enc_write(cjs_bz_enc *e, const uint8_t *in, size_t n);
int cjs_bzip2_enc_finish(cjs_bz_enc *e);
size_t cjs_bzip2_enc_pending(const cjs_bz_enc *e);
int cjs_bzip2_enc_read(cjs_bz_enc *e, uint8_t *out, size_t cap, size_t *got);
void cjs_bzip2_enc_destroy(cjs_bz_enc *e);
/* Compress and hand out the tables of the stream: the indexed forms return, beside the stream, the cjs_bz_index of exactly that
 * stream and, if asked, its cjs_bz_lines -- what cjs_bzip2_index_build and cjs_bzip2_lines_build give on the result, entry for
 * entry, without the table pass and the full decode those two take: the compressor holds every field when it packs (a block's
 * bits, CRC and input span; the newlines are one more read of the input, which is in device memory then).  The stream is
 * byte-identical to the plain call's; the plain calls are untouched.  The index is multistream = 0.  *idx / *lines are new objects
 * (cjs_bzip2_index_destroy / cjs_bzip2_lines_destroy).  lines == NULL: no line table is made (and the input is not read again).
 * idx == NULL: CJS_E_INVALID_ARG.  On any failure *idx and *lines are NULL (and *out of the host form), nothing leaks.
 * cjs_bzip2_compress_indexed: cjs_bzip2_compress' arguments, rules and modes (one device; opts->n_devices > 1; inputs above
 * CJS_CHUNK_BYTES in waves): every shard hands its blocks' rows to the calling thread, which sets them at the shard's bit offset.
 * cjs_bzip2_compress_device_indexed: cjs_bzip2_compress_device's arguments and rules; 16 bytes per block come down with the
 * packer's scalars, in front of the one synchronisation the plain call makes.  The context keeps 16 bytes per block of device and
 * pinned memory from its first indexed call on.
 * Streaming: an encoder made with CJS_FLAG_ENC_INDEX (and CJS_FLAG_ENC_LINES) in opts->flags keeps 36 bytes of host memory per
 * block written -- the only thing that grows with the stream -- and cjs_bzip2_enc_index hands the tables out once _finish has
 * returned 0, any number of times, whether or not the output has been read.  Before that, for an encoder made without the flag,
 * for lines != NULL without CJS_FLAG_ENC_LINES, and for NULL e or idx: CJS_E_INVALID_ARG (the encoder does not stay failed for
 * it); a failed encoder returns its code.  No input at all: an index of no entries, stream_bytes 14.
 * Not covered: cjs_bzip2_compress_batch[_device], the cjs_bzip2_shard_* phases, the decoder, BWTC. */
#define CJS_FLAG_ENC_INDEX 4u   /* cjs_bzip2_enc_create: keep the index of the stream being written */
#define CJS_FLAG_ENC_LINES 8u   /* ... and its line table (implies CJS_FLAG_ENC_INDEX) */
int cjs_bzip2_compress_indexed(const uint8_t *in, size_t n, int level, uint8_t **out, size_t *out_n, cjs_bz_index **idx,
                               cjs_bz_lines **lines, const cjs_opts *opts);
int cjs_bzip2_enc_index(cjs_bz_enc *e, cjs_bz_index **idx, cjs_bz_lines **lines);
/* Streaming form of cjs_bzip2_decompress: the .bz2 stream is written in pieces of any size, the decoded bytes are read in pieces
 * of any size, and the bytes read, in order, are exactly what cjs_bzip2_decompress(all written bytes, multistream) returns; a
 * stream that fails fails with the same code and the same cjs_last_error_detail().  The device and host memory a decoder holds
 * depend on chunk_bytes, out_bytes and the stream's level, never on the bytes written or produced.
 * A PULL model, unlike the encoder (a block of ~45 stream bytes can decode to 46 MB): _write only copies into the input window,
 * as much as it has room for (*taken, which may be 0), and never starts GPU work.  _read hands out bytes still held from the
 * last step; when none are left it runs steps while one is due and hands out from the first that produced bytes.  *got == 0
 * with return code 0 means "write more, or finish"; after _finish it means the stream has ended (_done returns 1).
 * PROGRESS: after a _write that took fewer than n bytes, calling _read until *got == 0 guarantees that the next _write takes at
 * least one byte.  Once the stream's end has been decided (the end-of-stream of a non-multistream decoder, or a failure that is
 * still waiting behind unread bytes) later writes are taken and dropped: the reference never reads those bytes.
 * A step is due when chunk_bytes new stream bytes wait (0 = the default, 64 MiB, or CJS_DEC_CHUNK_BYTES; clamped to 64 KiB ..
 * 1 GiB), when the input window (chunk_bytes + one block's extent) is full, or after _finish.  It decodes the whole blocks the
 * window holds, at most out_bytes of output (0 = the default, 256 MiB; raised to one block's largest expansion, 52 x 100000 x L
 * with L the header's level, 9 with multistream).  Held: the window on the host (pinned) and one upload of it on the device, one
 * output buffer of out_bytes on each side, and one device scratch arena of ~28 B per byte of (out_bytes / (100000 L)) blocks.
 * Stream errors come from _read, and only once every byte in front of the failing point has been read: exactly the decoded
 * bytes of all blocks in front of the first failing block (for an error of the chain walk -- bad magic, bad stream CRC, initial
 * position out of bounds -- the blocks in front of where the walk stopped).  Nothing of a failing block is delivered: the
 * reference's output stream has also seen the bytes of a block whose CRC then fails (it writes before it checks); this decoder
 * withholds them.  The verdicts of the first four bytes (bad magic, level out of range, fewer than four bytes at _finish) are
 * decided on the host, with no device.  NULL d, NULL in with n > 0, NULL taken, NULL got, NULL out with cap > 0 and _write after
 * _finish: CJS_E_INVALID_ARG at once, before the device is touched (the device is first touched by the first _read that runs a
 * step).  After any failing call the decoder stays failed: every later call returns the same code; _destroy is always safe.
 * opts->device is honoured, n_devices and stats are ignored.  One decoder is driven by one thread at a time; decoders are
 * independent of each other and of the pools cjs_bzip2_decompress keeps.  Synchronous: no worker thread.
 * CJS_DEBUG (read at _create): one "[cjs dec step]" line per step on stderr.  CJS_DEC_STREAM_EAGER=1 (read at _create; for
 * tests): a step is due on whatever has been written. */
typedef struct cjs_bz_dec cjs_bz_dec;
int cjs_bzip2_dec_create(cjs_bz_dec **d, int multistream, size_t chunk_bytes, size_t out_bytes, const cjs_opts *opts);
int cjs_bzip2_dec_write(cjs_bz_dec *d, const uint8_t *in, size_t n, size_t *taken);
int cjs_bzip2_dec_finish(cjs_bz_dec *d);
int cjs_bzip2_dec_read(cjs_bz_dec *d, uint8_t *out, size_t cap, size_t *got);
int cjs_bzip2_dec_done(const cjs_bz_dec *d);     /* 1: the stream has ended and every byte has been read */
void cjs_bzip2_dec_destroy(cjs_bz_dec *d);
void cjs_free(void *p);
/* Memory kept between calls (allocating and freeing multi-GB scratch costs more than compressing 100 MB):
 * cjs_bzip2_compress keeps its per-device workspace (~70 B per input byte of the largest call so far) and staging buffers;
 * cjs_bzip2_decompress / _table / _decompress_block keep their device scratch buffers (~25 B per output byte) in a
 * per-device pool; result buffers given back with cjs_free stay pinned for the next result (at most CJS_PINNED_RESULT_MB
 * megabytes of idle ones, default 2048; 0 = results are plain malloc).  cjs_trim() returns all of it to the driver;
 * environment CJS_NO_CTX_CACHE=1: never keep device memory. */
void cjs_trim(void);
const char *cjs_strerror(int code);
/* Detail text of the most recent FAILED call on the calling thread, "" if it had none: the reference's optDetail
 * of _throw(status, optDetail) (J/Bzip2_joined_.js:1385-1391), e.g. "bad magic", "level out of range",
 * "initial position out of bounds", "Bad block CRC (got 1a2b3c4d expected 5e6f7081)", "Bad stream CRC (got .. expected ..)"
 * (:1413,1417,1450,1757,1783).  A front appends it to cjs_strerror(code) after ": ".  Valid until the thread's next call. */
const char *cjs_last_error_detail(void);
int cjs_device_count(void);
const char *cjs_version(void);

/* ---- device-resident pipeline (input already in HBM, output left in HBM): what bench.py times.
 * A context owns the per-GPU workspace (sized for max_input bytes at `level`) and one stream. */
typedef struct cjs_ctx cjs_ctx;
int cjs_ctx_create(cjs_ctx **ctx, int device, size_t max_input, int level);
/* context of the batch path (cjs_bzip2_compress_batch_device): its workspace takes batches of up to max_input bytes in all and
 * max_items inputs in one pass per stage (larger batches run in several passes).  Only the batch entry point takes it. */
int cjs_ctx_create_batch(cjs_ctx **ctx, int device, size_t max_input, size_t max_items, int level);
/* as above, but the per-block workspace (suffix sorter, MTF, Huffman) is sized for at most
 * max_range_blocks blocks per call: for cjs_bzip2_compress_device_range on a replicated stream */
int cjs_ctx_create_sharded(cjs_ctx **ctx, int device, size_t max_input, long max_range_blocks, int level);
void cjs_ctx_destroy(cjs_ctx *ctx);
/* Calls on this context that are given a cjs_stats: on != 0 (default) synchronise the stream between the stages and fill the
 * per-stage times; on == 0 only record events (whole call, every full-size launch of the dominant kernel) -- what bench.py
 * sets for its timed loop. */
void cjs_ctx_set_stage_times(cjs_ctx *ctx, int on);
/* d_in/d_out are device pointers; d_out has out_cap bytes; *out_n receives the stream length.
 * Synchronous on return (the context stream has drained). */
int cjs_bzip2_compress_device(cjs_ctx *ctx, const uint8_t *d_in, size_t n, int level,
                              uint8_t *d_out, size_t out_cap, size_t *out_n, cjs_stats *stats);
/* ... and the block index (and, lines != NULL, the line table) of that stream: see cjs_bzip2_compress_indexed. */
int cjs_bzip2_compress_device_indexed(cjs_ctx *ctx, const uint8_t *d_in, size_t n, int level, uint8_t *d_out, size_t out_cap,
                                      size_t *out_n, cjs_bz_index **idx, cjs_bz_lines **lines, cjs_stats *stats);
/* Batch form of cjs_bzip2_compress_device on a cjs_ctx_create_batch context: input k is d_in[in_off[k] .. in_off[k+1]) (in_off: HOST array of
 * count + 1 ascending offsets).  Stream k is left at d_out + out_off[k], out_len[k] bytes (4-byte-aligned offsets, out_off /
 * out_len host arrays of `count` entries).  The streams are assembled in the context's staging buffer and reach d_out in one copy
 * once all sizes are known: when the last stream ends past out_cap (max of out_off[k] + out_len[k]) the call returns
 * CJS_E_OUTPUT_TOO_SMALL and d_out is left untouched (out_off / out_len still describe the layout).  d_out must be 4-byte aligned.  Synchronous on return. */
int cjs_bzip2_compress_batch_device(cjs_ctx *ctx, const uint8_t *d_in, const size_t *in_off, size_t count, int level,
                                    uint8_t *d_out, size_t out_cap, size_t *out_off, size_t *out_len);
/* Sharded variant for one-process-per-GPU jobs: compress only blocks [first, first+count) of the
 * stream held (replicated) in d_in, writing the block bit-strings from bit 0 of d_out WITHOUT the
 * 'BZh' header / trailer.  Returns the bit length and the per-block CRCs so the ranks can fold the
 * stream CRC and bit offsets (host side, a few bytes per rank; no data-path collective).
 * count = -1 means "to the end".  *total_blocks receives the number of blocks of the stream. */
int cjs_bzip2_compress_device_range(cjs_ctx *ctx, const uint8_t *d_in, size_t n, int level,
                                    long first_block, long count, uint8_t *d_out, size_t out_cap,
                                    uint64_t *out_bits, uint32_t *block_crcs, long crc_cap,
                                    long *total_blocks, cjs_stats *stats);

/* ---- one process (or thread) per GPU: the three phases of a multi-GPU Bzip2.compressFile (replaces the block
 * loop J/Bzip2_joined_.js:2233-2247 for `world` GPUs).  Every rank holds the stream in its GPU's memory.  The library calls no
 * collective: between the phases the CALLER exchanges two small tables with whatever transport it owns (bench.py:
 * torch.distributed all_gather over RCCL; cjs_bzip2_compress with n_devices > 1: worker threads and host memory).
 *   1. cjs_bzip2_shard_tiles : boundary tables of this rank's share of the 4 KiB input tiles -> d_share
 *                              (cjs_bzip2_shard_share_bytes(n, world) bytes, the same for every rank);
 *      exchange: all-gather of the shares, rank order, back to back -> d_shares (world x share bytes);
 *   2. cjs_bzip2_shard_blocks: block boundaries of the stream (replicated: serial by the format, Q1-Q3), then this rank's
 *                              contiguous range of blocks through RLE1 / CRC / BWT / MTF / Huffman tables -> *meta;
 *                              world == 1 may pass d_shares = NULL (no phase 1);
 *      exchange: all-gather of the metas (32 bytes per rank);
 *   3. cjs_bzip2_shard_pack  : the rank's blocks at their FINAL bit offset.  The ranks' fragments are disjoint runs of whole
 *                              32-bit words of the one .bz2 stream: bytes [frag_off, frag_off + frag_len) of d_out are stream
 *                              bytes [stream_off, stream_off + frag_len); rank 0 writes 'BZh<level>', the last rank with blocks
 *                              the trailer and the combined CRC.  The word two ranks share is completed by the earlier one
 *                              (what follows is always the 48-bit block magic).  *stream_len (optional) = length of the stream.
 * Each call is synchronous (the context's stream has drained on return). */
typedef struct cjs_shard_meta {
  uint64_t bits;          /* bit length of this rank's blocks, without header / trailer */
  uint64_t total_blocks;  /* blocks of the whole stream (must agree between the ranks) */
  uint64_t first_block;   /* this rank's contiguous range: [first_block, first_block + blocks) */
  uint32_t blocks;
  uint32_t crc_fold;      /* the range's block CRCs folded from 0: c = rol1(c) ^ crc (J/Bzip2_joined_.js:2237) */
} cjs_shard_meta;
size_t cjs_bzip2_shard_share_bytes(size_t n, int world);
int cjs_bzip2_shard_tiles(cjs_ctx *ctx, const uint8_t *d_in, size_t n, int rank, int world, void *d_share);
int cjs_bzip2_shard_blocks(cjs_ctx *ctx, const uint8_t *d_in, size_t n, int level, int rank, int world, const void *d_shares,
                           cjs_shard_meta *meta, cjs_stats *stats);
int cjs_bzip2_shard_pack(cjs_ctx *ctx, int level, int rank, int world, const cjs_shard_meta *metas, uint8_t *d_out, size_t out_cap,
                         size_t *frag_off, size_t *frag_len, uint64_t *stream_off, uint64_t *stream_len);

/* ---- stage-level entry points (host buffers; used by the parity tests to localise a mismatch).
 * in = nb consecutive blocks of block_len bytes (last one may be shorter).
 * cjs_stage_bwt: cyclic!=0 -> BWT.bwtransform2 semantics (J/Bzip2_joined_.js:928-971, Q4),
 *                cyclic==0 -> BWT.bwtransform semantics (J/BWTC_joined_.js:1125-1145). */
int cjs_stage_bwt(const uint8_t *in, size_t n, int block_len, int cyclic, uint8_t *out, int32_t *pidx, const cjs_opts *opts);
/* The cyclic form over blocks of different lengths, the geometry of the batched compressor (one block per slot): blocks = nb slots
 * of stride bytes, block k = the first len[k] bytes of slot k (what lies behind them in the slot is never looked at as text); out
 * has the same layout and only out[k*stride .. k*stride + len[k]) is defined.  CJS_E_INVALID_ARG, before anything is launched,
 * for nb == 0 or nb > 65535, a stride that is 0 or no multiple of 16, and any len[k] that is 0 or exceeds stride. */
int cjs_stage_bwt_var(const uint8_t *blocks, uint32_t nb, uint32_t stride, const uint32_t *len, uint8_t *out, int32_t *pidx,
                      const cjs_opts *opts);
/* readBlock (J/Bzip2_joined_.js:1954-1985) for the whole stream: RLE1 bytes of all blocks,
 * concatenated with stride = level*100000-19; per block length / crc / input start */
int cjs_stage_rle1(const uint8_t *in, size_t n, int level, uint8_t *blocks, size_t blocks_cap,
                   uint32_t *block_len, uint32_t *block_crc, uint64_t *block_start, long cap, long *nblocks, const cjs_opts *opts);
/* The same with a block capacity of the caller's choice (cjs_stage_rle1 is this with cap = level*100000-19, world 1,
 * range_blocks 0, work_fill -1): blocks with stride cap; per block length, crc, input start and input end (block_end and last_len
 * may be null); *last_len = length of the last block as the boundary walk hands it to the host.  world > 1: the tile tables are
 * made share by share as the ranks of a sharded job make them (ranks without tiles included) and unpacked from one gathered
 * buffer.  range_blocks > 0: the workspace is carved for that many blocks per pass and the blocks' bytes and CRCs are made window
 * by window, [0, range_blocks), [range_blocks, 2*range_blocks), ...  work_fill 0..255: workspace, share buffer and device rows
 * are filled with that byte first; < 0: left as allocated.  CJS_E_INVALID_ARG, before anything is launched, for cap < 2 (the
 * block-count bound divides by cap*4/5), cap > 899981, world == 0 or > 65535, and more than 65535 blocks per pass. */
int cjs_stage_rle1_cap(const uint8_t *in, size_t n, uint32_t cap, uint32_t world, uint32_t range_blocks, int work_fill,
                       uint8_t *blocks, size_t blocks_cap, uint32_t *block_len, uint32_t *block_crc, uint64_t *block_start,
                       uint64_t *block_end, long cap_blocks, long *nblocks, uint32_t *last_len, const cjs_opts *opts);
/* The three stage-0 kernels of the batched compressor, each with exactly the caller's arrays.  Inputs k < count: in[se[2k] ..
 * se[2k+1]).  (1) len2[k] = min(RLE1 length, cap + 1) << 1 | (last byte absorbed into a count byte; defined where the length is
 * <= cap).  (2) the block walk over inputs item[0 .. nitem): blocks of item j into table slots tbase[j] .. tbase[j+1] (s / e
 * relative to the input, len), their true number to nblk[j]; all table_slots >= tbase[nitem] slots come back in walk_s / walk_e /
 * walk_len, filled with work_fill where the kernel wrote nothing.  (3) the RLE1 bytes of nmat blocks in[mat_s[j] .. mat_e[j]), the
 * first mat_len[j] of them into rows + j*stride (rows pre-filled with work_fill), and the blocks' CRCs (row_crc may be null).
 * CJS_E_INVALID_ARG, before anything is launched, for cap outside 2 .. 899981, ranges outside in or reversed, item[j] >= count,
 * tbase not ascending or beyond table_slots, mat_len[j] > stride, nmat > 65535. */
int cjs_stage_rle1_batch(const uint8_t *in, size_t in_n, const uint64_t *se, uint32_t count, uint32_t cap, int work_fill,
                         uint64_t *len2, const uint32_t *item, const uint32_t *tbase, uint32_t nitem, uint32_t table_slots,
                         uint64_t *walk_s, uint64_t *walk_e, uint32_t *walk_len, uint32_t *nblk, const uint64_t *mat_s,
                         const uint64_t *mat_e, const uint32_t *mat_len, uint32_t nmat, uint32_t stride, uint8_t *rows,
                         uint32_t *row_crc, const cjs_opts *opts);
/* MTF + RLE2 (J/Bzip2_joined_.js:2064-2139) for nb blocks: U and block bytes with the same layout as
 * cjs_stage_bwt; A = u16 symbols with stride block_len+1 */
int cjs_stage_mtf(const uint8_t *U, const uint8_t *blocks, size_t n, int block_len, uint16_t *A, uint32_t *npos,
                  uint32_t *freq /* nb*258 */, uint32_t *alphabet /* nb */, const cjs_opts *opts);
/* The same over blocks of different lengths, as both compressors call the stage: blocks = nb slots of stride bytes (any stride
 * >= 1, odd ones included: the pipeline's rows start at odd addresses, the batch compressor's at multiples of 16), block k = the
 * first len[k] bytes of slot k; what the slots hold behind a block's end must not matter.  The whole workspace is filled with the
 * byte work_fill before the run, as a workspace left behind by an earlier call would be.  Out, per block: A (row of stride + 1
 * symbols, npos[k] of them defined), npos, freq[258], alphabet, alist[256] (the used byte values, ascending, alphabet[k] of them
 * defined) and nheads (the number of runs).  CJS_E_INVALID_ARG, before anything is launched, for nb == 0 or nb > 65535,
 * stride == 0, any len[k] that is 0 or exceeds stride, and a stride with more tiles than the stage scans (above 4 Mi). */
int cjs_stage_mtf_var(const uint8_t *blocks, uint32_t nb, uint32_t stride, const uint32_t *len, int work_fill, uint16_t *A,
                      uint32_t *npos, uint32_t *freq /* nb*258 */, uint32_t *alphabet /* nb */, uint8_t *alist /* nb*256 */,
                      uint32_t *nheads /* nb */, const cjs_opts *opts);
/* Huffman tables + selectors (J/Bzip2_joined_.js:1989-2054,2147-2163) for one symbol stream */
int cjs_stage_huff(const uint16_t *A, uint32_t npos, uint32_t alphabet, uint8_t *selectors, uint8_t *lengths /* 6*258 */,
                   uint32_t *ngroups, const cjs_opts *opts);
/* The same for nb blocks at once, followed by the bit packing of each block, so that both implementations of the tables can be
 * pinned block by block.  A holds nb*a_stride symbols; block k: A[k*a_stride .. + npos[k]) (values 0 .. alphabet[k]+1, end of
 * block last; npos[k] <= a_stride and < 50*32768), used byte values used[k*256 .. + alphabet[k]) ascending, block CRC and BWT
 * index as given.  path: 0 = the rule of the compressors, 1 = one workgroup per block, 2 = the chain of kernels.
 * Out: ngroups[k]; selectors at k*ceil(a_stride/50) (ceil(npos[k]/50) of them); code lengths [nb][6][258] (tables >= ngroups[k]
 * and symbols >= alphabet[k]+2 are 0); the block's bare bit string (magic, CRC, randomised bit, pidx, used map, table count,
 * selectors, code lengths, data; zero-padded to whole bytes) at bits + k*bits_stride and its length in bits nbits[k].
 * CJS_E_INVALID_ARG for symbols out of range, a used list that is not ascending, nb > 65535, or a bit string longer than
 * bits_stride bytes. */
int cjs_stage_huff_blocks(const uint16_t *A, size_t a_stride, uint32_t nb, const uint32_t *npos, const uint32_t *alphabet,
                          const uint8_t *used, const uint32_t *block_crc, const uint32_t *pidx, int path,
                          uint32_t *ngroups, uint8_t *selectors, uint8_t *lengths, uint8_t *bits, size_t bits_stride,
                          uint64_t *nbits, const cjs_opts *opts);

/* cjs_stage_radix EXISTS FOR TESTS; no product path calls it: the radix sorter (csrc/radix.hip: radix_passes, radix_pass_segments)
 * with the template arguments, bit range, geometry and workspace of the caller's choice, host buffers in and out.
 * The sort: stable, by 8-bit digits from lo_bit upwards while the digit's low bit lies below hi_bit, so the word sorted on is
 * (key >> lo_bit) & (2^(8*P) - 1), P = ceil((hi_bit - lo_bit) / 8), clipped at the key width: whole digits, not [lo_bit, hi_bit).
 * keys: n keys of key_bytes (4 or 8) each.  vals: n 32-bit values that move with them, or NULL (key-only passes).
 * Geometry: nseg segments of stride keys, the last one n_last (1 <= n_last <= stride, n == (nseg-1)*stride + n_last), each sorted
 * on its own in the same launches; nseg == 1 (then stride == n_last == n) is the plain sort, run without a geometry.
 * work_cap >= n: the sorter's workspace is carved for work_cap keys (RadixWork::hist_tiles_for / segs_for), as the product's
 * workspaces are, so radix_passes refuses geometries with more tiles or segments than that, with CJS_E_INVALID_ARG.
 * flags: CJS_RADIX_DIG hands the passes a byte-per-key array (a pass leaves the next digit of every key there and the next pass
 * counts from it); CJS_RADIX_SEGMENTS goes through radix_pass_segments (4-byte keys, n_last == stride, no DIG);
 * CJS_RADIX_FIRST_HIST: first_hist[nseg * tps * 256], tps = ceil(stride / 4096), holds the counts of the first digit per tile
 * (row (seg * tps + tile) * 256 + digit), is copied into the workspace and the first pass counts nothing itself;
 * CJS_RADIX_GEN: text[0 .. n) holds the segments' bytes and no keys or vals are read: the first pass makes the sentinel keys of
 * round 1 of the suffix sort from them (seven 9-bit symbols byte + 1, 0 past the segment's end, first symbol on top, the segment's
 * parity in bit 63; value = position in the segment); key_bytes 8, lo_bit 0, hi_bit 63 and no other flag; the text is followed
 * by 16 bytes of slack on the device, as the compressors carve it.
 * work_fill: before the run this byte fills the whole workspace (tile counts, chunk sums, digit totals), the byte-per-key array,
 * both buffer pairs (the input is copied in behind the fill) and 1 KiB of guard behind each key, value and byte array.
 * Out: keys_out / vals_out (vals_out unless key-only) = the buffer pair the sort ended in, *cur_out = which one (0: the one the input
 * was put into), *guard_bad = the guard bytes that no longer hold work_fill, counted on the host.  A call that radix_passes refuses
 * still sets *guard_bad and leaves keys_out, vals_out and *cur_out alone; its code is returned unchanged.
 * n == 0: 0, nothing is launched (every caller of the sorter guards n > 0: the kernels read key n_last - 1 of a short tile).
 * CJS_E_INVALID_ARG, before anything is launched: key_bytes not 4 or 8, lo_bit < 0, lo_bit >= hi_bit, hi_bit above the key width,
 * a geometry that breaks the rules above, work_cap < n or above 2^26, unknown flag bits or a combination ruled out above, a NULL
 * array that the flags call for, NULL keys_out, cur_out or guard_bad, NULL vals_out where values move. */
#define CJS_RADIX_DIG 1u
#define CJS_RADIX_SEGMENTS 2u
#define CJS_RADIX_FIRST_HIST 4u
#define CJS_RADIX_GEN 8u
int cjs_stage_radix(const void *keys, int key_bytes, const uint32_t *vals, const uint8_t *text, const uint32_t *first_hist, uint32_t n,
                    int lo_bit, int hi_bit, uint32_t nseg, uint32_t stride, uint32_t n_last, size_t work_cap, uint32_t flags,
                    int work_fill, void *keys_out, uint32_t *vals_out, int *cur_out, uint64_t *guard_bad, const cjs_opts *opts);

/* Serial entropy stage of BWTC.decompressFile (J/BWTC_joined_.js:1827-1913): range decoder + adaptive model + RLE2 + MTF
 * inverse, i.e. everything before BWT.unbwtransform.  Host logic only (the one entry point that needs no device; the chain
 * is serial by the format).  *cols receives the BWT columns of all non-empty blocks back to back (malloc'd, cjs_free);
 * lens[k] / pidx[k] for up to cap blocks; *level = the stream's level.  Returns the number of blocks or a negative code. */
long cjs_stage_bwtc_entropy_decode(const uint8_t *in, size_t n, uint8_t **cols, size_t *cols_n, uint32_t *lens, uint32_t *pidx,
                                   long cap, int *level);

/* The back half of BWTC.compressFile in its two parts, so that a mismatch of a stream can be placed (tests/bwtc_cases.py).
 * A coder step is one 64-bit word: sy | lt << 16 | tot << 32 for encodeFreq(sy, lt, tot), the same with bit 63 set and the
 * shift in tot's place for encodeShift (J/BWTC_joined_.js:92-113).
 * cjs_stage_bwtc_model: the adaptive model (J/BWTC_joined_.js:1791-1819) of nb blocks in ONE launch of the kernel the compressor
 * uses at `level` (DefSumModel for 1..5, FenwickModel for 6..9), with the compressor's launch shape.  Block k: RLE2 symbols
 * A[k*a_stride .. + nsym[k]), values 0 .. alphabet[k] (alphabet[k] = number of byte values of the block, 1..256), no end-of-block
 * symbol.  Out: nsteps[k] and the steps at steps + k*step_stride (step_stride >= 2 * nsym[k]).  CJS_E_INVALID_ARG for symbols
 * out of range, a row longer than its stride, nb == 0 or level outside 1..9. */
int cjs_stage_bwtc_model(const uint16_t *A, size_t a_stride, uint32_t nb, const uint32_t *nsym, const uint32_t *alphabet, int level,
                         uint64_t *steps, size_t step_stride, uint32_t *nsteps, const cjs_opts *opts);
/* cjs_stage_bwtc_code: the host range coder over a caller's step list: encodeStart(first_byte, 1), the step loop of
 * cjs_bwtc_compress, encodeFinish (J/BWTC_joined_.js:40-153).  Host logic only, needs no device.  mode 0: one thread;
 * mode 1: split across two threads (what cjs_bwtc_compress does unless CJS_BWTC_SPLIT_CODER=0).  *out: malloc'd, cjs_free.
 * CJS_E_INVALID_ARG for a step with sy == 0, lt + sy > tot (or > 1 << shift), a shift outside 1..16 or bits 49..62 set. */
int cjs_stage_bwtc_code(const uint64_t *steps, size_t n, int first_byte, int mode, uint8_t **out, size_t *out_n);

#ifdef __cplusplus
}
#endif
#endif
