// cjs_napi.cc — thin N-API shim over the C ABI of libcjs_hip.so (include/cjs_hip.h).
// It does no compression work: it dlopen()s the HIP library that sits next to the package, hands it
// the bytes of a Uint8Array/Buffer and wraps the malloc'd result as an external ArrayBuffer whose
// finalizer calls cjs_free.  Coercion of streams/arrays and error -> exception mapping live in the JS
// fronts (Bzip2.js / BWTC.js), exactly where the reference does them (Util.coerceInputStream etc.).
#include <node_api.h>
#include <dlfcn.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "cjs_hip.h"

namespace {

struct Api {
  void* handle = nullptr;
  int (*bzip2_compress)(const uint8_t*, size_t, int, uint8_t**, size_t*, const cjs_opts*) = nullptr;
  int (*bzip2_decompress)(const uint8_t*, size_t, int, uint8_t**, size_t*, const cjs_opts*) = nullptr;
  int (*bwtc_compress)(const uint8_t*, size_t, int, uint8_t**, size_t*, const cjs_opts*) = nullptr;
  int (*bwtc_decompress)(const uint8_t*, size_t, uint8_t**, size_t*, const cjs_opts*) = nullptr;
  long (*bzip2_table)(const uint8_t*, size_t, int, uint64_t*, uint32_t*, long, const cjs_opts*) = nullptr;
  int (*bzip2_decompress_block)(const uint8_t*, size_t, uint64_t, uint8_t**, size_t*, const cjs_opts*) = nullptr;
  int (*bzip2_compress_batch)(const uint8_t* const*, const size_t*, size_t, int, uint8_t**, size_t*, size_t*, const cjs_opts*) = nullptr;
  int (*bzip2_decompress_batch)(const uint8_t* const*, const size_t*, size_t, int, uint8_t**, size_t*, size_t*, int32_t*, const cjs_opts*) = nullptr;
  int (*bzip2_recover)(const uint8_t*, size_t, int, uint8_t**, size_t*, cjs_bz_found*, long, long*, const cjs_opts*) = nullptr;
  int (*index_build)(const uint8_t*, size_t, int, cjs_bz_index**, const cjs_opts*) = nullptr;
  int (*index_save)(const cjs_bz_index*, uint8_t**, size_t*) = nullptr;
  int (*index_load)(const uint8_t*, size_t, cjs_bz_index**) = nullptr;
  void (*index_destroy)(cjs_bz_index*) = nullptr;
  int (*read_ranges)(const uint8_t*, size_t, const cjs_bz_index*, const uint64_t*, const uint64_t*, size_t, uint8_t**, size_t*, size_t*, int32_t*,
                     const cjs_opts*) = nullptr;
  int (*search)(const uint8_t*, size_t, const cjs_bz_index*, const uint8_t*, const uint32_t*, uint32_t, uint32_t, uint64_t, uint64_t, cjs_bz_match*, size_t,
                cjs_bz_search_info*, const cjs_opts*) = nullptr;
  int (*search_regex)(const uint8_t*, size_t, const cjs_bz_index*, const uint8_t*, const uint32_t*, uint32_t, uint32_t, uint64_t, uint64_t, cjs_bz_match*, size_t,
                      cjs_bz_search_info*, const cjs_opts*) = nullptr;
  int (*regex_check)(const uint8_t*, const uint32_t*, uint32_t, uint32_t, uint32_t*, uint32_t*) = nullptr;
  int (*index_info)(const cjs_bz_index*, uint64_t*, uint64_t*, uint64_t*, int*) = nullptr;
  int (*compare)(const uint8_t*, size_t, const cjs_bz_index*, const uint8_t*, size_t, uint64_t, uint64_t, uint64_t, cjs_bz_diff*, size_t, cjs_bz_cmp_info*,
                 const cjs_opts*) = nullptr;
  int (*compare_streams)(const uint8_t*, size_t, const cjs_bz_index*, const uint8_t*, size_t, const cjs_bz_index*, uint64_t, uint64_t, cjs_bz_diff*, size_t,
                         cjs_bz_cmp_info*, const cjs_opts*) = nullptr;
  int (*lines_build)(const uint8_t*, size_t, const cjs_bz_index*, cjs_bz_lines**, const cjs_opts*) = nullptr;
  int (*lines_save)(const cjs_bz_lines*, uint8_t**, size_t*) = nullptr;
  int (*lines_load)(const uint8_t*, size_t, const cjs_bz_index*, cjs_bz_lines**) = nullptr;
  void (*lines_destroy)(cjs_bz_lines*) = nullptr;
  int (*lines_locate)(const uint8_t*, size_t, const cjs_bz_index*, const cjs_bz_lines*, const uint64_t*, size_t, uint64_t*, int32_t*, const cjs_opts*) = nullptr;
  int (*lines_number)(const uint8_t*, size_t, const cjs_bz_index*, const cjs_bz_lines*, const uint64_t*, size_t, uint64_t*, int32_t*, const cjs_opts*) = nullptr;
  int (*line_keys)(const uint8_t*, size_t, const cjs_bz_index*, const cjs_bz_lines*, uint64_t, uint64_t, uint64_t, cjs_bz_linekey*, size_t, cjs_bz_linekeys_info*,
                   const cjs_opts*) = nullptr;
  int (*line_keys_diff)(const cjs_bz_linekey*, size_t, const cjs_bz_linekey*, size_t, uint64_t, cjs_bz_hunk*, size_t, cjs_bz_ldiff_info*) = nullptr;
  int (*tally)(const uint8_t*, size_t, const cjs_bz_index*, const cjs_bz_lines*, uint64_t, uint64_t, uint64_t, uint32_t, uint32_t, const cjs_cut_range*, uint32_t,
               uint32_t, uint64_t, uint64_t, cjs_bz_tally*, size_t, cjs_bz_tally_info*, const cjs_opts*) = nullptr;
  int (*sort)(const uint8_t*, size_t, const cjs_bz_index*, const cjs_bz_lines*, uint64_t, uint64_t, uint32_t, uint32_t, const cjs_cut_range*, uint32_t, uint32_t,
              uint64_t*, uint64_t*, size_t, uint8_t**, size_t*, cjs_bz_sort_info*, const cjs_opts*) = nullptr;
  int (*cut)(const uint8_t*, size_t, const cjs_bz_index*, const cjs_bz_lines*, uint64_t, uint64_t, uint32_t, uint32_t, const cjs_cut_range*, uint32_t, uint8_t**,
             size_t*, cjs_bz_cut_info*, const cjs_opts*) = nullptr;
  int (*cut_list_parse)(const char*, cjs_cut_range*, uint32_t, uint32_t*) = nullptr;
  int (*enc_create)(cjs_bz_enc**, int, size_t, const cjs_opts*) = nullptr;
  int (*enc_write)(cjs_bz_enc*, const uint8_t*, size_t) = nullptr;
  int (*enc_finish)(cjs_bz_enc*) = nullptr;
  size_t (*enc_pending)(const cjs_bz_enc*) = nullptr;
  int (*enc_read)(cjs_bz_enc*, uint8_t*, size_t, size_t*) = nullptr;
  void (*enc_destroy)(cjs_bz_enc*) = nullptr;
  int (*enc_index)(cjs_bz_enc*, cjs_bz_index**, cjs_bz_lines**) = nullptr;
  int (*compress_indexed)(const uint8_t*, size_t, int, uint8_t**, size_t*, cjs_bz_index**, cjs_bz_lines**, const cjs_opts*) = nullptr;
  int (*dec_create)(cjs_bz_dec**, int, size_t, size_t, const cjs_opts*) = nullptr;
  int (*dec_write)(cjs_bz_dec*, const uint8_t*, size_t, size_t*) = nullptr;
  int (*dec_finish)(cjs_bz_dec*) = nullptr;
  int (*dec_read)(cjs_bz_dec*, uint8_t*, size_t, size_t*) = nullptr;
  int (*dec_done)(const cjs_bz_dec*) = nullptr;
  void (*dec_destroy)(cjs_bz_dec*) = nullptr;
  void (*free_)(void*) = nullptr;
  const char* (*strerror_)(int) = nullptr;
  const char* (*detail_)(void) = nullptr;
  int (*device_count)(void) = nullptr;
  const char* (*version)(void) = nullptr;
  void (*trim)(void) = nullptr;
  std::string error;
} api;

bool load_api() {
  if (api.handle) return true;
  Dl_info info;
  std::string dir = ".";
  if (dladdr((void*)&load_api, &info) && info.dli_fname) {
    dir = info.dli_fname;
    size_t p = dir.find_last_of('/');
    dir = p == std::string::npos ? "." : dir.substr(0, p);
  }
  const char* env = getenv("CJS_HIP_LIB");
  std::string path = env ? env : dir + "/../libcjs_hip.so";
  api.handle = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
  if (!api.handle) { api.error = std::string("cannot load libcjs_hip.so: ") + dlerror(); return false; }
#define SYM(field, name) *(void**)(&api.field) = dlsym(api.handle, name); if (!api.field) { api.error = "missing symbol " name; api.handle = nullptr; return false; }
  SYM(bzip2_compress, "cjs_bzip2_compress") SYM(bzip2_decompress, "cjs_bzip2_decompress")
  SYM(bwtc_compress, "cjs_bwtc_compress") SYM(bwtc_decompress, "cjs_bwtc_decompress")
  SYM(bzip2_table, "cjs_bzip2_table") SYM(bzip2_decompress_block, "cjs_bzip2_decompress_block")
  SYM(bzip2_compress_batch, "cjs_bzip2_compress_batch") SYM(bzip2_decompress_batch, "cjs_bzip2_decompress_batch")
  SYM(bzip2_recover, "cjs_bzip2_recover")
  SYM(index_build, "cjs_bzip2_index_build") SYM(index_save, "cjs_bzip2_index_save") SYM(index_load, "cjs_bzip2_index_load")
  SYM(index_destroy, "cjs_bzip2_index_destroy") SYM(read_ranges, "cjs_bzip2_read_ranges") SYM(search, "cjs_bzip2_search")
  SYM(search_regex, "cjs_bzip2_search_regex") SYM(regex_check, "cjs_regex_check")
  SYM(index_info, "cjs_bzip2_index_info") SYM(compare, "cjs_bzip2_compare") SYM(compare_streams, "cjs_bzip2_compare_streams")
  SYM(lines_build, "cjs_bzip2_lines_build") SYM(lines_save, "cjs_bzip2_lines_save") SYM(lines_load, "cjs_bzip2_lines_load")
  SYM(lines_destroy, "cjs_bzip2_lines_destroy") SYM(lines_locate, "cjs_bzip2_lines_locate") SYM(lines_number, "cjs_bzip2_lines_number")
  SYM(line_keys, "cjs_bzip2_line_keys") SYM(line_keys_diff, "cjs_line_keys_diff") SYM(tally, "cjs_bzip2_tally")
  SYM(sort, "cjs_bzip2_sort")
  SYM(cut, "cjs_bzip2_cut") SYM(cut_list_parse, "cjs_cut_list_parse")
  SYM(enc_create, "cjs_bzip2_enc_create") SYM(enc_write, "cjs_bzip2_enc_write") SYM(enc_finish, "cjs_bzip2_enc_finish")
  SYM(enc_pending, "cjs_bzip2_enc_pending") SYM(enc_read, "cjs_bzip2_enc_read") SYM(enc_destroy, "cjs_bzip2_enc_destroy")
  SYM(enc_index, "cjs_bzip2_enc_index") SYM(compress_indexed, "cjs_bzip2_compress_indexed")
  SYM(dec_create, "cjs_bzip2_dec_create") SYM(dec_write, "cjs_bzip2_dec_write") SYM(dec_finish, "cjs_bzip2_dec_finish")
  SYM(dec_read, "cjs_bzip2_dec_read") SYM(dec_done, "cjs_bzip2_dec_done") SYM(dec_destroy, "cjs_bzip2_dec_destroy")
  SYM(free_, "cjs_free") SYM(strerror_, "cjs_strerror") SYM(detail_, "cjs_last_error_detail") SYM(device_count, "cjs_device_count") SYM(version, "cjs_version") SYM(trim, "cjs_trim")
#undef SYM
  return true;
}

// Results are handed to JS as EXTERNAL ArrayBuffers over the library's (pinned, pooled) result buffers; V8 is told how much
// memory hangs on each one, so that it collects dropped results soon and their buffers go back to the pool instead of a new
// pinned buffer being made for every call (hipHostMalloc of a 32 MB result costs more than compressing 50 MB).
void finalize_buf(napi_env env, void* data, void* hint) {
  if (api.free_) api.free_(data);
  int64_t adj = 0;
  napi_adjust_external_memory(env, -(int64_t)(intptr_t)hint, &adj);
}

napi_value throw_code(napi_env env, int code) {
  napi_value err, msg, num;
  const char* text = api.strerror_ ? api.strerror_(code) : "cjs error";
  napi_create_string_utf8(env, text, NAPI_AUTO_LENGTH, &msg);
  napi_create_error(env, nullptr, msg, &err);
  napi_create_int32(env, code, &num);
  napi_set_named_property(env, err, "cjsCode", num);
  const char* detail = api.detail_ ? api.detail_() : "";        // the reference's optDetail (J/Bzip2_joined_.js:1385-1391)
  if (detail && detail[0]) {
    napi_value d;
    napi_create_string_utf8(env, detail, NAPI_AUTO_LENGTH, &d);
    napi_set_named_property(env, err, "cjsDetail", d);
  }
  napi_throw(env, err);
  return nullptr;
}

bool get_bytes(napi_env env, napi_value v, const uint8_t** p, size_t* n) {
  bool is_ta = false, is_buf = false;
  napi_is_buffer(env, v, &is_buf);
  if (is_buf) { void* d; napi_get_buffer_info(env, v, &d, n); *p = (const uint8_t*)d; return true; }
  napi_is_typedarray(env, v, &is_ta);
  if (is_ta) {
    napi_typedarray_type t; size_t len; void* d; napi_value ab; size_t off;
    napi_get_typedarray_info(env, v, &t, &len, &d, &ab, &off);
    if (t != napi_uint8_array && t != napi_uint8_clamped_array && t != napi_int8_array) return false;
    *p = (const uint8_t*)d; *n = len; return true;
  }
  return false;
}

napi_value wrap_result(napi_env env, uint8_t* data, size_t n) {
  napi_value ab, ta;
  int64_t adj = 0;
  if (napi_create_external_arraybuffer(env, data, n, finalize_buf, (void*)(intptr_t)n, &ab) == napi_ok) napi_adjust_external_memory(env, (int64_t)n, &adj);
  else {
    // some runtimes forbid external buffers: copy instead
    void* dst;
    napi_create_arraybuffer(env, n, &dst, &ab);
    memcpy(dst, data, n);
    api.free_(data);
  }
  napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &ta);
  return ta;
}

template <int KIND>   // 0 bzip2 compress, 1 bzip2 decompress, 2 bwtc compress, 3 bwtc decompress
napi_value call_stream(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 3; napi_value argv[3];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t* p = nullptr; size_t n = 0;
  if (argc < 1 || !get_bytes(env, argv[0], &p, &n)) { napi_throw_type_error(env, nullptr, "expected a Uint8Array or Buffer"); return nullptr; }
  int32_t arg = KIND == 1 ? 0 : 9;
  if (argc >= 2) napi_get_value_int32(env, argv[1], &arg);
  uint32_t flags = 0;                                           // third argument: cjs_opts.flags (bwtcCompress: CJS_FLAG_SIZE_UNKNOWN)
  if (argc >= 3) napi_get_value_uint32(env, argv[2], &flags);
  cjs_opts opts; memset(&opts, 0, sizeof opts);
  opts.struct_size = sizeof opts; opts.device = -1; opts.flags = flags;
  uint8_t* out = nullptr; size_t out_n = 0;
  static const uint8_t dummy = 0;
  if (!p) p = &dummy;
  int rc;
  if (KIND == 0) rc = api.bzip2_compress(p, n, arg, &out, &out_n, nullptr);
  else if (KIND == 1) rc = api.bzip2_decompress(p, n, arg, &out, &out_n, nullptr);
  else if (KIND == 2) rc = api.bwtc_compress(p, n, arg, &out, &out_n, flags ? &opts : nullptr);
  else rc = api.bwtc_decompress(p, n, &out, &out_n, nullptr);
  if (rc != 0) return throw_code(env, rc);
  return wrap_result(env, out, out_n);
}

// bzip2Table(input, multistream) -> Float64Array [pos0, size0, pos1, size1, ...]   (Bzip2.table)
napi_value bzip2_table(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 2; napi_value argv[2];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t* p = nullptr; size_t n = 0;
  if (argc < 1 || !get_bytes(env, argv[0], &p, &n)) { napi_throw_type_error(env, nullptr, "expected a Uint8Array or Buffer"); return nullptr; }
  int32_t multi = 0;
  if (argc >= 2) napi_get_value_int32(env, argv[1], &multi);
  long cap = (long)(n / 32 + 64);
  uint64_t* pos = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)cap);
  uint32_t* size = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)cap);
  static const uint8_t dummy = 0;
  long nb = api.bzip2_table(p ? p : &dummy, n, multi, pos, size, cap, nullptr);
  if (nb < 0) { free(pos); free(size); return throw_code(env, (int)nb); }
  if (nb > cap) nb = cap;
  napi_value ab, ta; void* dst;
  napi_create_arraybuffer(env, sizeof(double) * 2 * (size_t)nb, &dst, &ab);
  for (long i = 0; i < nb; i++) { ((double*)dst)[2 * i] = (double)pos[i]; ((double*)dst)[2 * i + 1] = (double)size[i]; }
  free(pos); free(size);
  napi_create_typedarray(env, napi_float64_array, 2 * (size_t)nb, ab, 0, &ta);
  return ta;
}
// bzip2DecompressBlock(input, bitpos) -> Uint8Array   (Bzip2.decompressBlock)
napi_value bzip2_block(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 2; napi_value argv[2];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t* p = nullptr; size_t n = 0;
  if (argc < 2 || !get_bytes(env, argv[0], &p, &n)) { napi_throw_type_error(env, nullptr, "expected (Uint8Array, bit position)"); return nullptr; }
  double bit = 0; napi_get_value_double(env, argv[1], &bit);
  uint8_t* out = nullptr; size_t out_n = 0;
  static const uint8_t dummy = 0;
  const int rc = api.bzip2_decompress_block(p ? p : &dummy, n, (uint64_t)bit, &out, &out_n, nullptr);
  if (rc != 0) return throw_code(env, rc);
  return wrap_result(env, out, out_n);
}

// bzip2BuildIndex(input, multistream) -> Uint8Array: the serialised block index (Bzip2.buildIndex)
napi_value bzip2_build_index(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 2; napi_value argv[2];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t* p = nullptr; size_t n = 0;
  if (argc < 1 || !get_bytes(env, argv[0], &p, &n)) { napi_throw_type_error(env, nullptr, "expected a Uint8Array or Buffer"); return nullptr; }
  int32_t multi = 0;
  if (argc >= 2) napi_get_value_int32(env, argv[1], &multi);
  static const uint8_t dummy = 0;
  cjs_bz_index* ix = nullptr;
  int rc = api.index_build(p ? p : &dummy, n, multi, &ix, nullptr);
  if (rc != 0) return throw_code(env, rc);
  uint8_t* raw = nullptr; size_t raw_n = 0;
  rc = api.index_save(ix, &raw, &raw_n);
  api.index_destroy(ix);
  if (rc != 0) return throw_code(env, rc);
  return wrap_result(env, raw, raw_n);
}

// bzip2ReadRanges(input, index, ranges) -> { data: Uint8Array, layout: Float64Array, detail: string }   (Bzip2.readRanges)
// index: the serialised index; ranges: Float64Array of (offset, length) pairs.  layout holds (offset in data, length, status) per
// range; detail is the lowest-index failing range's ("" when none failed).
napi_value bzip2_read_ranges(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 3; napi_value argv[3];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t *p = nullptr, *ip = nullptr; size_t n = 0, in = 0;
  bool is_ta = false;
  if (argc >= 3) napi_is_typedarray(env, argv[2], &is_ta);
  napi_typedarray_type t = napi_int8_array; size_t len = 0; void* rd = nullptr; napi_value rab; size_t roff = 0;
  if (is_ta) napi_get_typedarray_info(env, argv[2], &t, &len, &rd, &rab, &roff);
  if (argc < 3 || !get_bytes(env, argv[0], &p, &n) || !get_bytes(env, argv[1], &ip, &in) || !is_ta || t != napi_float64_array || len % 2) {
    napi_throw_type_error(env, nullptr, "expected (Uint8Array, Uint8Array index, Float64Array of offset / length pairs)"); return nullptr;
  }
  const size_t count = len / 2;
  const double* r = (const double*)rd;
  std::vector<uint64_t> off(count + 1), ln(count + 1);
  for (size_t k = 0; k < count; k++) {
    const uint64_t o = r[2 * k] >= 0 && r[2 * k] <= 9007199254740992.0 ? (uint64_t)r[2 * k] : 0, l = r[2 * k + 1] >= 0 && r[2 * k + 1] <= 9007199254740992.0 ? (uint64_t)r[2 * k + 1] : 0;
    if ((double)o != r[2 * k] || (double)l != r[2 * k + 1]) {      // (negative, NaN, above 2^53 or with a fraction)
      napi_throw_type_error(env, nullptr, "offsets and lengths are integers from 0 to 2^53"); return nullptr;
    }
    off[k] = (uint64_t)r[2 * k]; ln[k] = (uint64_t)r[2 * k + 1];
  }
  static const uint8_t dummy = 0;
  cjs_bz_index* ix = nullptr;
  int rc = api.index_load(ip ? ip : &dummy, in, &ix);
  if (rc != 0) return throw_code(env, rc);
  std::vector<size_t> o_off(count + 1), o_len(count + 1); std::vector<int32_t> status(count + 1);
  uint8_t* out = nullptr;
  rc = api.read_ranges(p ? p : &dummy, n, ix, off.data(), ln.data(), count, &out, o_off.data(), o_len.data(), status.data(), nullptr);
  std::string detail = api.detail_();                            // (before the next call of the library on this thread)
  api.index_destroy(ix);
  if (rc != 0) return throw_code(env, rc);
  size_t total = 0;
  for (size_t k = 0; k < count; k++) total += o_len[k];
  napi_value res, lab, lta, dstr; void* ldst;
  napi_create_object(env, &res);
  napi_set_named_property(env, res, "data", wrap_result(env, out, total));
  napi_create_arraybuffer(env, sizeof(double) * 3 * count, &ldst, &lab);
  for (size_t k = 0; k < count; k++) { ((double*)ldst)[3 * k] = (double)o_off[k]; ((double*)ldst)[3 * k + 1] = (double)o_len[k]; ((double*)ldst)[3 * k + 2] = (double)status[k]; }
  napi_create_typedarray(env, napi_float64_array, 3 * count, lab, 0, &lta);
  napi_set_named_property(env, res, "layout", lta);
  napi_create_string_utf8(env, detail.c_str(), NAPI_AUTO_LENGTH, &dstr);
  napi_set_named_property(env, res, "detail", dstr);
  return res;
}

// bzip2Search(input, index, patterns, lengths, flags, offset, length, limit) -> { matches: Float64Array, total, badBlocks,
// firstBadBlock, detail }   (Bzip2.search).  patterns: the patterns' bytes back to back; lengths: Float64Array, one per pattern;
// length < 0: to the end; limit < 0: every match (a count query first).  matches holds (offset, pattern) pairs.
// bzip2SearchRegex: the same arguments with pattern texts (Bzip2.searchRegex); matches holds (offset, pattern, length) triples.
napi_value search_call(napi_env env, napi_callback_info info, bool regex) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 8; napi_value argv[8];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t *p = nullptr, *ip = nullptr, *pp = nullptr; size_t n = 0, in = 0, pn = 0;
  bool is_ta = false;
  if (argc >= 4) napi_is_typedarray(env, argv[3], &is_ta);
  napi_typedarray_type t = napi_int8_array; size_t npat = 0; void* ld = nullptr; napi_value lab; size_t loff = 0;
  if (is_ta) napi_get_typedarray_info(env, argv[3], &t, &npat, &ld, &lab, &loff);
  if (argc < 8 || !get_bytes(env, argv[0], &p, &n) || !get_bytes(env, argv[1], &ip, &in) || !get_bytes(env, argv[2], &pp, &pn) || !is_ta || t != napi_float64_array) {
    napi_throw_type_error(env, nullptr, "expected (Uint8Array, Uint8Array index, Uint8Array patterns, Float64Array lengths, flags, offset, length, limit)"); return nullptr;
  }
  double flags = 0, off = 0, len = 0, limit = 0;
  napi_get_value_double(env, argv[4], &flags); napi_get_value_double(env, argv[5], &off); napi_get_value_double(env, argv[6], &len); napi_get_value_double(env, argv[7], &limit);
  if (!(off >= 0 && off <= 9007199254740992.0 && off == (double)(uint64_t)off) || !(len <= 9007199254740992.0 && len == (double)(int64_t)len) ||
      !(limit <= 9007199254740992.0 && limit == (double)(int64_t)limit)) {
    napi_throw_type_error(env, nullptr, "offsets and lengths are integers from 0 to 2^53"); return nullptr;
  }
  std::vector<uint32_t> p_off(npat + 1, 0);
  uint64_t sum = 0;
  for (size_t j = 0; j < npat; j++) {
    const double l = ((const double*)ld)[j];
    sum += l >= 0 && l <= 65536.0 ? (uint64_t)l : 65536u;      // (an absurd length stays one: the library refuses it)
    p_off[j + 1] = (uint32_t)std::min<uint64_t>(sum, 0xFFFFFFFFull);
  }
  if (sum != pn || npat > 1000000) { napi_throw_type_error(env, nullptr, "the pattern lengths do not add up to the pattern bytes"); return nullptr; }
  static const uint8_t dummy = 0;
  cjs_bz_index* ix = nullptr;
  int rc = api.index_load(ip ? ip : &dummy, in, &ix);
  if (rc != 0) return throw_code(env, rc);
  cjs_bz_search_info si;
  memset(&si, 0, sizeof si);
  std::vector<cjs_bz_match> found;
  const uint64_t ulen = len < 0 ? ~0ull : (uint64_t)len;
  size_t cap = limit < 0 ? 0 : (size_t)limit;
  const auto search = regex ? api.search_regex : api.search;
  const size_t per = regex ? 3 : 2;
  if (limit < 0) {                                                 // the count query
    rc = search(p ? p : &dummy, n, ix, pp ? pp : &dummy, p_off.data(), (uint32_t)npat, (uint32_t)flags, (uint64_t)off, ulen, nullptr, 0, &si, nullptr);
    cap = (size_t)si.n_matches;
  }
  if (rc == 0 && (limit >= 0 || cap)) {
    try { found.resize(cap); } catch (...) { api.index_destroy(ix); napi_throw_error(env, nullptr, "out of memory"); return nullptr; }
    rc = search(p ? p : &dummy, n, ix, pp ? pp : &dummy, p_off.data(), (uint32_t)npat, (uint32_t)flags, (uint64_t)off, ulen, cap ? found.data() : nullptr, cap, &si, nullptr);
  }
  std::string detail = rc == 0 && !si.n_bad_blocks ? "" : api.detail_();      // (before the next call of the library on this thread)
  if (rc != 0) { napi_value e = throw_code(env, rc); api.index_destroy(ix); return e; }      // (the detail goes into the error first)
  api.index_destroy(ix);
  const size_t got = (size_t)std::min<uint64_t>(cap, si.n_matches);
  napi_value res, mab, mta, v; void* mdst;
  napi_create_object(env, &res);
  napi_create_arraybuffer(env, sizeof(double) * per * got, &mdst, &mab);
  for (size_t k = 0; k < got; k++) {
    double* m = (double*)mdst + per * k;
    m[0] = (double)found[k].off; m[1] = (double)found[k].pattern;
    if (regex) m[2] = (double)found[k].reserved;
  }
  napi_create_typedarray(env, napi_float64_array, per * got, mab, 0, &mta);
  napi_set_named_property(env, res, "matches", mta);
  napi_create_double(env, (double)si.n_matches, &v); napi_set_named_property(env, res, "total", v);
  napi_create_double(env, (double)si.n_bad_blocks, &v); napi_set_named_property(env, res, "badBlocks", v);
  napi_create_double(env, si.n_bad_blocks ? (double)si.first_bad_block : -1.0, &v); napi_set_named_property(env, res, "firstBadBlock", v);
  napi_create_string_utf8(env, detail.c_str(), NAPI_AUTO_LENGTH, &v); napi_set_named_property(env, res, "detail", v);
  return res;
}

napi_value bzip2_search(napi_env env, napi_callback_info info) { return search_call(env, info, false); }
napi_value bzip2_search_regex(napi_env env, napi_callback_info info) { return search_call(env, info, true); }

// regexCheck(patterns, lengths, flags) -> Float64Array of (states, maxLen) pairs, one per pattern   (Bzip2.regexCheck; no device)
napi_value regex_check(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 3; napi_value argv[3];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t* pp = nullptr; size_t pn = 0;
  bool is_ta = false;
  if (argc >= 2) napi_is_typedarray(env, argv[1], &is_ta);
  napi_typedarray_type t = napi_int8_array; size_t npat = 0; void* ld = nullptr; napi_value lab; size_t loff = 0;
  if (is_ta) napi_get_typedarray_info(env, argv[1], &t, &npat, &ld, &lab, &loff);
  if (argc < 3 || !get_bytes(env, argv[0], &pp, &pn) || !is_ta || t != napi_float64_array) {
    napi_throw_type_error(env, nullptr, "expected (Uint8Array patterns, Float64Array lengths, flags)"); return nullptr;
  }
  double flags = 0;
  napi_get_value_double(env, argv[2], &flags);
  std::vector<uint32_t> p_off(npat + 1, 0);
  uint64_t sum = 0;
  for (size_t j = 0; j < npat; j++) {
    const double l = ((const double*)ld)[j];
    sum += l >= 0 && l <= 65536.0 ? (uint64_t)l : 65536u;
    p_off[j + 1] = (uint32_t)std::min<uint64_t>(sum, 0xFFFFFFFFull);
  }
  if (sum != pn || npat > 1000000) { napi_throw_type_error(env, nullptr, "the pattern lengths do not add up to the pattern bytes"); return nullptr; }
  static const uint8_t dummy = 0;
  std::vector<uint32_t> states(npat + 1), max_len(npat + 1);
  const int rc = api.regex_check(pp ? pp : &dummy, p_off.data(), (uint32_t)npat, (uint32_t)flags, states.data(), max_len.data());
  if (rc != 0) return throw_code(env, rc);
  napi_value ab, ta; void* dst;
  napi_create_arraybuffer(env, sizeof(double) * 2 * npat, &dst, &ab);
  for (size_t j = 0; j < npat; j++) { ((double*)dst)[2 * j] = states[j]; ((double*)dst)[2 * j + 1] = max_len[j]; }
  napi_create_typedarray(env, napi_float64_array, 2 * npat, ab, 0, &ta);
  return ta;
}

// bzip2Compare(input, index, other, otherIndex, otherOffset, offset, length, limit) -> { diffs: Float64Array, total, firstDiff,
// compared, lenA, lenB, badBlocks, firstBadBlock, badBlocksB, firstBadBlockB, detail }   (Bzip2.compare, Bzip2.compareStreams).
// otherIndex: null = `other` is plain bytes, byte k of it decoded byte otherOffset + k; a serialised index = `other` is the stream
// of that index.  length < 0: to the end; limit < 0: every difference (a count query first).  diffs holds (offset, a, b) triples.
napi_value bzip2_compare(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 8; napi_value argv[8];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t *p = nullptr, *ip = nullptr, *op = nullptr, *oip = nullptr; size_t n = 0, in = 0, on = 0, oin = 0;
  napi_valuetype oit = napi_undefined;
  if (argc >= 4) napi_typeof(env, argv[3], &oit);
  const bool two = oit != napi_null && oit != napi_undefined;
  if (argc < 8 || !get_bytes(env, argv[0], &p, &n) || !get_bytes(env, argv[1], &ip, &in) || !get_bytes(env, argv[2], &op, &on) ||
      (two && !get_bytes(env, argv[3], &oip, &oin))) {
    napi_throw_type_error(env, nullptr, "expected (Uint8Array, Uint8Array index, Uint8Array other, Uint8Array index or null, otherOffset, offset, length, limit)"); return nullptr;
  }
  double ooff = 0, off = 0, len = 0, limit = 0;
  napi_get_value_double(env, argv[4], &ooff); napi_get_value_double(env, argv[5], &off); napi_get_value_double(env, argv[6], &len); napi_get_value_double(env, argv[7], &limit);
  if (!(off >= 0 && off <= 9007199254740992.0 && off == (double)(uint64_t)off) || !(ooff >= 0 && ooff <= 9007199254740992.0 && ooff == (double)(uint64_t)ooff) ||
      !(len <= 9007199254740992.0 && len == (double)(int64_t)len) || !(limit <= 9007199254740992.0 && limit == (double)(int64_t)limit)) {
    napi_throw_type_error(env, nullptr, "offsets and lengths are integers from 0 to 2^53"); return nullptr;
  }
  static const uint8_t dummy = 0;
  cjs_bz_index *ix = nullptr, *oix = nullptr;
  int rc = api.index_load(ip ? ip : &dummy, in, &ix);
  if (rc != 0) return throw_code(env, rc);
  if (two && (rc = api.index_load(oip ? oip : &dummy, oin, &oix)) != 0) { api.index_destroy(ix); return throw_code(env, rc); }
  uint64_t blocks = 0, len_a = 0, len_b = (uint64_t)ooff + on, sb = 0; int multi = 0;
  api.index_info(ix, &blocks, &len_a, &sb, &multi);
  if (two) api.index_info(oix, &blocks, &len_b, &sb, &multi);
  cjs_bz_cmp_info ci;
  memset(&ci, 0, sizeof ci);
  std::vector<cjs_bz_diff> diffs;
  const uint64_t ulen = len < 0 ? ~0ull : (uint64_t)len;
  auto call = [&](cjs_bz_diff* d, size_t cap) {
    return two ? api.compare_streams(p ? p : &dummy, n, ix, op ? op : &dummy, on, oix, (uint64_t)off, ulen, d, cap, &ci, nullptr)
               : api.compare(p ? p : &dummy, n, ix, op ? op : &dummy, on, (uint64_t)ooff, (uint64_t)off, ulen, d, cap, &ci, nullptr);
  };
  size_t cap = limit < 0 ? 0 : (size_t)limit;
  if (limit < 0) {                                                 // the count query
    rc = call(nullptr, 0);
    cap = (size_t)ci.n_diffs;
  }
  if (rc == 0 && (limit >= 0 || cap)) {
    try { diffs.resize(cap); } catch (...) { api.index_destroy(ix); api.index_destroy(oix); napi_throw_error(env, nullptr, "out of memory"); return nullptr; }
    rc = call(cap ? diffs.data() : nullptr, cap);
  }
  std::string detail = rc == 0 && !ci.n_bad_blocks && !ci.n_bad_blocks_b ? "" : api.detail_();      // (before the next call of the library on this thread)
  api.index_destroy(ix); api.index_destroy(oix);
  if (rc != 0) return throw_code(env, rc);
  const size_t got = (size_t)std::min<uint64_t>(cap, ci.n_diffs);
  napi_value res, dab, dta, v; void* ddst;
  napi_create_object(env, &res);
  napi_create_arraybuffer(env, sizeof(double) * 3 * got, &ddst, &dab);
  for (size_t k = 0; k < got; k++) { ((double*)ddst)[3 * k] = (double)diffs[k].off; ((double*)ddst)[3 * k + 1] = (double)diffs[k].a; ((double*)ddst)[3 * k + 2] = (double)diffs[k].b; }
  napi_create_typedarray(env, napi_float64_array, 3 * got, dab, 0, &dta);
  napi_set_named_property(env, res, "diffs", dta);
  napi_create_double(env, (double)ci.n_diffs, &v); napi_set_named_property(env, res, "total", v);
  napi_create_double(env, ci.n_diffs ? (double)ci.first_diff : -1.0, &v); napi_set_named_property(env, res, "firstDiff", v);
  napi_create_double(env, (double)ci.compared, &v); napi_set_named_property(env, res, "compared", v);
  napi_create_double(env, (double)len_a, &v); napi_set_named_property(env, res, "lenA", v);
  napi_create_double(env, (double)len_b, &v); napi_set_named_property(env, res, "lenB", v);
  napi_create_double(env, (double)ci.n_bad_blocks, &v); napi_set_named_property(env, res, "badBlocks", v);
  napi_create_double(env, ci.n_bad_blocks ? (double)ci.first_bad_block : -1.0, &v); napi_set_named_property(env, res, "firstBadBlock", v);
  napi_create_double(env, (double)ci.n_bad_blocks_b, &v); napi_set_named_property(env, res, "badBlocksB", v);
  napi_create_double(env, ci.n_bad_blocks_b ? (double)ci.first_bad_block_b : -1.0, &v); napi_set_named_property(env, res, "firstBadBlockB", v);
  napi_create_string_utf8(env, detail.c_str(), NAPI_AUTO_LENGTH, &v); napi_set_named_property(env, res, "detail", v);
  return res;
}

// bzip2BuildLineIndex(input, index) -> Uint8Array: the serialised line table of the stream under its serialised block index
// (Bzip2.buildLineIndex)
napi_value bzip2_build_line_index(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 2; napi_value argv[2];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t *p = nullptr, *ip = nullptr; size_t n = 0, in = 0;
  if (argc < 2 || !get_bytes(env, argv[0], &p, &n) || !get_bytes(env, argv[1], &ip, &in)) {
    napi_throw_type_error(env, nullptr, "expected (Uint8Array, Uint8Array index)"); return nullptr;
  }
  static const uint8_t dummy = 0;
  cjs_bz_index* ix = nullptr;
  int rc = api.index_load(ip ? ip : &dummy, in, &ix);
  if (rc != 0) return throw_code(env, rc);
  cjs_bz_lines* lt = nullptr;
  rc = api.lines_build(p ? p : &dummy, n, ix, &lt, nullptr);
  api.index_destroy(ix);
  if (rc != 0) return throw_code(env, rc);
  uint8_t* raw = nullptr; size_t raw_n = 0;
  rc = api.lines_save(lt, &raw, &raw_n);
  api.lines_destroy(lt);
  if (rc != 0) return throw_code(env, rc);
  return wrap_result(env, raw, raw_n);
}

// bzip2LinesAsk(input, index, lineIndex, questions, kind) -> { answers: Float64Array, status: Float64Array, detail: string }
// (Bzip2.lineStarts: kind 0, questions = line numbers; Bzip2.lineNumbers: kind 1, questions = decoded offsets).  questions:
// Float64Array of integers from 0 to 2^53; detail is the lowest-index failing question's ("" when none failed).
napi_value bzip2_lines_ask(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 5; napi_value argv[5];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t *p = nullptr, *ip = nullptr, *lp = nullptr; size_t n = 0, in = 0, ln = 0;
  bool is_ta = false;
  if (argc >= 4) napi_is_typedarray(env, argv[3], &is_ta);
  napi_typedarray_type t = napi_int8_array; size_t count = 0; void* qd = nullptr; napi_value qab; size_t qoff = 0;
  if (is_ta) napi_get_typedarray_info(env, argv[3], &t, &count, &qd, &qab, &qoff);
  if (argc < 5 || !get_bytes(env, argv[0], &p, &n) || !get_bytes(env, argv[1], &ip, &in) || !get_bytes(env, argv[2], &lp, &ln) || !is_ta || t != napi_float64_array) {
    napi_throw_type_error(env, nullptr, "expected (Uint8Array, Uint8Array index, Uint8Array line index, Float64Array questions, kind)"); return nullptr;
  }
  int32_t kind = 0;
  napi_get_value_int32(env, argv[4], &kind);
  std::vector<uint64_t> q(count + 1), a(count + 1); std::vector<int32_t> status(count + 1);
  for (size_t k = 0; k < count; k++) {
    const double v = ((const double*)qd)[k];
    if (!(v >= 0 && v <= 9007199254740992.0 && v == (double)(uint64_t)v)) {      // (negative, NaN, above 2^53 or with a fraction)
      napi_throw_type_error(env, nullptr, "line numbers and offsets are integers from 0 to 2^53"); return nullptr;
    }
    q[k] = (uint64_t)v;
  }
  static const uint8_t dummy = 0;
  cjs_bz_index* ix = nullptr;
  int rc = api.index_load(ip ? ip : &dummy, in, &ix);
  if (rc != 0) return throw_code(env, rc);
  cjs_bz_lines* lt = nullptr;
  rc = api.lines_load(lp ? lp : &dummy, ln, ix, &lt);
  if (rc != 0) { api.index_destroy(ix); return throw_code(env, rc); }
  rc = (kind ? api.lines_number : api.lines_locate)(p ? p : &dummy, n, ix, lt, q.data(), count, a.data(), status.data(), nullptr);
  std::string detail = api.detail_();                            // (before the next call of the library on this thread)
  api.lines_destroy(lt);
  api.index_destroy(ix);
  if (rc != 0) return throw_code(env, rc);
  napi_value res, ab, ta, dstr; void* dst;
  napi_create_object(env, &res);
  napi_create_arraybuffer(env, sizeof(double) * count, &dst, &ab);
  for (size_t k = 0; k < count; k++) ((double*)dst)[k] = (double)a[k];
  napi_create_typedarray(env, napi_float64_array, count, ab, 0, &ta);
  napi_set_named_property(env, res, "answers", ta);
  napi_create_arraybuffer(env, sizeof(double) * count, &dst, &ab);
  bool failed = false;
  for (size_t k = 0; k < count; k++) { ((double*)dst)[k] = (double)status[k]; failed = failed || status[k]; }
  napi_create_typedarray(env, napi_float64_array, count, ab, 0, &ta);
  napi_set_named_property(env, res, "status", ta);
  napi_create_string_utf8(env, failed ? detail.c_str() : "", NAPI_AUTO_LENGTH, &dstr);
  napi_set_named_property(env, res, "detail", dstr);
  return res;
}

// A whole number from 0 to 2^53 out of a JS number (false: negative, NaN, above 2^53 or with a fraction).
bool get_whole(napi_env env, napi_value v, uint64_t* out) {
  double d = 0;
  if (napi_get_value_double(env, v, &d) != napi_ok || !(d >= 0 && d <= 9007199254740992.0 && d == (double)(uint64_t)d)) return false;
  *out = (uint64_t)d;
  return true;
}

// bzip2LineKeys(input, index, lineIndex, first, count, seed) -> { keys: Uint8Array, lines, badBlocks, firstBadBlock, detail }
// (Bzip2.lineKeys).  keys: the 16-byte records (cjs_bz_linekey, little-endian: u64 hash, u32 len, u32 check) of lines first ..
// first + count - 1 (count < 0: to the last); lines: their number; first, count and seed are integers from 0 to 2^53.
napi_value bzip2_line_keys(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 6; napi_value argv[6];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t *p = nullptr, *ip = nullptr, *lp = nullptr; size_t n = 0, in = 0, ln = 0;
  if (argc < 6 || !get_bytes(env, argv[0], &p, &n) || !get_bytes(env, argv[1], &ip, &in) || !get_bytes(env, argv[2], &lp, &ln)) {
    napi_throw_type_error(env, nullptr, "expected (Uint8Array, Uint8Array index, Uint8Array line index, first, count, seed)"); return nullptr;
  }
  uint64_t first = 0, count = ~0ull, seed = 0;
  double c = -1;
  napi_get_value_double(env, argv[4], &c);
  if (!get_whole(env, argv[3], &first) || (c >= 0 && !get_whole(env, argv[4], &count)) || !(c >= 0 || c == -1) || !get_whole(env, argv[5], &seed)) {
    napi_throw_type_error(env, nullptr, "first, count and seed are integers from 0 to 2^53"); return nullptr;
  }
  static const uint8_t dummy = 0;
  cjs_bz_index* ix = nullptr;
  int rc = api.index_load(ip ? ip : &dummy, in, &ix);
  if (rc != 0) return throw_code(env, rc);
  cjs_bz_lines* lt = nullptr;
  rc = api.lines_load(lp ? lp : &dummy, ln, ix, &lt);
  if (rc != 0) { api.index_destroy(ix); return throw_code(env, rc); }
  cjs_bz_linekeys_info ki;
  rc = api.line_keys(p ? p : &dummy, n, ix, lt, first, count, seed, nullptr, 0, &ki, nullptr);      // the count query: the table alone
  napi_value res = nullptr, ab, ta, v; void* dst = nullptr;
  std::string detail;
  if (rc == 0) {
    napi_create_arraybuffer(env, sizeof(cjs_bz_linekey) * (size_t)ki.n_lines, &dst, &ab);
    if (ki.n_lines) rc = api.line_keys(p ? p : &dummy, n, ix, lt, first, count, seed, (cjs_bz_linekey*)dst, (size_t)ki.n_lines, &ki, nullptr);
    if (rc == 0 && ki.n_bad_blocks) detail = api.detail_();      // (before the next call of the library on this thread)
  }
  api.lines_destroy(lt);
  api.index_destroy(ix);
  if (rc != 0) return throw_code(env, rc);
  napi_create_object(env, &res);
  napi_create_typedarray(env, napi_uint8_array, sizeof(cjs_bz_linekey) * (size_t)ki.n_lines, ab, 0, &ta);
  napi_set_named_property(env, res, "keys", ta);
  napi_create_double(env, (double)ki.n_lines, &v); napi_set_named_property(env, res, "lines", v);
  napi_create_double(env, (double)ki.n_bad_blocks, &v); napi_set_named_property(env, res, "badBlocks", v);
  napi_create_double(env, ki.n_bad_blocks ? (double)ki.first_bad_block : -1.0, &v); napi_set_named_property(env, res, "firstBadBlock", v);
  napi_create_string_utf8(env, detail.c_str(), NAPI_AUTO_LENGTH, &v); napi_set_named_property(env, res, "detail", v);
  return res;
}

// a cut LIST argument: a cut-style string (cjs_cut_list_parse) or a Float64Array of (lo, hi) pairs, hi < 0: to the end of the line.
// false: an exception is pending
static bool get_cut_list(napi_env env, napi_value v, std::vector<cjs_cut_range>& sel, uint32_t& nsel) {
  sel.assign(64, cjs_cut_range{0, 0});
  nsel = 0;
  napi_valuetype kind = napi_undefined;
  napi_typeof(env, v, &kind);
  if (kind == napi_string) {
    size_t len = 0;
    napi_get_value_string_utf8(env, v, nullptr, 0, &len);
    std::string list(len + 1, 0);
    napi_get_value_string_utf8(env, v, &list[0], len + 1, &len);
    const int rc = api.cut_list_parse(list.c_str(), sel.data(), 64, &nsel);
    if (rc != 0) { throw_code(env, rc); return false; }
  } else {
    bool is_ta = false;
    napi_is_typedarray(env, v, &is_ta);
    napi_typedarray_type t = napi_int8_array; size_t len = 0; void* d = nullptr; napi_value ab; size_t off = 0;
    if (is_ta) napi_get_typedarray_info(env, v, &t, &len, &d, &ab, &off);
    if (!is_ta || t != napi_float64_array || (len & 1)) { napi_throw_type_error(env, nullptr, "list is a string or a Float64Array of (lo, hi) pairs"); return false; }
    const double* q = (const double*)d;
    sel.resize(len / 2 ? len / 2 : 1);
    for (size_t k = 0; k < len / 2; k++) {
      const double lo = q[2 * k], hi = q[2 * k + 1] < 0 ? 4294967295.0 : q[2 * k + 1];
      if (!(lo >= 0 && lo <= 4294967295.0 && hi <= 4294967295.0 && lo == (double)(uint32_t)lo && hi == (double)(uint32_t)hi)) {
        napi_throw_type_error(env, nullptr, "a unit number is an integer that fits 32 bits"); return false;
      }
      sel[k].lo = (uint32_t)lo; sel[k].hi = (uint32_t)hi;
    }
    nsel = len / 2 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)(len / 2);      // (the library refuses none and more than 64)
  }
  return true;
}

// bzip2Tally(input, index, lineIndex, first, count, seed, order, minCount, maxCount, limit, mode, delim, list) -> { groups: Uint8Array, nLines, nDistinct,
// nGroups, nBadLines, maxCount, badBlocks, firstBadBlock, detail } (Bzip2.tallyLines).  groups: the 32-byte records (cjs_bz_tally,
// little-endian: u64 hash, u32 len, u32 check, u64 first, u64 count) of the first `limit` groups (limit < 0: all of them; the
// window's lines by the table bound their number) of lines first .. first + count - 1 (count < 0: to the last); order 0: by first
// occurrence, 1: by descending count.  The numbers are integers from 0 to 2^53.  mode 2: whole lines (delim and list are not looked
// at); mode 0 / 1 with a delimiter byte and a list as bzip2Cut takes them: the tally of that cut.
napi_value bzip2_tally(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 13; napi_value argv[13];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t *p = nullptr, *ip = nullptr, *lp = nullptr; size_t n = 0, in = 0, ln = 0;
  uint32_t mode = 2, delim = 0;
  if (argc < 13 || !get_bytes(env, argv[0], &p, &n) || !get_bytes(env, argv[1], &ip, &in) || !get_bytes(env, argv[2], &lp, &ln) ||
      napi_get_value_uint32(env, argv[10], &mode) != napi_ok || napi_get_value_uint32(env, argv[11], &delim) != napi_ok) {
    napi_throw_type_error(env, nullptr, "expected (Uint8Array, Uint8Array index, Uint8Array line index, first, count, seed, order, minCount, maxCount, limit, mode, "
                          "delimiter byte, list)");
    return nullptr;
  }
  std::vector<cjs_cut_range> sel;
  uint32_t nsel = 0;
  if (mode != 2 && !get_cut_list(env, argv[12], sel, nsel)) return nullptr;
  uint64_t first = 0, count = ~0ull, seed = 0, order = 0, lo = 0, hi = 0, limit = 0;
  double c = -1, lim = -1;
  napi_get_value_double(env, argv[4], &c);
  napi_get_value_double(env, argv[9], &lim);
  if (!get_whole(env, argv[3], &first) || (c >= 0 && !get_whole(env, argv[4], &count)) || !(c >= 0 || c == -1) || !get_whole(env, argv[5], &seed) ||
      !get_whole(env, argv[6], &order) || !get_whole(env, argv[7], &lo) || !get_whole(env, argv[8], &hi) || (lim >= 0 && !get_whole(env, argv[9], &limit)) ||
      !(lim >= 0 || lim == -1)) {
    napi_throw_type_error(env, nullptr, "first, count, seed, minCount, maxCount and limit are integers from 0 to 2^53"); return nullptr;
  }
  static const uint8_t dummy = 0;
  cjs_bz_index* ix = nullptr;
  int rc = api.index_load(ip ? ip : &dummy, in, &ix);
  if (rc != 0) return throw_code(env, rc);
  cjs_bz_lines* lt = nullptr;
  rc = api.lines_load(lp ? lp : &dummy, ln, ix, &lt);
  if (rc != 0) { api.index_destroy(ix); return throw_code(env, rc); }
  cjs_bz_linekeys_info ki;
  rc = api.line_keys(p ? p : &dummy, n, ix, lt, first, count, seed, nullptr, 0, &ki, nullptr);      // the window's lines: the table alone
  cjs_bz_tally_info ti;
  std::vector<cjs_bz_tally> groups;
  std::string detail;
  if (rc == 0) {
    const size_t cap = (size_t)(lim < 0 || limit > ki.n_lines ? ki.n_lines : limit);
    groups.resize(cap ? cap : 1);
    rc = api.tally(p ? p : &dummy, n, ix, lt, first, count, seed, mode, delim, nsel ? sel.data() : nullptr, nsel, order > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)order, lo, hi, cap ? groups.data() : nullptr, cap, &ti,
                   nullptr);
    if (rc == 0) groups.resize((size_t)(ti.n_groups < cap ? ti.n_groups : cap));
    if (rc == 0 && ti.n_bad_blocks) detail = api.detail_();      // (before the next call of the library on this thread)
  }
  if (rc != 0) throw_code(env, rc);                           // (the detail is read before the next call of the library on this thread)
  api.lines_destroy(lt);
  api.index_destroy(ix);
  if (rc != 0) return nullptr;
  napi_value res = nullptr, ab, ta, v; void* dst = nullptr;
  napi_create_arraybuffer(env, sizeof(cjs_bz_tally) * groups.size(), &dst, &ab);
  if (!groups.empty()) memcpy(dst, groups.data(), sizeof(cjs_bz_tally) * groups.size());
  napi_create_object(env, &res);
  napi_create_typedarray(env, napi_uint8_array, sizeof(cjs_bz_tally) * groups.size(), ab, 0, &ta);
  napi_set_named_property(env, res, "groups", ta);
  napi_create_double(env, (double)ti.n_lines, &v); napi_set_named_property(env, res, "nLines", v);
  napi_create_double(env, (double)ti.n_distinct, &v); napi_set_named_property(env, res, "nDistinct", v);
  napi_create_double(env, (double)ti.n_groups, &v); napi_set_named_property(env, res, "nGroups", v);
  napi_create_double(env, (double)ti.n_bad_lines, &v); napi_set_named_property(env, res, "nBadLines", v);
  napi_create_double(env, (double)ti.max_count, &v); napi_set_named_property(env, res, "maxCount", v);
  napi_create_double(env, (double)ti.n_bad_blocks, &v); napi_set_named_property(env, res, "badBlocks", v);
  napi_create_double(env, ti.n_bad_blocks ? (double)ti.first_bad_block : -1.0, &v); napi_set_named_property(env, res, "firstBadBlock", v);
  napi_create_string_utf8(env, detail.c_str(), NAPI_AUTO_LENGTH, &v); napi_set_named_property(env, res, "detail", v);
  return res;
}

// bzip2Sort(input, index, lineIndex, first, count, flags, limit, wantText, mode, delim, list) -> { lines: Float64Array, counts: Float64Array, text: Uint8Array
// or undefined, nLines, nOut, nDistinct, textBytes, rounds } (Bzip2.sortLines): the numbers of lines first .. first + count - 1 (count < 0:
// to the last) in LC_ALL=C order of their content, equal lines by ascending number; flags 1: descending content, 2: one entry per
// run of equal lines with the run's size as its count; the first `limit` entries (limit < 0: all); wantText: their lines, each with
// a newline.  mode 2: whole lines; mode 0 / 1 with a delimiter byte and a list as bzip2Cut takes them: the sort of that cut.  The
// numbers are integers from 0 to 2^53.
napi_value bzip2_sort(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 11; napi_value argv[11];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t *p = nullptr, *ip = nullptr, *lp = nullptr; size_t n = 0, in = 0, ln = 0;
  uint32_t mode = 2, delim = 0, flags = 0;
  bool want_text = false;
  if (argc < 11 || !get_bytes(env, argv[0], &p, &n) || !get_bytes(env, argv[1], &ip, &in) || !get_bytes(env, argv[2], &lp, &ln) ||
      napi_get_value_uint32(env, argv[5], &flags) != napi_ok || napi_get_value_bool(env, argv[7], &want_text) != napi_ok ||
      napi_get_value_uint32(env, argv[8], &mode) != napi_ok || napi_get_value_uint32(env, argv[9], &delim) != napi_ok) {
    napi_throw_type_error(env, nullptr, "expected (Uint8Array, Uint8Array index, Uint8Array line index, first, count, flags, limit, wantText, mode, delimiter byte, list)");
    return nullptr;
  }
  std::vector<cjs_cut_range> sel;
  uint32_t nsel = 0;
  if (mode != 2 && !get_cut_list(env, argv[10], sel, nsel)) return nullptr;
  uint64_t first = 0, count = ~0ull, limit = 0;
  double c = -1, lim = -1;
  napi_get_value_double(env, argv[4], &c);
  napi_get_value_double(env, argv[6], &lim);
  if (!get_whole(env, argv[3], &first) || (c >= 0 && !get_whole(env, argv[4], &count)) || !(c >= 0 || c == -1) || (lim >= 0 && !get_whole(env, argv[6], &limit)) ||
      !(lim >= 0 || lim == -1)) {
    napi_throw_type_error(env, nullptr, "first, count and limit are integers from 0 to 2^53"); return nullptr;
  }
  static const uint8_t dummy = 0;
  cjs_bz_index* ix = nullptr;
  int rc = api.index_load(ip ? ip : &dummy, in, &ix);
  if (rc != 0) return throw_code(env, rc);
  cjs_bz_lines* lt = nullptr;
  rc = api.lines_load(lp ? lp : &dummy, ln, ix, &lt);
  if (rc != 0) { api.index_destroy(ix); return throw_code(env, rc); }
  cjs_bz_linekeys_info ki;
  rc = api.line_keys(p ? p : &dummy, n, ix, lt, first, count, 0, nullptr, 0, &ki, nullptr);      // the window's lines: the table alone
  cjs_bz_sort_info si;
  std::vector<uint64_t> lines, counts;
  uint8_t* text = nullptr; size_t text_n = 0;
  if (rc == 0) {
    const size_t cap = (size_t)(lim < 0 || limit > ki.n_lines ? ki.n_lines : limit);
    lines.resize(cap ? cap : 1); counts.resize(cap ? cap : 1);
    rc = api.sort(p ? p : &dummy, n, ix, lt, first, count, mode, delim, nsel ? sel.data() : nullptr, nsel, flags, cap ? lines.data() : nullptr,
                  cap ? counts.data() : nullptr, cap, want_text ? &text : nullptr, want_text ? &text_n : nullptr, &si, nullptr);
    if (rc == 0) { lines.resize((size_t)(si.n_out < cap ? si.n_out : cap)); counts.resize(lines.size()); }
  }
  if (rc != 0) throw_code(env, rc);                           // (the detail is read before the next call of the library on this thread)
  api.lines_destroy(lt);
  api.index_destroy(ix);
  if (rc != 0) return nullptr;
  napi_value res = nullptr, ab, ta, v; void* dst = nullptr;
  napi_create_object(env, &res);
  const char* names[2] = {"lines", "counts"};
  const std::vector<uint64_t>* arrays[2] = {&lines, &counts};
  for (int k = 0; k < 2; k++) {
    napi_create_arraybuffer(env, sizeof(double) * lines.size(), &dst, &ab);
    for (size_t i = 0; i < lines.size(); i++) ((double*)dst)[i] = (double)(*arrays[k])[i];
    napi_create_typedarray(env, napi_float64_array, lines.size(), ab, 0, &ta);
    napi_set_named_property(env, res, names[k], ta);
  }
  if (want_text) {
    napi_create_arraybuffer(env, text_n, &dst, &ab);
    if (text_n) memcpy(dst, text, text_n);
    api.free_(text);
    napi_create_typedarray(env, napi_uint8_array, text_n, ab, 0, &ta);
    napi_set_named_property(env, res, "text", ta);
  }
  napi_create_double(env, (double)si.n_lines, &v); napi_set_named_property(env, res, "nLines", v);
  napi_create_double(env, (double)si.n_out, &v); napi_set_named_property(env, res, "nOut", v);
  napi_create_double(env, (double)si.n_distinct, &v); napi_set_named_property(env, res, "nDistinct", v);
  napi_create_double(env, (double)si.text_bytes, &v); napi_set_named_property(env, res, "textBytes", v);
  napi_create_double(env, (double)si.rounds, &v); napi_set_named_property(env, res, "rounds", v);
  return res;
}

// bzip2Cut(input, index, lineIndex, mode, delim, list, first, count) -> Uint8Array (Bzip2.cutLines): the fields (mode 0, delimiter
// byte delim) or byte positions (mode 1) that `list` selects of lines first .. first + count - 1 (count < 0: to the last), each
// line's output behind the other's (cjs_bzip2_cut).  list: a cut-style string ("1,3-5,7-"; cjs_cut_list_parse) or a Float64Array of
// (lo, hi) pairs, hi < 0: to the end of the line.  The result is an external ArrayBuffer over the library's buffer.
napi_value bzip2_cut(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 8; napi_value argv[8];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t *p = nullptr, *ip = nullptr, *lp = nullptr; size_t n = 0, in = 0, ln = 0;
  uint32_t mode = 0, delim = 0;
  if (argc < 8 || !get_bytes(env, argv[0], &p, &n) || !get_bytes(env, argv[1], &ip, &in) || !get_bytes(env, argv[2], &lp, &ln) ||
      napi_get_value_uint32(env, argv[3], &mode) != napi_ok || napi_get_value_uint32(env, argv[4], &delim) != napi_ok) {
    napi_throw_type_error(env, nullptr, "expected (Uint8Array, Uint8Array index, Uint8Array line index, mode, delimiter byte, list, first, count)"); return nullptr;
  }
  uint64_t first = 0, count = ~0ull;
  double c = -1;
  napi_get_value_double(env, argv[7], &c);
  if (!get_whole(env, argv[6], &first) || (c >= 0 && !get_whole(env, argv[7], &count)) || !(c >= 0 || c == -1)) {
    napi_throw_type_error(env, nullptr, "first and count are integers from 0 to 2^53"); return nullptr;
  }
  std::vector<cjs_cut_range> sel;
  uint32_t nsel = 0;
  if (!get_cut_list(env, argv[5], sel, nsel)) return nullptr;
  static const uint8_t dummy = 0;
  cjs_bz_index* ix = nullptr;
  int rc = api.index_load(ip ? ip : &dummy, in, &ix);
  if (rc != 0) return throw_code(env, rc);
  cjs_bz_lines* lt = nullptr;
  rc = api.lines_load(lp ? lp : &dummy, ln, ix, &lt);
  if (rc != 0) { api.index_destroy(ix); return throw_code(env, rc); }
  uint8_t* out = nullptr; size_t out_n = 0;
  cjs_bz_cut_info ci;
  rc = api.cut(p ? p : &dummy, n, ix, lt, first, count, mode, delim, sel.data(), nsel, &out, &out_n, &ci, nullptr);
  if (rc != 0) throw_code(env, rc);                           // (the detail is read before the next call of the library on this thread)
  api.lines_destroy(lt);
  api.index_destroy(ix);
  return rc != 0 ? nullptr : wrap_result(env, out, out_n);
}

// lineKeysDiff(keysA, keysB, maxEdits) -> { hunks: Float64Array, edits, common, minimal } (Bzip2.diffLines): the line diff of two
// arrays of 16-byte records on the host (cjs_line_keys_diff); hunks holds four numbers per hunk: aFirst, aCount, bFirst, bCount.
napi_value line_keys_diff(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 3; napi_value argv[3];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t *a = nullptr, *b = nullptr; size_t na = 0, nb = 0;
  uint64_t max_edits = 0;
  if (argc < 3 || !get_bytes(env, argv[0], &a, &na) || !get_bytes(env, argv[1], &b, &nb) || na % sizeof(cjs_bz_linekey) || nb % sizeof(cjs_bz_linekey) ||
      !get_whole(env, argv[2], &max_edits)) {
    napi_throw_type_error(env, nullptr, "expected (Uint8Array keys, Uint8Array keys, maxEdits): 16 bytes per key"); return nullptr;
  }
  // (a typed array's bytes may stand at any address: the records are copied to where they are aligned)
  std::vector<cjs_bz_linekey> ka(na / sizeof(cjs_bz_linekey) + 1), kb(nb / sizeof(cjs_bz_linekey) + 1);
  if (na) memcpy(ka.data(), a, na);
  if (nb) memcpy(kb.data(), b, nb);
  cjs_bz_ldiff_info di;
  int rc = api.line_keys_diff(ka.data(), na / sizeof(cjs_bz_linekey), kb.data(), nb / sizeof(cjs_bz_linekey), max_edits, nullptr, 0, &di);
  if (rc != 0) return throw_code(env, rc);
  std::vector<cjs_bz_hunk> h((size_t)di.n_hunks + 1);
  rc = api.line_keys_diff(ka.data(), na / sizeof(cjs_bz_linekey), kb.data(), nb / sizeof(cjs_bz_linekey), max_edits, h.data(), (size_t)di.n_hunks, &di);
  if (rc != 0) return throw_code(env, rc);
  napi_value res, ab, ta, v; void* dst;
  napi_create_object(env, &res);
  napi_create_arraybuffer(env, sizeof(double) * 4 * (size_t)di.n_hunks, &dst, &ab);
  for (size_t k = 0; k < (size_t)di.n_hunks; k++) {
    double* d = (double*)dst + 4 * k;
    d[0] = (double)h[k].a_first; d[1] = (double)h[k].a_count; d[2] = (double)h[k].b_first; d[3] = (double)h[k].b_count;
  }
  napi_create_typedarray(env, napi_float64_array, 4 * (size_t)di.n_hunks, ab, 0, &ta);
  napi_set_named_property(env, res, "hunks", ta);
  napi_create_double(env, (double)di.edits, &v); napi_set_named_property(env, res, "edits", v);
  napi_create_double(env, (double)di.common, &v); napi_set_named_property(env, res, "common", v);
  napi_get_boolean(env, di.minimal != 0, &v); napi_set_named_property(env, res, "minimal", v);
  return res;
}

// bzip2Recover(input, asStream) -> { data: Uint8Array, found: Float64Array }   (Bzip2.recoverFile)
// found holds six numbers per block candidate, ascending: bitpos, end_bit, out_off, size, status, crc (cjs_bz_found).
napi_value bzip2_recover(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 2; napi_value argv[2];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t* p = nullptr; size_t n = 0;
  if (argc < 1 || !get_bytes(env, argv[0], &p, &n)) { napi_throw_type_error(env, nullptr, "expected a Uint8Array or Buffer"); return nullptr; }
  int32_t as_stream = 0;
  if (argc >= 2) napi_get_value_int32(env, argv[1], &as_stream);
  static const uint8_t dummy = 0;
  long cap = (long)(n / 64 + 1024), nf = 0;                     // (more magics than that: one more call)
  std::vector<cjs_bz_found> found;
  uint8_t* out = nullptr; size_t out_n = 0;
  for (;;) {
    found.resize((size_t)cap);
    const int rc = api.bzip2_recover(p ? p : &dummy, n, as_stream, &out, &out_n, found.data(), cap, &nf, nullptr);
    if (rc != 0) return throw_code(env, rc);
    if (nf <= cap) break;
    api.free_(out);
    cap = nf;
  }
  napi_value res, ab, ta; void* dst;
  napi_create_object(env, &res);
  napi_set_named_property(env, res, "data", wrap_result(env, out, out_n));
  napi_create_arraybuffer(env, sizeof(double) * 6 * (size_t)nf, &dst, &ab);
  for (long i = 0; i < nf; i++) {
    const cjs_bz_found& f = found[(size_t)i];
    double* d = (double*)dst + 6 * i;
    d[0] = (double)f.bitpos; d[1] = (double)f.end_bit; d[2] = (double)f.out_off; d[3] = (double)f.size; d[4] = (double)f.status; d[5] = (double)f.crc;
  }
  napi_create_typedarray(env, napi_float64_array, 6 * (size_t)nf, ab, 0, &ta);
  napi_set_named_property(env, res, "found", ta);
  return res;
}

// bzip2CompressBatch(array of Uint8Array / Buffer, level) -> array of Uint8Array   (Bzip2.compressFiles)
// The streams are views of ONE external ArrayBuffer over the library's result buffer.
napi_value bzip2_batch(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 2; napi_value argv[2];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool is_arr = false;
  if (argc >= 1) napi_is_array(env, argv[0], &is_arr);
  if (!is_arr) { napi_throw_type_error(env, nullptr, "expected an array of Uint8Array or Buffer"); return nullptr; }
  int32_t level = 9;
  if (argc >= 2) napi_get_value_int32(env, argv[1], &level);
  uint32_t count = 0;
  napi_get_array_length(env, argv[0], &count);
  std::vector<const uint8_t*> ptr(count + 1, nullptr);
  std::vector<size_t> len(count + 1, 0), off(count + 1, 0), slen(count + 1, 0);
  for (uint32_t k = 0; k < count; k++) {
    napi_value v;
    napi_get_element(env, argv[0], k, &v);
    if (!get_bytes(env, v, &ptr[k], &len[k])) { napi_throw_type_error(env, nullptr, "expected an array of Uint8Array or Buffer"); return nullptr; }
  }
  uint8_t* out = nullptr;
  const int rc = api.bzip2_compress_batch(ptr.data(), len.data(), count, level, &out, off.data(), slen.data(), nullptr);
  if (rc != 0) return throw_code(env, rc);
  size_t total = 0;
  for (uint32_t k = 0; k < count; k++) total = off[k] + slen[k] > total ? off[k] + slen[k] : total;
  napi_value res;
  napi_create_array_with_length(env, count, &res);
  if (!count) return res;
  napi_value ab;
  int64_t adj = 0;
  if (napi_create_external_arraybuffer(env, out, total, finalize_buf, (void*)(intptr_t)total, &ab) == napi_ok) napi_adjust_external_memory(env, (int64_t)total, &adj);
  else {
    void* dst;
    napi_create_arraybuffer(env, total, &dst, &ab);
    if (total) memcpy(dst, out, total);
    api.free_(out);
  }
  for (uint32_t k = 0; k < count; k++) {
    napi_value ta;
    napi_create_typedarray(env, napi_uint8_array, slen[k], ab, off[k], &ta);
    napi_set_element(env, res, k, ta);
  }
  return res;
}

// bzip2DecompressBatch(array of Uint8Array / Buffer, multistream) -> array of Uint8Array   (Bzip2.decompressFiles)
// The outputs are views of ONE external ArrayBuffer over the library's result buffer.  If an input fails, the error of the
// lowest-index one is thrown (throw_code: its detail) with `cjsIndex`.
napi_value bzip2_decompress_batch(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 2; napi_value argv[2];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool is_arr = false;
  if (argc >= 1) napi_is_array(env, argv[0], &is_arr);
  if (!is_arr) { napi_throw_type_error(env, nullptr, "expected an array of Uint8Array or Buffer"); return nullptr; }
  int32_t multi = 0;
  if (argc >= 2) napi_get_value_int32(env, argv[1], &multi);
  uint32_t count = 0;
  napi_get_array_length(env, argv[0], &count);
  std::vector<const uint8_t*> ptr(count + 1, nullptr);
  std::vector<size_t> len(count + 1, 0), off(count + 1, 0), olen(count + 1, 0);
  std::vector<int32_t> status(count + 1, 0);
  for (uint32_t k = 0; k < count; k++) {
    napi_value v;
    napi_get_element(env, argv[0], k, &v);
    if (!get_bytes(env, v, &ptr[k], &len[k])) { napi_throw_type_error(env, nullptr, "expected an array of Uint8Array or Buffer"); return nullptr; }
  }
  uint8_t* out = nullptr;
  const int rc = api.bzip2_decompress_batch(ptr.data(), len.data(), count, multi, &out, off.data(), olen.data(), status.data(), nullptr);
  if (rc != 0) return throw_code(env, rc);
  for (uint32_t k = 0; k < count; k++) if (status[k] != 0) {
    api.free_(out);
    throw_code(env, status[k]);
    napi_value exc, idx;
    if (napi_get_and_clear_last_exception(env, &exc) == napi_ok) {
      napi_create_uint32(env, k, &idx);
      napi_set_named_property(env, exc, "cjsIndex", idx);
      napi_throw(env, exc);
    }
    return nullptr;
  }
  size_t total = 0;
  for (uint32_t k = 0; k < count; k++) total = off[k] + olen[k] > total ? off[k] + olen[k] : total;
  napi_value res;
  napi_create_array_with_length(env, count, &res);
  if (!count) return res;
  napi_value ab;
  int64_t adj = 0;
  if (napi_create_external_arraybuffer(env, out, total, finalize_buf, (void*)(intptr_t)total, &ab) == napi_ok) napi_adjust_external_memory(env, (int64_t)total, &adj);
  else {
    void* dst;
    napi_create_arraybuffer(env, total, &dst, &ab);
    if (total) memcpy(dst, out, total);
    api.free_(out);
  }
  for (uint32_t k = 0; k < count; k++) {
    napi_value ta;
    napi_create_typedarray(env, napi_uint8_array, olen[k], ab, off[k], &ta);
    napi_set_element(env, res, k, ta);
  }
  return res;
}

// The tables an indexed compress call made, in the serialised forms bzip2BuildIndex / bzip2BuildLineIndex return, set as `index`
// and `lineIndex` (null without a line table) of obj; both objects are destroyed here.  False: an exception is pending.
bool set_tables(napi_env env, napi_value obj, cjs_bz_index* ix, cjs_bz_lines* lt) {
  uint8_t *raw = nullptr, *lraw = nullptr; size_t raw_n = 0, lraw_n = 0;
  int rc = api.index_save(ix, &raw, &raw_n);
  if (!rc && lt) rc = api.lines_save(lt, &lraw, &lraw_n);
  api.index_destroy(ix);
  if (lt) api.lines_destroy(lt);
  if (rc != 0) { api.free_(raw); api.free_(lraw); throw_code(env, rc); return false; }
  napi_value nul;
  napi_get_null(env, &nul);
  napi_set_named_property(env, obj, "index", wrap_result(env, raw, raw_n));
  napi_set_named_property(env, obj, "lineIndex", lt ? wrap_result(env, lraw, lraw_n) : nul);
  return true;
}

// bzip2CompressIndexed(input, level, wantLines) -> { data, index, lineIndex }: the stream of bzip2Compress and the tables of
// exactly that stream (Bzip2.compressFileIndexed)
napi_value bzip2_compress_indexed(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 3; napi_value argv[3];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  const uint8_t* p = nullptr; size_t n = 0;
  if (argc < 1 || !get_bytes(env, argv[0], &p, &n)) { napi_throw_type_error(env, nullptr, "expected a Uint8Array or Buffer"); return nullptr; }
  int32_t level = 9;
  if (argc >= 2) napi_get_value_int32(env, argv[1], &level);
  bool want_lines = true;
  if (argc >= 3) napi_get_value_bool(env, argv[2], &want_lines);
  static const uint8_t dummy = 0;
  uint8_t* out = nullptr; size_t out_n = 0;
  cjs_bz_index* ix = nullptr; cjs_bz_lines* lt = nullptr;
  const int rc = api.compress_indexed(p ? p : &dummy, n, level, &out, &out_n, &ix, want_lines ? &lt : nullptr, nullptr);
  if (rc != 0) return throw_code(env, rc);
  napi_value res;
  napi_create_object(env, &res);
  napi_set_named_property(env, res, "data", wrap_result(env, out, out_n));
  if (!set_tables(env, res, ix, lt)) return nullptr;
  return res;
}

// ---- streaming encoder (cjs_bzip2_enc_*): bzip2EncCreate(level, chunkBytes[, flags]) -> handle (flags: cjs_opts.flags, 4 = keep
// the index of the stream, 8 = and its line table); bzip2EncIndex(handle, wantLines) -> { index, lineIndex } once finished;
// bzip2EncWrite(handle, bytes);
// bzip2EncFinish(handle); bzip2EncPending(handle) -> number; bzip2EncRead(handle, maxBytes) -> Uint8Array (at most maxBytes of
// what is pending, never blocks); bzip2EncDestroy(handle).  The handle is an external whose finalizer destroys the encoder if
// bzip2EncDestroy has not.
struct EncHandle { cjs_bz_enc* e = nullptr; };
void finalize_enc(napi_env, void* data, void*) {
  EncHandle* h = (EncHandle*)data;
  if (h->e && api.enc_destroy) api.enc_destroy(h->e);
  delete h;
}
EncHandle* enc_arg(napi_env env, napi_callback_info info, size_t want, napi_value* argv) {
  size_t argc = want;
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  void* p = nullptr;
  if (argc < want || napi_get_value_external(env, argv[0], &p) != napi_ok || !p || !((EncHandle*)p)->e) {
    napi_throw_type_error(env, nullptr, "expected an open encoder handle");
    return nullptr;
  }
  return (EncHandle*)p;
}
napi_value enc_create(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 3; napi_value argv[3];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  int32_t level = 9; double chunk = 0; uint32_t flags = 0;
  if (argc >= 1) napi_get_value_int32(env, argv[0], &level);
  if (argc >= 2) napi_get_value_double(env, argv[1], &chunk);
  if (argc >= 3) napi_get_value_uint32(env, argv[2], &flags);
  cjs_opts opts; memset(&opts, 0, sizeof opts);
  opts.struct_size = sizeof opts; opts.device = -1; opts.flags = flags;
  EncHandle* h = new EncHandle();
  const int rc = api.enc_create(&h->e, level, chunk > 0 ? (size_t)chunk : 0, flags ? &opts : nullptr);
  if (rc != 0) { delete h; return throw_code(env, rc); }
  napi_value v;
  if (napi_create_external(env, h, finalize_enc, nullptr, &v) != napi_ok) { api.enc_destroy(h->e); delete h; napi_throw_error(env, nullptr, "cannot create the encoder handle"); return nullptr; }
  return v;
}
napi_value enc_write(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  EncHandle* h = enc_arg(env, info, 2, argv);
  if (!h) return nullptr;
  const uint8_t* p = nullptr; size_t n = 0;
  if (!get_bytes(env, argv[1], &p, &n)) { napi_throw_type_error(env, nullptr, "expected a Uint8Array or Buffer"); return nullptr; }
  const int rc = api.enc_write(h->e, n ? p : nullptr, n);
  if (rc != 0) return throw_code(env, rc);
  napi_value v; napi_get_undefined(env, &v); return v;
}
napi_value enc_finish(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  EncHandle* h = enc_arg(env, info, 1, argv);
  if (!h) return nullptr;
  const int rc = api.enc_finish(h->e);
  if (rc != 0) return throw_code(env, rc);
  napi_value v; napi_get_undefined(env, &v); return v;
}
napi_value enc_index(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  EncHandle* h = enc_arg(env, info, 2, argv);
  if (!h) return nullptr;
  bool want_lines = false;
  napi_get_value_bool(env, argv[1], &want_lines);
  cjs_bz_index* ix = nullptr; cjs_bz_lines* lt = nullptr;
  const int rc = api.enc_index(h->e, &ix, want_lines ? &lt : nullptr);
  if (rc != 0) return throw_code(env, rc);
  napi_value res;
  napi_create_object(env, &res);
  if (!set_tables(env, res, ix, lt)) return nullptr;
  return res;
}
napi_value enc_pending(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  EncHandle* h = enc_arg(env, info, 1, argv);
  if (!h) return nullptr;
  napi_value v; napi_create_double(env, (double)api.enc_pending(h->e), &v); return v;
}
napi_value enc_read(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  EncHandle* h = enc_arg(env, info, 2, argv);
  if (!h) return nullptr;
  double cap = 0;
  napi_get_value_double(env, argv[1], &cap);
  size_t n = api.enc_pending(h->e);
  if (cap < (double)n) n = cap > 0 ? (size_t)cap : 0;
  napi_value ab, ta; void* dst = nullptr;
  if (napi_create_arraybuffer(env, n, &dst, &ab) != napi_ok) { napi_throw_error(env, nullptr, "cannot allocate the output piece"); return nullptr; }
  size_t got = 0;
  static uint8_t dummy;
  const int rc = api.enc_read(h->e, dst ? (uint8_t*)dst : &dummy, n, &got);
  if (rc != 0) return throw_code(env, rc);
  napi_create_typedarray(env, napi_uint8_array, got, ab, 0, &ta);
  return ta;
}
napi_value enc_destroy(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  void* p = nullptr;
  if (argc >= 1 && napi_get_value_external(env, argv[0], &p) == napi_ok && p) {
    EncHandle* h = (EncHandle*)p;
    if (h->e && api.enc_destroy) api.enc_destroy(h->e);
    h->e = nullptr;
  }
  napi_value v; napi_get_undefined(env, &v); return v;
}

// ---- streaming decoder (cjs_bzip2_dec_*), a pull model: bzip2DecCreate(multistream, chunkBytes, outBytes) -> handle;
// bzip2DecWrite(handle, bytes) -> number of bytes taken (may be 0: read until empty, then write again); bzip2DecFinish(handle);
// bzip2DecRead(handle, buf) -> number of decoded bytes put at the front of the Uint8Array buf (0: write more, or after finish the
// end; this call runs the GPU steps and throws the stream's error once the bytes in front of it have been read);
// bzip2DecDone(handle) -> boolean; bzip2DecDestroy(handle).  The handle's finalizer destroys a decoder still open.
struct DecHandle { cjs_bz_dec* d = nullptr; };
void finalize_dec(napi_env, void* data, void*) {
  DecHandle* h = (DecHandle*)data;
  if (h->d && api.dec_destroy) api.dec_destroy(h->d);
  delete h;
}
DecHandle* dec_arg(napi_env env, napi_callback_info info, size_t want, napi_value* argv) {
  size_t argc = want;
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  void* p = nullptr;
  if (argc < want || napi_get_value_external(env, argv[0], &p) != napi_ok || !p || !((DecHandle*)p)->d) {
    napi_throw_type_error(env, nullptr, "expected an open decoder handle");
    return nullptr;
  }
  return (DecHandle*)p;
}
napi_value dec_create(napi_env env, napi_callback_info info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  size_t argc = 3; napi_value argv[3];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  int32_t multi = 0; double chunk = 0, out_bytes = 0;
  if (argc >= 1) napi_get_value_int32(env, argv[0], &multi);
  if (argc >= 2) napi_get_value_double(env, argv[1], &chunk);
  if (argc >= 3) napi_get_value_double(env, argv[2], &out_bytes);
  DecHandle* h = new DecHandle();
  const int rc = api.dec_create(&h->d, multi, chunk > 0 ? (size_t)chunk : 0, out_bytes > 0 ? (size_t)out_bytes : 0, nullptr);
  if (rc != 0) { delete h; return throw_code(env, rc); }
  napi_value v;
  if (napi_create_external(env, h, finalize_dec, nullptr, &v) != napi_ok) { api.dec_destroy(h->d); delete h; napi_throw_error(env, nullptr, "cannot create the decoder handle"); return nullptr; }
  return v;
}
napi_value dec_write(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  DecHandle* h = dec_arg(env, info, 2, argv);
  if (!h) return nullptr;
  const uint8_t* p = nullptr; size_t n = 0, taken = 0;
  if (!get_bytes(env, argv[1], &p, &n)) { napi_throw_type_error(env, nullptr, "expected a Uint8Array or Buffer"); return nullptr; }
  const int rc = api.dec_write(h->d, n ? p : nullptr, n, &taken);
  if (rc != 0) return throw_code(env, rc);
  napi_value v; napi_create_double(env, (double)taken, &v); return v;
}
napi_value dec_finish(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  DecHandle* h = dec_arg(env, info, 1, argv);
  if (!h) return nullptr;
  const int rc = api.dec_finish(h->d);
  if (rc != 0) return throw_code(env, rc);
  napi_value v; napi_get_undefined(env, &v); return v;
}
napi_value dec_read(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  DecHandle* h = dec_arg(env, info, 2, argv);
  if (!h) return nullptr;
  const uint8_t* p = nullptr; size_t cap = 0, got = 0;
  if (!get_bytes(env, argv[1], &p, &cap)) { napi_throw_type_error(env, nullptr, "expected a Uint8Array or Buffer to read into"); return nullptr; }
  const int rc = api.dec_read(h->d, cap ? const_cast<uint8_t*>(p) : nullptr, cap, &got);
  if (rc != 0) return throw_code(env, rc);
  napi_value v; napi_create_double(env, (double)got, &v); return v;
}
napi_value dec_done(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  DecHandle* h = dec_arg(env, info, 1, argv);
  if (!h) return nullptr;
  napi_value v; napi_get_boolean(env, api.dec_done(h->d) == 1, &v); return v;
}
napi_value dec_destroy(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  void* p = nullptr;
  if (argc >= 1 && napi_get_value_external(env, argv[0], &p) == napi_ok && p) {
    DecHandle* h = (DecHandle*)p;
    if (h->d && api.dec_destroy) api.dec_destroy(h->d);
    h->d = nullptr;
  }
  napi_value v; napi_get_undefined(env, &v); return v;
}

napi_value device_count(napi_env env, napi_callback_info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  napi_value v; napi_create_int32(env, api.device_count(), &v); return v;
}
napi_value version(napi_env env, napi_callback_info) {
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  napi_value v; napi_create_string_utf8(env, api.version(), NAPI_AUTO_LENGTH, &v); return v;
}

napi_value trim(napi_env env, napi_callback_info) {          // releases the workspace the library keeps between compress calls
  if (!load_api()) { napi_throw_error(env, nullptr, api.error.c_str()); return nullptr; }
  api.trim();
  napi_value v; napi_get_undefined(env, &v); return v;
}

napi_value init(napi_env env, napi_value exports) {
  napi_property_descriptor props[] = {
    {"bzip2Compress", nullptr, call_stream<0>, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2Decompress", nullptr, call_stream<1>, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bwtcCompress", nullptr, call_stream<2>, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bwtcDecompress", nullptr, call_stream<3>, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2CompressBatch", nullptr, bzip2_batch, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2DecompressBatch", nullptr, bzip2_decompress_batch, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2Table", nullptr, bzip2_table, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2DecompressBlock", nullptr, bzip2_block, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2Recover", nullptr, bzip2_recover, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2BuildIndex", nullptr, bzip2_build_index, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2ReadRanges", nullptr, bzip2_read_ranges, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2Search", nullptr, bzip2_search, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2SearchRegex", nullptr, bzip2_search_regex, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"regexCheck", nullptr, regex_check, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2Compare", nullptr, bzip2_compare, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2BuildLineIndex", nullptr, bzip2_build_line_index, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2LinesAsk", nullptr, bzip2_lines_ask, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2LineKeys", nullptr, bzip2_line_keys, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"lineKeysDiff", nullptr, line_keys_diff, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2Tally", nullptr, bzip2_tally, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2Sort", nullptr, bzip2_sort, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2Cut", nullptr, bzip2_cut, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2CompressIndexed", nullptr, bzip2_compress_indexed, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2EncIndex", nullptr, enc_index, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2EncCreate", nullptr, enc_create, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2EncWrite", nullptr, enc_write, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2EncFinish", nullptr, enc_finish, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2EncPending", nullptr, enc_pending, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2EncRead", nullptr, enc_read, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2EncDestroy", nullptr, enc_destroy, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2DecCreate", nullptr, dec_create, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2DecWrite", nullptr, dec_write, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2DecFinish", nullptr, dec_finish, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2DecRead", nullptr, dec_read, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2DecDone", nullptr, dec_done, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"bzip2DecDestroy", nullptr, dec_destroy, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"deviceCount", nullptr, device_count, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"version", nullptr, version, nullptr, nullptr, nullptr, napi_default, nullptr},
    {"trim", nullptr, trim, nullptr, nullptr, nullptr, napi_default, nullptr},
  };
  napi_define_properties(env, exports, sizeof(props) / sizeof(props[0]), props);
  return exports;
}

}  // namespace

NAPI_MODULE(cjs_napi, init)
