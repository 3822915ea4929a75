// huff.hip — the entropy stage's workspace: the sub-buffers of huff_layout (huff_rules.h), carved in its order.
#include "cjs_internal.h"
#include "huff.h"

namespace cjs {

size_t HuffWork::bytes_needed(size_t max_blocks, uint32_t stride) {
  return huff_layout_bytes(huff_layout(max_blocks, stride));
}
// sub-buffer I of the layout; false when the arena is too small for it
template <HuffBuf I, typename T>
static bool take_buf(Arena& a, const HuffLayout& L, T*& p) {
  static_assert(sizeof(T) == HUFF_ELEM_BYTES[I], "huff_layout counts elements of this size");
  return (p = a.take<T>(L.n[I])) != nullptr;
}
int HuffWork::carve(Arena& a, size_t max_blocks_, uint32_t stride) {
  max_blocks = max_blocks_;
  max_stride = stride;
  const HuffLayout L = huff_layout(max_blocks, stride);
  b.sel_stride = L.sel_stride; b.tile_stride = L.tile_stride;
  bool ok = take_buf<HB_SEL>(a, L, b.sel);
  ok &= take_buf<HB_SELJ>(a, L, b.selj); ok &= take_buf<HB_BCOST>(a, L, b.bcost);
  ok &= take_buf<HB_LENS>(a, L, b.lens); ok &= take_buf<HB_CODES>(a, L, b.codes);
  ok &= take_buf<HB_NGROUPS>(a, L, b.ngroups); ok &= take_buf<HB_BITLEN>(a, L, b.bitlen); ok &= take_buf<HB_BITOFF>(a, L, b.bitoff);
  ok &= take_buf<HB_SCALARS>(a, L, scalars);
  ok &= take_buf<HB_DATABITS>(a, L, b.databits); ok &= take_buf<HB_TILEOFF>(a, L, b.tileoff);
  ok &= take_buf<HB_WL>(a, L, b.wl); ok &= take_buf<HB_WFREQ>(a, L, b.wfreq);
  return ok ? 0 : CJS_E_OUT_OF_MEMORY;
}

}  // namespace cjs
