// enc_pieces.h -- host arithmetic of the compress pipeline's pieces (pipeline.hip, blocks_through_tables): into how
// many runs the blocks of a call go, so that MTF / RLE2 and the Huffman tables of one run overlap the suffix sort of the next.
// Plain integers.  No HIP in here (tests/host/enc_pieces_check.cc compiles it with the host compiler).
#pragma once
#include <stdint.h>

namespace cjs {

constexpr uint64_t ENC_PIECE_BYTES = 400000000ull;      // bytes of blocks (cnt * cap) from which a call goes in pieces
constexpr uint32_t ENC_PIECES = 4;

// pieces: into how many runs the blocks are cut; per: the blocks of a run = ceil(cnt / pieces).  The runs that hold a block
// number table_piece_count() <= pieces: 5 blocks in 4 pieces are runs of 2, 2 and 1.
struct TablePieces { uint32_t pieces, per; };

// One piece when the call measures its stages (the stage timers run on one stream), when the context has no tail stream, or
// when its blocks hold fewer than min_bytes bytes (every piece pays the sort's launches again); else ENC_PIECES.
inline TablePieces table_pieces(uint32_t cnt, uint32_t cap, uint64_t min_bytes, bool stage_times, bool has_tail) {
  const uint32_t pieces = (stage_times || !has_tail || (uint64_t)cnt * cap < min_bytes) ? 1u : ENC_PIECES;
  return TablePieces{pieces, (uint32_t)(((uint64_t)cnt + pieces - 1) / pieces)};
}

// the runs of `cnt` blocks that hold a block: ceil(cnt / per); none for no block
inline uint32_t table_piece_count(uint32_t cnt, const TablePieces& p) {
  return p.per ? (uint32_t)(((uint64_t)cnt + p.per - 1) / p.per) : 0u;
}

// run i < table_piece_count(): blocks [k0, k0 + kc) of the call, kc >= 1; only the last run may hold fewer than `per`
inline void table_piece(uint32_t cnt, const TablePieces& p, uint32_t i, uint32_t& k0, uint32_t& kc) {
  const uint64_t at = (uint64_t)i * p.per;
  k0 = (uint32_t)at;
  kc = (uint32_t)(cnt - at < p.per ? cnt - at : p.per);
}

}  // namespace cjs
