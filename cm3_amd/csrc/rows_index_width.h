// Which index width a launch of the data-movement kernels of batch.hip computes in, as pure functions of the sizes the launchers
// already have.  Plain C++17, no HIP: batch.hip includes this header and calls it, tests/test_rows_index_width.py compiles it alone
// and walks it on a machine without a GPU.
// Five kernels exist in two widths: 32-bit unit arithmetic (a 64-bit division per unit costs more than the copy) whenever every value
// a lane forms in the index type I stays below 2^32, else a build with I = size_t.  "Every value" is the last unit index PLUS what a
// lane of the last workgroup adds to it before it finds out that it is past the end: the slack each rule leaves below 2^32.
//   k_rows_copy<I>, k_rows_tile<I>        grid-stride loops of `blocks` workgroups of 256 lanes: a lane forms g + stride once past the
//                                         end, stride = blocks * 256 (the row-granular path of k_rows_tile strides over ROWS, at
//                                         most as many as elements and with a smaller stride: inside the same rule; byte offsets
//                                         there are formed in size_t, once per row)
//   k_ck_transitions_gather<I>            kCkUnitsPerLane units per lane, 256 lanes apart: the last workgroup reaches up to
//                                         kCkUnitsPerLane * 256 units past the end
//   k_ck_transitions_pack<I>              byte offsets into a ring column, 16-byte pieces, kPkPiecesPerLane per lane; ring rows are
//                                         turned into transitions with row + (ring_size - ring_start) < 2 * ring_size
//   k_transitions_gather<P>               decides in the kernel (`small`): trans_index_small() is that statement, the launcher calls it
//                                         for cm3_rows_last_index_width() only
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CM3_WIDTH_HD __host__ __device__ inline
#else
#define CM3_WIDTH_HD inline
#endif

namespace cm3 {

constexpr size_t kIndex32End = (size_t)1 << 32;   // what a 32-bit index cannot hold
constexpr size_t kRowsLanes = 256;                // lanes per workgroup of every kernel here

// ---- cm3_rows_scatter / cm3_rows_gather (k_rows_copy) and cm3_rows_tile (k_rows_tile): grid-stride loops over `most` units -----------
constexpr size_t kRowsCopyMaxBlocks = 4096, kRowsTileMaxBlocks = 2048;
inline size_t rows_copy_blocks(size_t most) {
  size_t blocks = (most + 255) / 256;
  return blocks < 1 ? 1 : (blocks > kRowsCopyMaxBlocks ? kRowsCopyMaxBlocks : blocks);
}
inline size_t rows_tile_blocks(size_t most) {
  const size_t blocks = (most + 255) / 256;
  return blocks > kRowsTileMaxBlocks ? kRowsTileMaxBlocks : blocks;
}
// most: units of the largest column; blocks: workgroups along x.  One rule for both kernels.
inline bool rows_stride_index_narrow(size_t most, size_t blocks) { return most + blocks * kRowsLanes < kIndex32End; }

// ---- cm3_checkers_transitions_gather / cm3_checkers_ring_expand (k_ck_transitions_gather) -------------------------------------------
constexpr int kCkUnitsPerLane = 4;
inline bool ck_gather_index_narrow(size_t most) { return most + kCkUnitsPerLane * kRowsLanes < kIndex32End; }

// ---- cm3_checkers_transitions_pack (k_ck_transitions_pack) --------------------------------------------------------------------------
constexpr int kPkPiecesPerLane = 4;
// most: bytes of the largest ring column (ring_size rows); the slack is two 16-byte pieces per lane slot of a workgroup
inline bool ck_pack_index_narrow(size_t most, size_t ring_size) {
  return most + 32 * kPkPiecesPerLane * kRowsLanes < kIndex32End && 2 * ring_size < kIndex32End;
}

// ---- cm3_transitions_gather_f32 / cm3_transitions_route_f32 (k_transitions_gather) --------------------------------------------------
constexpr int kTransUnitsPerLane = 4;
constexpr size_t kTransMaxBlocks = 16384;
inline size_t trans_blocks_for(size_t units) {
  const size_t per_block = kTransUnitsPerLane * kRowsLanes;
  const size_t blocks = (units + per_block - 1) / per_block;
  return blocks < 1 ? 1 : (blocks > kTransMaxBlocks ? kTransMaxBlocks : blocks);
}
// total: units of the launch; stride: lanes of the grid.  Evaluated per lane in the kernel, and by the launcher for the report.
CM3_WIDTH_HD bool trans_index_small(size_t total, size_t stride) { return total + (size_t)kTransUnitsPerLane * stride < ((size_t)1 << 32); }

}  // namespace cm3
