// mpg_bucket.h -- index arithmetic of the survivor bucketing, shared by the
// kernels (cull tail, range_sum_kernel, range_scan_kernel, scatter_kernel),
// the host sizing in get_workspace and the host replay of
// tests/native/bucket_replay.cpp.
//
// The cull leaves one row of byte counts per 64-configuration tile:
//   cnt8[tile][W*32]  byte p = candidates of pair p in the tile (<= 64),
//                     W*8 dwords, exactly the cull wave's LDS histogram.
// Tiles are cut into ranges of kRangeTiles consecutive tiles (the unit of one
// scatter wave) and ranges into groups of kGroupRanges consecutive ranges
// (the unit of one range_sum block):
//   part[range][W*32]  u32: candidates of pair p in the group's ranges before
//                      this one (exclusive prefix inside the group)
//   grp[group][W*32]   u32: the group's candidates of pair p; range_scan turns
//                      the column into the exclusive base of the group.
// slot base of (pair p, range r) = seg_start[p] + grp[group(r)][p] + part[r][p]
#pragma once

#include "mpg_math.h"

#ifndef MPG_RANGE_TILES
#define MPG_RANGE_TILES 8
#endif

namespace mpg {

constexpr int kRangeTiles = MPG_RANGE_TILES;  // tiles per range (profiles/r07a/bucketing_ab.txt)
constexpr int kGroupRanges = 16;              // ranges per group
// range_sum_kernel keeps a group's sums as two 16-bit halves per word
static_assert(64 * kRangeTiles * kGroupRanges < 65536, "a group's count of one pair must fit 16 bits");

MPG_INLINE int bk_row_words(int W) { return W * 8; }  // dwords of a count row
MPG_INLINE int bk_cols(int W) { return W * 32; }      // pair columns of a part / grp row (and bytes of a count row)
MPG_INLINE long long bk_tiles(long long n) { return (n + 63) / 64; }
MPG_INLINE int bk_ranges(int n_tiles) { return (n_tiles + kRangeTiles - 1) / kRangeTiles; }
MPG_INLINE int bk_groups(int n_ranges) { return (n_ranges + kGroupRanges - 1) / kGroupRanges; }
// tiles [first, end) of range r
MPG_INLINE int bk_range_first(int r) { return r * kRangeTiles; }
MPG_INLINE int bk_range_end(int r, int n_tiles) {
  const int e = (r + 1) * kRangeTiles;
  return e < n_tiles ? e : n_tiles;
}
// ranges [first, end) of group g
MPG_INLINE int bk_group_first(int g) { return g * kGroupRanges; }
MPG_INLINE int bk_group_end(int g, int n_ranges) {
  const int e = (g + 1) * kGroupRanges;
  return e < n_ranges ? e : n_ranges;
}
MPG_INLINE int bk_group_of(int r) { return r / kGroupRanges; }
// (range, dword) sums one block keeps in LDS; a launch with no more of them
// in all has range_scan_kernel do the range sums itself (one launch fewer)
constexpr int kSumSlots = 4096;
MPG_INLINE bool bk_fold_sum(int n_ranges, int W) { return (long long)n_ranges * bk_row_words(W) <= kSumSlots; }
// the tile of a cull wave (block of `block` threads, thread tid) and whether
// it owns a count row: the grid is ceil(n / block) blocks, so waves past the
// last tile exist whenever n is no multiple of the block
MPG_INLINE long long bk_wave_tile(long long block_idx, int block, int tid) {
  return ((block_idx * block) >> 6) + (tid >> 6);
}
MPG_INLINE bool bk_tile_has_row(long long tile, int n_tiles) { return tile < (long long)n_tiles; }
// element counts of the buffers for a workspace of `cap` configurations
MPG_INLINE size_t bk_cnt_words(int W, long long cap) { return (size_t)bk_tiles(cap) * (size_t)bk_row_words(W); }
MPG_INLINE size_t bk_part_words(int W, long long cap) {
  return (size_t)bk_ranges((int)bk_tiles(cap)) * (size_t)bk_cols(W);
}
MPG_INLINE size_t bk_grp_words(int W, long long cap) {
  return (size_t)bk_groups(bk_ranges((int)bk_tiles(cap))) * (size_t)bk_cols(W);
}

}  // namespace mpg
