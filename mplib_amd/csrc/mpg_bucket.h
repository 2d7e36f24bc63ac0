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
constexpr int kSumCols = 256;  // count-row dwords summed at a time: wider rows (W > 32) take several passes
static_assert(kGroupRanges * kSumCols <= kSumSlots, "a group's sums must fit the block's LDS");
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

// ---------------------------------------------------------------------------
// Narrow-phase task list.  The candidates of all pairs, laid end to end in
// seg_start order, are cut into tasks of one pair each.  A TaskPlan gives the
// task size by global candidate offset: from g[l] on (up to g[l + 1]) tasks
// hold s[l] candidates.  One level is the plain list (tasks of ts candidates);
// further levels halve the size towards the end of the list, so the persistent
// waves of the narrow kernels run out of work at nearly the same time instead
// of each finishing a full-size task after the queue has emptied (guided
// self-scheduling: the size at offset g follows (all - g) / (c * target)).
// range_scan_kernel fills the plan and keeps it behind the task prefix;
// narrow_kernel, closed_form_kernel and contact_kernel read their ranges from
// it, tests/native/task_plan.cpp replays both on the host.
// ---------------------------------------------------------------------------
constexpr int kTaperLevels = 4;
constexpr uint32_t kPlanEnd = 0xffffffffu;  // start of a level that is not in use
struct TaskPlan {
  uint32_t n;                // levels in use, >= 1
  uint32_t g[kTaperLevels];  // g[0] = 0, ascending; kPlanEnd past the levels in use
  uint32_t s[kTaperLevels];  // s[0] = ts, each further one half the one before
};
// words of a plan behind prefix[n_pairs + 3]
constexpr int kPlanWords = 1 + 2 * kTaperLevels;
constexpr int kPrefixTail = 4 + kPlanWords;  // task count, task counter, ts, candidates, plan

// the launch's task size: all / target tasks within [ts_min, ts_max], a multiple of 8
MPG_INLINE uint32_t bk_task_size(uint32_t all, uint32_t target_tasks, uint32_t ts_min, uint32_t ts_max) {
  uint32_t ts = target_tasks ? (uint32_t)(((unsigned long long)all + target_tasks - 1) / target_tasks) : ts_max;
  ts = ts < ts_min ? ts_min : (ts > ts_max ? ts_max : ts);
  return (ts + 7u) & ~7u;
}

// Levels beyond the first only where the clamp to ts_max was hit (all >
// target_tasks * ts_max): level l >= 1 starts where c * target_tasks *
// s[l - 1] candidates remain, with s[l] = s[l - 1] / 2 not below max(s_min,
// ts_min).  Every smaller launch keeps one level.
MPG_INLINE TaskPlan bk_task_plan(uint32_t all, uint32_t target_tasks, uint32_t ts_min, uint32_t ts_max, double c,
                                 uint32_t s_min) {
  TaskPlan pl;
  pl.n = 1;
  pl.g[0] = 0;
  pl.s[0] = bk_task_size(all, target_tasks, ts_min, ts_max);
  const uint32_t lowest = s_min > ts_min ? s_min : ts_min;
  bool on = target_tasks && (unsigned long long)all > (unsigned long long)target_tasks * ts_max;
#pragma unroll
  for (int l = 1; l < kTaperLevels; ++l) {  // (no break, constant indices: the plan stays in registers)
    const uint32_t half = pl.s[l - 1] / 2;
    on = on && half >= lowest && half != 0;
    const double rem = c * (double)target_tasks * (double)pl.s[l - 1];  // candidates left where the level starts
    const uint32_t g = rem < (double)all ? all - (uint32_t)rem : 0u;
    pl.g[l] = !on ? kPlanEnd : (g > pl.g[l - 1] ? g : pl.g[l - 1]);
    pl.s[l] = on ? half : pl.s[l - 1];
    if (on) pl.n = (uint32_t)l + 1;
  }
  return pl;
}

MPG_INLINE void bk_plan_store(const TaskPlan& pl, uint32_t* words) {
  words[0] = pl.n;
#pragma unroll
  for (int l = 0; l < kTaperLevels; ++l) {
    words[1 + l] = pl.g[l];
    words[1 + kTaperLevels + l] = pl.s[l];
  }
}
MPG_INLINE TaskPlan bk_plan_load(const uint32_t* words) {
  TaskPlan pl;
  pl.n = words[0];
#pragma unroll
  for (int l = 0; l < kTaperLevels; ++l) {
    pl.g[l] = words[1 + l];
    pl.s[l] = words[1 + kTaperLevels + l];
  }
  return pl;
}

// level l's part [lo, hi) of the pair at global offsets [start, start + len): empty when hi <= lo
MPG_INLINE void bk_level_span(uint32_t start, uint32_t len, const TaskPlan& pl, int l, uint32_t* lo, uint32_t* hi) {
  const uint32_t end = start + len;
  const uint32_t next = l + 1 < kTaperLevels ? pl.g[l + 1] : kPlanEnd;
  *lo = start > pl.g[l] ? start : pl.g[l];
  *hi = end < next ? end : next;
}

// tasks of the pair at [start, start + len): each level's part of the pair
// is cut from its beginning into tasks of s[l] candidates (the last one short)
MPG_INLINE uint32_t bk_pair_tasks(uint32_t start, uint32_t len, const TaskPlan& pl) {
  uint32_t tasks = 0;
#pragma unroll
  for (int l = 0; l < kTaperLevels; ++l) {
    uint32_t lo, hi;
    bk_level_span(start, len, pl, l, &lo, &hi);
    if (hi > lo) tasks += (hi - lo + pl.s[l] - 1) / pl.s[l];
  }
  return tasks;
}

// candidates [t0, t1) of the pair's k-th task, local to the pair (k <
// bk_pair_tasks); one level: (k * ts, min(len, k * ts + ts))
MPG_INLINE void bk_task_range(uint32_t start, uint32_t len, uint32_t k, const TaskPlan& pl, uint32_t* t0,
                              uint32_t* t1) {
  *t0 = *t1 = len;  // k past the pair's tasks: empty
#pragma unroll
  for (int l = 0; l < kTaperLevels; ++l) {
    uint32_t lo, hi;
    bk_level_span(start, len, pl, l, &lo, &hi);
    if (hi <= lo) continue;
    const uint32_t nt = (hi - lo + pl.s[l] - 1) / pl.s[l];
    if (k < nt) {
      const uint32_t b = lo - start + k * pl.s[l], e = hi - start;
      *t0 = b;
      *t1 = e - b < pl.s[l] ? e : b + pl.s[l];
      return;
    }
    k -= nt;
  }
}

}  // namespace mpg
