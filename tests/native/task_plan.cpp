// Test shim: the narrow phase's task list (mplib_amd/csrc/mpg_bucket.h:
// bk_task_plan, bk_pair_tasks, bk_task_range) compiled for the host.
// task_plan_check replays range_scan_kernel's per-pair loop on given segment
// lengths and walks every task the way narrow_kernel, closed_form_kernel and
// contact_kernel do (binary search of the pair, then the task's range).  All
// sums are carried in 64 bits next to the kernels' 32-bit ones, so a 32-bit
// overflow shows as a mismatch.  Not part of the product.
//
// Stand-alone (for a sanitizer run): g++ -DTASK_PLAN_MAIN
//   -fsanitize=address,undefined task_plan.cpp && ./a.out
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../mplib_amd/csrc/mpg_bucket.h"

using namespace mpg;

namespace {

#define CHECK(c) \
  do {           \
    if (!(c)) return __LINE__; \
  } while (0)

// task_pair of mpg_kernels.hip: prefix[p] <= tk < prefix[p + 1]
int task_pair(const uint32_t* prefix, int n_pairs, uint32_t tk) {
  int lo = 0, hi = n_pairs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= tk) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace

extern "C" {

void task_plan_consts(int* out) { out[0] = kTaperLevels; }

// the plan of a launch: out = n, g[kTaperLevels], s[kTaperLevels]
void task_plan_fill(uint32_t all, uint32_t target_tasks, uint32_t ts_min, uint32_t ts_max, double c, uint32_t s_min,
                    uint32_t* out) {
  bk_plan_store(bk_task_plan(all, target_tasks, ts_min, ts_max, c, s_min), out);
}

// 0, or the line of the first failed check.  seg_len: candidates per pair;
// n_levels / n_tasks (may be NULL): the plan's levels and the task count.
int task_plan_check(const uint32_t* seg_len, int n_pairs, uint32_t target_tasks, uint32_t ts_min, uint32_t ts_max,
                    double c, uint32_t s_min, int* n_levels, long long* n_tasks) {
  CHECK(n_pairs >= 1 && ts_min >= 1 && ts_min <= ts_max);
  unsigned long long all64 = 0;
  for (int p = 0; p < n_pairs; ++p) all64 += seg_len[p];
  CHECK(all64 < 0xffffffffull - 2ull * ts_max);  // the kernels' 32-bit sums
  const uint32_t all = (uint32_t)all64;
  const TaskPlan pl = bk_task_plan(all, target_tasks, ts_min, ts_max, c, s_min);
  if (n_levels) *n_levels = (int)pl.n;
  // the plan itself
  CHECK(pl.n >= 1 && pl.n <= (uint32_t)kTaperLevels && pl.g[0] == 0);
  CHECK(pl.s[0] == bk_task_size(all, target_tasks, ts_min, ts_max));
  CHECK(pl.s[0] >= ts_min && pl.s[0] <= ((ts_max + 7u) & ~7u) && pl.s[0] % 8 == 0);
  const uint32_t lowest = s_min > ts_min ? s_min : ts_min;
  for (uint32_t l = 1; l < (uint32_t)kTaperLevels; ++l) {
    if (l < pl.n) {
      CHECK(pl.g[l] >= pl.g[l - 1] && pl.g[l] <= all);
      CHECK(pl.s[l] == pl.s[l - 1] / 2 && pl.s[l] >= lowest && pl.s[l] >= 1);
    } else {
      CHECK(pl.g[l] == kPlanEnd);
    }
  }
  // launches that do not hit the upper clamp keep one level
  if (!target_tasks || all64 <= (unsigned long long)target_tasks * ts_max) CHECK(pl.n == 1);
  // the stored words read back as the same plan
  uint32_t words[kPlanWords];
  bk_plan_store(pl, words);
  const TaskPlan rd = bk_plan_load(words);
  CHECK(rd.n == pl.n);
  for (int l = 0; l < kTaperLevels; ++l) CHECK(rd.g[l] == pl.g[l] && rd.s[l] == pl.s[l]);

  // range_scan_kernel's loop: segment starts and the task prefix
  std::vector<uint32_t> seg_start(n_pairs), prefix(n_pairs + 1);
  uint32_t cl = 0, ct = 0;
  unsigned long long cl64 = 0, ct64 = 0;
  for (int p = 0; p < n_pairs; ++p) {
    seg_start[p] = cl;
    prefix[p] = ct;
    const uint32_t tasks = bk_pair_tasks(cl, seg_len[p], pl);
    // level by level in 64 bits
    unsigned long long want = 0;
    const unsigned long long s0 = cl64, e0 = cl64 + seg_len[p];
    for (uint32_t l = 0; l < pl.n; ++l) {
      const unsigned long long gl = pl.g[l], gn = l + 1 < pl.n ? pl.g[l + 1] : ~0ull;
      const unsigned long long lo = s0 > gl ? s0 : gl, hi = e0 < gn ? e0 : gn;
      if (hi > lo) want += (hi - lo + pl.s[l] - 1) / pl.s[l];
    }
    CHECK(tasks == want);
    CHECK((seg_len[p] == 0) == (tasks == 0));
    cl += seg_len[p];
    ct += tasks;
    cl64 += seg_len[p];
    ct64 += tasks;
    CHECK(cl == cl64 && ct == ct64);
  }
  prefix[n_pairs] = ct;
  if (n_tasks) *n_tasks = (long long)ct64;
  CHECK(ct64 >= (all64 + pl.s[0] - 1) / pl.s[0]);
  // one level: the plain list
  if (pl.n == 1)
    for (int p = 0; p < n_pairs; ++p) CHECK(prefix[p + 1] - prefix[p] == (seg_len[p] + pl.s[0] - 1) / pl.s[0]);

  // every task, as the narrow kernels take it
  int pair = -1;          // pair of the previous task
  uint32_t covered = 0;   // end of the previous task inside its pair
  for (uint32_t tk = 0; tk < ct; ++tk) {
    const int p = task_pair(prefix.data(), n_pairs, tk);
    CHECK(p >= 0 && p < n_pairs && prefix[p] <= tk && tk < prefix[p + 1]);
    if (p != pair) {  // the pair before is complete, pairs without candidates have no task
      if (pair >= 0) CHECK(covered == seg_len[pair]);
      for (int q = pair + 1; q < p; ++q) CHECK(seg_len[q] == 0);
      pair = p;
      covered = 0;
    }
    const uint32_t k = tk - prefix[p];
    uint32_t t0 = 0, t1 = 0;
    bk_task_range(seg_start[p], seg_len[p], k, pl, &t0, &t1);
    CHECK(t0 == covered && t1 > t0 && t1 <= seg_len[p]);  // in order, none empty
    // the level that holds the task's first candidate bounds its size, and
    // the task does not reach into the next level
    const unsigned long long g0 = (unsigned long long)seg_start[p] + t0, g1 = (unsigned long long)seg_start[p] + t1;
    uint32_t l = 0;
    while (l + 1 < pl.n && g0 >= pl.g[l + 1]) ++l;
    CHECK(t1 - t0 <= pl.s[l]);
    if (l + 1 < pl.n) CHECK(g1 <= pl.g[l + 1]);
    if (pl.n == 1) {  // the formula before the plan
      const unsigned long long b = (unsigned long long)k * pl.s[0], e = b + pl.s[0];
      CHECK(t0 == b && t1 == (e < seg_len[p] ? e : seg_len[p]));
    }
    covered = t1;
  }
  if (pair >= 0) CHECK(covered == seg_len[pair]);
  for (int q = pair + 1; q < n_pairs; ++q) CHECK(seg_len[q] == 0);
  // past a pair's tasks: empty
  for (int p = 0; p < n_pairs && p < 64; ++p) {
    uint32_t t0 = 0, t1 = 1;
    bk_task_range(seg_start[p], seg_len[p], prefix[p + 1] - prefix[p], pl, &t0, &t1);
    CHECK(t0 >= t1);
  }
  return 0;
}

}  // extern "C"

#ifdef TASK_PLAN_MAIN
namespace {
uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd(uint32_t n) {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) % n);
}
}  // namespace

int main() {
  int bad = 0;
  for (int round = 0; round < 200; ++round) {
    const int n_pairs = 1 + (int)rnd(160);
    const uint32_t target = round % 7 == 0 ? 0u : 1u + rnd(round % 2 ? 16u : 3072u);
    const uint32_t big = round % 5 == 0 ? 1u << 20 : 400u;
    std::vector<uint32_t> len(n_pairs);
    for (auto& v : len) v = rnd(4) == 0 ? 0u : rnd(big);
    int levels = 0;
    long long tasks = 0;
    const int rc = task_plan_check(len.data(), n_pairs, target, 8, 128, round % 3 ? 0.5 : 0.25, round % 3 ? 16 : 64, &levels, &tasks);
    if (rc) {
      std::printf("task_plan.cpp:%d (round %d, pairs %d, target %u)\n", rc, round, n_pairs, target);
      bad = 1;
    }
  }
  {  // the largest launch: 2^20 configurations of 160 pairs, every pair a candidate
    std::vector<uint32_t> len(160, 1u << 20);
    const int rc = task_plan_check(len.data(), 160, 3072, 8, 128, 0.5, 16, nullptr, nullptr);
    if (rc) {
      std::printf("task_plan.cpp:%d (full launch)\n", rc);
      bad = 1;
    }
  }
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
#endif
