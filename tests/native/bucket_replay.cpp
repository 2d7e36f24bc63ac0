// Test shim: the survivor bucketing's index arithmetic (mplib_amd/csrc/
// mpg_bucket.h) compiled for the host.  bucket_index_check walks the launch
// geometry of one call (cull waves, ranges, groups) against the workspace
// sizes; bucket_replay replays cull tail -> range_sum -> range_scan -> scatter
// on given survivor words, every store bounds-checked against the buffers
// get_workspace would allocate, and compares the candidate lists with
// per-pair sorted lists built directly.  The range sums and the scan are
// replayed thread by thread with the kernels' own loops (the passes over a
// count row wider than kSumCols dwords, the scan's column passes above 1024
// pair columns, the task prefix's rounds of 1024 pairs and their carries); a
// missing barrier cannot show here, an index or a carry that is wrong does.
// Not part of the product.
//
// Stand-alone (for a sanitizer run): g++ -DBUCKET_REPLAY_MAIN
//   -fsanitize=address,undefined bucket_replay.cpp && ./a.out
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../mplib_amd/csrc/mpg_bucket.h"

using namespace mpg;

namespace {

constexpr uint32_t kStale = 0xa5a5a5a5u;  // what an earlier, larger call may have left behind

#define CHECK(c) \
  do {           \
    if (!(c)) return __LINE__; \
  } while (0)

// the task list's settings of the product build (MPG_TASK_MIN, MPG_TASK,
// MPG_TAPER_C, MPG_TAPER_MIN of mpg_kernels.hip) and 4 * narrow blocks
constexpr uint32_t kTsMin = 8, kTsMax = 128, kTaperMin = 64, kTargetTasks = 3072;
constexpr double kTaperC = 0.25;

struct U2 {
  uint32_t x, y;
};

// range_sum_groups<NT> of mpg_kernels.hip: the block's NT threads run one
// after the other between its barriers.  sums is the block's LDS: kSumSlots
// entries that nothing clears, neither before the call nor between the passes
// over the row's dwords (j0), so an index that reaches into another pass's or
// another range's slot shows in the result.
int range_sum_groups(int NT, const std::vector<uint32_t>& cnt, int n_tiles, int W, std::vector<uint32_t>& part,
                     std::vector<uint32_t>& grp, int g0, int ng, std::vector<U2>& sums, int* passes) {
  const int rw = bk_row_words(W), C = bk_cols(W);
  const int n_ranges = bk_ranges(n_tiles);
  const int r0 = bk_group_first(g0), nr = bk_group_end(g0 + ng - 1, n_ranges) - r0;
  *passes = 0;
  for (int j0 = 0; j0 < rw; j0 += kSumCols) {
    ++*passes;
    const int jc = kSumCols < rw - j0 ? kSumCols : rw - j0;
    for (int tid = 0; tid < NT; ++tid)
      for (int i = tid; i < nr * jc; i += NT) {
        const int rl = i / jc, jl = i % jc;
        const int t0 = bk_range_first(r0 + rl), t1 = bk_range_end(r0 + rl, n_tiles);
        uint32_t lo = 0, hi = 0;
        for (int k = 0; k < kRangeTiles; ++k) {
          if (t0 + k >= t1) continue;
          const size_t at = (size_t)(j0 + jl) + (size_t)(t0 + k) * rw;
          CHECK(at < cnt.size());
          const uint32_t x = cnt[at];
          lo += x & 0x00ff00ffu;
          hi += (x >> 8) & 0x00ff00ffu;
        }
        CHECK(i < kSumSlots);
        sums[i] = U2{lo, hi};
      }
    // __syncthreads()
    for (int tid = 0; tid < NT; ++tid)
      for (int i = tid; i < ng * jc; i += NT) {
        const int gl = i / jc, jl = i % jc;
        const int rl1 = bk_group_end(g0 + gl, n_ranges) - r0;
        uint32_t lo = 0, hi = 0;
        for (int rl = bk_group_first(gl); rl < rl1; ++rl) {
          const size_t at = (size_t)(r0 + rl) * C + 4 * (size_t)(j0 + jl);
          CHECK(at + 4 <= part.size());
          part[at] = lo & 0xffffu, part[at + 1] = hi & 0xffffu, part[at + 2] = lo >> 16, part[at + 3] = hi >> 16;
          CHECK(rl * jc + jl < kSumSlots);
          const U2 s = sums[rl * jc + jl];
          lo += s.x;
          hi += s.y;
        }
        const size_t at = (size_t)(g0 + gl) * C + 4 * (size_t)(j0 + jl);
        CHECK(at + 4 <= grp.size());
        grp[at] = lo & 0xffffu, grp[at + 1] = hi & 0xffffu, grp[at + 2] = lo >> 16, grp[at + 3] = hi >> 16;
      }
    // __syncthreads()
  }
  return 0;
}

// wave_inclusive_scan over the 1024 values of a block, per wave of 64
void wave_scans(const uint32_t* v, uint32_t* incl, uint32_t* last16) {
  for (int wv = 0; wv < 16; ++wv) {
    uint32_t run = 0;
    for (int lane = 0; lane < 64; ++lane) incl[wv * 64 + lane] = run += v[wv * 64 + lane];
    last16[wv] = run;
  }
}

// range_scan_kernel of mpg_kernels.hip after its range sums, its 1024 threads
// one after the other between its barriers: the column scan in passes of
// min(C, 1024) columns (c0), then the segment starts and the task prefix in
// rounds of 1024 pairs (p0) with the carries cl / ct.  tail = prefix[n_pairs..]:
// the task count and the candidate count as the kernel leaves them.
int range_scan(int W, int n_groups, int n_pairs, std::vector<uint32_t>& grp, std::vector<uint32_t>& seg_len,
               std::vector<uint32_t>& seg_start, std::vector<uint32_t>& prefix, int* col_passes, int* rounds) {
  const int NT = 1024, C = bk_cols(W);
  std::vector<uint32_t> slab(NT, kStale), my_len(NT, 0u);
  const bool one = C <= 1024;
  const int CP = C < 1024 ? C : 1024, S = 1024 / CP, per = (n_groups + S - 1) / S;
  *col_passes = 0;
  for (int c0 = 0; c0 < C; c0 += CP) {
    ++*col_passes;
    for (int tid = 0; tid < NT; ++tid) {
      const int s = tid / CP, cl = tid % CP, col = c0 + cl;
      const bool act = s < S && col < C;
      const int lo = s * per, hi = act ? (n_groups < lo + per ? n_groups : lo + per) : lo;
      uint32_t sum = 0;
      for (int i = lo; i < hi; ++i) {
        const size_t at = (size_t)lo * C + col + (size_t)(i - lo) * C;
        CHECK(at < grp.size());
        sum += grp[at];
      }
      slab[tid] = sum;
    }
    // __syncthreads()
    for (int tid = 0; tid < NT; ++tid) {
      const int s = tid / CP, cl = tid % CP, col = c0 + cl;
      const bool act = s < S && col < C;
      const int lo = s * per, hi = act ? (n_groups < lo + per ? n_groups : lo + per) : lo;
      uint32_t run = 0, tot = 0;
      for (int k = 0; k < S; ++k) {
        CHECK(k * CP + cl < NT);
        const uint32_t x = slab[k * CP + cl];
        run += k < s ? x : 0u;
        tot += x;
      }
      for (int i = lo; i < hi; ++i) {
        const size_t at = (size_t)lo * C + col + (size_t)(i - lo) * C;
        const uint32_t x = grp[at];
        grp[at] = run;
        run += x;
      }
      if (act && s == 0 && col < n_pairs) {
        CHECK((size_t)col < seg_len.size());
        seg_len[col] = tot;
        my_len[tid] = tot;
      } else if (act && s == 0) {
        CHECK(tot == 0);  // no candidates in the columns past the last pair
      }
    }
    // __syncthreads(): slab is reused
  }
  uint32_t all = 0;
  for (int tid = 0; tid < NT; ++tid) {
    uint32_t psum = 0;
    if (one) psum = my_len[tid];
    else
      for (int p = tid; p < n_pairs; p += 1024) psum += seg_len[p];
    all += psum;
  }
  const TaskPlan plan = bk_task_plan(all, kTargetTasks, kTsMin, kTsMax, kTaperC, kTaperMin);
  uint32_t cl = 0, ct = 0;  // carries over rounds (the same in every thread)
  std::vector<uint32_t> len(NT), il(NT), tasks(NT), it(NT), start(NT);
  uint32_t wl[16], wt[16];
  *rounds = 0;
  for (int p0 = 0; p0 < n_pairs; p0 += 1024) {
    ++*rounds;
    for (int tid = 0; tid < NT; ++tid) {
      const int p = p0 + tid;
      len[tid] = one ? my_len[tid] : (p < n_pairs ? seg_len[p] : 0u);
    }
    wave_scans(len.data(), il.data(), wl);
    // __syncthreads()
    uint32_t cl_next = cl;
    for (int k = 0; k < 16; ++k) cl_next += wl[k];
    for (int tid = 0; tid < NT; ++tid) {
      uint32_t bl = cl;
      for (int k = 0; k < tid / 64; ++k) bl += wl[k];
      start[tid] = bl + il[tid] - len[tid];
      tasks[tid] = bk_pair_tasks(start[tid], len[tid], plan);
    }
    wave_scans(tasks.data(), it.data(), wt);
    // __syncthreads()
    for (int tid = 0; tid < NT; ++tid) {
      const int p = p0 + tid;
      uint32_t bt = ct;
      for (int k = 0; k < tid / 64; ++k) bt += wt[k];
      if (p < n_pairs) {
        seg_start[p] = start[tid];
        prefix[p] = bt + it[tid] - tasks[tid];
      }
    }
    cl = cl_next;
    for (int k = 0; k < 16; ++k) ct += wt[k];
    // __syncthreads(): wl / wt are written again in the next round
  }
  CHECK(prefix.size() >= (size_t)n_pairs + 4);
  prefix[n_pairs] = ct;
  prefix[n_pairs + 1] = 0;
  prefix[n_pairs + 2] = plan.s[0];
  prefix[n_pairs + 3] = cl;
  // against the plain sums, pair by pair
  uint32_t at = 0, tk = 0;
  for (int p = 0; p < n_pairs; ++p) {
    CHECK(seg_start[p] == at && prefix[p] == tk);
    tk += bk_pair_tasks(at, seg_len[p], plan);
    at += seg_len[p];
  }
  CHECK(cl == at && cl == all && ct == tk);
  return 0;
}

}  // namespace

extern "C" {

void bucket_consts(int* out) {
  out[0] = kRangeTiles;
  out[1] = kGroupRanges;
}

// a launch of n configurations of a world with W mask words: out = tiles,
// ranges, groups, and whether launch_collide folds the range sums into the
// scan (bk_fold_sum)
void bucket_launch_shape(long long n, int W, int* out) {
  out[0] = (int)bk_tiles(n);
  out[1] = bk_ranges(out[0]);
  out[2] = bk_groups(out[1]);
  out[3] = bk_fold_sum(out[1], W) ? 1 : 0;
}

// one launch of n <= cap configurations, cull blocks of `block` threads
int bucket_index_check(long long n, long long cap, int W, int block) {
  CHECK(n >= 1 && n <= cap && W >= 1 && block % 64 == 0);
  const int n_tiles = (int)bk_tiles(n);
  const int n_ranges = bk_ranges(n_tiles), n_groups = bk_groups(n_ranges);
  // the ranges partition the tiles, the groups partition the ranges
  int next = 0;
  for (int r = 0; r < n_ranges; ++r) {
    CHECK(bk_range_first(r) == next && bk_range_end(r, n_tiles) > next);
    CHECK(bk_range_end(r, n_tiles) - next <= kRangeTiles);
    next = bk_range_end(r, n_tiles);
  }
  CHECK(next == n_tiles);
  next = 0;
  for (int g = 0; g < n_groups; ++g) {
    CHECK(bk_group_first(g) == next && bk_group_end(g, n_ranges) > next);
    for (int r = next; r < bk_group_end(g, n_ranges); ++r) CHECK(bk_group_of(r) == g);
    next = bk_group_end(g, n_ranges);
  }
  CHECK(next == n_ranges);
  // every tile has exactly one cull wave that passes the guard, no wave past
  // the last tile does, and every row lies inside cnt
  const long long grid = (n + block - 1) / block;
  std::vector<int> owner(n_tiles, 0);
  for (long long b = 0; b < grid; ++b)
    for (int tid = 0; tid < block; tid += 64) {
      const long long tile = bk_wave_tile(b, block, tid);
      CHECK(tile == (b * block + tid) / 64);
      if (!bk_tile_has_row(tile, n_tiles)) {
        CHECK(b * block + tid >= n);  // such a wave has no live lane
        continue;
      }
      CHECK(tile >= 0 && tile < n_tiles);
      ++owner[tile];
      CHECK((size_t)(tile + 1) * bk_row_words(W) <= bk_cnt_words(W, cap));
    }
  for (int t = 0; t < n_tiles; ++t) CHECK(owner[t] == 1);
  CHECK((size_t)n_ranges * bk_cols(W) <= bk_part_words(W, cap));
  CHECK((size_t)n_groups * bk_cols(W) <= bk_grp_words(W, cap));
  CHECK(bk_cols(W) == 4 * bk_row_words(W));
  return 0;
}

// surv: [W][cap] survivor words (bit b of word wd of configuration c: pair
// 32 wd + b survives), rows >= n ignored.  Returns 0 or the failing line.
// paths (may be NULL): the branches the launch took -- range sums folded into
// the scan (1) or not (0), passes over the count row's dwords, column passes
// of the scan, rounds of the task prefix, groups.
int bucket_replay(int W, int n_pairs, long long n, long long cap, int block, const uint32_t* surv,
                  long long* n_cand, int* paths) {
  CHECK(n >= 1 && n <= cap && n_pairs <= 32 * W);
  const int rw = bk_row_words(W), C = bk_cols(W);
  const int n_tiles = (int)bk_tiles(n), n_ranges = bk_ranges(n_tiles), n_groups = bk_groups(n_ranges);
  std::vector<uint32_t> cnt(bk_cnt_words(W, cap), kStale), part(bk_part_words(W, cap), kStale),
      grp(bk_grp_words(W, cap), kStale);
  const uint8_t* c8 = reinterpret_cast<const uint8_t*>(cnt.data());
  // cull tail: each wave's histogram is its tile's row
  const long long grid = (n + block - 1) / block;
  for (long long b = 0; b < grid; ++b)
    for (int tid = 0; tid < block; tid += 64) {
      const long long tile = bk_wave_tile(b, block, tid);
      if (!bk_tile_has_row(tile, n_tiles)) continue;
      std::vector<uint32_t> hist(rw, 0u);
      for (int lane = 0; lane < 64; ++lane) {
        const long long cfg = b * block + tid + lane;
        if (cfg >= n) continue;
        for (int k = 0; k < W; ++k)
          for (uint32_t x = surv[(long long)k * cap + cfg]; x; x &= x - 1u) {
            const int p = k * 32 + __builtin_ctz(x);
            hist[p >> 2] += 1u << (8 * (p & 3));
          }
      }
      for (int i = 0; i < rw; ++i) {
        CHECK((size_t)(tile * rw + i) < cnt.size());
        cnt[tile * rw + i] = hist[i];
      }
    }
  // the range sums as launch_collide runs them: by range_scan_kernel's one
  // block of 1024 threads for every group (bk_fold_sum), or by
  // range_sum_kernel, one block of 256 threads per group
  const bool fold = bk_fold_sum(n_ranges, W);
  int sum_passes = 0, col_passes = 0, rounds = 0;
  {
    std::vector<U2> sums(kSumSlots, U2{kStale, kStale});
    if (fold) {
      const int rc = range_sum_groups(1024, cnt, n_tiles, W, part, grp, 0, n_groups, sums, &sum_passes);
      if (rc) return rc;
    } else {
      for (int g = 0; g < n_groups; ++g) {
        const int rc = range_sum_groups(256, cnt, n_tiles, W, part, grp, g, 1, sums, &sum_passes);
        if (rc) return rc;
      }
    }
  }
  // every part and grp entry of the launch has been written (nothing stale
  // of an earlier call is left where the scatter reads), and holds what the
  // count bytes say
  for (int p = 0; p < C; ++p)
    for (int g = 0; g < n_groups; ++g) {
      uint32_t in_group = 0;
      for (int r = bk_group_first(g); r < bk_group_end(g, n_ranges); ++r) {
        CHECK(part[(size_t)r * C + p] == in_group);
        for (int t = bk_range_first(r); t < bk_range_end(r, n_tiles); ++t) in_group += c8[(size_t)t * C + p];
      }
      CHECK(grp[(size_t)g * C + p] == in_group);
    }
  // range_scan_kernel: group totals -> group bases, seg_len, seg_start, task prefix
  std::vector<uint32_t> seg_len(n_pairs > 0 ? n_pairs : 1, kStale), seg_start(seg_len.size(), kStale),
      prefix((size_t)(n_pairs > 0 ? n_pairs : 1) + kPrefixTail, kStale);
  {
    const int rc = range_scan(W, n_groups, n_pairs, grp, seg_len, seg_start, prefix, &col_passes, &rounds);
    if (rc) return rc;
  }
  const uint32_t total = prefix[n_pairs + 3];
  *n_cand = total;
  if (paths) {
    paths[0] = fold ? 1 : 0;
    paths[1] = sum_passes;
    paths[2] = col_passes;
    paths[3] = rounds;
    paths[4] = n_groups;
  }
  // scatter_kernel: one wave per (word, tile); the slot bases of a tile are
  // the range's plus the counts of the range's tiles before it
  std::vector<uint32_t> cand((size_t)total, kStale);
  std::vector<char> written((size_t)total, 0);
  for (int r = 0; r < n_ranges; ++r)
    for (int wd = 0; wd < W; ++wd) {
      uint32_t run[32];
      for (int b = 0; b < 32; ++b) {
        const int p = wd * 32 + b;
        run[b] = p < n_pairs ? seg_start[p] + grp[(size_t)bk_group_of(r) * C + p] + part[(size_t)r * C + p] : 0u;
      }
      for (int t = bk_range_first(r); t < bk_range_end(r, n_tiles); ++t)
        for (int b = 0; b < 32; ++b) {
          const uint32_t c = c8[(size_t)t * C + wd * 32 + b];
          uint32_t pre = 0;
          for (int k = 0; k < kRangeTiles - 1; ++k)
            if (bk_range_first(r) + k < t) pre += c8[(size_t)(bk_range_first(r) + k) * C + wd * 32 + b];
          if (wd * 32 + b < n_pairs)
            CHECK(run[b] == seg_start[wd * 32 + b] + grp[(size_t)bk_group_of(r) * C + wd * 32 + b] +
                                part[(size_t)r * C + wd * 32 + b] + pre);
          if (c == 0) continue;
          uint32_t rank = 0;
          for (int lane = 0; lane < 64; ++lane) {
            const long long cfg = (long long)t * 64 + lane;
            if (cfg >= n || !((surv[(long long)wd * cap + cfg] >> b) & 1u)) continue;
            const size_t at = (size_t)run[b] + rank++;
            CHECK(wd * 32 + b < n_pairs && at < cand.size() && !written[at]);
            cand[at] = (uint32_t)cfg;
            written[at] = 1;
          }
          CHECK(rank == c);
          run[b] += c;
        }
    }
  // against the lists built directly: per pair, configurations in order
  size_t at = 0;
  for (int p = 0; p < n_pairs; ++p) {
    CHECK(seg_start[p] == at);
    for (long long cfg = 0; cfg < n; ++cfg)
      if ((surv[(long long)(p >> 5) * cap + cfg] >> (p & 31)) & 1u) {
        CHECK(at < cand.size() && written[at] && cand[at] == (uint32_t)cfg);
        ++at;
      }
    CHECK(at == (size_t)seg_start[p] + seg_len[p]);
  }
  CHECK(at == cand.size());
  return 0;
}

}  // extern "C"

#ifdef BUCKET_REPLAY_MAIN
int main() {
  uint64_t s = 0x9e3779b97f4a7c15ull;
  auto rnd = [&]() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return (uint32_t)(s >> 32);
  };
  const int R = 64 * kRangeTiles;
  const long long sizes[] = {1, 63, 64, 65, 255, 256, 257, R - 1, R, R + 1, 3 * R + 17, 64LL * R + 5, 20000};
  int bad = 0;
  for (int W : {1, 5, 18, 35, 65, 70})
    for (int block : {64, 128, 256})
      for (long long n : sizes) {
        const long long cap = n + (rnd() % 3) * 1000;
        const int n_pairs = 32 * W - (int)(rnd() % 31);
        std::vector<uint32_t> surv((size_t)W * cap);
        for (auto& x : surv) x = rnd() & rnd() & rnd() & rnd();  // about two survivors per word
        for (int p = n_pairs; p < 32 * W; ++p)
          for (long long c = 0; c < cap; ++c) surv[(size_t)(p >> 5) * cap + c] &= ~(1u << (p & 31));
        long long nc = 0;
        int rc = bucket_index_check(n, cap, W, block);
        if (!rc) rc = bucket_replay(W, n_pairs, n, cap, block, surv.data(), &nc, nullptr);
        if (rc) {
          std::printf("W %d block %d n %lld cap %lld: failed at line %d\n", W, block, n, cap, rc);
          ++bad;
        }
      }
  std::printf("%s\n", bad ? "FAILED" : "bucket replay ok");
  return bad != 0;
}
#endif
