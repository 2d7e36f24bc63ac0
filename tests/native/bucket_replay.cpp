// Test shim: the survivor bucketing's index arithmetic (mplib_amd/csrc/
// mpg_bucket.h) compiled for the host.  bucket_index_check walks the launch
// geometry of one call (cull waves, ranges, groups) against the workspace
// sizes; bucket_replay replays cull tail -> range_sum -> range_scan -> scatter
// on given survivor words, every store bounds-checked against the buffers
// get_workspace would allocate, and compares the candidate lists with
// per-pair sorted lists built directly.  Not part of the product.
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

}  // namespace

extern "C" {

void bucket_consts(int* out) {
  out[0] = kRangeTiles;
  out[1] = kGroupRanges;
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
int bucket_replay(int W, int n_pairs, long long n, long long cap, int block, const uint32_t* surv,
                  long long* n_cand) {
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
  // range_sum_kernel: one block per group, one dword (four pairs) per lane
  for (int g = 0; g < n_groups; ++g) {
    const int r0 = bk_group_first(g), nr = bk_group_end(g, n_ranges) - r0;
    for (int j = 0; j < rw; ++j) {
      uint32_t plo = 0, phi = 0;
      for (int rl = 0; rl < nr; ++rl) {
        const int t0 = bk_range_first(r0 + rl), t1 = bk_range_end(r0 + rl, n_tiles);
        uint32_t lo = 0, hi = 0;
        for (int k = 0; k < kRangeTiles; ++k) {
          if (t0 + k >= t1) continue;
          CHECK((size_t)((long long)(t0 + k) * rw + j) < cnt.size());
          const uint32_t x = cnt[(long long)(t0 + k) * rw + j];
          lo += x & 0x00ff00ffu;
          hi += (x >> 8) & 0x00ff00ffu;
        }
        const size_t at = (size_t)(r0 + rl) * C + 4 * j;
        CHECK(at + 4 <= part.size());
        part[at] = plo & 0xffffu, part[at + 1] = phi & 0xffffu, part[at + 2] = plo >> 16, part[at + 3] = phi >> 16;
        plo += lo, phi += hi;
      }
      const size_t at = (size_t)g * C + 4 * j;
      CHECK(at + 4 <= grp.size());
      grp[at] = plo & 0xffffu, grp[at + 1] = phi & 0xffffu, grp[at + 2] = plo >> 16, grp[at + 3] = phi >> 16;
    }
  }
  // range_scan_kernel: group totals -> group bases, seg_len, seg_start
  std::vector<uint32_t> seg_len(n_pairs > 0 ? n_pairs : 1, 0u), seg_start(seg_len.size(), 0u);
  for (int col = 0; col < C; ++col) {
    uint32_t run = 0;
    for (int g = 0; g < n_groups; ++g) {
      const uint32_t x = grp[(size_t)g * C + col];
      grp[(size_t)g * C + col] = run;
      run += x;
    }
    if (col < n_pairs) seg_len[col] = run;
    else CHECK(run == 0);
  }
  uint32_t total = 0;
  for (int p = 0; p < n_pairs; ++p) {
    seg_start[p] = total;
    total += seg_len[p];
  }
  *n_cand = total;
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
  for (int W : {1, 5, 18})
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
        if (!rc) rc = bucket_replay(W, n_pairs, n, cap, block, surv.data(), &nc);
        if (rc) {
          std::printf("W %d block %d n %lld cap %lld: failed at line %d\n", W, block, n, cap, rc);
          ++bad;
        }
      }
  std::printf("%s\n", bad ? "FAILED" : "bucket replay ok");
  return bad != 0;
}
#endif
