// Test shim: compiles the product's RRTConnect header
// (mplib_amd/csrc/mpg_rrt.h, the code the rrt_* kernels run) and
// mpg_plan_batch's argument checks (mpg_args_host.h) for the host with
// g++ -ffp-contract=off.  The rows advance in lockstep as on the device: one
// validity callback per round carries every row's slot block, so a test can
// answer it with the CPU oracle.  Not part of the product.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../mplib_amd/csrc/mpg_args_host.h"

extern "C" {

// flags[i] = 0 where state i is valid (the collide pass's convention)
typedef void (*rrt_valid_fn)(const double* states, long n, unsigned char* flags);

// fill_rrt_view: 0 and the derived figures, or 1 (MPG_E_INVALID) / 2
// (MPG_E_UNSUPPORTED) and the reason in msg
int rrt_host_view(const double* lo, const double* hi, int dof, long Q, int G, double range, int max_rounds,
                  int max_nodes, int max_waypoints, int check_every, unsigned so2_mask, double* range_out,
                  double* lvs_out, int* block_out, char* msg, int msg_size) {
  mpg_plan_options o{range, max_rounds, max_nodes, max_waypoints, check_every, 0, so2_mask};
  mpg::RrtView v{};
  bool unsupported = false;
  const std::string why = mpg_args::fill_rrt_view(v, o, lo, hi, dof, Q, G, &unsupported);
  if (msg && msg_size > 0) {
    std::strncpy(msg, why.c_str(), (size_t)msg_size - 1);
    msg[msg_size - 1] = 0;
  }
  if (!why.empty()) return unsupported ? 2 : 1;
  if (range_out) *range_out = v.range;
  if (lvs_out) *lvs_out = v.lvs;
  if (block_out) *block_out = v.block;
  return 0;
}

double rrt_host_sample(const double* lo, const double* hi, int dof, unsigned long long row_seed, int k, int j) {
  mpg::RrtView v{};
  v.dof = dof;
  for (int d = 0; d < dof; ++d) v.lo[d] = lo[d], v.hi[d] = hi[d];
  return mpg::rrt_sample(v, row_seed, k, j);
}

unsigned long long rrt_host_row_seed(unsigned long long seed, unsigned long long row) {
  return mpg::rrt_row_seed(seed, row);
}

// mpg_plan_batch without a device.  0, or fill_rrt_view's refusal.
int rrt_host_plan(const double* lo, const double* hi, int dof, const double* start, const double* goal, long Q, int G,
                  const unsigned long long* row_seed, double range, int max_rounds, int max_nodes, int max_waypoints,
                  unsigned long long seed, unsigned so2_mask, rrt_valid_fn valid, double* path, int* n_waypoints,
                  unsigned char* status, int* iterations, int* tree_sizes) {
  using namespace mpg;
  mpg_plan_options o{range, max_rounds, max_nodes, max_waypoints, 1, seed, so2_mask};
  RrtView v{};
  bool unsupported = false;
  if (!mpg_args::fill_rrt_view(v, o, lo, hi, dof, Q, G, &unsupported).empty()) return unsupported ? 2 : 1;
  const size_t q = (size_t)Q, tree = (size_t)2 * max_nodes, first = (size_t)(1 + G), blk = (size_t)v.block;
  std::vector<double> nodes(q * tree * dof), slots(q * std::max(first, blk) * dof), newstate(q * dof);
  std::vector<int32_t> parent(q * tree), phase(q), added(q), prop(q * RRT_P_INTS);
  std::vector<uint8_t> flags(q * std::max(first, blk));
  std::vector<uint64_t> seeds(q);
  for (size_t r = 0; r < q; ++r) {
    std::copy(start + r * dof, start + (r + 1) * dof, slots.begin() + r * first * dof);
    std::copy(goal + r * G * dof, goal + (r + 1) * G * dof, slots.begin() + (r * first + 1) * dof);
  }
  valid(slots.data(), (long)(q * first), flags.data());
  const std::vector<uint8_t> f0(flags.begin(), flags.begin() + q * first);  // the init writes the slot blocks
  long active = 0;
  for (size_t r = 0; r < q; ++r) {
    seeds[r] = row_seed ? row_seed[r] : rrt_row_seed(seed, r);
    active += rrt_init_row(v, start + r * dof, goal + r * G * dof, f0.data() + r * first, nodes.data() + r * tree * dof,
                           parent.data() + r * tree, tree_sizes + 2 * r, &phase[r], &added[r], iterations + r,
                           &prop[RRT_P_INTS * r], n_waypoints + r, status + r);
    for (long long k = 0; k < (long long)(blk + max_waypoints) * dof; ++k)
      *rrt_fill_start(v, k, slots.data() + r * blk * dof, path + r * max_waypoints * dof) = start[r * dof + k % dof];
  }
  double target[kRrtDof];
  std::vector<size_t> rows;  // the callback sees the blocks of the rows still planning (the device checks them all)
  std::vector<double> cs(slots.size());
  std::vector<uint8_t> cf(flags.size());
  for (int round = 0; round < max_rounds && active > 0; ++round) {
    rows.clear();
    for (size_t r = 0; r < q; ++r) {
      if (phase[r] == RRT_DONE) continue;
      rows.push_back(r);
      double* const nd_r = nodes.data() + r * tree * dof;
      const int t = rrt_target(v, seeds[r], phase[r], iterations + r, added[r], nd_r, target);
      const double* const tn = rrt_node(v, nd_r, t, 0);
      double bd = INFINITY;
      int bi = 0;
      rrt_nearest_scan(v, tn, tree_sizes[2 * r + t], target, 0, 1, &bd, &bi);
      const double* const near = tn + (size_t)bi * dof;
      double* const ds = newstate.data() + r * dof;
      const int nd = rrt_steer(v, t, near, bi, target, ds, &prop[RRT_P_INTS * r]);
      const int count = prop[RRT_P_INTS * r + RRT_P_COUNT];
      for (int s = 0; s < v.block; ++s)
        rrt_slot_state(v, t, near, ds, nd, s < count ? s : 0, slots.data() + (r * blk + s) * dof);
    }
    for (size_t k = 0; k < rows.size(); ++k)
      std::copy(slots.begin() + rows[k] * blk * dof, slots.begin() + (rows[k] + 1) * blk * dof, cs.begin() + k * blk * dof);
    valid(cs.data(), (long)(rows.size() * blk), cf.data());
    for (size_t k = 0; k < rows.size(); ++k)
      std::copy(cf.begin() + k * blk, cf.begin() + (k + 1) * blk, flags.begin() + rows[k] * blk);
    for (size_t r = 0; r < q; ++r)
      active -= rrt_commit(v, round, &prop[RRT_P_INTS * r], newstate.data() + r * dof, flags.data() + r * blk,
                           nodes.data() + r * tree * dof, parent.data() + r * tree, tree_sizes + 2 * r, &phase[r],
                           &added[r], status + r);
  }
  std::vector<int32_t> idx((size_t)max_waypoints);
  for (size_t r = 0; r < q; ++r)
    rrt_finish_row(v, &prop[RRT_P_INTS * r], nodes.data() + r * tree * dof, parent.data() + r * tree, idx.data(),
                   path + r * max_waypoints * dof, n_waypoints + r, status + r);
  return 0;
}

}
