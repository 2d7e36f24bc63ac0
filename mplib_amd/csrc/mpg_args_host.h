// mpg_args_host.h -- the argument checks and launch set-up the batch entry
// points share (no HIP): each returns a reason, the entry point turns it into
// set_error.  tests/native/args_host.cpp compiles it for the CPU tests.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/mpgpu.h"
#include "mpg_ik.h"
#include "mpg_rrt.h"
#include "mpg_topp.h"

namespace mpg_args __attribute__((visibility("hidden"))) {  // nothing of it among the library's exports

inline bool mem_ok(int mem) { return mem == MPG_MEM_HOST || mem == MPG_MEM_DEVICE; }

// `count` poses of 7 doubles (p, wxyz): finite values, quaternion norm within tol of 1
enum PoseFault { POSE_OK = 0, POSE_NONFINITE, POSE_NORM };
inline PoseFault check_pose7(const double* p7, size_t count, double tol) {
  for (size_t k = 0; k < count; ++k) {
    const double* p = p7 + 7 * k;
    for (int c = 0; c < 7; ++c)
      if (!std::isfinite(p[c])) return POSE_NONFINITE;
    const double nq = std::sqrt(p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6]);
    if (!(std::fabs(nq - 1.0) <= tol)) return POSE_NORM;
  }
  return POSE_OK;
}
inline std::string pose_message(PoseFault f, const char* what) {
  if (f == POSE_NONFINITE) return std::string("non-finite ") + what;  // what: "free pose", "goal pose"
  return std::string(what) + " quaternion is not of unit norm (within 1e-6)";
}

// the free frames' columns (the last n_free links) of n link-pose rows
inline PoseFault check_free_columns(const double* rows, int64_t n, int n_links, int n_free, double tol) {
  for (int64_t i = 0; i < n && n_free; ++i)
    if (const PoseFault f = check_pose7(rows + ((size_t)i * n_links + (n_links - n_free)) * 7, (size_t)n_free, tol))
      return f;
  return POSE_OK;
}

// free_pose / free_rows of a call that takes the free poses (n: its rows -- configurations, or edges); NULL: fine
inline const char* check_free_args(const double* free_pose, int64_t free_rows, int64_t n, int n_free) {
  if (free_pose && free_rows != 1 && free_rows != n)
    return "free_rows must be 1 (shared by the batch) or n (one pose set per row)";
  if (free_pose && n_free == 0) return "the world has no free frames";
  return nullptr;
}

// r.lo / r.hi (arrays of the sampler's capacity) from lower / upper; NULL: fine
template <class Range>
const char* fill_sample_range(Range& r, const double* lower, const double* upper, int dof) {
  if (dof < 0 || dof > (int)(sizeof(r.lo) / sizeof(double))) return "dof out of range";
  for (int k = 0; k < dof; ++k) {
    if (!(std::isfinite(lower[k]) && std::isfinite(upper[k]) && lower[k] <= upper[k]))
      return "sampling range must be finite with lower <= upper";
    r.lo[k] = lower[k];
    r.hi[k] = upper[k];
  }
  return nullptr;
}

// what mpg_ik_batch and mpg_screw_batch share of an IkView, from the world's
// tables t (mpg_world::IkTables): the link's chain, the slots' kinds and
// limits, the mask (NULL: nothing frozen) and which chain joints move
template <class Tables>
void fill_ik_view(mpg::IkView& iv, const Tables& t, int link, int dof, const uint8_t* mask) {
  iv.link = link;
  iv.cs = t.chain_start[link];
  iv.cl = t.chain_len[link];
  for (int d = 0; d < dof; ++d) {
    iv.kind[d] = t.kind[d];
    iv.bounded[d] = std::isfinite(t.lo[d]) && std::isfinite(t.hi[d]);
    iv.frozen[d] = mask && mask[d] ? 1 : 0;
    iv.lo[d] = t.lo[d];
    iv.hi[d] = t.hi[d];
  }
  for (int k = 0; k < iv.cl; ++k) {
    const int src = t.joint_q_source[t.chain_joints[iv.cs + k] - 1];
    iv.move[k] = src >= 0 && !iv.frozen[src];
  }
}

// mpg_plan_batch: the options against their limits, then the planner's view
// from the dof slots' limits (lo / hi, as mpg_world::IkTables holds them) and
// the SO2 bits.  An empty string, or the reason; *unsupported: it is
// MPG_E_UNSUPPORTED's, not MPG_E_INVALID's.
inline std::string fill_rrt_view(mpg::RrtView& v, const mpg_plan_options& o, const double* lo, const double* hi, int dof,
                                 int64_t Q, int32_t G, bool* unsupported) {
  *unsupported = false;
  if (dof > mpg::kRrtDof) {
    *unsupported = true;
    return "mpg_plan_batch supports dof <= 32";
  }
  if (Q < 0) return "Q < 0";
  if (G < 1 || G > mpg::kRrtGoals) return "G outside [1, 16]";
  if (o.max_nodes < 2 || o.max_nodes > 65536) return "max_nodes outside [2, 65536]";
  if (o.max_waypoints < 2 || o.max_waypoints > 4096) return "max_waypoints outside [2, 4096]";
  if (o.max_rounds < 1) return "max_rounds < 1";
  if (o.check_every < 1) return "check_every < 1";
  if (!std::isfinite(o.range)) return "non-finite range";
  if (dof < 32 && (o.so2_mask >> dof) != 0) return "so2_mask has a bit at or above dof";
  v = mpg::RrtView{};
  v.dof = dof;
  v.goals = G;
  v.max_rounds = o.max_rounds;
  v.max_nodes = o.max_nodes;
  v.max_waypoints = o.max_waypoints;
  v.so2_mask = o.so2_mask;
  double extent = 0.0;  // CompoundStateSpace::getMaximumExtent, weights 1
  for (int d = 0; d < dof; ++d) {
    if (mpg::rrt_so2(v, d)) {
      v.lo[d] = -mpg::kRrtPi, v.hi[d] = mpg::kRrtPi;
      extent += mpg::kRrtPi;
      continue;
    }
    if (!(std::isfinite(lo[d]) && std::isfinite(hi[d]) && lo[d] <= hi[d]))
      return "dof slot " + std::to_string(d) + ": a joint with neither finite limits nor an SO2 bit cannot be planned";
    v.lo[d] = lo[d], v.hi[d] = hi[d];
    extent += hi[d] - lo[d];
  }
  if (!(extent > 0.0)) return "the state space has no extent";
  v.lvs = extent * 0.01;                               // SpaceInformation::setup
  v.range = o.range > 1e-6 ? o.range : 0.2 * extent;  // SelfConfig::configurePlannerRange
  const double segs = std::ceil(v.range / v.lvs);
  if (!(segs < 1e6)) return "range / (0.01 * extent) exceeds 10^6 validator states per motion";
  v.block = (int)segs + 2;  // goal tree: the new state, then the motion's; one more for a motion an ulp over range
  const int64_t tree_doubles = (int64_t)2 * o.max_nodes * std::max(dof, 1);
  if (Q > ((int64_t)1 << 31) / tree_doubles)
    return "Q * 2 * max_nodes * dof = " + std::to_string(Q) + " * " + std::to_string(tree_doubles) +
           " exceeds 2^31 doubles of tree storage";
  if (Q > ((int64_t)1 << 31) / std::max(v.block, 1 + G))
    return "Q * " + std::to_string(std::max(v.block, 1 + G)) + " states per round exceeds 2^31";
  return std::string();
}

// mpg_topp_batch: the options, the limits and the sizes against their bounds,
// then the call's view.  An empty string, or the reason; *unsupported as above.
inline std::string fill_topp_view(mpg::ToppView& v, const mpg_topp_options& o, int dof, int64_t rows,
                                  int32_t max_waypoints, const double* vel, const double* acc, bool* unsupported) {
  *unsupported = false;
  if (dof > mpg::kToppDof) {
    *unsupported = true;
    return "mpg_topp_batch supports dof <= 32";
  }
  if (rows < 0) return "rows < 0";
  if (!(o.step > 0) || !std::isfinite(o.step)) return "step must be > 0";
  if (o.grid_per_segment < 1 || o.grid_per_segment > 64) return "grid_per_segment outside [1, 64]";
  if (o.min_grid < 2 || o.min_grid > 65536) return "min_grid outside [2, 65536]";
  if (o.max_samples < 1 || o.max_samples > 65536) return "max_samples outside [1, 65536]";
  if (max_waypoints < 2 || max_waypoints > 4096) return "max_waypoints outside [2, 4096]";
  if (dof > 0 && (!vel || !acc)) return "vel_limits / acc_limits is NULL";
  v = mpg::ToppView{};
  v.dof = dof;
  v.max_waypoints = max_waypoints;
  v.grid_per_segment = o.grid_per_segment;
  v.min_grid = o.min_grid;
  v.max_samples = o.max_samples;
  v.ncap = std::max(o.min_grid, o.grid_per_segment * (max_waypoints - 1));
  v.step = o.step;
  for (int d = 0; d < dof; ++d) {
    if (!(std::isfinite(vel[d]) && vel[d] > 0)) return "vel_limits[" + std::to_string(d) + "] must be finite and > 0";
    if (!(std::isfinite(acc[d]) && acc[d] > 0)) return "acc_limits[" + std::to_string(d) + "] must be finite and > 0";
    v.vmax[d] = vel[d];
    v.amax[d] = acc[d];
  }
  const int64_t cap = (int64_t)1 << 31, d1 = std::max(dof, 1);
  if (rows > cap / ((int64_t)max_waypoints * d1)) return "rows * max_waypoints * dof exceeds 2^31";
  if (rows > cap / ((int64_t)o.max_samples * d1)) return "rows * max_samples * dof exceeds 2^31";
  if (rows > cap / ((int64_t)v.ncap + 1)) return "rows * (Ncap + 1) exceeds 2^31";
  return std::string();
}

// the host-memory rows of mpg_topp_batch: the counts against max_waypoints, finite values inside a row's count
inline std::string check_topp_rows(const double* path, const int32_t* n_waypoints, int64_t rows, int32_t max_waypoints,
                                   int dof) {
  for (int64_t r = 0; r < rows; ++r) {
    const int32_t n = n_waypoints[r];
    if (n > max_waypoints) return "n_waypoints[" + std::to_string(r) + "] exceeds max_waypoints";
    const double* p = path + (size_t)r * max_waypoints * dof;
    for (int64_t e = 0; e < (int64_t)std::max(n, 0) * dof; ++e)
      if (!std::isfinite(p[e])) return "non-finite path value in row " + std::to_string(r);
  }
  return std::string();
}

// dynamic LDS of ik_clik_kernel and screw_kernel (a wave per block): 64 lanes' slots and the tables of cl joints
inline size_t ik_lds_bytes(int cl) {
  const size_t c = (size_t)std::max(cl, 1);
  return sizeof(double) * (mpg::kIkSlot * 64 + mpg::IKT_DOUBLES) * c + sizeof(int) * mpg::IKT_INTS * c;
}

}  // namespace mpg_args
