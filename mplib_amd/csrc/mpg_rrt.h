// mpg_rrt.h -- RRTConnect of one (start, goals) row, one growTree call at a
// time, shared by rrt_init_kernel / rrt_propose_kernel / rrt_commit_kernel
// (mpg_kernels.hip) and the host-side test (tests/test_rrt_host.py compiles
// this header with g++ -ffp-contract=off).
//
//   RRTConnect::solve / growTree   [ext OMPL 1.6.0] as csrc/host/planner.cpp restates them in its
//                                  serial loop (set_speculative_connect(False))
//   PlanSpace::distance, interpolate, equal, valid_segment_count, satisfies_bounds   csrc/host/planner.cpp
//
// The arithmetic is a + (b - a) * t, sums of |diff| in dimension order, one
// division per motion, ceil and comparisons: no library call whose result
// could differ between host and device, so the two agree bit for bit.
//
// A row is a small machine.  EXTEND starts an iteration: the iteration's
// sample, one growTree on the iteration's tree (even iterations the start
// tree, odd ones the goal tree).  CONNECT grows the other tree towards the
// state the extension added, once per round, while growTree answers ADVANCED.
// A round is: target and nearest node, the steered state and the states the
// motion validator looks at (rrt_steer, rrt_slot_state) -- the collide pass
// over those states -- rrt_commit.  The path of a row that connected is
// written once, after the last round (rrt_path_indices, rrt_path_slot): the
// walk up the two parent chains is a chain of dependent loads on one thread,
// and a round lasts as long as its slowest row.
//
// Storage of a row: nodes [2][max_nodes][dof] (tree 0 = start, 1 = goal,
// node-major), parent [2][max_nodes], sizes [2], and the few words below.
#pragma once
#include "../../include/mpgpu.h"
#include "mpg_math.h"

namespace mpg {

constexpr int kRrtDof = 32;
constexpr int kRrtGoals = 16;
constexpr double kRrtPi = 3.14159265358979323846;        // boost::math::constants::pi (SO2StateSpace)
constexpr double kRrtEps = 2.220446049250313080847e-16;  // std::numeric_limits<double>::epsilon()
constexpr uint64_t kRrtGolden = 0x9E3779B97F4A7C15ull;

enum { RRT_EXTEND = 0, RRT_CONNECT = 1, RRT_DONE = 2 };
// a round's proposal: the tree it grows, the nearest node, how many states the
// validator looks at (0: growTree returns TRAPPED without asking) and whether
// the motion ends at the target
enum { RRT_P_TREE = 0, RRT_P_PARENT = 1, RRT_P_COUNT = 2, RRT_P_REACHED = 3, RRT_P_SM = 4, RRT_P_GM = 5, RRT_P_INTS = 6 };

// the planner's tables, passed by value
struct RrtView {
  int dof, goals, max_rounds, max_nodes, max_waypoints;
  int block;  // states of a row's slot block: ceil(range / lvs) + 2
  unsigned so2_mask;
  double range;  // RRTConnect's maxDistance
  double lvs;    // longestValidSegment: 0.01 * extent
  double lo[kRrtDof], hi[kRrtDof];  // bounds = sampling range; an SO2 slot holds [-pi, pi]
};

MPG_INLINE bool rrt_so2(const RrtView& v, int i) { return ((v.so2_mask >> i) & 1u) != 0; }

// --- sampler: splitmix64 of the row seed and the value's index -------------
MPG_INLINE uint64_t rrt_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
MPG_INLINE uint64_t rrt_row_seed(uint64_t seed, uint64_t row) { return rrt_mix(seed + (row + 1ull) * kRrtGolden); }
// coordinate j of the sample of iteration k: row k of mpg_sample_uniform(lo, hi, seed = row_seed)
MPG_INLINE double rrt_sample(const RrtView& v, uint64_t row_seed, int k, int j) {
  const uint64_t i = (uint64_t)k * (uint64_t)v.dof + (uint64_t)j;
  const double u = (double)(rrt_mix(row_seed + (i + 1ull) * kRrtGolden) >> 11) * (1.0 / 9007199254740992.0);
  return v.lo[j] + (v.hi[j] - v.lo[j]) * u;
}

// --- state space ------------------------------------------------------------
MPG_INLINE double rrt_distance(const RrtView& v, const double* a, const double* b) {
  double dist = 0.0;
  for (int i = 0; i < v.dof; ++i) {
    double di;
    if (rrt_so2(v, i)) {
      const double d = std::fabs(a[i] - b[i]);
      di = d > kRrtPi ? 2.0 * kRrtPi - d : d;
    } else {
      const double diff = a[i] - b[i];
      di = std::fabs(diff) > 1e-150 ? std::fabs(diff) : std::sqrt(diff * diff);
    }
    dist += di;
  }
  return dist;
}

MPG_INLINE void rrt_interpolate(const RrtView& v, const double* a, const double* b, double t, double* out) {
  for (int i = 0; i < v.dof; ++i) {
    if (!rrt_so2(v, i)) {
      out[i] = a[i] + (b[i] - a[i]) * t;
      continue;
    }
    double diff = b[i] - a[i];
    if (std::fabs(diff) <= kRrtPi) {
      out[i] = a[i] + diff * t;
    } else {
      diff = diff > 0.0 ? 2.0 * kRrtPi - diff : -2.0 * kRrtPi - diff;
      double x = a[i] - diff * t;
      if (x > kRrtPi) x -= 2.0 * kRrtPi;
      else if (x < -kRrtPi) x += 2.0 * kRrtPi;
      out[i] = x;
    }
  }
}

MPG_INLINE bool rrt_equal(const RrtView& v, const double* a, const double* b) {
  for (int i = 0; i < v.dof; ++i)
    if (rrt_so2(v, i) ? !(std::fabs(a[i] - b[i]) < 2.0 * kRrtEps) : std::fabs(a[i] - b[i]) > 2.0 * kRrtEps) return false;
  return true;
}

MPG_INLINE bool rrt_in_bounds(const RrtView& v, const double* s) {
  for (int i = 0; i < v.dof; ++i) {
    if (rrt_so2(v, i)) {
      if (s[i] < -kRrtPi || s[i] > kRrtPi) return false;
    } else if (s[i] - kRrtEps > v.hi[i] || s[i] + kRrtEps < v.lo[i]) {
      return false;
    }
  }
  return true;
}

// validSegmentCount; a NaN distance counts as 0 segments
MPG_INLINE int rrt_segments(const RrtView& v, const double* a, const double* b) {
  const double c = std::ceil(rrt_distance(v, a, b) / v.lvs);
  return c >= 1.0 ? (c < 1073741824.0 ? (int)c : 1073741824) : 0;
}

MPG_INLINE void rrt_copy(int dof, const double* a, double* out) {
  for (int i = 0; i < dof; ++i) out[i] = a[i];
}
MPG_INLINE double* rrt_node(const RrtView& v, double* nodes, int tree, int i) {
  return nodes + ((size_t)tree * v.max_nodes + i) * v.dof;
}

// --- start of a row -----------------------------------------------------------
// flags: the collide pass's bytes of (start, goal 0 .. goals - 1).  Writes the
// roots -- every goal that is valid and inside the bounds, in the given order
// -- the machine's words and the status bits of an invalid start or goal set.
// True: the row plans.  (The row's slot block and path start as copies of the
// start state: rrt_fill_start.)
MPG_INLINE bool rrt_init_row(const RrtView& v, const double* start, const double* goals, const uint8_t* flags,
                             double* nodes, int32_t* parent, int32_t* sizes, int32_t* phase, int32_t* added,
                             int32_t* iter, int32_t* prop, int32_t* n_waypoints, uint8_t* status) {
  int st = 0;
  sizes[0] = sizes[1] = 0;
  if (flags[0] == 0 && rrt_in_bounds(v, start)) {
    rrt_copy(v.dof, start, rrt_node(v, nodes, 0, 0));
    parent[0] = -1;
    sizes[0] = 1;
  } else {
    st |= MPG_PLAN_START_INVALID;
  }
  int ng = 0;
  for (int g = 0; g < v.goals; ++g) {
    const double* s = goals + (size_t)g * v.dof;
    if (flags[1 + g] != 0 || !rrt_in_bounds(v, s)) continue;
    if (ng >= v.max_nodes) {
      st |= MPG_PLAN_NODES_EXHAUSTED;
      break;
    }
    rrt_copy(v.dof, s, rrt_node(v, nodes, 1, ng));
    parent[v.max_nodes + ng] = -1;
    ++ng;
  }
  sizes[1] = ng;
  if (ng == 0) st |= MPG_PLAN_GOAL_INVALID;
  *phase = st ? RRT_DONE : RRT_EXTEND;
  *added = 0;
  *iter = 0;
  for (int k = 0; k < RRT_P_INTS; ++k) prop[k] = 0;
  *n_waypoints = 0;
  *status = (uint8_t)st;
  return st == 0;
}
// value k of the (block + max_waypoints) * dof a row starts with -- its slot
// block, then its path, every state the start state: where it goes
MPG_INLINE double* rrt_fill_start(const RrtView& v, long long k, double* slots, double* path) {
  const long long nb = (long long)v.block * v.dof;
  return k < nb ? slots + k : path + (k - nb);
}

// --- a round, first half ------------------------------------------------------
// the tree this round grows and the state it grows towards
MPG_INLINE int rrt_target(const RrtView& v, uint64_t row_seed, int phase, int32_t* iter, int added, double* nodes,
                          double* target) {
  if (phase == RRT_EXTEND) {
    const int k = *iter;
    *iter = k + 1;
    for (int j = 0; j < v.dof; ++j) target[j] = rrt_sample(v, row_seed, k, j);
    return k & 1;
  }
  const int mine = (*iter - 1) & 1;  // the iteration's tree; the other one connects to its new state
  rrt_copy(v.dof, rrt_node(v, nodes, mine, added), target);
  return 1 - mine;
}

// nodes first, first + stride, ... < n of one tree: the first strict minimum
// of the distance to target among them, merged into (*bd, *bi)
MPG_INLINE void rrt_nearest_scan(const RrtView& v, const double* tree_nodes, int n, const double* target, int first,
                                 int stride, double* bd, int* bi) {
  for (int i = first; i < n; i += stride) {
    const double d = rrt_distance(v, tree_nodes + (size_t)i * v.dof, target);
    if (d < *bd) {
      *bd = d;
      *bi = i;
    }
  }
}
// (distance, index) order of the reduction: ties go to the lower index
MPG_INLINE bool rrt_nearer(double d, int i, double bd, int bi) { return d < bd || (d == bd && i < bi); }

// growTree up to the validity question: the state to add (ds), the proposal
// and the motion's segment count
MPG_INLINE int rrt_steer(const RrtView& v, int tree, const double* near, int near_index, const double* target,
                         double* ds, int32_t* prop) {
  prop[RRT_P_TREE] = tree;
  prop[RRT_P_PARENT] = near_index;
  prop[RRT_P_COUNT] = 0;
  prop[RRT_P_REACHED] = 0;
  const double dd = rrt_distance(v, near, target);
  bool reach = true;
  if (dd > v.range) {
    rrt_interpolate(v, near, target, v.range / dd, ds);
    if (rrt_equal(v, near, ds)) return 0;  // TRAPPED
    reach = false;
  } else {
    rrt_copy(v.dof, target, ds);
  }
  // start tree: checkMotion(near, ds); goal tree: isValid(ds) && checkMotion(ds, near)
  const int nd = tree == 0 ? rrt_segments(v, near, ds) : rrt_segments(v, ds, near);
  const int count = (tree == 0 ? 0 : 1) + (nd < 1 ? 1 : nd);
  if (count > v.block) return 0;  // cannot happen: the motion is at most range (+ a few ulps) long
  prop[RRT_P_COUNT] = count;
  prop[RRT_P_REACHED] = reach ? 1 : 0;
  return nd;
}

// state s of the proposal's `count`: checkMotion(s1, s2) looks at s2, then at
// interpolate(s1, s2, j / nd) for j = 1 .. nd - 1
MPG_INLINE void rrt_slot_state(const RrtView& v, int tree, const double* near, const double* ds, int nd, int s,
                               double* out) {
  if (s == 0) rrt_copy(v.dof, ds, out);
  else if (tree == 0) rrt_interpolate(v, near, ds, (double)s / (double)nd, out);
  else if (s == 1) rrt_copy(v.dof, near, out);
  else rrt_interpolate(v, ds, near, (double)(s - 1) / (double)nd, out);
}

// --- a round, second half -------------------------------------------------------
// growTree's answer from the flags of the row's block, the node, the machine's
// next state and the end of the row; a row that connects leaves its two
// connection nodes in the proposal for rrt_path_indices.  True: the row ended
// in this round.
MPG_INLINE bool rrt_commit(const RrtView& v, int round, int32_t* prop, const double* ds, const uint8_t* flags,
                           double* nodes, int32_t* parent, int32_t* sizes, int32_t* phase, int32_t* added,
                           uint8_t* status) {
  if (*phase == RRT_DONE) return false;
  const int t = prop[RRT_P_TREE] & 1;
  int count = prop[RRT_P_COUNT];
  if (count > v.block) count = v.block;
  bool ok = count > 0;
  for (int i = 0; i < count; ++i)
    if (flags[i] != 0) ok = false;
  int st = 0;
  bool done = false;
  if (!ok) {
    *phase = RRT_EXTEND;  // TRAPPED: the next iteration
  } else if (sizes[t] >= v.max_nodes) {
    st = MPG_PLAN_NODES_EXHAUSTED;
    done = true;
  } else {
    const int n = sizes[t];
    rrt_copy(v.dof, ds, rrt_node(v, nodes, t, n));
    parent[(size_t)t * v.max_nodes + n] = prop[RRT_P_PARENT];
    sizes[t] = n + 1;
    if (*phase == RRT_EXTEND) {
      *added = n;
      *phase = RRT_CONNECT;
    } else if (prop[RRT_P_REACHED]) {  // the new node and the extension's hold the same state
      prop[RRT_P_SM] = t == 0 ? n : *added;
      prop[RRT_P_GM] = t == 0 ? *added : n;
      st = MPG_PLAN_SOLVED;
      done = true;
    }  // else ADVANCED: CONNECT again, same target
  }
  if (!done && round + 1 >= v.max_rounds) {
    st = MPG_PLAN_ROUNDS_EXHAUSTED;
    done = true;
  }
  if (done) {
    *status = (uint8_t)(*status | st);
    *phase = RRT_DONE;
  }
  return done;
}

// --- the path of a solved row, after the last round -----------------------------
// RRTConnect's solution path of start-tree node sm and goal-tree node gm, which
// hold the same state: root .. sm, gm .. root without the duplicate, as
// indices into the row's [2 * max_nodes] nodes.  The waypoint count; -1 when
// it exceeds max_waypoints (idx is not written).  Each walk is bounded by
// max_nodes steps, so a bad index cannot loop.
MPG_INLINE int rrt_path_indices(const RrtView& v, const int32_t* parent, int sm, int gm, int32_t* idx) {
  const int cap = v.max_nodes;
  if (parent[sm] >= 0) sm = parent[sm];
  else gm = parent[cap + gm];
  int ns = 0, ng = 0;
  for (int m = sm, k = 0; m >= 0 && k < cap; m = parent[m], ++k) ++ns;
  for (int m = gm, k = 0; m >= 0 && k < cap; m = parent[cap + m], ++k) ++ng;
  const int n = ns + ng;
  if (n > v.max_waypoints) return -1;
  int pos = ns - 1;
  for (int m = sm, k = 0; m >= 0 && k < cap; m = parent[m], ++k, --pos) idx[pos] = m;
  pos = ns;
  for (int m = gm, k = 0; m >= 0 && k < cap; m = parent[cap + m], ++k, ++pos) idx[pos] = cap + m;
  return n;
}
// slot p of the row's path: waypoint p, the last one past the count
MPG_INLINE void rrt_path_slot(const RrtView& v, const double* nodes, const int32_t* idx, int n, int p, double* path) {
  rrt_copy(v.dof, nodes + (size_t)idx[p < n ? p : n - 1] * v.dof, path + (size_t)p * v.dof);
}
// the whole of it on one thread (the host; rrt_path_kernel spreads the slots
// over a wave).  idx: max_waypoints words of scratch.
MPG_INLINE void rrt_finish_row(const RrtView& v, const int32_t* prop, const double* nodes, const int32_t* parent,
                               int32_t* idx, double* path, int32_t* n_waypoints, uint8_t* status) {
  if (!(*status & MPG_PLAN_SOLVED)) return;
  const int n = rrt_path_indices(v, parent, prop[RRT_P_SM], prop[RRT_P_GM], idx);
  if (n < 0) {
    *status = (uint8_t)(*status | MPG_PLAN_TRUNCATED);  // the count stays 0, the slots the start state
    return;
  }
  *n_waypoints = n;
  for (int p = 0; p < v.max_waypoints; ++p) rrt_path_slot(v, nodes, idx, n, p, path);
}

}  // namespace mpg
