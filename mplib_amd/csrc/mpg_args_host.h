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

// dynamic LDS of ik_clik_kernel and screw_kernel (a wave per block): 64 lanes' slots and the tables of cl joints
inline size_t ik_lds_bytes(int cl) {
  const size_t c = (size_t)std::max(cl, 1);
  return sizeof(double) * (mpg::kIkSlot * 64 + mpg::IKT_DOUBLES) * c + sizeof(int) * mpg::IKT_INTS * c;
}

}  // namespace mpg_args
