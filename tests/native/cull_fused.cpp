// Test shim: the cull's fused SAT + support-height test and the item indexing
// of its sincos pass (mpg_broadphase.h, mpg_fk.h) compiled for the host, for
// tests/test_cull_fused.py.  Not part of the product.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../mplib_amd/csrc/mpg_fk.h"

extern "C" {
int cf_floats() { return mpg::kShFloats; }

// the table of hull V (nv vertices) about centre c, as the snapshot stores it
void cf_table(const double* V, int nv, const double* c, float* tab) { mpg::bp_support_table(V, nv, c, tab); }

// local OBB (centre, widened half extents) of a hull as bp_build records it
void cf_obb(const double* V, int nv, double* c, float* e) {
  for (int k = 0; k < 3; ++k) {
    double lo = DBL_MAX, hi = -DBL_MAX;
    for (int i = 0; i < nv; ++i) {
      lo = std::min(lo, V[3 * i + k]);
      hi = std::max(hi, V[3 * i + k]);
    }
    c[k] = 0.5 * (lo + hi);
    e[k] = mpg::widen(0.5 * (hi - lo) * (1.0 + 1e-12) + 1e-12);
  }
}

// The fused test against the two it replaces on n poses of one pair.  Per
// side: the local OBB centre c[3] and extents e[3], its table (or NULL:
// SH_NONE), and per pose the world transform T[n][12] (row-major R, then p)
// in fp64; the fp32 OBB is built from it the way the cull's records are.
// tot[0] += poses where bp_sat_support_separated differs from
// fobb_separated || bp_support_separated; tot[1], tot[2], tot[3] += poses the
// SAT separates, the support axes separate, neither separates.
void cf_compare(const double* ca, const float* ea, const float* taba, const double* Ta, const double* cb,
                const float* eb, const float* tabb, const double* Tb, long n, float margin, float sh_margin,
                long long* tot) {
  std::vector<float> tab((size_t)2 * mpg::kShFloats, 0.f);
  if (taba) std::copy(taba, taba + mpg::kShFloats, tab.begin());
  if (tabb) std::copy(tabb, tabb + mpg::kShFloats, tab.begin() + mpg::kShFloats);
  const int ia = taba ? 0 : (int)mpg::SH_NONE, ib = tabb ? 1 : (int)mpg::SH_NONE;
  auto obb = [](const double* c, const float* e, const double* T) {
    mpg::FObb o;
    for (int i = 0; i < 3; ++i) {
      o.c[i] = (float)(T[3 * i] * c[0] + T[3 * i + 1] * c[1] + T[3 * i + 2] * c[2] + T[9 + i]);
      o.e[i] = e[i];
    }
    for (int k = 0; k < 9; ++k) o.R[k] = (float)T[k];
    return o;
  };
  for (long i = 0; i < n; ++i) {
    const mpg::FObb A = obb(ca, ea, Ta + 12 * i), B = obb(cb, eb, Tb + 12 * i);
    const bool sat = mpg::fobb_separated(A, B, margin);
    const bool sup = mpg::bp_support_separated(A, B, ia, ib, tab.data(), sh_margin);
    const bool fused = mpg::bp_sat_support_separated(A, B, ia, ib, tab.data(), margin, sh_margin);
    tot[0] += fused != (sat || sup);
    tot[sat ? 1 : sup ? 2 : 3] += 1;
  }
}

// revolute_sources of a joint table: the slots to out (room for nj), their number returned
int cf_rev_sources(const int* joint_type, const int* joint_q_source, int nj, int* out) {
  const std::vector<int> r = mpg::revolute_sources(joint_type, joint_q_source, nj);
  std::copy(r.begin(), r.end(), out);
  return (int)r.size();
}

// every thread of a block of `block` threads runs bp_sincos_items: visits[k *
// n_rev + r] += 1 per item (k, r) taken; returned: the items outside
// [0, total) x [0, n_rev)
long cf_sincos_items(int block, int total, int n_rev, int* visits) {
  long bad = 0;
  for (int tid = 0; tid < block; ++tid)
    mpg::bp_sincos_items((uint32_t)tid, (uint32_t)block, (uint32_t)total, (uint32_t)n_rev, [&](uint32_t k, uint32_t r) {
      if (k >= (uint32_t)total || r >= (uint32_t)n_rev) ++bad;
      else ++visits[k * n_rev + r];
    });
  return bad;
}
}
