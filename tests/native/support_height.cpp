// Test shim: the cull's support-height tables and axes (mpg_broadphase.h)
// compiled for the host, for tests/test_support_height.py.  Not part of the
// product.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "../../mplib_amd/csrc/mpg_broadphase.h"

extern "C" {
int sh_floats() { return mpg::kShFloats; }
int sh_k() { return mpg::kShK; }

// the table of hull V (nv vertices) about centre c, as the snapshot stores it
void sh_table(const double* V, int nv, const double* c, float* tab) { mpg::bp_support_table(V, nv, c, tab); }

// bp_support_height for n directions given in fp32
void sh_height(const float* tab, const float* dirs, long n, float* out) {
  for (long i = 0; i < n; ++i) out[i] = mpg::bp_support_height(tab, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
}

// local OBB (centre, widened half extents) of a hull as bp_build records it
// from the geometry record: e = widen(half extent * (1 + 1e-12) + 1e-12)
void sh_obb(const double* V, int nv, double* c, float* e) {
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

// Replay of the cull's two pair tests on n poses of one pair.  Per side: the
// local OBB centre c[3] and extents e[3], its table (or NULL: SH_NONE), and
// per pose the world transform T[n][12] (row-major R, then p) in fp64; the
// fp32 OBB is built from it the way the cull's records are (centre = T * c
// rounded to fp32, rotation rounded to fp32).  out[i]: 0 = the OBB SAT
// separates, 1 = the support-height axes separate, 2 = kept.
void sh_replay(const double* ca, const float* ea, const float* taba, const double* Ta, const double* cb,
               const float* eb, const float* tabb, const double* Tb, long n, float margin, float sh_margin,
               unsigned char* out) {
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
    if (mpg::fobb_separated(A, B, margin)) out[i] = 0;
    else if ((taba || tabb) && mpg::bp_support_separated(A, B, ia, ib, tab.data(), sh_margin)) out[i] = 1;
    else out[i] = 2;
  }
}
}
