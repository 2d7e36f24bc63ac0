// mpg_screw.h -- the straight-line screw motion of one (goal, start) row, shared
// by screw_kernel (mpg_kernels.hip) and the host-side test
// (tests/test_screw_host.py compiles this header with g++ -ffp-contract=off).
//
//   plan_screw           mplib/planner.py:526-671 (without TOPP-RA: the joint-space waypoints)
//   pose2exp_coordinate  mplib/planner.py:575-605, with its two np.isclose branches
//   getLinkJacobian      src/pinocchio_model.cpp:340-359, local = false: the WORLD columns
//                        oMi[j].act(S_j) that ik_fk (mpg_ik.h) leaves in the lane
//
// The row state is mpg_ik.h's IkLane.  The lane of a continuous joint holds
// (cos, sin); its angle is read from the last stored waypoint, because the
// reference adds the step to the user qpos and only then takes cosine and sine.
#pragma once
#include "mpg_ik.h"

namespace mpg {

// the tables of a call, passed by value next to DevWorld.  Of iv the link, the
// chain, move[] and the limit tables (bounded, lo, hi: the joints' own limits)
// are used; no slot is frozen.
struct ScrewView {
  IkView iv;
  double qpos_step;
  int max_waypoints;
  unsigned char offchain[kIkDof];  // slot d belongs to no joint of the link's chain: it keeps its start value
};

enum { SCREW_EXP_GENERAL = 0, SCREW_EXP_TRANSLATION = 1, SCREW_EXP_ROT_PI = 2 };

// pose2exp_coordinate(T) * theta: tw = (v, omega) * theta.  Returns the branch
// rot2so3 took: np.isclose(trace, 3) drops the rotation (omega = 0, theta = 1),
// np.isclose(trace, -1) gives up (tw is zero).
MPG_INLINE int screw_exp_coordinate(const SE3& T, double* tw) {
  const double* R = T.R;
  const double tr = (R[0] + R[4]) + R[8];
  double om[3] = {0.0, 0.0, 0.0}, theta = 1.0;
  int branch = SCREW_EXP_TRANSLATION;
  if (!(fabs(tr - 3.0) <= 1e-8 + 1e-5 * 3.0)) {
    if (fabs(tr + 1.0) <= 1e-8 + 1e-5 * 1.0) {
#pragma unroll
      for (int i = 0; i < 6; ++i) tw[i] = 0.0;
      return SCREW_EXP_ROT_PI;
    }
    theta = acos((tr - 1.0) / 2.0);
    double st, ct;
    mpg_sincos(theta, &st, &ct);
    const double f = 0.5 / st;
    om[0] = f * (R[7] - R[5]);
    om[1] = f * (R[2] - R[6]);
    om[2] = f * (R[3] - R[1]);
    branch = SCREW_EXP_GENERAL;
  }
  // inv_left_jacobian = I / theta - ss / 2 + ((1 / theta - 1 / (2 tan(theta / 2))) ss) ss
  double sh, ch;
  mpg_sincos(theta / 2.0, &sh, &ch);
  const double c = 1.0 / theta - 0.5 / (sh / ch);
  const double ss[9] = {0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double s2 = ((c * ss[3 * i]) * ss[j] + (c * ss[3 * i + 1]) * ss[3 + j]) + (c * ss[3 * i + 2]) * ss[6 + j];
      const double m = ((i == j ? 1.0 : 0.0) / theta - 0.5 * ss[3 * i + j]) + s2;
      v += m * T.p[j];
    }
    tw[i] = v * theta;
    tw[3 + i] = om[i] * theta;
  }
  return branch;
}

// One step from the columns ik_fk left: dq = J^T (J J^T)^-1 tw scaled to
// |dq| = qpos_step, dtw = J dq, both scaled by |tw| / |dtw| when |dtw| > |tw|
// (*last); q += dq, tw -= dtw.  cur: the last stored waypoint; next: receives
// the chain's slots of the new state.  *dn: |dtw|.  false: a non-positive
// pivot, nothing is touched.  dq_k is formed three times from the same
// operands instead of being kept per joint: the same bits each time.
template <class J>
MPG_INLINE bool screw_step(const J& jt, const ScrewView& sv, const IkLane& L, const double* cur, double* next,
                           double* tw, double* dn, bool* last) {
  const IkView& iv = sv.iv;
  double A[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) A[i] = 0.0;
  for (int k = 0; k < iv.cl; ++k) {
    if (!jt.move(k)) continue;
    double c[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) c[i] = L.at(k, IK_COL + i);
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) A[6 * a + b] += c[a] * c[b];
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) y[i] = tw[i];
  if (!ik_spd_solve6(A, y)) return false;
  double n2 = 0.0;
  for (int k = 0; k < iv.cl; ++k) {
    if (!jt.move(k)) continue;
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) s += L.at(k, IK_COL + a) * y[a];
    n2 += s * s;
  }
  const double scale = sv.qpos_step / sqrt(n2);
  double dtw[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < iv.cl; ++k) {
    if (!jt.move(k)) continue;
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) s += L.at(k, IK_COL + a) * y[a];
    const double dq = s * scale;
#pragma unroll
    for (int a = 0; a < 6; ++a) dtw[a] += L.at(k, IK_COL + a) * dq;
  }
  const double nd = ik_norm6(dtw), nt = ik_norm6(tw);
  const bool fin = nd > nt;
  const double ratio = fin ? nt / nd : 1.0;
  for (int k = 0; k < iv.cl; ++k) {
    if (!jt.move(k)) continue;
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) s += L.at(k, IK_COL + a) * y[a];
    double dq = s * scale;
    if (fin) dq = dq * ratio;
    const int d = jt.src(k);
    if (jt.type(k) >= MPG_JOINT_RUBX) {
      const double a = cur[d] + dq;
      double sa, ca;
      mpg_sincos(a, &sa, &ca);
      next[d] = a;
      L.at(k, IK_Q) = ca;
      L.at(k, IK_S) = sa;
    } else {
      const double a = L.at(k, IK_Q) + dq;
      next[d] = a;
      L.at(k, IK_Q) = a;
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    if (fin) dtw[a] = dtw[a] * ratio;
    tw[a] -= dtw[a];
  }
  *dn = fin ? ik_norm6(dtw) : nd;
  *last = fin;
  return true;
}

// plan_screw's own limit test (planner.py:639-647) of the chain's slots of q: no wrap
template <class J>
MPG_INLINE bool screw_chain_outside(const J& jt, const IkView& iv, const double* q) {
  bool out = false;
  for (int k = 0; k < iv.cl; ++k) {
    const int d = jt.src(k);
    if (d < 0 || !iv.bounded[d]) continue;
    out = out || q[d] < iv.lo[d] - 1e-3 || q[d] > iv.hi[d] + 1e-3;
  }
  return out;
}

// One whole row on one lane: the waypoints go to path [max_waypoints][dof] as
// they are accepted, the slots past *count repeat the last one.  Returns the
// row's MPG_SCREW_* end bit.  Every pass stores a waypoint or ends the row, so
// max_waypoints bounds the loop for any input.
template <class J>
MPG_INLINE int screw_row(const DevWorld& w, const J& jt, const ScrewView& sv, const IkLane& L, const double* goal7,
                         const double* qstart, double* path, int* count) {
  const IkView& iv = sv.iv;
  const int dof = w.dof;
  bool off_outside = false;  // the slots outside the chain never move: tested once
  for (int d = 0; d < dof; ++d) {
    const double q = qstart[d];
    path[d] = q;
    if (sv.offchain[d] && iv.bounded[d]) off_outside = off_outside || q < iv.lo[d] - 1e-3 || q > iv.hi[d] + 1e-3;
  }
  ik_load_row(jt, iv, L, qstart);
  const SE3 Tl = link_from_oMi(w, ik_fk(jt, iv, L), iv.link, nullptr);
  double tw[6];
  int n = 1, st = 0;
  if (screw_exp_coordinate(se3_mul(ik_pose_se3(goal7), ik_se3_inverse(Tl)), tw) == SCREW_EXP_ROT_PI) {
    st = MPG_SCREW_ROT_PI;
  } else {
    for (;;) {
      ik_fk(jt, iv, L);
      // the new state goes to slot n at once; it counts only when n moves on
      // (the padding below overwrites a state that was not accepted)
      double* p = path + (size_t)n * dof;
      double dn;
      bool last;
      if (!screw_step(jt, sv, L, p - dof, p, tw, &dn, &last)) {
        st = MPG_SCREW_SINGULAR;
        break;
      }
      if (dn < 1e-4) {
        st = MPG_SCREW_STALLED;
        break;
      }
      if (off_outside || screw_chain_outside(jt, iv, p)) {
        st = MPG_SCREW_LIMIT;
        break;
      }
      for (int d = 0; d < dof; ++d)
        if (sv.offchain[d]) p[d] = qstart[d];
      ++n;
      if (last) {
        st = MPG_SCREW_REACHED;
        break;
      }
      if (n >= sv.max_waypoints) {
        st = MPG_SCREW_TRUNCATED;
        break;
      }
    }
  }
  const double* lastp = path + (size_t)(n - 1) * dof;
  for (int i = n; i < sv.max_waypoints; ++i)
    for (int d = 0; d < dof; ++d) path[(size_t)i * dof + d] = lastp[d];
  *count = n;
  return st;
}

}  // namespace mpg
