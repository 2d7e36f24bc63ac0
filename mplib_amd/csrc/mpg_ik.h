// mpg_ik.h -- closed-loop inverse kinematics of one (goal, seed) row, shared by
// ik_clik_kernel / ik_finish_kernel (mpg_kernels.hip) and the host-side test
// (tests/test_ik_host.py compiles this header with g++ -ffp-contract=off).
//
//   computeIKCLIK        src/pinocchio_model.cpp:376-433; [ext pinocchio 2.6.21] computeJointJacobian
//                        (LOCAL), log3 / log6, integrate -- as csrc/host/kinjac.cpp restates them
//   check_joint_limit    mplib/planner.py:170-191
//   distance_6D          mplib/planner.py:165-168
//
// A row's state lives in an IkLane: per joint of the link's chain kIkSlot
// doubles -- the joint value (continuous joints: cos, sin) and the joint's
// Jacobian column.  On the device that is LDS laid out [joint][component][lane]
// (the chain index is wave-uniform, so nothing is indexed per lane and nothing
// goes to scratch); on the host a plain array.
#pragma once
#include "mpg_fk.h"

namespace mpg {

constexpr int kIkChain = 15;  // joints above the link: 15 * kIkSlot * 64 lanes * 8 B = 60 KiB of LDS per wave
constexpr int kIkDof = 32;
constexpr int kIkSlot = 8;
enum { IK_Q = 0, IK_S = 1, IK_COL = 2 };  // value (continuous: cos), sin, column (linear, angular)
enum { IKK_NONE = 0, IKK_REVOLUTE = 1, IKK_PRISMATIC = 2 };  // kind of the joint behind a dof slot

// the IK's tables, passed by value next to DevWorld
struct IkView {
  int link, cs, cl;  // user link, its chain in DevWorld::chain_joints
  int max_iter;
  double eps, dt, damp, threshold;
  unsigned char move[kIkChain + 1];  // chain joint k has a dof slot that is not masked
  unsigned char kind[kIkDof];        // IKK_* of slot d
  unsigned char bounded[kIkDof];     // lo / hi of slot d are finite
  unsigned char frozen[kIkDof];      // mask
  double lo[kIkDof], hi[kIkDof];     // limits; the sampling range of a continuous joint is [-pi, pi]
};

struct IkLane {
  double* base;
  int stride;
  MPG_INLINE double& at(int k, int c) const { return base[(k * kIkSlot + c) * stride]; }
};

// Where a row's step reads the constants of chain joint k from.  IkJointsWorld:
// the snapshot (the host test, one read per row).  IkJointsTable: a compact
// copy the IK kernel makes in LDS once per wave -- the step walks the chain
// three times per iteration, and a dependent pair of snapshot loads per joint
// and walk (chain_joints[k], then the joint's record) was most of its time.
struct IkJointsWorld {
  const DevWorld& w;
  const IkView& iv;
  MPG_INLINE int j0(int k) const { return w.chain_joints[iv.cs + k] - 1; }
  MPG_INLINE int type(int k) const { return w.joint_type[j0(k)]; }
  MPG_INLINE int src(int k) const { return w.joint_q_source[j0(k)]; }
  MPG_INLINE bool move(int k) const { return iv.move[k] != 0; }
  MPG_INLINE double qconst(int k) const { return w.joint_q_const[j0(k)]; }
  MPG_INLINE cptr<double> axis(int k) const { return w.joint_axis + 3 * j0(k); }
  MPG_INLINE cptr<double> place(int k) const { return w.joint_place + 12 * j0(k); }
};
enum { IKT_QCONST = 0, IKT_AXIS = 1, IKT_PLACE = 4, IKT_DOUBLES = 16, IKT_TYPE = 0, IKT_SRC = 1, IKT_MOVE = 2, IKT_INTS = 3 };
struct IkJointsTable {
  const double* td;  // [cl][IKT_DOUBLES]
  const int* ti;     // [cl][IKT_INTS]
  MPG_INLINE int type(int k) const { return ti[IKT_INTS * k + IKT_TYPE]; }
  MPG_INLINE int src(int k) const { return ti[IKT_INTS * k + IKT_SRC]; }
  MPG_INLINE bool move(int k) const { return ti[IKT_INTS * k + IKT_MOVE] != 0; }
  MPG_INLINE double qconst(int k) const { return td[IKT_DOUBLES * k + IKT_QCONST]; }
  MPG_INLINE const double* axis(int k) const { return td + IKT_DOUBLES * k + IKT_AXIS; }
  MPG_INLINE const double* place(int k) const { return td + IKT_DOUBLES * k + IKT_PLACE; }
};

MPG_INLINE void ik_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
MPG_INLINE void ik_matv(const double* R, const double* x, double* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = (R[3 * i] * x[0] + R[3 * i + 1] * x[1]) + R[3 * i + 2] * x[2];
}
MPG_INLINE void ik_mattv(const double* R, const double* x, double* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = (R[i] * x[0] + R[3 + i] * x[1]) + R[6 + i] * x[2];
}

MPG_INLINE SE3 ik_se3_inverse(const SE3& M) {
  SE3 o;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o.R[3 * i + j] = M.R[3 * j + i];
  double rp[3];
  ik_mattv(M.R, M.p, rp);
#pragma unroll
  for (int k = 0; k < 3; ++k) o.p[k] = -rp[k];
  return o;
}

// (x, y, z, qw, qx, qy, qz) -> SE3
template <class P>
MPG_INLINE SE3 ik_pose_se3(P pose) {
  SE3 T;
  quat_to_mat(pose[3], pose[4], pose[5], pose[6], T.R);
  T.p[0] = pose[0];
  T.p[1] = pose[1];
  T.p[2] = pose[2];
  return T;
}

// pinocchio::log3: the rotation vector of R (angle in [0, pi])
MPG_INLINE void ik_log3(const double* R, double* w) {
  constexpr double kPi = 3.14159265358979323846;
  const double tr = (R[0] + R[4]) + R[8];
  double theta;
  if (tr > 3.0) theta = 0.0;
  else if (tr < -1.0) theta = kPi;
  else theta = acos((tr - 1.0) / 2.0);
  if (theta >= kPi - 1e-2) {  // near pi: from the diagonal, signs from the skew part
    double sphi, cphi;
    mpg_sincos(theta - kPi, &sphi, &cphi);
    const double beta = theta * theta / (1.0 + cphi);
    const double t0 = (R[0] + cphi) * beta, t1 = (R[4] + cphi) * beta, t2 = (R[8] + cphi) * beta;
    w[0] = (R[7] > R[5] ? 1.0 : -1.0) * (t0 > 0 ? sqrt(t0) : 0.0);
    w[1] = (R[2] > R[6] ? 1.0 : -1.0) * (t1 > 0 ? sqrt(t1) : 0.0);
    w[2] = (R[3] > R[1] ? 1.0 : -1.0) * (t2 > 0 ? sqrt(t2) : 0.0);
  } else {
    double st = 1.0, ct;
    if (theta > 1e-4) mpg_sincos(theta, &st, &ct);
    const double t = (theta > 1e-4 ? theta / st : 1.0) / 2.0;
    w[0] = t * (R[7] - R[5]);
    w[1] = t * (R[2] - R[6]);
    w[2] = t * (R[3] - R[1]);
  }
}

// pinocchio::log6(M).toVector(): (linear, angular)
MPG_INLINE void ik_log6(const SE3& M, double* o) {
  double w[3];
  ik_log3(M.R, w);
  const double t = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]), t2 = t * t;
  double alpha, beta;
  if (t < 1e-4) {
    alpha = 1.0 - t2 / 12.0 - t2 * t2 / 720.0;
    beta = 1.0 / 12.0 + t2 / 720.0;
  } else {
    double st, ct;
    mpg_sincos(t, &st, &ct);
    alpha = t * st / (2.0 * (1.0 - ct));
    beta = 1.0 / t2 - st / (2.0 * t * (1.0 - ct));
  }
  double wxp[3];
  ik_cross(w, M.p, wxp);
  const double wp = (w[0] * M.p[0] + w[1] * M.p[1]) + w[2] * M.p[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[k] = alpha * M.p[k] - 0.5 * wxp[k] + (beta * wp) * w[k];
    o[3 + k] = w[k];
  }
}

// solves A x = b in place for a symmetric 6x6 A given by its lower triangle
// (row-major); false at a non-positive pivot.  Fully unrolled: every index is
// a constant, so A and b stay in registers.
MPG_INLINE bool ik_spd_solve6(double* A, double* b) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[6 * j + j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= A[6 * j + k] * A[6 * j + k];
    ok = ok && d > 0;
    const double l = sqrt(d);
    A[6 * j + j] = l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = A[6 * i + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= A[6 * i + k] * A[6 * j + k];
      A[6 * i + j] = s / l;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= A[6 * i + k] * b[k];
    b[i] = s / A[6 * i + i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = b[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= A[6 * k + i] * b[k];
    b[i] = s / A[6 * i + i];
  }
  return ok;
}

// the row's joint values into the lane: qpos_user2pin for the chain's joints
template <class J>
MPG_INLINE void ik_load_row(const J& jt, const IkView& iv, const IkLane& L, const double* qrow) {
  for (int k = 0; k < iv.cl; ++k) {
    const int src = jt.src(k);
    const double v = src >= 0 ? qrow[src] : jt.qconst(k);
    if (jt.type(k) >= MPG_JOINT_RUBX) {
      double s, c;
      mpg_sincos(v, &s, &c);
      L.at(k, IK_Q) = c;
      L.at(k, IK_S) = s;
    } else {
      L.at(k, IK_Q) = v;
    }
  }
}

// qpos_pin2user of the chain's joints with a dof slot into the row
template <class J>
MPG_INLINE void ik_store_row(const J& jt, const IkView& iv, const IkLane& L, double* qrow) {
  for (int k = 0; k < iv.cl; ++k) {
    const int src = jt.src(k);
    if (src < 0) continue;
    qrow[src] = jt.type(k) >= MPG_JOINT_RUBX ? atan2(L.at(k, IK_S), L.at(k, IK_Q)) : L.at(k, IK_Q);
  }
}

// forwardKinematics along the chain (chain_oMi's products in its order);
// leaves every moving joint's WORLD column oMi[j].act(S_j) in the lane and
// returns oMi[jid]
template <class J>
MPG_INLINE SE3 ik_fk(const J& jt, const IkView& iv, const IkLane& L) {
  SE3 T;
  se3_identity(T);
  for (int k = 0; k < iv.cl; ++k) {
    const int type = jt.type(k);
    const bool rev = joint_is_revolute(type);
    double sc[2] = {0.0, 1.0}, v = 0.0;
    if (!rev) {
      v = L.at(k, IK_Q);
    } else if (type >= MPG_JOINT_RUBX) {
      sc[0] = L.at(k, IK_S);
      sc[1] = L.at(k, IK_Q);
    } else {
      mpg_sincos(L.at(k, IK_Q), &sc[0], &sc[1]);
    }
    const SE3 M = rev ? joint_motion(type, jt.axis(k), 0.0, sc) : joint_motion(type, jt.axis(k), v);
    const SE3 li = se3_mul(load_se3(jt.place(k)), M);
    T = k == 0 ? li : se3_mul(T, li);
    if (!jt.move(k)) continue;
    // the joint's motion subspace in its own frame: a unit vector, or the axis
    const int t = rev ? (type >= MPG_JOINT_RUBX ? type - MPG_JOINT_RUBX : type) : type - MPG_JOINT_PX;
    double ax[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) ax[c] = t < 3 ? (t == c ? 1.0 : 0.0) : jt.axis(k)[c];
    double aw[3], lin[3];
    ik_matv(T.R, ax, aw);
    if (rev) ik_cross(T.p, aw, lin);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      L.at(k, IK_COL + c) = rev ? lin[c] : aw[c];
      L.at(k, IK_COL + 3 + c) = rev ? aw[c] : 0.0;
    }
  }
  return T;
}

// one damped least-squares step from the columns ik_fk left: v = -J^T (J J^T +
// damp I)^-1 err dt, q = integrate(q, v).  false: a non-positive pivot, the
// joint values are untouched.
template <class J>
MPG_INLINE bool ik_update(const J& jt, const IkView& iv, const IkLane& L, const SE3& oMjid, const double* err) {
  double A[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) A[i] = 0.0;
  for (int k = 0; k < iv.cl; ++k) {
    if (!jt.move(k)) continue;
    // computeJointJacobian: the column in the joint's own frame, oMi[jid].actInv(column)
    double lin[3], ang[3], pxw[3], d[3], c[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      lin[i] = L.at(k, IK_COL + i);
      ang[i] = L.at(k, IK_COL + 3 + i);
    }
    ik_cross(oMjid.p, ang, pxw);
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = lin[i] - pxw[i];
    ik_mattv(oMjid.R, d, c);
    ik_mattv(oMjid.R, ang, c + 3);
#pragma unroll
    for (int i = 0; i < 6; ++i) L.at(k, IK_COL + i) = c[i];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) A[6 * a + b] += c[a] * c[b];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) A[6 * a + a] += iv.damp;
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) y[i] = err[i];
  if (!ik_spd_solve6(A, y)) return false;
  for (int k = 0; k < iv.cl; ++k) {
    if (!jt.move(k)) continue;
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) s += L.at(k, IK_COL + a) * y[a];
    const double v = -s * iv.dt;
    if (jt.type(k) >= MPG_JOINT_RUBX) {  // pinocchio::integrate of a continuous joint
      const double ca = L.at(k, IK_Q), sa = L.at(k, IK_S);
      double so, co;
      mpg_sincos(v, &so, &co);
      const double c2 = co * ca - so * sa, s2 = so * ca + co * sa;
      const double n = (3.0 - (c2 * c2 + s2 * s2)) / 2.0;
      L.at(k, IK_Q) = c2 * n;
      L.at(k, IK_S) = s2 * n;
    } else {
      L.at(k, IK_Q) += v;
    }
  }
  return true;
}

MPG_INLINE double ik_norm6(const double* e) {
  double n2 = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) n2 += e[i] * e[i];
  return sqrt(n2);
}

// check_joint_limit for slot d: wraps q, true when the joint fails
MPG_INLINE bool ik_wrap_limit(const IkView& iv, int d, double& q) {
  constexpr double kTwoPi = 2.0 * 3.14159265358979323846;
  if (!iv.bounded[d] || iv.kind[d] == IKK_NONE) return false;
  const double lo = iv.lo[d], hi = iv.hi[d];
  if (iv.kind[d] == IKK_REVOLUTE) {
    if (fabs(q - lo) < 1e-3) return false;
    q -= kTwoPi * floor((q - lo) / kTwoPi);
    return q > hi + 1e-3;
  }
  return q < lo - 1e-3 || q > hi + 1e-3;
}

// distance_6D of two (p, wxyz) poses
template <class P>
MPG_INLINE double ik_distance_6d(P a, const double* b) {
  double dp = 0.0, dm = 0.0, ds = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) dp += (a[i] - b[i]) * (a[i] - b[i]);
#pragma unroll
  for (int i = 3; i < 7; ++i) {
    dm += (a[i] - b[i]) * (a[i] - b[i]);
    ds += (a[i] + b[i]) * (a[i] + b[i]);
  }
  return sqrt(dp) + sqrt(dm < ds ? dm : ds);
}

// steps 2 and 3b of a row: wrap and limit bit, link pose and threshold bit;
// returns the bits to add to the row's status
MPG_INLINE int ik_finish_row(const DevWorld& w, const IkView& iv, const double* goal7, double* qrow) {
  bool fail = false;
  for (int d = 0; d < w.dof; ++d) {
    double q = qrow[d];
    fail = ik_wrap_limit(iv, d, q) || fail;
    qrow[d] = q;
  }
  double pose7[7];
  link_from_oMi(w, chain_oMi(w, qrow, iv.link), iv.link, pose7);
  const bool within = ik_distance_6d(goal7, pose7) < iv.threshold;
  return (fail ? 0 : MPG_IK_IN_LIMITS) | (within ? MPG_IK_WITHIN_THRESHOLD : 0);
}

// one whole row on one lane (the host test's loop; ik_clik_kernel runs the
// same calls with its lanes claiming rows)
MPG_INLINE int ik_solve_row(const DevWorld& w, const IkView& iv, const IkLane& L, const double* goal7, double* qrow,
                            double* err, int* iters) {
  const SE3 Ginv = se3_mul(load_se3(w.link_place + 12 * iv.link), ik_se3_inverse(ik_pose_se3(goal7)));
  const IkJointsWorld jt{w, iv};
  ik_load_row(jt, iv, L, qrow);
  int st = 0, it = 0;
  for (; it <= iv.max_iter; ++it) {
    const SE3 T = ik_fk(jt, iv, L);
    ik_log6(se3_mul(Ginv, T), err);
    if (ik_norm6(err) < iv.eps) {
      st = MPG_IK_CONVERGED;
      break;
    }
    if (it >= iv.max_iter) break;
    if (!ik_update(jt, iv, L, T, err)) {
      st = MPG_IK_SINGULAR;
      break;
    }
  }
  ik_store_row(jt, iv, L, qrow);
  *iters = it;
  return st;
}

}  // namespace mpg
