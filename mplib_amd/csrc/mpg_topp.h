// mpg_topp.h -- the time-optimal parametrisation of one joint-space path
// (TOPP-RA, Pham & Pham 2018), shared by topp_row_kernel / topp_sample_kernel
// (mpg_kernels.hip) and the host-side test (tests/test_topp_host.py compiles
// this header with g++ -ffp-contract=off).  DESIGN.md section 14 states the
// algorithm; include/mpgpu.h (mpg_topp_batch) is its contract.
//
//   Planner.TOPP        mplib/planner.py:358-375: a cubic spline through the
//                       waypoints at s = linspace(0, 1, n), TOPP-RA under the
//                       joint velocity and acceleration limits, samples at
//                       linspace(0, duration, int(duration / step))
//   discretisation      toppra's default: first-order interpolation
//   output              toppra's ParametrizeConstAccel
//
// fp64 with + - * / sqrt and comparisons only.  A row is worked on by the
// `lanes` lanes of a policy P: ToppSerial (one lane, the host) or the kernel's
// wave of 64.  The lanes split index ranges -- joints, constraint rows, pairs of
// constraint rows -- and meet in P::wmin, a minimum over all lanes that every
// lane receives.  A minimum over a fixed set of values does not depend on the
// order it is taken in and no sum is split over lanes, so both policies give
// the same bits.  A NaN candidate counts as the bound 0, whatever lane meets it.
#pragma once
#include "../../include/mpgpu.h"
#include "mpg_math.h"

namespace mpg {

constexpr int kToppDof = 32;
constexpr int kToppRows = 2 * kToppDof + 1;  // constraint rows of one interval
constexpr double kToppXCap = 1e12;           // the velocity bound on x where no joint moves

// the tables of a call, passed by value
struct ToppView {
  int dof, max_waypoints, grid_per_segment, min_grid, max_samples;
  int ncap;  // grid stride - 1: max(min_grid, grid_per_segment * (max_waypoints - 1))
  double step;
  double vmax[kToppDof], amax[kToppDof];
};

// a row's workspace: M [max_waypoints][dof], K / x / t [ncap + 1]
struct ToppRowBufs {
  double *M, *K, *x, *t;
};

struct ToppSerial {
  static MPG_INLINE int lane() { return 0; }
  static MPG_INLINE int lanes() { return 1; }
  static MPG_INLINE double wmin(double v) { return v; }
  static MPG_INLINE void sync() {}
};

MPG_INLINE bool topp_finite(double v) { return v - v == 0.0; }
MPG_INLINE double topp_min(double a, double b) { return b < a ? b : a; }
// a candidate bound on x: NaN counts as 0
MPG_INLINE double topp_bound(double best, double c) { return c == c ? topp_min(best, c) : 0.0; }

MPG_INLINE int topp_grid(const ToppView& v, int n) {
  const int g = v.grid_per_segment * (n - 1);
  return g > v.min_grid ? g : v.min_grid;
}

// The second derivatives M [n][dof] of the C2 cubic spline through q [n][dof]
// at the uniform knots i / (n - 1), not-a-knot ends.  cp: n doubles of scratch
// (the Thomas solve's upper diagonal, the same for every joint).  A lane per
// joint; the sums are each joint's own.
template <class P>
MPG_INLINE void topp_spline(const double* q, int n, int dof, double* M, double* cp) {
  const double h = 1.0 / (double)(n - 1);
  const double h2 = h * h;
  for (int j = P::lane(); j < dof; j += P::lanes()) {
    if (n == 2) {
      M[j] = 0.0;
      M[dof + j] = 0.0;
    } else if (n == 3) {
      const double m = ((q[j] - 2.0 * q[dof + j]) + q[2 * dof + j]) / h2;
      M[j] = m;
      M[dof + j] = m;
      M[2 * dof + j] = m;
    } else {
      // rows 1 and n - 2: 6 M_i = rhs_i; between: M_{i-1} + 4 M_i + M_{i+1} = rhs_i
      double c = 0.0, d = 0.0;
      for (int i = 1; i <= n - 2; ++i) {
        const double rhs =
            6.0 * ((q[(size_t)(i - 1) * dof + j] - 2.0 * q[(size_t)i * dof + j]) + q[(size_t)(i + 1) * dof + j]) / h2;
        const bool end = i == 1 || i == n - 2;
        const double a = end ? 0.0 : 1.0, b = end ? 6.0 : 4.0, cc = end ? 0.0 : 1.0;
        const double den = b - a * c;
        d = (rhs - a * d) / den;
        c = cc / den;
        if (j == 0) cp[i] = c;
        M[(size_t)i * dof + j] = d;
      }
    }
  }
  P::sync();
  if (n < 4) return;
  for (int j = P::lane(); j < dof; j += P::lanes()) {
    double m = M[(size_t)(n - 2) * dof + j];
    for (int i = n - 3; i >= 1; --i) {
      m = M[(size_t)i * dof + j] - cp[i] * m;
      M[(size_t)i * dof + j] = m;
    }
    M[j] = 2.0 * M[dof + j] - M[2 * dof + j];
    M[(size_t)(n - 1) * dof + j] = 2.0 * M[(size_t)(n - 2) * dof + j] - M[(size_t)(n - 3) * dof + j];
  }
  P::sync();
}

// joint j of the spline at s: value, first and second derivative (the segment: min(floor(s (n - 1)), n - 2))
MPG_INLINE void topp_spline_eval(const double* q, const double* M, int n, int dof, int j, double s, double* val,
                                 double* d1, double* d2) {
  const double h = 1.0 / (double)(n - 1);
  int i = (int)(s * (double)(n - 1));
  i = i > n - 2 ? n - 2 : (i < 0 ? 0 : i);
  const double s0 = (double)i / (double)(n - 1), s1 = (double)(i + 1) / (double)(n - 1);
  const double a = s1 - s, b = s - s0;
  const double q0 = q[(size_t)i * dof + j], q1 = q[(size_t)(i + 1) * dof + j];
  const double m0 = M[(size_t)i * dof + j], m1 = M[(size_t)(i + 1) * dof + j];
  const double h6 = 6.0 * h;
  *val = ((m0 * ((a * a) * a)) / h6 + (m1 * ((b * b) * b)) / h6) + ((q0 / h - (m0 * h) / 6.0) * a + (q1 / h - (m1 * h) / 6.0) * b);
  *d1 = ((m1 * (b * b)) / (2.0 * h) - (m0 * (a * a)) / (2.0 * h)) + ((q1 - q0) / h - ((m1 - m0) * h) / 6.0);
  *d2 = (m0 * a + m1 * b) / h;
}

// The constraint rows of interval k, lo <= cu u + cx x <= hi with cu >= 0 (a
// row with cu < 0 is negated), into rows [4][kToppRows] as (cu, cx, lo, hi):
// 0 .. dof - 1 the acceleration at k, dof .. 2 dof - 1 the acceleration at k + 1
// of the state x + 2 delta u, 2 dof the continuation into [0, Knext].  Returns
// this lane's share of the velocity bound on x_k (kToppXCap where it has none).
template <class P>
MPG_INLINE double topp_rows(const ToppView& v, const double* q, const double* M, int n, int N, int k, double Knext,
                            double* rows) {
  const int dof = v.dof, R = 2 * dof + 1;
  const double delta = 1.0 / (double)N, d2 = 2.0 * delta;
  double xb = kToppXCap;
  for (int e = P::lane(); e < R; e += P::lanes()) {
    double cu, cx, lo, hi;
    if (e == 2 * dof) {
      cu = d2, cx = 1.0, lo = 0.0, hi = Knext;
    } else {
      const bool next = e >= dof;
      const int j = next ? e - dof : e;
      double val, qp, qpp;
      topp_spline_eval(q, M, n, dof, j, (double)(next ? k + 1 : k) / (double)N, &val, &qp, &qpp);
      cu = next ? qp + d2 * qpp : qp;
      cx = qpp;
      lo = -v.amax[j];
      hi = v.amax[j];
      if (!next && qp != 0.0) {
        const double r = v.vmax[j] / qp;
        xb = topp_bound(xb, r * r);
      }
      if (cu < 0.0) {
        const double t = lo;
        cu = -cu, cx = -cx, lo = -hi, hi = -t;
      }
    }
    rows[e] = cu;
    rows[kToppRows + e] = cx;
    rows[2 * kToppRows + e] = lo;
    rows[3 * kToppRows + e] = hi;
  }
  P::sync();
  return xb;
}

// K_k: the largest x in [0, xmax_k] for which some u satisfies every row, u
// eliminated by Fourier-Motzkin.  The lower bound on u of row i and the upper
// bound of row j give (cx_j cu_i - cx_i cu_j) x <= hi_j cu_i - lo_i cu_j; a row
// without u bounds x itself.  x = 0, u = 0 satisfies every row, so only the
// upper bounds on x can bind.  xb: topp_rows' return.
template <class P>
MPG_INLINE double topp_controllable(int dof, const double* rows, double xb) {
  const int R = 2 * dof + 1;
  const double *cu = rows, *cx = rows + kToppRows, *lo = rows + 2 * kToppRows, *hi = rows + 3 * kToppRows;
  double best = xb;
  for (int p = P::lane(); p < R * R; p += P::lanes()) {
    const int i = p / R, j = p - i * R;
    if (i == j) {
      if (cu[i] == 0.0) {
        if (cx[i] > 0.0) best = topp_bound(best, hi[i] / cx[i]);
        else if (cx[i] < 0.0) best = topp_bound(best, lo[i] / cx[i]);
        else if (!(cx[i] == 0.0)) best = 0.0;
      } else if (!(cu[i] > 0.0)) {
        best = 0.0;  // NaN
      }
      continue;
    }
    if (!(cu[i] > 0.0) || !(cu[j] > 0.0)) continue;
    const double coef = cx[j] * cu[i] - cx[i] * cu[j];
    const double rhs = hi[j] * cu[i] - lo[i] * cu[j];
    if (coef > 0.0) best = topp_bound(best, rhs / coef);
    else if (!(coef <= 0.0)) best = 0.0;
  }
  best = P::wmin(best);
  P::sync();  // the rows are free again
  return best > 0.0 ? best : 0.0;
}

// the largest u the acceleration rows allow at x.  The continuation row is the
// caller's min(x + 2 delta u, Knext): the same bound, and x_{k+1} = Knext
// exactly where it binds.
template <class P>
MPG_INLINE double topp_max_u(int dof, const double* rows, double x) {
  const int R = 2 * dof;
  const double *cu = rows, *cx = rows + kToppRows, *hi = rows + 3 * kToppRows;
  double best = 1e300;
  for (int r = P::lane(); r < R; r += P::lanes())
    if (cu[r] > 0.0) best = topp_min(best, (hi[r] - cx[r] * x) / cu[r]);
  best = P::wmin(best);
  P::sync();
  return best;
}

// One whole row: the spline's moments, the controllable sets K (backward), the
// profile x (forward), the times t, all to b with the slots past the row's grid
// repeating the last value.  rows: 4 * kToppRows doubles every lane sees (LDS in
// the kernel).  Returns the MPG_TOPP_* status; *duration and *n_samples as
// mpg_topp_batch states them.  Every lane returns the same values.
template <class P>
MPG_INLINE int topp_row(const ToppView& v, const double* q, int n, const ToppRowBufs& b, double* rows, double* duration,
                        int* n_samples) {
  const int dof = v.dof, stride = v.ncap + 1;
  *duration = 0.0;
  *n_samples = 0;
  n = n > v.max_waypoints ? v.max_waypoints : n;
  int st = 0;
  if (n < 2) {
    st = MPG_TOPP_NO_PATH;
  } else {
    double same = 1.0;  // 0: some value differs from the first waypoint's
    for (int e = P::lane(); e < n * dof; e += P::lanes()) {
      double a = q[e], c = q[e % dof];
      uint64_t ua, uc;
      memcpy(&ua, &a, 8);
      memcpy(&uc, &c, 8);
      if (ua != uc) same = 0.0;
    }
    if (P::wmin(same) != 0.0) st = MPG_TOPP_ZERO_LENGTH;
  }
  if (st) {
    for (int k = P::lane(); k < stride; k += P::lanes()) b.K[k] = 0.0, b.x[k] = 0.0, b.t[k] = 0.0;
    P::sync();
    return st;
  }
  const int N = topp_grid(v, n);
  const double delta = 1.0 / (double)N, d2 = 2.0 * delta;
  topp_spline<P>(q, n, dof, b.M, b.K);  // K is free until the backward pass
  double Kn = 0.0;
  if (P::lane() == 0) b.K[N] = 0.0;
  for (int k = N - 1; k >= 0; --k) {
    const double xb = topp_rows<P>(v, q, b.M, n, N, k, Kn, rows);
    Kn = topp_controllable<P>(dof, rows, xb);
    if (P::lane() == 0) b.K[k] = Kn;
  }
  P::sync();
  double x = 0.0, t = 0.0;
  bool stalled = false;
  if (P::lane() == 0) b.x[0] = 0.0, b.t[0] = 0.0;
  for (int k = 0; k < N; ++k) {
    const double Knext = b.K[k + 1];
    topp_rows<P>(v, q, b.M, n, N, k, Knext, rows);
    const double u = topp_max_u<P>(dof, rows, x);
    double xn = x + d2 * u;
    xn = xn > 0.0 ? xn : 0.0;  // NaN: 0
    xn = topp_min(xn, Knext);
    stalled = stalled || (x == 0.0 && xn == 0.0);
    t = t + d2 / (sqrt(x) + sqrt(xn));
    x = xn;
    if (P::lane() == 0) b.x[k + 1] = x, b.t[k + 1] = t;
  }
  for (int k = N + 1 + P::lane(); k < stride; k += P::lanes()) b.K[k] = 0.0, b.x[k] = x, b.t[k] = t;
  P::sync();
  if (stalled || !topp_finite(t)) return MPG_TOPP_STALLED;
  *duration = t;
  const double md = t / v.step;
  if (md >= (double)v.max_samples + 1.0) return MPG_TOPP_OK | MPG_TOPP_TRUNCATED;
  *n_samples = (int)md;
  return MPG_TOPP_OK;
}

// Sample slot i of a row: time, position, velocity, acceleration [dof].  m =
// the row's n_samples; slots past it repeat the last sample, a row without
// samples holds its first waypoint and zeros.
MPG_INLINE void topp_sample(const ToppView& v, const double* q, int n, const ToppRowBufs& b, double duration, int m,
                            int i, double* time, double* pos, double* vel, double* acc) {
  const int dof = v.dof;
  if (m <= 0) {
    *time = 0.0;
    for (int j = 0; j < dof; ++j) pos[j] = q[j], vel[j] = 0.0, acc[j] = 0.0;
    return;
  }
  n = n > v.max_waypoints ? v.max_waypoints : n;
  i = i < m ? i : m - 1;
  const int N = topp_grid(v, n);
  const double t = m > 1 ? ((double)i * duration) / (double)(m - 1) : 0.0;
  int lo = 0, hi = N - 1;  // the largest k <= N - 1 with t_k <= t
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (b.t[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  const int k = lo;
  const double delta = 1.0 / (double)N;
  const double sk = (double)k / (double)N, sk1 = (double)(k + 1) / (double)N;
  const double tau = t - b.t[k];
  const double sq = sqrt(b.x[k]);
  const double udd = (b.x[k + 1] - b.x[k]) / (2.0 * delta);
  const double sd = sq + udd * tau;
  double s = (sk + sq * tau) + (0.5 * udd) * (tau * tau);
  s = s < sk ? sk : (s > sk1 ? sk1 : s);
  *time = t;
  for (int j = 0; j < dof; ++j) {
    double val, qp, qpp;
    topp_spline_eval(q, b.M, n, dof, j, s, &val, &qp, &qpp);
    pos[j] = val;
    vel[j] = qp * sd;
    acc[j] = qp * udd + qpp * (sd * sd);
  }
}

}  // namespace mpg
