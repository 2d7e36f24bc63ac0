// Test shim: compiles the product's time-parametrisation header
// (mplib_amd/csrc/mpg_topp.h, the code topp_row_kernel and topp_sample_kernel
// run) and mpg_topp_batch's argument checks (mpg_args_host.h) for the host with
// g++ -ffp-contract=off, so tests can compare them with a numpy restatement on a
// machine without a GPU.  Not part of the product.
#include <cstdio>
#include <vector>

#include "../../mplib_amd/csrc/mpg_args_host.h"

extern "C" {

// The argument checks of mpg_topp_batch: 0, or MPG_E_INVALID / MPG_E_UNSUPPORTED with the reason in msg.
// path / n_waypoints NULL: the host-memory row checks are skipped (as for MPG_MEM_DEVICE).
int topp_host_check(int dof, long rows, int max_waypoints, const double* vel, const double* acc, double step,
                    int grid_per_segment, int min_grid, int max_samples, const double* path, const int* n_waypoints,
                    char* msg, int cap) {
  mpg::ToppView v{};
  const mpg_topp_options o{step, grid_per_segment, min_grid, max_samples};
  bool unsupported = false;
  std::string why = mpg_args::fill_topp_view(v, o, dof, rows, max_waypoints, vel, acc, &unsupported);
  int rc = why.empty() ? MPG_OK : (unsupported ? MPG_E_UNSUPPORTED : MPG_E_INVALID);
  if (!rc && path && n_waypoints && rows > 0) {
    why = mpg_args::check_topp_rows(path, n_waypoints, rows, max_waypoints, dof);
    if (!why.empty()) rc = MPG_E_INVALID;
  }
  std::snprintf(msg, (size_t)cap, "%s", why.c_str());
  return rc;
}

// the spline's moments M [n][dof] of q [n][dof]
void topp_host_spline(const double* q, int n, int dof, double* M) {
  std::vector<double> cp((size_t)n + 1);
  mpg::topp_spline<mpg::ToppSerial>(q, n, dof, M, cp.data());
}

// value, first and second derivative [ns][dof] at s [ns]
void topp_host_spline_eval(const double* q, const double* M, int n, int dof, const double* s, int ns, double* val,
                           double* d1, double* d2) {
  for (int i = 0; i < ns; ++i)
    for (int j = 0; j < dof; ++j)
      mpg::topp_spline_eval(q, M, n, dof, j, s[i], val + (size_t)i * dof + j, d1 + (size_t)i * dof + j,
                            d2 + (size_t)i * dof + j);
}

// mpg_topp_batch on the host, without its argument checks: the outputs of the
// call, and the controllable sets grid_k [rows][Ncap + 1].  1: refused.
int topp_host_rows(const double* path, const int* n_waypoints, long rows, int max_waypoints, int dof, const double* vel,
                   const double* acc, double step, int grid_per_segment, int min_grid, int max_samples, double* times,
                   double* position, double* velocity, double* acceleration, int* n_samples, double* duration,
                   unsigned char* status, double* grid_x, double* grid_t, double* grid_k) {
  mpg::ToppView v{};
  const mpg_topp_options o{step, grid_per_segment, min_grid, max_samples};
  bool unsupported = false;
  if (!mpg_args::fill_topp_view(v, o, dof, rows, max_waypoints, vel, acc, &unsupported).empty()) return 1;
  const size_t pstride = (size_t)max_waypoints * dof, gstride = (size_t)v.ncap + 1;
  std::vector<double> M(pstride + 1), R(4 * mpg::kToppRows);
  for (long r = 0; r < rows; ++r) {
    const mpg::ToppRowBufs b{M.data(), grid_k + r * gstride, grid_x + r * gstride, grid_t + r * gstride};
    const double* q = path + r * pstride;
    double dur;
    int m;
    status[r] = (unsigned char)mpg::topp_row<mpg::ToppSerial>(v, q, n_waypoints[r], b, R.data(), &dur, &m);
    duration[r] = dur;
    n_samples[r] = m;
    for (int i = 0; i < max_samples; ++i) {
      const size_t slot = (size_t)r * max_samples + i;
      mpg::topp_sample(v, q, n_waypoints[r], b, dur, m, i, times + slot, position + slot * dof, velocity + slot * dof,
                       acceleration + slot * dof);
    }
  }
  return 0;
}

}
