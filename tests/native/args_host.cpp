// Test shim: the batch entry points' shared argument checks and launch set-up
// (mplib_amd/csrc/mpg_args_host.h) behind a C interface for
// tests/test_args_host.py.  With -DARGS_HOST_MAIN the file is a stand-alone
// program that walks the same cases (for a sanitizer build); it prints
// "ok <checks>" or the first failure and exits 1.  Not part of the product.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../mplib_amd/csrc/mpg_args_host.h"

namespace {
struct Range {  // the sampler's SampleRange
  double lo[64], hi[64];
};
struct Tables {  // mpg_world::IkTables, as fill_ik_view reads it
  const int *chain_start, *chain_len, *chain_joints, *joint_q_source;
  const double *lo, *hi;
  const unsigned char* kind;
};
}  // namespace

extern "C" {

int args_mem_ok(int mem) { return mpg_args::mem_ok(mem); }

int args_check_pose7(const double* p7, long count, double tol) { return mpg_args::check_pose7(p7, (size_t)count, tol); }

// the message's length; out holds at most cap - 1 characters of it
int args_pose_message(int fault, const char* what, char* out, int cap) {
  const std::string m = mpg_args::pose_message((mpg_args::PoseFault)fault, what);
  std::snprintf(out, (size_t)cap, "%s", m.c_str());
  return (int)m.size();
}

int args_check_free_columns(const double* rows, long n, int n_links, int n_free, double tol) {
  return mpg_args::check_free_columns(rows, n, n_links, n_free, tol);
}

const char* args_check_free_args(const double* free_pose, long free_rows, long n, int n_free) {
  return mpg_args::check_free_args(free_pose, free_rows, n, n_free);
}

// lo_out / hi_out [64]: what the range holds afterwards (zero past dof)
const char* args_fill_sample_range(const double* lower, const double* upper, int dof, double* lo_out, double* hi_out) {
  Range r{};
  const char* why = mpg_args::fill_sample_range(r, lower, upper, dof);
  std::memcpy(lo_out, r.lo, sizeof(r.lo));
  std::memcpy(hi_out, r.hi, sizeof(r.hi));
  return why;
}

// head: link, cs, cl; the arrays as IkView holds them
void args_fill_ik_view(const int* chain_start, const int* chain_len, const int* chain_joints, const int* joint_q_source,
                       const double* lo, const double* hi, const unsigned char* kind, int link, int dof,
                       const unsigned char* mask, int* head, unsigned char* move, unsigned char* kind_out,
                       unsigned char* bounded, unsigned char* frozen, double* lo_out, double* hi_out) {
  mpg::IkView iv{};
  mpg_args::fill_ik_view(iv, Tables{chain_start, chain_len, chain_joints, joint_q_source, lo, hi, kind}, link, dof, mask);
  head[0] = iv.link, head[1] = iv.cs, head[2] = iv.cl;
  std::memcpy(move, iv.move, sizeof(iv.move));
  std::memcpy(kind_out, iv.kind, sizeof(iv.kind));
  std::memcpy(bounded, iv.bounded, sizeof(iv.bounded));
  std::memcpy(frozen, iv.frozen, sizeof(iv.frozen));
  std::memcpy(lo_out, iv.lo, sizeof(iv.lo));
  std::memcpy(hi_out, iv.hi, sizeof(iv.hi));
}

unsigned long args_ik_lds_bytes(int cl) { return (unsigned long)mpg_args::ik_lds_bytes(cl); }

}  // extern "C"

#ifdef ARGS_HOST_MAIN
namespace {
int g_checks = 0;
#define EXPECT(cond)                                                \
  do {                                                              \
    ++g_checks;                                                     \
    if (!(cond)) {                                                  \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);         \
      return 1;                                                     \
    }                                                               \
  } while (0)

int run() {
  using namespace mpg_args;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double tol = 1e-6;
  // poses: heap arrays of the exact size, so an overrun is the sanitizer's to see
  // 1 +- 1e-6: the double 0.999999 lies 2.9e-17 outside the tolerance (1 - 0.999999 is exact and larger than
  // the double 1e-6), so the lower norm is its neighbour towards 1; the double 1.000001 lies inside
  for (const double norm : {std::nextafter(1.0 - 1e-6, 1.0), 1.0, 1.0 + 1e-6}) {
    std::vector<double> p{0.1, 0.2, 0.3, norm, 0, 0, 0};
    EXPECT(check_pose7(p.data(), 1, tol) == POSE_OK);
  }
  for (const double norm : {1.0 - 2e-6, 1.0 + 2e-6}) {
    std::vector<double> p{0.1, 0.2, 0.3, 0, norm, 0, 0};
    EXPECT(check_pose7(p.data(), 1, tol) == POSE_NORM);
  }
  for (int slot = 0; slot < 7; ++slot)
    for (const double bad : {nan, inf, -inf}) {
      std::vector<double> p{0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0};
      p[7 + slot] = bad;  // the second pose
      EXPECT(check_pose7(p.data(), 1, tol) == POSE_OK);
      EXPECT(check_pose7(p.data(), 2, tol) == POSE_NONFINITE);
    }
  EXPECT(check_pose7(nullptr, 0, tol) == POSE_OK);
  EXPECT(pose_message(POSE_NONFINITE, "goal pose") == "non-finite goal pose");
  EXPECT(pose_message(POSE_NORM, "free pose").find("unit norm") != std::string::npos);
  {  // 2 rows of 3 links, the last one free: only its columns are looked at
    std::vector<double> rows(2 * 3 * 7, nan);
    for (int i = 0; i < 2; ++i) {
      double* f = rows.data() + (i * 3 + 2) * 7;
      for (int c = 0; c < 7; ++c) f[c] = c == 3 ? 1.0 : 0.0;
    }
    EXPECT(check_free_columns(rows.data(), 2, 3, 1, tol) == POSE_OK);
    EXPECT(check_free_columns(rows.data(), 2, 3, 0, tol) == POSE_OK);
    rows[(1 * 3 + 2) * 7 + 3] = 0.5;
    EXPECT(check_free_columns(rows.data(), 1, 3, 1, tol) == POSE_OK);
    EXPECT(check_free_columns(rows.data(), 2, 3, 1, tol) == POSE_NORM);
  }
  const double pose[7] = {0, 0, 0, 1, 0, 0, 0};
  const long n = 5;
  EXPECT(!check_free_args(pose, 1, n, 2) && !check_free_args(pose, n, n, 2));
  for (const long bad : {0l, 2l, n + 1}) EXPECT(std::strstr(check_free_args(pose, bad, n, 2), "free_rows"));
  EXPECT(!check_free_args(nullptr, 0, n, 0) && !check_free_args(nullptr, 3, n, 2));
  EXPECT(std::strstr(check_free_args(pose, 1, n, 0), "no free frames"));
  {
    Range r{};
    std::vector<double> lo(64, -1.0), hi(64, 1.0);
    EXPECT(!fill_sample_range(r, nullptr, nullptr, 0));
    EXPECT(!fill_sample_range(r, lo.data(), hi.data(), 64) && r.lo[63] == -1.0 && r.hi[63] == 1.0);
    EXPECT(fill_sample_range(r, lo.data(), hi.data(), 65) && fill_sample_range(r, lo.data(), hi.data(), -1));
    hi[2] = -1.0;  // lo == hi
    EXPECT(!fill_sample_range(r, lo.data(), hi.data(), 3));
    hi[2] = -1.5;  // lo > hi
    EXPECT(std::strstr(fill_sample_range(r, lo.data(), hi.data(), 3), "lower <= upper"));
    EXPECT(!fill_sample_range(r, lo.data(), hi.data(), 2));
    hi[1] = inf;
    EXPECT(fill_sample_range(r, lo.data(), hi.data(), 2));
  }
  {  // link 1 under joints 1, 2 (a mimic: no slot of its own), 3; slot 1 has no lower limit
    const std::vector<int> cs{0, 1}, cl{1, 3}, cj{1, 1, 2, 3}, src{0, -1, 1};
    const std::vector<double> lo{-1.0, -inf}, hi{1.0, 2.0};
    const std::vector<unsigned char> kind{1, 2}, mask{0, 1};
    const Tables t{cs.data(), cl.data(), cj.data(), src.data(), lo.data(), hi.data(), kind.data()};
    mpg::IkView iv{};
    fill_ik_view(iv, t, 1, 2, nullptr);
    EXPECT(iv.link == 1 && iv.cs == 1 && iv.cl == 3);
    EXPECT(iv.move[0] == 1 && iv.move[1] == 0 && iv.move[2] == 1);
    EXPECT(iv.kind[0] == 1 && iv.kind[1] == 2 && iv.bounded[0] == 1 && iv.bounded[1] == 0);
    EXPECT(iv.frozen[0] == 0 && iv.frozen[1] == 0 && iv.lo[1] == -inf && iv.hi[1] == 2.0);
    fill_ik_view(iv, t, 1, 2, mask.data());
    EXPECT(iv.frozen[0] == 0 && iv.frozen[1] == 1 && iv.move[0] == 1 && iv.move[1] == 0 && iv.move[2] == 0);
  }
  EXPECT(ik_lds_bytes(1) == 4236 && ik_lds_bytes(0) == 4236 && ik_lds_bytes(7) == 7 * 4236);
  EXPECT(mem_ok(MPG_MEM_HOST) && mem_ok(MPG_MEM_DEVICE) && !mem_ok(-1) && !mem_ok(2));
  return 0;
}
}  // namespace

int main() {
  if (run()) return 1;
  std::printf("ok %d\n", g_checks);
  return 0;
}
#endif
