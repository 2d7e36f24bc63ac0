// Test shim: compiles the product's screw-motion header
// (mplib_amd/csrc/mpg_screw.h, the code screw_kernel runs) for the host with
// g++ -ffp-contract=off, so tests can compare it with a numpy restatement of
// planner.py's plan_screw on a machine without a GPU.  Not part of the product.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../mplib_amd/csrc/mpg_screw.h"

namespace {

struct HostWorld {
  mpg::DevWorld w{};
  std::vector<int> cs, cl, cj;
  HostWorld(int nj, const int* jt, const int* jp, const int* jqs, const double* jqc, const double* jax,
            const double* jpl, int dof, int n_links, const int* lp, const double* lpl) {
    w.nj = nj; w.dof = dof; w.n_links = n_links;
    w.joint_type = jt; w.joint_parent = jp; w.joint_q_source = jqs; w.joint_q_const = jqc;
    w.joint_axis = jax; w.joint_place = jpl; w.link_parent = lp; w.link_place = lpl;
    for (int l = 0; l < n_links; ++l) {  // the chains as mpg_world_create builds them
      std::vector<int> c;
      for (int j = lp[l]; j > 0; j = jp[j - 1]) c.push_back(j);
      std::reverse(c.begin(), c.end());
      cs.push_back((int)cj.size());
      cl.push_back((int)c.size());
      cj.insert(cj.end(), c.begin(), c.end());
    }
    w.link_chain_start = cs.data(); w.link_chain_len = cl.data(); w.chain_joints = cj.data();
  }
};

}  // namespace

extern "C" {

// n transforms (R row-major [9], p [3]) -> twist [6], branch (SCREW_EXP_*)
void screw_host_exp(const double* T12, long n, double* tw, int* branch) {
  for (long i = 0; i < n; ++i) branch[i] = mpg::screw_exp_coordinate(mpg::load_se3(T12 + 12 * i), tw + 6 * i);
}

// n rows of mpg_screw_batch's integration (no collide pass), the view built as
// mpg_screw_batch builds it.  1: refused.
int screw_host_rows(int nj, const int* jt, const int* jp, const int* jqs, const double* jqc, const double* jax,
                    const double* jpl, int dof, int n_links, const int* lp, const double* lpl, int link,
                    const double* lo, const double* hi, const double* goal, const double* q_start, long n,
                    double qpos_step, int max_waypoints, double* path, int* count, unsigned char* status) {
  HostWorld H(nj, jt, jp, jqs, jqc, jax, jpl, dof, n_links, lp, lpl);
  if (link < 0 || link >= n_links || H.cl[link] > mpg::kIkChain || dof > mpg::kIkDof || max_waypoints < 2) return 1;
  mpg::ScrewView sv{};
  mpg::IkView& iv = sv.iv;
  iv.link = link;
  iv.cs = H.cs[link];
  iv.cl = H.cl[link];
  sv.qpos_step = qpos_step;
  sv.max_waypoints = max_waypoints;
  for (int d = 0; d < dof; ++d) {
    iv.lo[d] = lo[d];
    iv.hi[d] = hi[d];
    iv.bounded[d] = std::isfinite(lo[d]) && std::isfinite(hi[d]);
    sv.offchain[d] = 1;
  }
  int moving = 0;
  for (int k = 0; k < iv.cl; ++k) {
    const int src = jqs[H.cj[iv.cs + k] - 1];
    iv.move[k] = src >= 0;
    if (src >= 0) {
      sv.offchain[src] = 0;
      ++moving;
    }
  }
  if (moving < 6) return 1;
  std::vector<double> lane(mpg::kIkSlot * (size_t)std::max(iv.cl, 1));
  const mpg::IkLane L{lane.data(), 1};
  const mpg::IkJointsWorld jw{H.w, iv};
  for (long i = 0; i < n; ++i)
    status[i] = (unsigned char)mpg::screw_row(H.w, jw, sv, L, goal + 7 * i, q_start + (size_t)i * dof,
                                              path + (size_t)i * max_waypoints * dof, count + i);
  return 0;
}

}
