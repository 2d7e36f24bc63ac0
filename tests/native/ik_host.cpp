// Test shim: compiles the product's IK header (mplib_amd/csrc/mpg_ik.h, the
// code ik_clik_kernel / ik_finish_kernel run) for the host with g++
// -ffp-contract=off, so tests can compare it with compute_IK_CLIK and a numpy
// restatement of planner.py on a machine without a GPU.  Not part of the product.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../mplib_amd/csrc/mpg_ik.h"

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

mpg::IkView view(const HostWorld& H, int link, const double* lo, const double* hi, const unsigned char* kind,
                 const unsigned char* mask) {
  mpg::IkView iv{};
  iv.link = link;
  iv.cs = H.cs[link];
  iv.cl = H.cl[link];
  for (int d = 0; d < H.w.dof; ++d) {
    iv.kind[d] = kind[d];
    iv.lo[d] = lo[d];
    iv.hi[d] = hi[d];
    iv.bounded[d] = std::isfinite(lo[d]) && std::isfinite(hi[d]);
    iv.frozen[d] = mask && mask[d];
  }
  for (int k = 0; k < iv.cl; ++k) {
    const int src = H.w.joint_q_source[H.cj[iv.cs + k] - 1];
    iv.move[k] = src >= 0 && !iv.frozen[src];
  }
  return iv;
}

}  // namespace

extern "C" {

// n rows of mpg_ik_batch's steps 1 and 2 (and the threshold bit), one goal per row
int ik_host_rows(int nj, const int* jt, const int* jp, const int* jqs, const double* jqc, const double* jax,
                 const double* jpl, int dof, int n_links, const int* lp, const double* lpl, int link, const double* lo,
                 const double* hi, const unsigned char* kind, const unsigned char* mask, const double* goal,
                 const double* q_init, long n, double eps, int max_iter, double dt, double damp, double threshold,
                 double* q_out, unsigned char* status, double* err, int* iters) {
  HostWorld H(nj, jt, jp, jqs, jqc, jax, jpl, dof, n_links, lp, lpl);
  if (link < 0 || link >= n_links || H.cl[link] > mpg::kIkChain || dof > mpg::kIkDof) return 1;
  mpg::IkView iv = view(H, link, lo, hi, kind, mask);
  iv.eps = eps; iv.max_iter = max_iter; iv.dt = dt; iv.damp = damp; iv.threshold = threshold;
  std::vector<double> lane(mpg::kIkSlot * (size_t)std::max(iv.cl, 1));
  const mpg::IkLane L{lane.data(), 1};
  for (long i = 0; i < n; ++i) {
    double* q = q_out + i * dof;
    std::copy(q_init + i * dof, q_init + (i + 1) * dof, q);
    int st = mpg::ik_solve_row(H.w, iv, L, goal + 7 * i, q, err + 6 * i, iters + i);
    st |= mpg::ik_finish_row(H.w, iv, goal + 7 * i, q);
    status[i] = (unsigned char)st;
  }
  return 0;
}

// check_joint_limit of n rows of nd slots: q wrapped in place, fail[i * nd + d] per slot
void ik_host_wrap(int nd, const double* lo, const double* hi, const unsigned char* kind, double* q, long n,
                  unsigned char* fail) {
  mpg::IkView iv{};
  for (int d = 0; d < nd; ++d) {
    iv.kind[d] = kind[d];
    iv.lo[d] = lo[d];
    iv.hi[d] = hi[d];
    iv.bounded[d] = std::isfinite(lo[d]) && std::isfinite(hi[d]);
  }
  for (long i = 0; i < n; ++i)
    for (int d = 0; d < nd; ++d) fail[i * nd + d] = mpg::ik_wrap_limit(iv, d, q[i * nd + d]);
}

double ik_host_distance_6d(const double* a, const double* b) { return mpg::ik_distance_6d(a, b); }

}
