// Test shim: the cull's lookup grids (mpg_broadphase.h bp_grid_*) compiled for
// the host, for tests/test_cull_grid.py; with -DCULL_GRID_MAIN a program of
// its own (sanitizer builds).  Not part of the product.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../mplib_amd/csrc/mpg_broadphase.h"

namespace {
struct Grid {
  mpg::BpGridPlan plan;
  std::vector<int> cand_slot;  // per candidate: its record, or -1 when it went back to the loop
  std::vector<float> gf, sobj;
  std::vector<int> gi;
  std::vector<uint32_t> words;
};
}  // namespace

extern "C" {
// nobj candidates (box lo / hi [nobj][3], radius r, np[i] partners listed in
// sid), ns statics given as the cull's fp32 records sobj[ns][BS_STRIDE];
// coordinate bound X and cull margin as world creation passes them
void* grid_new(int nobj, const double* lo, const double* hi, const double* r, const int* np, const int* sid, int ns,
               const float* sobj, double X, double margin, long long budget) {
  Grid* G = new Grid();
  G->sobj.assign(sobj, sobj + (size_t)mpg::BS_STRIDE * ns);
  int at = 0;
  for (int i = 0; i < nobj; ++i) {
    mpg::BpGridObj o;
    o.m = i;
    o.r = r[i];
    for (int k = 0; k < 3; ++k) o.lo[k] = lo[3 * i + k], o.hi[k] = hi[3 * i + k];
    for (int k = 0; k < np[i]; ++k) o.sid.push_back(sid[at + k]), o.pair.push_back(at + k);
    at += np[i];
    if (mpg::bp_grid_candidate(o.sid.size())) G->plan.obj.push_back(o);
  }
  mpg::bp_grid_choose(G->plan, X, margin, budget);
  G->plan.sobb.assign((size_t)15 * ns, 0.0);
  for (int s = 0; s < ns; ++s) {
    const float* rec = sobj + mpg::BS_STRIDE * s;
    double* S = G->plan.sobb.data() + 15 * (size_t)s;
    for (int k = 0; k < 3; ++k) S[k] = rec[mpg::BS_C + k], S[12 + k] = rec[mpg::BS_E + k];
    for (int k = 0; k < 9; ++k) S[3 + k] = rec[mpg::BS_R + k];
  }
  G->cand_slot.assign(nobj, -1);
  std::vector<int> E;
  int e = 0;
  for (size_t i = 0; i < G->plan.obj.size(); ++i) {
    G->cand_slot[G->plan.obj[i].m] = (int)i;
    E.push_back(e);
    e += (int)G->plan.obj[i].sid.size();
  }
  E.push_back(e);
  mpg::bp_grid_records(G->plan, E, G->gf, G->gi);
  mpg::bp_grid_fill(G->plan, G->words);
  return G;
}
void grid_free(void* g) { delete (Grid*)g; }
double grid_h(void* g) { return ((Grid*)g)->plan.h; }
double grid_cell_pad(void* g) { return ((Grid*)g)->plan.cell_pad; }
long long grid_cells(void* g) { return ((Grid*)g)->plan.cells; }
int grid_slot(void* g, int cand) { return ((Grid*)g)->cand_slot[cand]; }
void grid_dims(void* g, int slot, int* n, float* o) {
  const mpg::BpGridObj& ob = ((Grid*)g)->plan.obj[slot];
  for (int k = 0; k < 3; ++k) n[k] = ob.n[k], o[k] = ob.o[k];
}
unsigned long long grid_hash(void* g) {  // FNV-1a of the words and the records
  const Grid* G = (Grid*)g;
  unsigned long long h = 1469598103934665603ull;
  auto eat = [&](const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  };
  eat(G->words.data(), 4 * G->words.size());
  eat(G->gf.data(), 4 * G->gf.size());
  eat(G->gi.data(), 4 * G->gi.size());
  return h;
}
// what the cull's lookup yields for n fp32 centres of record `slot`: the cell
// word, or every partner bit outside the grid; cell[i] = the cell or -1
void grid_lookup(void* g, int slot, const float* c, long n, uint32_t* out, int* cell) {
  const Grid* G = (Grid*)g;
  const float* gf = G->gf.data() + mpg::GF_STRIDE * slot;
  const int* gi = G->gi.data() + mpg::GI_STRIDE * slot;
  for (long i = 0; i < n; ++i) {
    const int k = mpg::bp_grid_cell(gf, gi, c + 3 * i);
    out[i] = k < 0 ? (uint32_t)gi[mpg::GI_FULL] : G->words[k];
    if (cell) cell[i] = k;
  }
}
// the bits the product's fp32 sphere test keeps for the same centres
void grid_sphere(void* g, int slot, const float* c, long n, float margin, uint32_t* out) {
  const Grid* G = (Grid*)g;
  const mpg::BpGridObj& ob = G->plan.obj[slot];
  for (long i = 0; i < n; ++i) {
    uint32_t kb = 0u;
    for (size_t k = 0; k < ob.sid.size(); ++k)
      kb |= (uint32_t)!mpg::fsphere_obb_separated(c + 3 * i, (float)ob.r, G->sobj.data() + mpg::BS_STRIDE * ob.sid[k], margin)
            << k;
    out[i] = kb;
  }
}
float grid_widen(double v) { return mpg::widen(v); }
}

#ifdef CULL_GRID_MAIN
// builder + lookup on a small random world, for sanitizer runs: every sphere
// keep must be a lookup keep
int main() {
  std::mt19937 rng(7);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  const int ns = 33, nobj = 4;
  std::vector<float> sobj((size_t)mpg::BS_STRIDE * ns, 0.f);
  for (int s = 0; s < ns; ++s) {
    float* r = sobj.data() + mpg::BS_STRIDE * s;
    for (int k = 0; k < 3; ++k) r[mpg::BS_C + k] = (float)U(rng), r[mpg::BS_E + k] = (float)(0.02 + 0.1 * std::fabs(U(rng)));
    const double a = 3.0 * U(rng), cs = std::cos(a), sn = std::sin(a);
    const float R[9] = {(float)cs, (float)-sn, 0.f, (float)sn, (float)cs, 0.f, 0.f, 0.f, 1.f};
    for (int k = 0; k < 9; ++k) r[mpg::BS_R + k] = R[k];
  }
  const double lo[12] = {-1, -1, -1, -0.5, -0.5, 0, 0.1, 0.1, 0.1, -1, -1, -1}, hi[12] = {1, 1, 1, 0.5, 0.5, 1, 0.1, 0.1, 0.1, 1, 1, 1};
  const double r[4] = {0.1, 0.2, 0.05, 0.1};
  const int np[4] = {32, 7, 6, 33};
  std::vector<int> sid;
  for (int i = 0; i < nobj; ++i)
    for (int k = 0; k < np[i]; ++k) sid.push_back(k);
  void* g = grid_new(nobj, lo, hi, r, np, sid.data(), ns, sobj.data(), 4.0, 0.0186, 1 << 16);
  long bad = 0, n = 0;
  for (int c = 0; c < nobj; ++c) {
    const int slot = grid_slot(g, c);
    if (slot < 0) continue;
    std::vector<float> pts(3 * 20000);
    for (float& v : pts) v = (float)(1.2 * U(rng));
    std::vector<uint32_t> a(20000), b(20000);
    grid_lookup(g, slot, pts.data(), 20000, a.data(), nullptr);
    grid_sphere(g, slot, pts.data(), 20000, 0.0186f, b.data());
    for (int i = 0; i < 20000; ++i) bad += (b[i] & ~a[i]) != 0u, ++n;
  }
  std::printf("cells %lld h %.4f points %ld bad %ld slot33 %d\n", grid_cells(g), grid_h(g), n, bad, grid_slot(g, 3));
  const int ok = bad == 0 && grid_slot(g, 3) < 0 && grid_slot(g, 0) >= 0;
  grid_free(g);
  return ok ? 0 : 1;
}
#endif
