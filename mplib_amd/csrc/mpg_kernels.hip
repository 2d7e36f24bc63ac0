// mpg_kernels.hip -- MI355X (gfx950) kernels and the C ABI of include/mpgpu.h.
//
// Hot path: one batched launch evaluates, per joint configuration,
//   setQposAll(q) -> FK -> getLinkPose quaternion round trip -> collision
//   object transforms (src/articulated_model.cpp:101-127,
//   src/fcl_model.cpp:139-148), then every pair of the world's pair table
//   with fcl::collide semantics for CollisionRequest() (GST_LIBCCD ->
//   ccdMPRIntersect, FCL 0.7.0 / libccd 2.1), then the ACM filter
//   (src/planning_world.cpp:265-274).
//
// Two phases per chunk of configurations (DESIGN.md "Kernels"):
//   A  cull_kernel      lane per configuration: fp32 FK + conservative broad
//                       phase (mpg_broadphase.h) -> survivor bits [word][cfg]
//      (cull also writes the per-tile survivor counts)
//      range_sum / range_scan / scatter: bucket the survivors
//                       into per-pair candidate lists (deterministic, no
//                       global atomics)
//   B  narrow_kernel    wave per 64 candidates of ONE pair: exact fp64 FK of
//                       the two objects' chains + libccd MPR; hull reads are
//                       wave-uniform scalar loads.
// A pair culled in A is separated by more than kBpMargin, so MPR would say
// "no intersection": the output bits equal evaluating every pair.
//
// Everything that decides an output bit (phase B) is fp64 with
// -ffp-contract=off, bit-identical to the reference's operation order.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mpgpu.h"
#include "mpg_math.h"
#include "mpg_fk.h"
#include "mpg_ik.h"
#include "mpg_screw.h"
#include "mpg_rrt.h"
#include "mpg_bucket.h"
#include "mpg_hostpipe.h"
#include "mpg_args_host.h"

using namespace mpg;

namespace {


thread_local std::string g_last_error;

int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define HIP_TRY(expr)                                                                 \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess)                                                             \
      return set_error(MPG_E_HIP, std::string(#expr " failed: ") + hipGetErrorString(_e)); \
  } while (0)

// ---------------------------------------------------------------------------
// FCL GJK objects + libccd MPR
// ---------------------------------------------------------------------------
struct GObj {
  CQ4 rot, rot_inv;  // libccd ccd_quat_t (ccd_real)
  CV3 pos;
  int geom;
  int type;
};

// vertex i of hull `geom` (AoSoA-4 groups: x0..3, y0..3, z0..3)
__device__ __forceinline__ V3 hull_vertex(const DevWorld& w, cptr<double> HV, int geom, int i) {
  const cptr<double> G = HV + 12 * (size_t)(w.geom_gstart[geom] + (i >> 2)) + (i & 3);
  return v3(G[0], G[4], G[8]);
}

// Dot product in Eigen's Vector3d::dot order, as Convex::findExtremeVertex
// evaluates v_C.dot(vertex): (x0*p0 + x1*p1) + x2*p2.
__device__ __forceinline__ double edot(const V3& d, const V3& p) { return (d.x * p.x + d.y * p.y) + d.z * p.z; }

// Convex::findExtremeVertex, linear branch (hulls of <= 32 vertices, or whose
// faces failed FCL's ValidateTopology): argmax dir . vertex (fp64), first
// maximum wins.  The AoSoA groups are padded with copies of the hull's first
// vertex, which can never win the strict '>', so the result equals the
// unpadded scan.  Only for directions without a cell.
__device__ __forceinline__ V3 convex_full_scan(const DevWorld& w, cptr<double> HV, int geom, const V3& dir) {
  const int g0 = w.geom_gstart[geom], ng = w.geom_ng[geom];
  const cptr<double> P = HV + 12 * (size_t)g0;
  double best = -DBL_MAX;
  int bi = 0;
  for (int g = 0; g < ng; ++g) {
    const cptr<double> G = P + 12 * g;
    double dd[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) dd[k] = (dir.x * G[k] + dir.y * G[4 + k]) + dir.z * G[8 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (dd[k] > best) {
        best = dd[k];
        bi = 4 * g + k;
      }
  }
  const cptr<double> B = P + 12 * (bi >> 2) + (bi & 3);
  return v3(B[0], B[4], B[8]);
}

// Convex::findExtremeVertex, neighbour-walk branch [ext FCL 0.7.0
// geometry/shape/convex-inl.h] (hulls of > 32 vertices whose faces passed
// ValidateTopology, oracle/collide_oracle.c support_convex): start at vertex
// 0, scan the current vertex's neighbour list (FindVertexNeighbors: sorted,
// from the faces), step to every unvisited neighbour whose value is >= the
// best so far, until a pass moves nowhere.
//
// Most supports never walk: the direction's cell record settles them
// (walk_cell_fast).  The few that must walk -- a lane or two per wave every
// few MPR steps -- are resolved by the whole wave together, one pending lane
// at a time (wave_walk): per step of the climb the active lanes load the
// current vertex's neighbours and their dot products in parallel and the
// pass's sequential '>=' scan replays from LDS, so a climb costs one memory
// round trip per step instead of one per neighbour, and the per-lane rare path
// no longer holds the other 63 lanes for the length of a serial walk.
constexpr int kWalkWords = kMaxWalkVerts / 64;
struct WalkScratch {  // one per wave (blocks of <= 512 threads)
  uint64_t vis[kWalkWords];
  double dd[64];
  int vi[64];
};

__device__ __forceinline__ WalkScratch& walk_scratch() {
  __shared__ WalkScratch s_walk[8];  // one per wave: 256-thread blocks, the 512-thread latency server
  return s_walk[(threadIdx.x >> 6) & 7];
}

// LDS written by some lanes of this wave, read by others: keep the compiler
// from moving the accesses across (the LDS unit serves one wave in order)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double lane_bcast(double v, int L) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, L);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), L);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// The climb for one (wave-uniform) direction d, by the wave's active lanes
// (rank among nact), from vertex 0 or resumed from a prefix record (pre:
// mpg_hullcells.h WalkPrefix, the state where the host's replay stopped).
// Returns the final vertex index (uniform).
// A hull above kMaxWalkVerts vertices keeps its visited set in one slot of the
// world's global pool (big_vis, zero while free): the wave's first active lane
// claims a free slot (big_busy 0 -> 1), the wave clears the slot's words after
// the climb and releases it.  Holders never wait, so a wave that finds every
// slot taken only spins until one of them finishes.
__device__ __forceinline__ int big_vis_acquire(const DevWorld& w, int rank) {
  int slot = 0;
  if (rank == 0) {
    const int n = w.big_slots;
    int k = (int)((blockIdx.x * 8u + (threadIdx.x >> 6)) % (unsigned)n);
    while (atomicCAS(&w.big_busy[k], 0, 1) != 0) k = k + 1 == n ? 0 : k + 1;
    slot = k;
  }
  // rank 0 is the first active lane
  return __builtin_amdgcn_readfirstlane(slot);
}

__device__ __forceinline__ int wave_walk(const DevWorld& w, cptr<double> HV, int geom, const V3& d, int rank,
                                         int nact, cptr<int> pre) {
  WalkScratch& S = walk_scratch();
  const cptr<int> hd = w.hull_nbr + 2 * w.geom_nbr[geom];
  const int nwords = (w.geom_nvert[geom] + 63) >> 6;
  const bool big = nwords > kWalkWords;  // no cell tables either: pre == nullptr
  const int slot = big ? big_vis_acquire(w, rank) : -1;
  // the visited set: the wave's LDS bitset or the pool slot, one flat pointer
  unsigned long long* vis = big ? w.big_vis + (size_t)slot * w.big_words : (unsigned long long*)S.vis;
  if (big) {
    if (rank == 0) atomicOr(&vis[0], 1ull);  // vertex 0: the start (the slot is zero)
    __threadfence();
  } else {
    for (int j = rank; j < nwords; j += nact)
      S.vis[j] = pre ? (uint64_t)(uint32_t)pre[4 + 2 * j] | ((uint64_t)(uint32_t)pre[5 + 2 * j] << 32) : (j == 0 ? 1ull : 0ull);
  }
  wave_lds_sync();
  int bi = pre ? pre[0] : 0, pv = pre ? pre[1] : 0, k0 = pre ? pre[2] : 0;
  bool keep = pre ? pre[3] != 0 : false, first = true;
  double best = edot(d, hull_vertex(w, HV, geom, bi));
  do {
    const int v = first ? pv : bi;  // the pass scans v's list (v fixed for the pass)
    const int skip = first ? k0 : 0;
    bool moved = first && keep;
    first = false;
    const int start = hd[2 * v] + skip, cnt = hd[2 * v + 1] - skip;
    for (int c0 = 0; c0 < cnt; c0 += nact) {
      const int m = min(cnt - c0, nact);
      if (rank < m) {
        const cptr<double> e = w.nbr_ent + 4 * (size_t)(start + c0 + rank);
        const int vi = (int)e[3];
        const uint64_t bit = 1ull << (vi & 63);
        // test-and-set (a neighbour list has no repeats)
        const bool seen = (atomicOr(&vis[vi >> 6], (unsigned long long)bit) & bit) != 0ull;
        S.vi[rank] = seen ? -1 : vi;
        S.dd[rank] = seen ? 0.0 : (d.x * e[0] + d.y * e[1]) + d.z * e[2];
      }
      wave_lds_sync();
      for (int k = 0; k < m; ++k) {  // the pass's scan, in list order
        const int vi = S.vi[k];
        const double dd = S.dd[k];
        if (vi >= 0 && dd >= best) {
          moved = true;
          bi = vi;
          best = dd;
        }
      }
      wave_lds_sync();
    }
    bi = __builtin_amdgcn_readfirstlane(bi);
    keep = moved;
  } while (keep);
  if (big) {  // leave the slot zero, then free it
    for (int j = rank; j < nwords; j += nact) atomicExch(&vis[j], 0ull);
    __threadfence();
    wave_lds_sync();
    if (rank == 0) atomicExch(&w.big_busy[slot], 0);
  }
  return bi;
}

// true if some neighbour of vertex vi has a dot product strictly above dd: then
// the walk cannot end at vi (every vertex it evaluates is compared with the
// running maximum, which only grows)
__device__ __forceinline__ bool neighbour_beats(const DevWorld& w, cptr<double> HV, int geom, int vi, double dd,
                                                const V3& d) {
  const cptr<int> hd = w.hull_nbr + 2 * (w.geom_nbr[geom] + vi);
  const cptr<double> e = w.nbr_ent + 4 * (size_t)hd[0];
  const int cnt = hd[1];
  for (int k = 0; k < cnt; ++k)
    if ((d.x * e[4 * k] + d.y * e[4 * k + 1]) + d.z * e[4 * k + 2] > dd) return true;
  return false;
}

// Walk-hull support through its cell record (mpg_hullcells.h
// build_walk_cells).  In a trap-free subcell the walk ends at the unique
// global maximum, the maximum of the record's linear list: returned, pend =
// false.  In a trapped subcell whose fine cell has a certified endpoint (one
// climb path for the whole fine cone) that vertex is returned.  Otherwise (a
// tie at the maximum, or an uncertified fine cell) pend = true with the
// linear list's first maximum in hand, for walk_resolve_wave.
__device__ __forceinline__ V3 walk_cell_fast(const DevWorld& w, cptr<double> HV, int geom, cptr<double> R, int sub,
                                             int fine, int fine2, const V3& d, bool& pend, int& pre,
                                             unsigned long long t_cell = 0) {
#ifdef MPG_STATS  // phase stamps (s_memtime after the value each phase produces)
  unsigned long long t_rec = 0, t_ovf = 0;
#endif
  const long long no = (long long)R[9];
  const int n = (int)(no & ((1 << kCellCountBits) - 1));
  const cptr<double> ovf = w.wcell_ovf + 4 * (size_t)(no >> kCellCountBits);
  // first maximum (strict '>', as the reference's scan) ...
  double best = -DBL_MAX;
  int g = 0;
  double di[kCellInline];
#pragma unroll
  for (int k = 0; k < kCellInline; ++k) {
    di[k] = (d.x * R[3 * k] + d.y * R[3 * k + 1]) + d.z * R[3 * k + 2];
    if (k < n && di[k] > best) {
      best = di[k];
      g = k;
    }
  }
#ifdef MPG_STATS
  asm volatile("" ::"v"(best));
  t_rec = __builtin_amdgcn_s_memtime();
#endif
  int nmax = 0;  // ... and how many entries reach it (a tie when > 1)
  // the overflow entries kOvfBatch at a time: their loads issued together
  // (one memory round per batch, not per entry), then compared in list order
  for (int k0 = kCellInline; k0 < n; k0 += kOvfBatch) {
    double ex[kOvfBatch], ey[kOvfBatch], ez[kOvfBatch];
#pragma unroll
    for (int j = 0; j < kOvfBatch; ++j) {
      const cptr<double> e = ovf + 4 * (min(k0 + j, n - 1) - kCellInline);
      ex[j] = e[0];
      ey[j] = e[1];
      ez[j] = e[2];
    }
#pragma unroll
    for (int j = 0; j < kOvfBatch; ++j) {
      if (k0 + j >= n) break;
      const double dd = (d.x * ex[j] + d.y * ey[j]) + d.z * ez[j];
      if (dd > best) {  // a new maximum: the inline entries are all below it
        best = dd;
        g = k0 + j;
        nmax = 1;
      } else if (dd == best) {
        ++nmax;
      }
    }
  }
#ifdef MPG_STATS
  asm volatile("" ::"v"(best));
  t_ovf = __builtin_amdgcn_s_memtime();
#endif
  // the inline entries, compared with the final maximum (short lists repeat
  // their first entry: count only k < n)
#pragma unroll
  for (int k = 0; k < kCellInline; ++k) nmax += (k < n && di[k] == best) ? 1 : 0;
  bool tie = nmax > 1;
  const uint64_t free_mask = (uint64_t)__double_as_longlong(R[11]);
  const bool sub_free = (free_mask >> sub) & 1ull;
  pend = !(sub_free && !tie);
  int endp = -1;
  if (__builtin_expect(!sub_free, 0)) {  // trapped subcell: its fine cell's certified endpoint, if any
    const cptr<double> A = w.wcell_aux + kWalkAux * (size_t)(R[10] - 1.0);
    const int t = (int)A[0] + __popcll(~free_mask & ((1ull << sub) - 1ull));
    endp = w.wcell_end[(size_t)t * (kSub2K * kSub2K) + fine];
    if (endp <= -2) endp = w.wcell_end2[(size_t)(-2 - endp) * (kSub3K * kSub3K) + fine2];
    pend = endp < 0;
    pre = endp <= -2 ? -2 - endp : -1;
  }
#ifdef MPG_STATS
  if (w.stats && t_cell) {  // support phases, first active lane: cell lookup -> record + inline dots ->
    asm volatile("" ::"v"(pend));  // overflow entries -> tie / trap checks
    const unsigned long long t_end = __builtin_amdgcn_s_memtime();
    if ((uint32_t)__lane_id() == (uint32_t)__builtin_ctzll(__ballot(true))) {
      atomicAdd(&w.stats[49], t_rec - t_cell);
      atomicAdd(&w.stats[50], t_ovf - t_rec);
      atomicAdd(&w.stats[51], t_end - t_ovf);
      atomicAdd(&w.stats[52], 1ull);
    }
  }
  if (w.stats) {
    atomicAdd(&w.stats[10], 1ull);
    if (!pend) atomicAdd(&w.stats[11], 1ull);
    if (endp >= 0) atomicAdd(&w.stats[14], 1ull);
    if (pend) atomicAdd(&w.stats[sub_free ? 16 : 17], 1ull);  // pending: tie / uncertified fine cell
  }
#endif
  if (endp >= 0) return hull_vertex(w, HV, geom, endp);
  const cptr<double> e = g < kCellInline ? R + 3 * g : ovf + 4 * (g - kCellInline);
  return v3(e[0], e[1], e[2]);
}

// The pending lanes of a wave, one at a time by every active lane.  For lane
// L's trapped cell: the walk ends at the first maximum g of the walk list when
// every other listed vertex has a strictly greater neighbour (g itself when
// adjacent, else usually its witness, else a neighbour scan); the entries are
// checked in parallel.  g is the global first maximum, already in lane L's p.
// If that fails (a local maximum of the non-convex triangulation, a tie, or no
// cell) the climb is run (wave_walk).
__device__ __forceinline__ V3 walk_resolve_wave(const DevWorld& w, cptr<double> HV, int geom, const V3& d, int c,
                                                bool pend, int pre, V3 p) {
  unsigned long long pm = __ballot(pend);
  if (__builtin_expect(pm == 0ull, 1)) return p;
  const unsigned long long act = __ballot(true);
  const int nact = __popcll(act);
  const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(act >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)act, 0u));
  const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  while (pm) {
    const int L = __builtin_ctzll(pm);
    pm &= pm - 1ull;
    // lane L's hull (the same on every lane when the wave's pair is uniform)
    const int geomL = __builtin_amdgcn_readlane(geom, L);
    const int cb = w.geom_cbase[geomL];
    const V3 dL = v3(lane_bcast(d.x, L), lane_bcast(d.y, L), lane_bcast(d.z, L));
    const int cL = __builtin_amdgcn_readlane(c, L);
    const int preL = __builtin_amdgcn_readlane(pre, L);
    if (preL >= 0) {  // undecided finer cell: resume the climb where the host's replay stopped
      const int bi = wave_walk(w, HV, geomL, dL, rank, nact, w.wcell_pre + kWalkPre * (size_t)preL);
      if (lane == L) p = hull_vertex(w, HV, geomL, bi);
#ifdef MPG_STATS
      if (w.stats && rank == 0) atomicAdd(&w.stats[18], 1ull);
#endif
      continue;
    }
    bool ok = false;
#ifdef MPG_STATS
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
    if (cL >= 0) {
      const double info = w.wcell_rec[kCellRec * (size_t)(cb + cL) + 10];
#ifdef MPG_WALK_NOVERIFY  // timing ablation: every pending lane climbs
      ok = false;
#else
      ok = info > 0.0;  // trap-free cell but tied: straight to the walk
#endif
      if (ok) {
        const cptr<double> A = w.wcell_aux + kWalkAux * (size_t)(info - 1.0);
        const int nw = (int)A[1];
        const cptr<double> E = A + kWalkAux;  // walk-list entries
        double bL = -DBL_MAX;
        int gL = 0;
        for (int k = 0; k < nw; ++k) {  // its first maximum (uniform)
          const cptr<double> e = E + kWalkAux * k;
          const double dd = (dL.x * e[5] + dL.y * e[6]) + dL.z * e[7];
          if (dd > bL) {
            bL = dd;
            gL = k;
          }
        }
        bool fail = false;
        for (int k = rank; k < nw; k += nact) {
          if (k == gL) continue;
          const cptr<double> a = E + kWalkAux * k;
          const double dd = (dL.x * a[5] + dL.y * a[6]) + dL.z * a[7];
          // the maximum g is a neighbour of this entry and strictly above it
          if (gL < 32 && ((((uint32_t)a[4]) >> gL) & 1u) && bL > dd) continue;
          const double dw = (dL.x * a[1] + dL.y * a[2]) + dL.z * a[3];
          if (dw > dd) continue;
          if (!neighbour_beats(w, HV, geomL, (int)a[0], dd, dL)) fail = true;
        }
        ok = __ballot(fail) == 0ull;
      }
    }
#ifdef MPG_STATS
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (w.stats && rank == 0) {
      atomicAdd(&w.stats[ok ? 12 : 13], 1ull);
      atomicAdd(&w.stats[9], t1 - t0);
    }
#endif
    if (!ok) {
      const int bi = wave_walk(w, HV, geomL, dL, rank, nact, nullptr);
      if (lane == L) p = hull_vertex(w, HV, geomL, bi);
#ifdef MPG_STATS
      if (w.stats && rank == 0) atomicAdd(&w.stats[15], __builtin_amdgcn_s_memtime() - t1);
#endif
    }
  }
  return p;
}

// Convex support in the hull frame (FCL 0.7.0 supportConvex: the ccd
// direction converted to Vector3<double>, findExtremeVertex in fp64).  Called
// by all active lanes of the wave together (geom is wave-uniform).
__device__ __forceinline__ V3 convex_support_fast(const DevWorld& w, cptr<double> HV, int geom, const V3& d, bool& pend,
                                                  int& cell, int& pre) {
  const int cb = w.geom_cbase[geom];
  pend = false;
  cell = -1;
  pre = -1;
  if (w.geom_nbr[geom] >= 0) {  // neighbour-walk hull (wave-uniform branch)
    int sub = 0, fine = 0, fine2 = 0;
    pend = true;
#ifdef MPG_STATS
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
    cell = cb >= 0 ? hull_cell_sub(d.x, d.y, d.z, w.walk_subk, &sub, &fine, &fine2) : -1;
    unsigned long long t_cell = 0;
#ifdef MPG_STATS
    asm volatile("" ::"v"(cell), "v"(sub), "v"(fine));
    t_cell = __builtin_amdgcn_s_memtime();
    if (w.stats && (uint32_t)__lane_id() == (uint32_t)__builtin_ctzll(__ballot(true))) atomicAdd(&w.stats[48], t_cell - t0);
#endif
    V3 p = v3(0.0, 0.0, 0.0);
    if (cell >= 0)
      p = walk_cell_fast(w, HV, geom, w.wcell_rec + kCellRec * (size_t)(cb + cell), sub, fine, fine2, d, pend, pre,
                         t_cell);
    return p;
  }
  const int c = cb >= 0 ? hull_cell(d.x, d.y, d.z) : -1;
  if (c < 0) return convex_full_scan(w, HV, geom, d);
  double p[3];
  cell_record_support(w.cell_rec + kCellRec * (size_t)(cb + c), w.cell_ovf, d.x, d.y, d.z, p);
  return v3(p[0], p[1], p[2]);
}

__device__ __forceinline__ V3 convex_support_local(const DevWorld& w, cptr<double> HV, int geom, const V3& d) {
  bool pend;
  int cell, pre;
  const V3 p = convex_support_fast(w, HV, geom, d, pend, cell, pre);
  if (w.geom_nbr[geom] < 0) return p;
  return walk_resolve_wave(w, HV, geom, d, cell, pend, pre, p);
}

// support mapping of one shape in its own frame (FCL shapeToGJK supports:
// supportConvex, supportBox, supportSphere, supportCap, supportCyl), in the
// libccd scalar: the shape parameters are the ccd_real values FCL's
// *ToGJK functions store (box: dim = side / 2; capsule / cylinder: height =
// lz / 2).
__device__ __forceinline__ CV3 support_local(const DevWorld& w, cptr<double> HV, int geom, int type, const CV3& dir) {
  const cptr<double> rec = w.geom_rec + G_STRIDE * geom;
  CV3 v;
  if (type == MPG_GEOM_CONVEX) {
    const V3 p = convex_support_local(w, HV, geom, to_v3(dir));
    v = cv3(p.x, p.y, p.z);
  } else if (type == MPG_GEOM_BOX) {
    const ccd_real hx = (ccd_real)(rec[G_PARAM + 0] / 2.0), hy = (ccd_real)(rec[G_PARAM + 1] / 2.0),
                   hz = (ccd_real)(rec[G_PARAM + 2] / 2.0);
    v = CV3{(dir.x >= 0 ? ccd_real(1) : ccd_real(-1)) * hx, (dir.y >= 0 ? ccd_real(1) : ccd_real(-1)) * hy,
            (dir.z >= 0 ? ccd_real(1) : ccd_real(-1)) * hz};
  } else if (type == MPG_GEOM_SPHERE) {
    const ccd_real r = (ccd_real)rec[G_PARAM];
    v = vscale(vscale(dir, r), ccd_real(1) / std::sqrt(vdot(dir, dir)));
  } else if (type == MPG_GEOM_CAPSULE) {
    const ccd_real r = (ccd_real)rec[G_PARAM], h = (ccd_real)(rec[G_PARAM + 1] / 2.0);
    const CV3 n = vscale(vnormalize(dir), r);
    CV3 p1 = CV3{0, 0, h}, p2 = CV3{0, 0, -h};
    p1 = vadd(p1, n);
    p2 = vadd(p2, n);
    v = dir.z > 0 ? p1 : p2;
  } else if (type == MPG_GEOM_CONE) {  // supportCone (coneToGJK: height = lz / 2)
    const ccd_real r = (ccd_real)rec[G_PARAM], h = (ccd_real)(rec[G_PARAM + 1] / 2.0);
    ccd_real zdist = dir.x * dir.x + dir.y * dir.y;
    ccd_real len = zdist + dir.z * dir.z;
    zdist = std::sqrt(zdist);
    len = std::sqrt(len);
    const ccd_real sin_a = r / std::sqrt(r * r + 4 * h * h);
    if (dir.z > len * sin_a) {
      v = CV3{0, 0, h};
    } else if (zdist > 0) {
      const ccd_real rad = r / zdist;
      v = CV3{rad * dir.x, rad * dir.y, -h};
    } else {
      v = CV3{0, 0, -h};
    }
  } else if (type == MPG_GEOM_TRIANGLE) {  // supportTriangle: first maximum of dir . (p - c), ccd_real
    const cptr<double> G = HV + 12 * (size_t)w.geom_gstart[geom];
    const CV3 c = cv3(rec[G_INTERIOR], rec[G_INTERIOR + 1], rec[G_INTERIOR + 2]);
    ccd_real maxdot = -FLT_MAX;
    v = cv3(G[0], G[4], G[8]);
    for (int i = 0; i < 3; ++i) {
      const CV3 p = cv3(G[i], G[4 + i], G[8 + i]);
      const ccd_real dot = vdot(dir, vsub(p, c));
      if (dot > maxdot) {
        v = p;
        maxdot = dot;
      }
    }
  } else if (type == MPG_GEOM_ELLIPSOID) {  // supportEllipsoid
    const ccd_real a = (ccd_real)rec[G_PARAM], b = (ccd_real)rec[G_PARAM + 1], c = (ccd_real)rec[G_PARAM + 2];
    const CV3 p = CV3{(a * a) * dir.x, (b * b) * dir.y, (c * c) * dir.z};
    v = vscale(p, ccd_real(1) / std::sqrt(vdot(p, dir)));
  } else {  // cylinder
    const ccd_real r = (ccd_real)rec[G_PARAM], h = (ccd_real)(rec[G_PARAM + 1] / 2.0);
    ccd_real zdist = dir.x * dir.x + dir.y * dir.y;
    zdist = std::sqrt(zdist);
    if (std::fabs(zdist) < kCcdEps) {
      v = CV3{0, 0, (dir.z > 0 ? ccd_real(1) : ccd_real(-1)) * h};
    } else {
      const ccd_real rad = r / zdist;
      v = CV3{rad * dir.x, rad * dir.y, (dir.z > 0 ? ccd_real(1) : ccd_real(-1)) * h};
    }
  }
  return v;
}

#include "mpg_gjk_indep.h"

// True extreme point of a shape along dir in its own frame, fp64 (every
// vertex for hulls, whatever FCL's walk would return): conservative range
// tests only, never an output bit.
__device__ __forceinline__ V3 support_local_exact(const DevWorld& w, cptr<double> HV, int geom, int type, const V3& dir) {
  const cptr<double> rec = w.geom_rec + G_STRIDE * geom;
  if (type == MPG_GEOM_CONVEX || type == MPG_GEOM_TRIANGLE) return convex_full_scan(w, HV, geom, dir);
  if (type == MPG_GEOM_BOX)
    return v3((dir.x >= 0 ? 1.0 : -1.0) * rec[G_PARAM] / 2.0, (dir.y >= 0 ? 1.0 : -1.0) * rec[G_PARAM + 1] / 2.0,
              (dir.z >= 0 ? 1.0 : -1.0) * rec[G_PARAM + 2] / 2.0);
  if (type == MPG_GEOM_SPHERE) return vscale(vscale(dir, rec[G_PARAM]), 1.0 / std::sqrt(vdot(dir, dir)));
  if (type == MPG_GEOM_ELLIPSOID) {
    const V3 p = v3(rec[G_PARAM] * rec[G_PARAM] * dir.x, rec[G_PARAM + 1] * rec[G_PARAM + 1] * dir.y,
                    rec[G_PARAM + 2] * rec[G_PARAM + 2] * dir.z);
    return vscale(p, 1.0 / std::sqrt(vdot(p, dir)));
  }
  const double r = rec[G_PARAM], h = rec[G_PARAM + 1] / 2.0;
  if (type == MPG_GEOM_CAPSULE) return vadd(v3(0.0, 0.0, dir.z > 0 ? h : -h), vscale(vnormalize(dir), r));
  if (type == MPG_GEOM_CONE) {  // the better of the apex and the base rim point along dir
    const double zd = std::sqrt(dir.x * dir.x + dir.y * dir.y);
    const double rad = zd > 0.0 ? r / zd : 0.0;
    const V3 rim = v3(rad * dir.x, rad * dir.y, -h);
    return dir.z * h > vdot(dir, rim) ? v3(0.0, 0.0, h) : rim;
  }
  const double zd = std::sqrt(dir.x * dir.x + dir.y * dir.y);  // cylinder
  const double rad = zd > 0.0 ? r / zd : 0.0;
  return v3(rad * dir.x, rad * dir.y, (dir.z > 0 ? 1.0 : -1.0) * h);
}

// libccd support of one GJK object: direction into the object frame
// (ccdQuatRotVec with rot_inv), local support, back to the world frame.  The
// geometry is the same on every lane of the wave (one pair per wave): say so,
// so parameter reads stay scalar loads.
__device__ __forceinline__ CV3 support(const DevWorld& w, cptr<double> HV, const GObj& o, const CV3& dir_world) {
  const CV3 dir = quat_rot(dir_world, o.rot_inv);
  const int geom = __builtin_amdgcn_readfirstlane(o.geom), type = __builtin_amdgcn_readfirstlane(o.type);
  return vadd(quat_rot(support_local(w, HV, geom, type, dir), o.rot), o.pos);
}

// centerConvex (interior point ccdVec3Set, rotated, translated) / centerShape
template <bool UNI = true>
__device__ __forceinline__ CV3 center(const DevWorld& w, const GObj& o) {
  const int t = UNI ? __builtin_amdgcn_readfirstlane(o.type) : o.type;
  if (t == MPG_GEOM_CONVEX || t == MPG_GEOM_TRIANGLE) {  // centerConvex / centerTriangle
    const cptr<double> rec = w.geom_rec + G_STRIDE * (UNI ? __builtin_amdgcn_readfirstlane(o.geom) : o.geom);
    return vadd(quat_rot(cv3(rec[G_INTERIOR], rec[G_INTERIOR + 1], rec[G_INTERIOR + 2]), o.rot), o.pos);
  }
  return o.pos;
}

__device__ __forceinline__ bool is_zero(ccd_real v) { return std::fabs(v) < kCcdEps; }

__device__ __forceinline__ bool ccd_eq(ccd_real _a, ccd_real _b) {
  const ccd_real ab = std::fabs(_a - _b);
  if (std::fabs(ab) < kCcdEps) return true;
  const ccd_real a = std::fabs(_a), b = std::fabs(_b);
  if (b > a) return ab < kCcdEps * b;
  return ab < kCcdEps * a;
}

__device__ __forceinline__ bool vec_is_origin(const CV3& v) {
  return ccd_eq(v.x, ccd_real(0)) && ccd_eq(v.y, ccd_real(0)) && ccd_eq(v.z, ccd_real(0));
}

// libccd __ccdSupport: v = support1(dir) - support2(-dir)
// UNI: the geometries are the same on every lane (one pair per wave): their
// parameters come through scalar loads; otherwise every lane has its own pair
template <bool UNI = true>
__device__ __forceinline__ CV3 msupport(const DevWorld& w, cptr<double> HV, const GObj& a,
                                        const GObj& b, const CV3& dir) {
  const CV3 da = quat_rot(dir, a.rot_inv), db = quat_rot(vscale(dir, ccd_real(-1)), b.rot_inv);
  const int ga = UNI ? __builtin_amdgcn_readfirstlane(a.geom) : a.geom, ta = UNI ? __builtin_amdgcn_readfirstlane(a.type) : a.type;
  const int gb = UNI ? __builtin_amdgcn_readfirstlane(b.geom) : b.geom, tb = UNI ? __builtin_amdgcn_readfirstlane(b.type) : b.type;
  // walk hulls: both fast paths first, then one resolve site for the lanes
  // either left pending (one inlined copy of the rare path instead of two)
  bool pa = false, pb = false;
  int ca = -1, cb = -1, qa = -1, qb = -1;
  CV3 la, lb;
  if (ta == MPG_GEOM_CONVEX) {
    const V3 p = convex_support_fast(w, HV, ga, to_v3(da), pa, ca, qa);
    la = cv3(p.x, p.y, p.z);
  } else {
    la = support_local(w, HV, ga, ta, da);
  }
  if (tb == MPG_GEOM_CONVEX) {
    const V3 p = convex_support_fast(w, HV, gb, to_v3(db), pb, cb, qb);
    lb = cv3(p.x, p.y, p.z);
  } else {
    lb = support_local(w, HV, gb, tb, db);
  }
  if (__builtin_expect(__ballot(pa || pb) != 0ull, 0)) {  // rare: laid out off the hot path
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
      const int g = s ? gb : ga;
      const CV3 l = s ? lb : la;
      const V3 p = walk_resolve_wave(w, HV, g, to_v3(s ? db : da), s ? cb : ca, s ? pb : pa, s ? qb : qa,
                                     v3(l.x, l.y, l.z));
      if (s) lb = cv3(p.x, p.y, p.z);
      else la = cv3(p.x, p.y, p.z);
    }
  }
  return vsub(vadd(quat_rot(la, a.rot), a.pos), vadd(quat_rot(lb, b.rot), b.pos));
}

// msupport on two half-waves: every lane of one half carries the same MPR
// state as its partner lane ^ 32 of the other; lanes of side 0 evaluate a's
// support, side 1 b's (at once, instead of one after the other on one lane),
// then the halves swap their world points.  The arithmetic of each support is
// msupport's, so the result is the same bits.  Geometry per lane (the halves
// hold different shapes).
__device__ __forceinline__ CV3 msupport_split(const DevWorld& w, cptr<double> HV, const GObj& a, const GObj& b,
                                              const CV3& dir, bool side) {
  const GObj o = side ? b : a;
  const CV3 dl = quat_rot(side ? vscale(dir, ccd_real(-1)) : dir, o.rot_inv);
  bool pend = false;
  int cell = -1, pre = -1;
  CV3 l;
  if (o.type == MPG_GEOM_CONVEX) {
    const V3 p = convex_support_fast(w, HV, o.geom, to_v3(dl), pend, cell, pre);
    l = cv3(p.x, p.y, p.z);
  } else {
    l = support_local(w, HV, o.geom, o.type, dl);
  }
  if (__builtin_expect(__ballot(pend) != 0ull, 0)) {
    const V3 p = walk_resolve_wave(w, HV, o.geom, to_v3(dl), cell, pend, pre, v3(l.x, l.y, l.z));
    l = cv3(p.x, p.y, p.z);
  }
  const CV3 mine = vadd(quat_rot(l, o.rot), o.pos);
  const CV3 other = CV3{__shfl_xor(mine.x, 32), __shfl_xor(mine.y, 32), __shfl_xor(mine.z, 32)};
  return side ? vsub(other, mine) : vsub(mine, other);
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// Link Isometry from a (p, wxyz) pose vector (FCLModel::updateCollisionObjects,
// src/fcl_model.cpp:151-167 / ArticulatedModel::setQpos re-matrix).
__device__ __forceinline__ SE3 link_from_pose7(const double* p7) {
  SE3 T;
  quat_to_mat(p7[3], p7[4], p7[5], p7[6], T.R);
  T.p[0] = p7[0];
  T.p[1] = p7[1];
  T.p[2] = p7[2];
  return T;
}

// Moving object -> FCL GJK object (shapeToGJK on link pose * offset).
// world transform of moving object `id` (link pose * collision origin) -- the
// Isometry FCLModel::updateCollisionObjects hands to setTransform
// USE_SC: joint (sin, cos) precomputed in `sc` (phase A), else computed inline
// sc_row: the configuration's [dof][2] (sin, cos), or nullptr (computed inline)
template <bool FROM_POSES>
__device__ __forceinline__ SE3 moving_tf_row(const DevWorld& w, const double* __restrict__ in,
                                             const double* sc_row, long long cfg, int id) {
  const int l = w.moving_link[id];
  const SE3 L = FROM_POSES ? link_from_pose7(in + (cfg * w.n_links + l) * 7)
                           : link_from_oMi(w, chain_oMi(w, in + cfg * w.dof, l, sc_row), l, nullptr);
  return se3_mul(L, load_se3(w.moving_offset + 12 * id));
}
template <bool FROM_POSES, bool USE_SC = true>
__device__ __forceinline__ SE3 moving_tf(const DevWorld& w, const double* __restrict__ in,
                                         const double* __restrict__ sc, long long cfg, int id) {
  return moving_tf_row<FROM_POSES>(w, in, USE_SC ? sc + cfg * w.dof * 2 : nullptr, cfg, id);
}

// Moving object -> FCL GJK object (shapeToGJK on link pose * offset).
template <bool FROM_POSES>
__device__ __forceinline__ GObj moving_obj(const DevWorld& w, const double* __restrict__ in,
                                           const double* __restrict__ sc, long long cfg, int id) {
  const SE3 T = moving_tf<FROM_POSES>(w, in, sc, cfg, id);
  GObj o;
  o.rot = gjk_rot_from_matrix(T.R);
  o.rot_inv = quat_invert2(o.rot);
  o.pos = cv3(T.p[0], T.p[1], T.p[2]);
  o.geom = w.moving_geom[id];
  o.type = w.geom_type[o.geom];
  return o;
}

// ---------------------------------------------------------------------------
// FCL 0.7.0 closed-form shape pairs (GJKSolver_libccd::shapeIntersect
// specialisations, both argument orders), boolean part; same operation order
// as the oracle (oracle/collide_oracle.c box_box_intersect & co.)
// ---------------------------------------------------------------------------
enum : int {
  CF_NONE = 0, CF_BOX_BOX = 1, CF_SPHERE_SPHERE = 2, CF_SPHERE_BOX = 3, CF_BOX_SPHERE = 4, CF_OCTREE = 5,
  CF_SPHERE_CAPSULE = 6, CF_CAPSULE_SPHERE = 7, CF_SPHERE_CYLINDER = 8, CF_CYLINDER_SPHERE = 9, CF_MESH = 10,
  CF_GJK = 11  // GST_INDEP worlds: FCL's own GJK (mpg_gjk_indep.h) in place of libccd MPR
};
// narrow-phase classes of the candidate lists: each its own kernel instance
enum : int { CLS_CLOSED = 0, CLS_OCTREE = 1, CLS_MESH = 2, CLS_GJK = 3 };
__host__ __device__ __forceinline__ int cf_class(int cf) {
  return cf == CF_OCTREE ? CLS_OCTREE : cf == CF_MESH ? CLS_MESH : cf == CF_GJK ? CLS_GJK : CLS_CLOSED;
}

// detail::boxBox2 (box_box-inl.h, from ODE dBoxBox): return_code != 0
__device__ __forceinline__ bool box_box_intersect(const double* side1, const SE3& T1, const double* side2,
                                                  const SE3& T2) {
  const double p[3] = {T2.p[0] - T1.p[0], T2.p[1] - T1.p[1], T2.p[2] - T1.p[2]};
  double pp[3], A[3], B[3], R[3][3], Q[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) pp[i] = (T1.R[i] * p[0] + T1.R[3 + i] * p[1]) + T1.R[6 + i] * p[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    A[i] = side1[i] * 0.5;
    B[i] = side2[i] * 0.5;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      R[i][j] = (T1.R[i] * T2.R[j] + T1.R[3 + i] * T2.R[3 + j]) + T1.R[6 + i] * T2.R[6 + j];
      Q[i][j] = std::fabs(R[i][j]);
    }
  double s = -DBL_MAX, s2, tmp;
  int code = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {  // axes u1, u2, u3
    tmp = pp[i];
    s2 = std::fabs(tmp) - (((Q[i][0] * B[0] + Q[i][1] * B[1]) + Q[i][2] * B[2]) + A[i]);
    if (s2 > 0) return false;
    if (s2 > s) {
      s = s2;
      code = 1 + i;
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {  // axes v1, v2, v3
    tmp = (T2.R[j] * p[0] + T2.R[3 + j] * p[1]) + T2.R[6 + j] * p[2];
    s2 = std::fabs(tmp) - (((Q[0][j] * A[0] + Q[1][j] * A[1]) + Q[2][j] * A[2]) + B[j]);
    if (s2 > 0) return false;
    if (s2 > s) {
      s = s2;
      code = 4 + j;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Q[i][j] += 1.0e-6;  // ODE's edge-axis tolerance
  const double eps = DBL_EPSILON, fudge = 1.05;
  auto edge = [&](double t, double rad, double n0, double n1, double n2, int c) -> bool {
    const double e2 = std::fabs(t) - rad;
    if (e2 > eps) return true;
    const double l = std::sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    if (l > eps) {
      const double e3 = e2 / l;
      if (e3 * fudge > s) {
        s = e3;
        code = c;
      }
    }
    return false;
  };
  // u1 x (v1, v2, v3)
  if (edge(pp[2] * R[1][0] - pp[1] * R[2][0], ((A[1] * Q[2][0] + A[2] * Q[1][0]) + B[1] * Q[0][2]) + B[2] * Q[0][1], 0,
           -R[2][0], R[1][0], 7)) return false;
  if (edge(pp[2] * R[1][1] - pp[1] * R[2][1], ((A[1] * Q[2][1] + A[2] * Q[1][1]) + B[0] * Q[0][2]) + B[2] * Q[0][0], 0,
           -R[2][1], R[1][1], 8)) return false;
  if (edge(pp[2] * R[1][2] - pp[1] * R[2][2], ((A[1] * Q[2][2] + A[2] * Q[1][2]) + B[0] * Q[0][1]) + B[1] * Q[0][0], 0,
           -R[2][2], R[1][2], 9)) return false;
  // u2 x (v1, v2, v3)
  if (edge(pp[0] * R[2][0] - pp[2] * R[0][0], ((A[0] * Q[2][0] + A[2] * Q[0][0]) + B[1] * Q[1][2]) + B[2] * Q[1][1],
           R[2][0], 0, -R[0][0], 10)) return false;
  if (edge(pp[0] * R[2][1] - pp[2] * R[0][1], ((A[0] * Q[2][1] + A[2] * Q[0][1]) + B[0] * Q[1][2]) + B[2] * Q[1][0],
           R[2][1], 0, -R[0][1], 11)) return false;
  if (edge(pp[0] * R[2][2] - pp[2] * R[0][2], ((A[0] * Q[2][2] + A[2] * Q[0][2]) + B[0] * Q[1][1]) + B[1] * Q[1][0],
           R[2][2], 0, -R[0][2], 12)) return false;
  // u3 x (v1, v2, v3)
  if (edge(pp[1] * R[0][0] - pp[0] * R[1][0], ((A[0] * Q[1][0] + A[1] * Q[0][0]) + B[1] * Q[2][2]) + B[2] * Q[2][1],
           -R[1][0], R[0][0], 0, 13)) return false;
  if (edge(pp[1] * R[0][1] - pp[0] * R[1][1], ((A[0] * Q[1][1] + A[1] * Q[0][1]) + B[0] * Q[2][2]) + B[2] * Q[2][0],
           -R[1][1], R[0][1], 0, 14)) return false;
  if (edge(pp[1] * R[0][2] - pp[0] * R[1][2], ((A[0] * Q[1][2] + A[1] * Q[0][2]) + B[0] * Q[2][1]) + B[1] * Q[2][0],
           -R[1][2], R[0][2], 0, 15)) return false;
  return code != 0;
}

// detail::sphereSphereIntersect
__device__ __forceinline__ bool sphere_sphere_intersect(double r1, const SE3& T1, double r2, const SE3& T2) {
  const double d0 = T2.p[0] - T1.p[0], d1 = T2.p[1] - T1.p[1], d2 = T2.p[2] - T1.p[2];
  const double len = std::sqrt((d0 * d0 + d1 * d1) + d2 * d2);
  return !(len > r1 + r2);
}

// detail::sphereBoxIntersect: X_BS = X_FB.inverse() * X_FS, nearestPointInBox
__device__ __forceinline__ bool sphere_box_intersect(double r, const SE3& TS, const double* side, const SE3& TB) {
  double c[3];
  bool clamped = false;
  double dd = 0.0;
  double d[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double inv_t = -((TB.R[i] * TB.p[0] + TB.R[3 + i] * TB.p[1]) + TB.R[6 + i] * TB.p[2]);
    c[i] = ((TB.R[i] * TS.p[0] + TB.R[3 + i] * TS.p[1]) + TB.R[6 + i] * TS.p[2]) + inv_t;
    const double h = side[i] / 2;
    double nq = c[i];
    if (c[i] < -h) {
      clamped = true;
      nq = -h;
    }
    if (c[i] > h) {
      clamped = true;
      nq = h;
    }
    d[i] = c[i] - nq;
  }
  dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  return !(clamped && dd > r * r);
}

// the sphere centre in the other shape's frame: X_FO.inverse() * X_FS
// translation, R^T p_S + (-(R^T p_O)) with Eigen's evaluation order
__device__ __forceinline__ void centre_in_frame(const SE3& TS, const SE3& TO, double* c) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double inv_t = -((TO.R[i] * TO.p[0] + TO.R[3 + i] * TO.p[1]) + TO.R[6 + i] * TO.p[2]);
    c[i] = ((TO.R[i] * TS.p[0] + TO.R[3 + i] * TS.p[1]) + TO.R[6 + i] * TS.p[2]) + inv_t;
  }
}

// detail::sphereCapsuleIntersect (sphere_capsule-inl.h): the closest point of
// the capsule's axis segment (0,0,+lz/2)-(0,0,-lz/2) to the sphere centre
// (lineSegmentPointClosestToPoint), then |diff| - r1 - r2 > 0 -> separated
__device__ __forceinline__ bool sphere_capsule_intersect(double r1, const SE3& TS, double r2, double lz,
                                                         const SE3& TC) {
  double c[3];
  centre_in_frame(TS, TC, c);
  const double s1z = 0.5 * lz, s2z = -s1z;
  const double vz = s2z - s1z;
  const double w2 = c[2] - s1z;
  const double c1 = (c[0] * 0.0 + c[1] * 0.0) + w2 * vz;
  const double c2 = (0.0 * 0.0 + 0.0 * 0.0) + vz * vz;
  double spz;
  if (c1 <= 0) spz = s1z;
  else if (c2 <= c1) spz = s2z;
  else spz = s1z + vz * (c1 / c2);
  const double d0 = c[0], d1 = c[1], d2 = c[2] - spz;
  const double dist = std::sqrt((d0 * d0 + d1 * d1) + d2 * d2) - r1 - r2;
  return !(dist > 0);
}

// detail::sphereCylinderIntersect (sphere_cylinder-inl.h): nearestPointInCylinder
// (clamp z to +-lz/2, the radial part to the radius), inside -> intersect,
// else squared distance against r^2
__device__ __forceinline__ bool sphere_cylinder_intersect(double r, const SE3& TS, double rc, double lz,
                                                          const SE3& TC) {
  double c[3], n[3];
  centre_in_frame(TS, TC, c);
  const double h = lz / 2;
  bool clamped = false;
  n[0] = c[0];
  n[1] = c[1];
  n[2] = c[2];
  if (c[2] > h) {
    n[2] = h;
    clamped = true;
  } else if (c[2] < -h) {
    n[2] = -h;
    clamped = true;
  }
  const double rd2 = c[0] * c[0] + c[1] * c[1];
  if (rd2 > rc * rc) {
    const double scale = rc / std::sqrt(rd2);
    n[0] = c[0] * scale;
    n[1] = c[1] * scale;
    clamped = true;
  }
  if (!clamped) return true;
  const double d0 = n[0] - c[0], d1 = n[1] - c[1], d2 = n[2] - c[2];
  return !(((d0 * d0 + d1 * d1) + d2 * d2) > r * r);
}

__device__ __forceinline__ bool closed_form(int kind, const DevWorld& w, int ga, const SE3& TA, int gb,
                                            const SE3& TB) {
  const cptr<double> pa = w.geom_rec + G_STRIDE * ga + G_PARAM, pb = w.geom_rec + G_STRIDE * gb + G_PARAM;
  const double sa[3] = {pa[0], pa[1], pa[2]}, sb[3] = {pb[0], pb[1], pb[2]};
  switch (kind) {
    case CF_BOX_BOX: return box_box_intersect(sa, TA, sb, TB);
    case CF_SPHERE_SPHERE: return sphere_sphere_intersect(sa[0], TA, sb[0], TB);
    case CF_SPHERE_BOX: return sphere_box_intersect(sa[0], TA, sb, TB);
    case CF_SPHERE_CAPSULE: return sphere_capsule_intersect(sa[0], TA, sb[0], sb[1], TB);
    case CF_CAPSULE_SPHERE: return sphere_capsule_intersect(sb[0], TB, sa[0], sa[1], TA);
    case CF_SPHERE_CYLINDER: return sphere_cylinder_intersect(sa[0], TA, sb[0], sb[1], TB);
    case CF_CYLINDER_SPHERE: return sphere_cylinder_intersect(sb[0], TB, sa[0], sa[1], TA);
    default: return sphere_box_intersect(sb[0], TB, sa, TA);  // CF_BOX_SPHERE
  }
}

// fcl::OBB::overlap -> obbDisjoint (fcl/math/bv/OBB-inl.h [ext FCL 0.7.0]):
// B = R1^T R2 (row-major), T = R1^T (c2 - c1), a / b the half extents; the
// |B| entries are widened by 1e-6 before the 15 separating-axis tests.
__device__ __forceinline__ bool obb_disjoint(const double* B, const double* T, const double* a, const double* b) {
  const double reps = 1e-6;
  double Bf[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) Bf[i] = std::fabs(B[i]) + reps;
  if (std::fabs(T[0]) > a[0] + ((Bf[0] * b[0] + Bf[1] * b[1]) + Bf[2] * b[2])) return true;
  if (std::fabs((B[0] * T[0] + B[3] * T[1]) + B[6] * T[2]) > b[0] + ((Bf[0] * a[0] + Bf[3] * a[1]) + Bf[6] * a[2]))
    return true;
  if (std::fabs(T[1]) > a[1] + ((Bf[3] * b[0] + Bf[4] * b[1]) + Bf[5] * b[2])) return true;
  if (std::fabs(T[2]) > a[2] + ((Bf[6] * b[0] + Bf[7] * b[1]) + Bf[8] * b[2])) return true;
  if (std::fabs((B[1] * T[0] + B[4] * T[1]) + B[7] * T[2]) > b[1] + ((Bf[1] * a[0] + Bf[4] * a[1]) + Bf[7] * a[2]))
    return true;
  if (std::fabs((B[2] * T[0] + B[5] * T[1]) + B[8] * T[2]) > b[2] + ((Bf[2] * a[0] + Bf[5] * a[1]) + Bf[8] * a[2]))
    return true;
#define MPG_B(i, j) B[3 * (i) + (j)]
#define MPG_BF(i, j) Bf[3 * (i) + (j)]
#pragma unroll
  for (int j = 0; j < 3; ++j) {  // A0 x Bj
    const int j1 = j == 0 ? 1 : 0, j2 = j == 2 ? 1 : 2;
    const double sv = T[2] * MPG_B(1, j) - T[1] * MPG_B(2, j);
    if (std::fabs(sv) > a[1] * MPG_BF(2, j) + a[2] * MPG_BF(1, j) + b[j1] * MPG_BF(0, j2) + b[j2] * MPG_BF(0, j1))
      return true;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {  // A1 x Bj
    const int j1 = j == 0 ? 1 : 0, j2 = j == 2 ? 1 : 2;
    const double sv = T[0] * MPG_B(2, j) - T[2] * MPG_B(0, j);
    if (std::fabs(sv) > a[0] * MPG_BF(2, j) + a[2] * MPG_BF(0, j) + b[j1] * MPG_BF(1, j2) + b[j2] * MPG_BF(1, j1))
      return true;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {  // A2 x Bj
    const int j1 = j == 0 ? 1 : 0, j2 = j == 2 ? 1 : 2;
    const double sv = T[1] * MPG_B(0, j) - T[0] * MPG_B(1, j);
    if (std::fabs(sv) > a[0] * MPG_BF(1, j) + a[1] * MPG_BF(0, j) + b[j1] * MPG_BF(2, j2) + b[j2] * MPG_BF(2, j1))
      return true;
  }
#undef MPG_B
#undef MPG_BF
  return false;
}

__device__ __forceinline__ GObj static_obj(const DevWorld& w, int sid) {
  const cptr<double> r = w.static_rec + S_STRIDE * sid;
  GObj o;
  // static_record stores the ccd_real values (exactly representable in fp64)
  o.rot = CQ4{(ccd_real)r[S_ROT], (ccd_real)r[S_ROT + 1], (ccd_real)r[S_ROT + 2], (ccd_real)r[S_ROT + 3]};
  o.rot_inv = CQ4{(ccd_real)r[S_ROTINV], (ccd_real)r[S_ROTINV + 1], (ccd_real)r[S_ROTINV + 2], (ccd_real)r[S_ROTINV + 3]};
  o.pos = cv3(r[S_POS], r[S_POS + 1], r[S_POS + 2]);
  o.geom = w.static_geom[sid];
  o.type = w.geom_type[o.geom];
  return o;
}

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// ---------------------------------------------------------------------------
// Phase A: one lane per configuration (mpg_broadphase.h).
//   1. fp32 FK over the tree -> per moving object its world OBB centre in LDS
//      ([object][3][lane]) and its rotation quaternion in the workspace
//      (rq[object][4][cfg]: its rotation as a quaternion, read back only by
//      the SAT stage);
//   2. pairs are walked grouped by their moving object (host-built schedule,
//      ACM-allowed pairs dropped): the object's centre is loaded once, then
//      a cheap bounding test per partner (sphere-OBB against static objects,
//      sphere-sphere against moving ones);
//   3. pairs that pass are queued per wave in LDS as (pair, lane) entries and
//      the 15-axis OBB SAT runs 64 queued entries at a time with every lane
//      busy -- one lane's survivor no longer makes the whole wave pay;
//   4. SAT survivors set the configuration's bit in an LDS survivor word,
//      written to surv[word][cfg] at the end (no global atomics).
// Also zeroes this configuration's outputs for phase B.
// ---------------------------------------------------------------------------
#ifndef MPG_TASK
#define MPG_TASK 128
#endif
#ifndef MPG_REFILL
#define MPG_REFILL 32
#endif
constexpr uint32_t kTask = MPG_TASK;  // narrow phase: candidates of one pair per wave task
// taper of the task size towards the end of the task list (mpg_bucket.h,
// bk_task_plan): a level starts where MPG_TAPER_C * target tasks * (the size
// before it) candidates remain, sizes halve down to MPG_TAPER_MIN.  Measured
// on cfg3 at 2^20 (profiles/r10a/taper_sweep.txt): tasks below 64 candidates
// cost more in drained waves than the shorter tail returns (a task lasts
// about one MPR's dependent chain however few candidates it holds), so the
// product tapers the last quarter task per wave from 128 to 64 and no further.
#ifndef MPG_TAPER_C
#define MPG_TAPER_C 0.25
#endif
#ifndef MPG_TAPER_MIN
#define MPG_TAPER_MIN 64
#endif
constexpr double kTaperC = MPG_TAPER_C;
constexpr uint32_t kTaperMin = MPG_TAPER_MIN;

// inclusive scan of one value per lane across the wave
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t u = __shfl_up(v, off);
    if (lane >= (uint32_t)off) v += u;
  }
  return v;
}

template <int BLOCK>
__device__ __forceinline__ FObb bp_obb(const DevWorld& w, const float* __restrict__ cen, const float* __restrict__ rq,
                                       long long cap, int id, int t, long long cfg) {
  FObb o;
  if (id < w.n_moving) {
    const float* q = rq + (size_t)id * 4 * cap + cfg;
    f_quat_to_mat(q[3 * cap], q[0], q[cap], q[2 * cap], o.R);
    const float* c = cen + (size_t)id * 3 * BLOCK + t;
    o.c[0] = c[0];
    o.c[1] = c[BLOCK];
    o.c[2] = c[2 * BLOCK];
    const cptr<float> g = w.bp.mobj + BM_STRIDE * id;
    o.e[0] = g[BM_E];
    o.e[1] = g[BM_E + 1];
    o.e[2] = g[BM_E + 2];
  } else {
    const cptr<float> g = w.bp.sobj + BS_STRIDE * (id - w.n_moving);
#pragma unroll
    for (int k = 0; k < 3; ++k) o.c[k] = g[BS_C + k];
#pragma unroll
    for (int k = 0; k < 9; ++k) o.R[k] = g[BS_R + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o.e[k] = g[BS_E + k];
  }
  return o;
}

// Both OBBs of a queue entry.  Moving-static entries reach the queue before
// moving-moving ones, so the lanes of most drains agree on which side is
// static: such a drain takes a wave-uniform branch with no divergent branch
// around either object's loads, and A's and B's loads (rq, the static record,
// the centres from LDS) are issued together in front of one wait.  A mixed
// drain fetches one object after the other.
template <int BLOCK>
__device__ __forceinline__ void bp_obb_pair(const DevWorld& w, const float* __restrict__ cen, const float* __restrict__ rq,
                                            long long cap, int ia, int ib, int t, long long cfg, FObb& A, FObb& B) {
  const unsigned long long act = __ballot(true);
  const unsigned long long ma = __ballot(ia < w.n_moving), mb = __ballot(ib < w.n_moving);
  auto moving = [&](int id, FObb& o) {
    const float* q = rq + (size_t)id * 4 * cap + cfg;
    const float qx = q[0], qy = q[cap], qz = q[2 * cap], qw = q[3 * cap];
    const float* c = cen + (size_t)id * 3 * BLOCK + t;
    o.c[0] = c[0];
    o.c[1] = c[BLOCK];
    o.c[2] = c[2 * BLOCK];
    const cptr<float> g = w.bp.mobj + BM_STRIDE * id;
    o.e[0] = g[BM_E];
    o.e[1] = g[BM_E + 1];
    o.e[2] = g[BM_E + 2];
    return [=, &o]() { f_quat_to_mat(qw, qx, qy, qz, o.R); };
  };
  auto fixed = [&](int id, FObb& o) {
    const cptr<float> g = w.bp.sobj + BS_STRIDE * (id - w.n_moving);
#pragma unroll
    for (int k = 0; k < 3; ++k) o.c[k] = g[BS_C + k];
#pragma unroll
    for (int k = 0; k < 9; ++k) o.R[k] = g[BS_R + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o.e[k] = g[BS_E + k];
  };
  if (ma == act && mb == 0ull) {
    auto ra = moving(ia, A);
    fixed(ib, B);
    ra();
  } else if (ma == act && mb == act) {
    auto ra = moving(ia, A);
    auto rb = moving(ib, B);
    ra();
    rb();
  } else {
    A = bp_obb<BLOCK>(w, cen, rq, cap, ia, t, cfg);
    B = bp_obb<BLOCK>(w, cen, rq, cap, ib, t, cfg);
  }
}

// One drain of the SAT queue: cnt (schedule entry, lane) entries, one per
// lane.  The pair's frame (mpg_broadphase.h bp_pair_frame) is formed once; a
// lane whose pair the 15 SAT axes keep and which has a support-height table
// takes the support-height axes at once on the OBBs and the frame it holds,
// and the pairs neither test separates are the candidates.  The support part
// is skipped for the whole wave when no lane needs it.
template <int BLOCK>
__device__ __forceinline__ void sat_drain(const DevWorld& w, const float* __restrict__ cen, const float* __restrict__ rq,
                                          long long cap, long long cfg0, uint32_t* survw, const uint32_t* queue,
                                          uint32_t head, uint32_t cnt, int wbase, uint32_t lane) {
  __builtin_amdgcn_wave_barrier();
  if (lane < cnt) {
    const uint32_t e = queue[(head + lane) & (kQueue - 1)];  // (schedule entry, lane)
    const cptr<int> r = w.sched_rec + SR_STRIDE * (int)(e >> 6);
    const int p = r[SR_P], sh = r[SR_SH], t = wbase + (int)(e & 63u);
    FObb A, B;
    bp_obb_pair<BLOCK>(w, cen, rq, cap, r[SR_A], r[SR_B], t, cfg0 + t, A, B);
    const BpPairFrame F = bp_pair_frame(A, B);
    bool keep = !bp_frame_sat_separated(A, B, F, w.bp_margin);
    // 16: diagnostics, the fused pass without its support part
    const bool more = keep && (sh & 0xffff) != SH_SKIP + 2 && !w.dbg(16);
    if (__ballot(more) != 0ull) {
      if (more) keep = !bp_frame_support_separated(A, B, F, (sh & 0xffff) - 2, (sh >> 16) - 2, w.bp.shtab, w.sh_margin);
    }
    if (keep) atomicOr(&survw[(p >> 5) * BLOCK + t], 1u << (p & 31));
  }
  __builtin_amdgcn_wave_barrier();
}

template <int BLOCK, bool FROM_POSES>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void cull_kernel(DevWorld w, const double* __restrict__ in, long long n,
                                                    uint8_t* __restrict__ flags, uint32_t* __restrict__ masks,
                                                    uint32_t* __restrict__ surv, float* __restrict__ rq,
                                                    double* __restrict__ sc, long long cap,
                                                    uint32_t* __restrict__ cnt, int n_tiles,
                                                    const uint32_t* __restrict__ grid) {
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  float* cen = lds_f;                                                    // [n_moving][3][BLOCK]
  float* save = cen + (size_t)w.n_moving * 3 * BLOCK;  // [n_saves - kRegSaves][12][BLOCK]
  uint32_t* survw = reinterpret_cast<uint32_t*>(save + (size_t)max(w.bp.n_saves - kRegSaves, 0) * 12 * BLOCK);  // [W][BLOCK]
  const int tid = threadIdx.x;
  uint32_t* queue = survw + (size_t)w.W * BLOCK + (tid >> 6) * kQueue;  // [BLOCK/64][kQueue]
  const uint32_t lane = lane_id();
  const int wbase = tid & ~63;
  const long long cfg0 = (long long)blockIdx.x * BLOCK;
  const long long cfg = cfg0 + tid;
  const bool live = cfg < n;
  const long long c = live ? cfg : n - 1;  // dead lanes shadow a valid row and never queue
  if (live) {
    flags[cfg] = 0;
    if (masks)
      for (int k = 0; k < w.W; ++k) masks[cfg * w.W + k] = 0u;
  }
  for (int k = 0; k < w.W; ++k) survw[k * BLOCK + tid] = 0u;
  if (w.dbg(14)) return;  // diagnostics: the launch and the output zeroing alone

  // object m's rotation (quaternion q) to rq, its OBB centre to cen
  auto store_obj = [&](int m, const float* q, const float* c) {
    if (live && !w.dbg(13)) {  // 13: diagnostics, FK without the rq stores
      float* r = rq + (size_t)m * 4 * cap + cfg;
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k * cap] = q[k];
    }
    float* r = cen + (size_t)m * 3 * BLOCK + tid;
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i * BLOCK] = c[i];
  };
  // link-pose input: the object's world transform
  auto put = [&](int m, const F34& T) {
    float q[4], c[3];
    f_mat_to_quat(T.R, q);
    const cptr<float> g = w.bp.mobj + BM_STRIDE * m;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      c[i] = T.R[3 * i] * g[BM_C] + T.R[3 * i + 1] * g[BM_C + 1] + T.R[3 * i + 2] * g[BM_C + 2] + T.p[i];
    store_obj(m, q, c);
  };
  // joint-value input: the object's joint frame J (and its quaternion jq)
  auto put_j = [&](int m, const F34& J, const float* jq) {
    MPG_FP32_CONTRACT
    float q[4], c[3];
    const cptr<float> oq = w.bp.oquat + 4 * m, oc = w.bp.ocen + 3 * m;
    const float o[4] = {oq[0], oq[1], oq[2], oq[3]};
    f_quat_mul(jq, o, q);
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = J.R[3 * i] * oc[0] + J.R[3 * i + 1] * oc[1] + J.R[3 * i + 2] * oc[2] + J.p[i];
    store_obj(m, q, c);
  };
  // a configuration outside the bounds the cull's margins assume (a prismatic
  // value beyond its travel bound, or a given link pose beyond the chain's
  // reach) is evaluated with every pair
  bool forced = false;
  if (FROM_POSES) {
    for (int m = 0; m < w.n_moving; ++m) put(m, bp_from_pose7(w.bp, in + (c * w.n_links + w.moving_link[m]) * 7, m));
    const int nk = w.n_links - w.n_free;
    for (int l = 0; l < nk; ++l) {
      const double* pl = in + (c * w.n_links + l) * 7;
      forced |= !(std::fabs(pl[0]) <= w.pose_bound && std::fabs(pl[1]) <= w.pose_bound && std::fabs(pl[2]) <= w.pose_bound);
    }
    // far test of the movable objects, exact in fp64: one whose bounding
    // sphere lies outside the ball that holds every link-borne object (far_r:
    // margin and slack included) meets none of them in this row -- its centre
    // is parked where every fp32 sphere test fails; the others have their
    // coordinates inside the bound the cull margin was sized for
    for (int k = 0; k < w.n_free; ++k) {
      const double* pl = in + (c * w.n_links + nk + k) * 7;
      const int m = w.free_obj[k];
      const cptr<double> gr = w.geom_rec + G_STRIDE * w.moving_geom[m];
      double R[9];
      quat_to_mat(pl[3], pl[4], pl[5], pl[6], R);
      double d2 = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double ci = R[3 * i] * gr[G_OBB_C] + R[3 * i + 1] * gr[G_OBB_C + 1] + R[3 * i + 2] * gr[G_OBB_C + 2] + pl[i];
        d2 += ci * ci;
      }
      // NaN compares false: such an object stays in, and the fp32 tests drop it
      if (std::sqrt(d2) - gr[G_RADIUS] > w.far_r) {
        float* r = cen + (size_t)m * 3 * BLOCK + tid;
        r[0] = kFarPark;
        r[BLOCK] = 0.f;
        r[2 * BLOCK] = 0.f;
      }
    }
  } else {
    bp_fk(w.bp, in + c * w.dof, save + tid, BLOCK, put_j);
    if (w.n_prism)
      for (int j = 0; j < w.nj; ++j)
        if (w.prism_bound[j] >= 0.0) forced |= !(std::fabs(in[c * w.dof + w.joint_q_source[j]]) <= w.prism_bound[j]);
  }
  if (w.dbg(1) || w.dbg(13)) {
    if (live && cen[tid] == 12345.f) flags[cfg] = 2;  // keep the records alive
    return;
  }

  uint32_t head = 0, tail = 0;  // wave-uniform queue cursors
  uint32_t dbg_keep = 0u;       // diagnostics (11): the bounding tests' bits, kept alive
  // queue the entries [eb, eb + 32) some lane kept (kb: this lane's bits);
  // drain 64 queued (pair, lane) entries through the SAT at a time
  auto push = [&](int eb, uint32_t kb) {
    if (!live) kb = 0u;
    if (w.dbg(11)) {
      dbg_keep += kb;
      return;
    }
    if (w.dbg(2)) {
      for (int i = 0; i < 32; ++i) {
        if (!((kb >> i) & 1u)) continue;
        const int p = w.sched_pair[eb + i];
        survw[(p >> 5) * BLOCK + tid] |= 1u << (p & 31);
      }
      return;
    }
    // one wave scan of the kept counts: each lane writes its own entries
    // (schedule index, lane) at its offset, no per-entry wave-level loop
    {
    const uint32_t c = (uint32_t)__popc(kb);
    // the prefix sum by bit planes of the counts (<= 32: six ballots), no LDS
    uint32_t ex = 0u, total = 0u;
#pragma unroll
    for (int bit = 0; bit < 6; ++bit) {
      const unsigned long long m = __ballot((c >> bit) & 1u);
      ex += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)) << bit;
      total += (uint32_t)__popcll(m) << bit;
    }
    const uint32_t incl = ex + c;
    if (total == 0u) return;
    if (tail - head + total <= (uint32_t)kQueue) {
      uint32_t pos = tail + incl - c;
      while (kb) {
        const int i = __builtin_ctz(kb);
        kb &= kb - 1u;
        queue[pos++ & (kQueue - 1)] = ((uint32_t)(eb + i) << 6) | lane;
      }
      tail += total;
      while (tail - head >= 64) {
        sat_drain<BLOCK>(w, cen, rq, cap, cfg0, survw, queue, head, 64, wbase, lane);
        head += 64;
      }
      return;
    }
    }
    // more than the queue holds: entry by entry, draining as it fills
    uint32_t any_kb = kb;  // entries some lane of the wave kept
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) any_kb |= (uint32_t)__shfl_xor((int)any_kb, sh);
    any_kb = __builtin_amdgcn_readfirstlane(any_kb);
    while (any_kb) {
      const int i = __builtin_ctz(any_kb);
      any_kb &= any_kb - 1u;
      const bool keep = (kb >> i) & 1u;
      const unsigned long long bal = __ballot(keep);
      if (keep) {
        const uint32_t rank =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        queue[(tail + rank) & (kQueue - 1)] = ((uint32_t)(eb + i) << 6) | lane;
      }
      tail += (uint32_t)__popcll(bal);
      if (tail - head >= 64) {
        sat_drain<BLOCK>(w, cen, rq, cap, cfg0, survw, queue, head, 64, wbase, lane);
        head += 64;
      }
    }
  };
  // moving-static pairs, static-major: the static's OBB record is loaded
  // once (scalar registers) for all its entries, each entry a moving object's
  // bounding sphere (centre from LDS); group 1 (objects whose reach ball
  // never comes near the static) only for link-pose input, which does not
  // assume the kinematics
  const int ns = w.n_static;
  // joint-value input with the lookup grids built (mpg_broadphase.h
  // bp_grid_*): a gridded object's centre picks one cell word, the kept bits
  // of all its group-0 partners (a centre outside its grid takes them all);
  // kGridGroup objects' loads are issued together, and the words are shifted
  // into blocks of 32 consecutive schedule entries for push.  The objects
  // without a grid keep the loop below, over their own entries (gst_start).
  const bool use_grid = !FROM_POSES && grid != nullptr && w.n_grid > 0 && !w.dbg(12) && !w.dbg(15);  // 15: diagnostics, lookups off
  if (use_grid) {
    int eb = w.grid_i[GI_E], fill = 0;
    unsigned long long acc = 0ull;
    for (int g0 = 0; g0 < w.n_grid; g0 += kGridGroup) {
      uint32_t wd[kGridGroup];
#pragma unroll
      for (int j = 0; j < kGridGroup; ++j) {
        const cptr<float> gf = w.grid_f + GF_STRIDE * (g0 + j);
        const cptr<int> gi = w.grid_i + GI_STRIDE * (g0 + j);
        const float* rm = cen + (size_t)gi[GI_M] * 3 * BLOCK + tid;
        const float cm[3] = {rm[0], rm[BLOCK], rm[2 * BLOCK]};
        const int cell = bp_grid_cell(gf, gi, cm);
        const uint32_t x = grid[cell < 0 ? 0 : cell];
        wd[j] = cell < 0 ? (uint32_t)gi[GI_FULL] : x;
      }
      static_assert(kGridGroup == 4, "the selection below names four words");
#pragma unroll 1
      for (int j = 0; j < kGridGroup; ++j) {
        const uint32_t x = j == 0 ? wd[0] : j == 1 ? wd[1] : j == 2 ? wd[2] : wd[3];
        acc |= (unsigned long long)x << fill;
        fill += w.grid_i[GI_STRIDE * (g0 + j) + GI_NP];
        const bool last = g0 + j + 1 == w.n_grid;
        while (fill >= 32 || (last && fill > 0)) {
          push(eb, (uint32_t)acc);
          acc >>= 32;
          eb += 32;
          fill = max(fill - 32, 0);
        }
      }
    }
  }
  for (int g = 0; g < (FROM_POSES ? 2 : 1) && !w.dbg(12); ++g) {  // 12: diagnostics, without these tests
    const cptr<int> sts = use_grid ? w.gst_start : w.st_start + g * (ns + 1);
    const int E0 = sts[0], E1 = sts[ns];
    if (E0 == E1) continue;
    int eb = E0;
    uint32_t kb = 0u;
    for (int sid = 0; sid < ns; ++sid) {
      const int e0 = sts[sid], e1 = sts[sid + 1];
      if (e0 == e1) continue;
      const cptr<float> rec = w.bp.sobj + BS_STRIDE * sid;
      float sr[BS_STRIDE];
#pragma unroll
      for (int k = 0; k < BS_STRIDE; ++k) sr[k] = rec[k];
#pragma unroll 2
      for (int e = e0; e < e1; ++e) {
        if (e - eb == 32) {
          push(eb, kb);
          eb = e;
          kb = 0u;
        }
        const float* rm = cen + (size_t)w.st_m[e] * 3 * BLOCK + tid;
        const float cm[3] = {rm[0], rm[BLOCK], rm[2 * BLOCK]};
        kb |= (uint32_t)!fsphere_obb_separated(cm, w.st_r[e], sr, w.bp_margin) << (e - eb);
      }
    }
    push(eb, kb);
  }
  // moving-moving pairs: bounding spheres (both centres from LDS)
  for (int m = 0; m < w.n_moving; ++m) {
    const int e0 = w.sched_start[m], e1 = w.sched_start[m + 1];
    if (e0 == e1) continue;
    const float* rm = cen + (size_t)m * 3 * BLOCK + tid;
    const float cm[3] = {rm[0], rm[BLOCK], rm[2 * BLOCK]};
    const float r_m = w.bp.mobj[BM_STRIDE * m + BM_R];
    for (int eb = e0; eb < e1; eb += 32) {
      const int ee = min(e1, eb + 32);
      uint32_t kb = 0u;
#pragma unroll 4
      for (int e = eb; e < ee; ++e) {
        const int o = w.sched_other[e];
        const float* ro = cen + (size_t)o * 3 * BLOCK + tid;
        const float dx = ro[0] - cm[0], dy = ro[BLOCK] - cm[1], dz = ro[2 * BLOCK] - cm[2];
        const float rr = r_m + w.bp.mobj[BM_STRIDE * o + BM_R] + w.bp_margin;
        kb |= (uint32_t)(dx * dx + dy * dy + dz * dz <= rr * rr) << (e - eb);
      }
      push(eb, kb);
    }
  }
  if (tail != head) sat_drain<BLOCK>(w, cen, rq, cap, cfg0, survw, queue, head, tail - head, wbase, lane);
  __builtin_amdgcn_wave_barrier();
  if (forced)
    for (int k = 0; k < w.W; ++k) survw[k * BLOCK + tid] = (uint32_t)w.all_mask[k];
  if (w.dbg(8) || w.dbg(11) || w.dbg(16)) {  // ablation: bounding tests + SAT only (11: without the queue and SAT; 16: SAT without the support axes)
    if (live && (survw[tid] == 12345u || dbg_keep == 12345u)) flags[cfg] = 2;
    return;
  }
  // survivor words -> surv, and this wave's candidate count per pair ->
  // its tile's row of byte counts cnt8[tile][W * 32] (mpg_bucket.h).  The
  // counts are a per-wave histogram in the idle queue area: 8-bit counters
  // (<= 64 each), four per word, every lane adding its own survivors; the
  // histogram is the row, stored whole (zeros included, so nothing clears
  // cnt between calls) by every wave that has a tile, live lanes or not.
  // Worlds with more pairs than the area holds (W > kQueue / 8) take one
  // ballot per distinct pair and write single bytes into a row that
  // launch_collide has zeroed.
  bool any = false;
  const long long tile = bk_wave_tile(blockIdx.x, BLOCK, tid);
  const bool has_row = bk_tile_has_row(tile, n_tiles);
  if (w.W * 8 <= kQueue) {
    uint32_t* hist = queue;
    for (int i = (int)lane; i < w.W * 8; i += 64) hist[i] = 0u;
    wave_lds_sync();
    for (int k = 0; k < w.W; ++k) {
      uint32_t x = live ? survw[k * BLOCK + tid] : 0u;
      if (live) surv[(long long)k * cap + cfg] = x;
      any |= x != 0u;
      while (x) {
        const int p = k * 32 + __builtin_ctz(x);
        x &= x - 1u;
        atomicAdd(&hist[p >> 2], 1u << (8 * (p & 3)));
      }
    }
    wave_lds_sync();
    if (has_row) {
      uint32_t* row = cnt + tile * bk_row_words(w.W);
      for (int i = (int)lane; i < bk_row_words(w.W); i += 64) row[i] = hist[i];
    }
  } else {
    for (int k = 0; k < w.W; ++k) {
      uint32_t x = live ? survw[k * BLOCK + tid] : 0u;
      if (live) surv[(long long)k * cap + cfg] = x;
      any |= x != 0u;
      for (;;) {
        const unsigned long long m = __ballot(x != 0u);
        if (m == 0) break;
        const uint32_t xl = __builtin_amdgcn_readlane(x, __builtin_ctzll(m));
        const int b = __builtin_ctz(xl);
        const unsigned long long bb = __ballot((x >> b) & 1u);
        x &= ~(1u << b);
        if (lane == 0 && has_row)
          reinterpret_cast<uint8_t*>(cnt)[tile * bk_cols(w.W) + k * 32 + b] = (uint8_t)__popcll(bb);
      }
    }
  }
  if (FROM_POSES || w.dbg(9)) return;  // 9: ablation without the sincos pass
  // Exact fp64 sin/cos of every revolute move-group joint for the narrow
  // phase's chain FK (the glibc sincos restatement), only for configurations
  // with a candidate pair (about a quarter of them): compacted across the
  // block through LDS (the SAT queues are free now) and given out joint by
  // joint, so every wave of the block works and no lane walks the joints in
  // series.
  uint32_t* list = survw + (size_t)w.W * BLOCK;  // [BLOCK] + per-wave counts [BLOCK / 64]
  uint32_t* wcnt = list + BLOCK;
  __syncthreads();
  const unsigned long long bal = __ballot(any);
  if (lane == 0) wcnt[tid >> 6] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t off = 0, total = 0;
  for (int k = 0; k < BLOCK / 64; ++k) {
    off += k < (tid >> 6) ? wcnt[k] : 0u;
    total += wcnt[k];
  }
  if (any)
    list[off + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] = tid;
  __syncthreads();
  // items (configuration k of the list, revolute source r), spread over the
  // whole block: a configuration's sc elements are adjacent items
  bp_sincos_items((uint32_t)tid, (uint32_t)BLOCK, total, (uint32_t)w.n_rev, [&](uint32_t k, uint32_t ri) {
    const long long r = cfg0 + list[k];
    const int src = w.rev_src[ri];
    double sv, cv;
    mpg_sincos(in[r * w.dof + src], &sv, &cv);
    sc[(r * w.dof + src) * 2] = sv;
    sc[(r * w.dof + src) * 2 + 1] = cv;
  });
}

// ---------------------------------------------------------------------------
// Deterministic bucketing of the survivor bits into per-pair candidate lists
// (no global atomics, no block waits for another): the cull's byte counts per
// (64-config tile, pair) -> sums per range of tiles, prefixed inside groups of
// ranges -> scan of the group totals per pair + task prefix -> scatter.
// Candidates of a pair end up contiguous and sorted by config.  Layouts and
// index arithmetic: mpg_bucket.h.
// ---------------------------------------------------------------------------
// The range sums of the groups [g0, g0 + ng) by one block of NT threads
// (ranges of these groups x min(row dwords, kSumCols) <= kSumSlots).  Lanes
// run along the count row (one dword = four pairs each), so every load is a
// contiguous piece of a row; the four byte counts are summed as two words of
// two 16-bit halves.  Then one thread per (group, dword) walks the group's
// ranges: part[range] = the exclusive prefix inside the group, grp[group] =
// the group's total (four pairs = one 16-byte store per lane).
template <int NT>
__device__ __forceinline__ void range_sum_groups(const uint32_t* __restrict__ cnt, int n_tiles, int W,
                                                 uint32_t* __restrict__ part, uint32_t* __restrict__ grp, int g0,
                                                 int ng, uint2* sums) {
  const int rw = bk_row_words(W), C = bk_cols(W);
  const int n_ranges = bk_ranges(n_tiles);
  const int r0 = bk_group_first(g0), nr = bk_group_end(g0 + ng - 1, n_ranges) - r0;
  for (int j0 = 0; j0 < rw; j0 += kSumCols) {
    const int jc = min(kSumCols, rw - j0);
    for (int i = threadIdx.x; i < nr * jc; i += NT) {
      const int rl = i / jc, jl = i % jc;
      const int t0 = bk_range_first(r0 + rl), t1 = bk_range_end(r0 + rl, n_tiles);
      const uint32_t* col = cnt + j0 + jl;
      uint32_t lo = 0, hi = 0;  // pairs 4j, 4j + 2 and 4j + 1, 4j + 3
#pragma unroll
      for (int k = 0; k < kRangeTiles; ++k) {
        const uint32_t x = t0 + k < t1 ? col[(long long)(t0 + k) * rw] : 0u;
        lo += x & 0x00ff00ffu;
        hi += (x >> 8) & 0x00ff00ffu;
      }
      sums[i] = make_uint2(lo, hi);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ng * jc; i += NT) {
      const int gl = i / jc, jl = i % jc;
      const int rl1 = bk_group_end(g0 + gl, n_ranges) - r0;
      uint32_t lo = 0, hi = 0;
      for (int rl = bk_group_first(gl); rl < rl1; ++rl) {
        *reinterpret_cast<uint4*>(part + (long long)(r0 + rl) * C + 4 * (j0 + jl)) =
            make_uint4(lo & 0xffffu, hi & 0xffffu, lo >> 16, hi >> 16);
        const uint2 s = sums[rl * jc + jl];
        lo += s.x;
        hi += s.y;
      }
      *reinterpret_cast<uint4*>(grp + (long long)(g0 + gl) * C + 4 * (j0 + jl)) =
          make_uint4(lo & 0xffffu, hi & 0xffffu, lo >> 16, hi >> 16);
    }
    __syncthreads();
  }
}

// one block per group of ranges
__global__ __launch_bounds__(256) void range_sum_kernel(const uint32_t* __restrict__ cnt, int n_tiles, int W,
                                                       uint32_t* __restrict__ part, uint32_t* __restrict__ grp) {
  __shared__ uint2 sums[kSumSlots];
  range_sum_groups<256>(cnt, n_tiles, W, part, grp, blockIdx.x, 1, sums);
}

#ifndef MPG_TASK_MIN
#define MPG_TASK_MIN 8
#endif
constexpr uint32_t kTaskMin = MPG_TASK_MIN;

constexpr int kScanRegs = 24;  // a 2^20 chunk of 5 mask words: 128 groups in 6 slabs of 22

__device__ __forceinline__ uint32_t block_sum1024(uint32_t v, uint32_t* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) s += red[k];
  return s;
}

// one block.  First the scan of the group totals: threads run along the pair
// index (each load instruction reads one contiguous piece of a grp row), the
// groups are cut into slabs across the block's threads (up to kScanRegs groups
// of a slab in registers, loads issued together) and combined through LDS; grp
// becomes the exclusive base of each group inside its pair and seg_len[p] the
// pair's total.  Worlds with more pair columns than the block has threads loop
// over the columns.  Small launches (cnt given: bk_fold_sum) first do
// range_sum_kernel's work for every group here, which saves its launch.
// Then the segment starts + prefix of narrow-phase tasks (ts candidates of
// one pair each), 1024 pairs per round.  The task size adapts to the batch:
// ts = total candidates / target tasks (the narrow grid's resident waves),
// clamped to [kTaskMin, kTask] and rounded up to a multiple of 8 -- small
// batches (cfg2's 2^16 self pairs: ~27k candidates) spread over the whole
// chip instead of a few hundred full waves.  A batch that hits the upper
// clamp (more than target tasks * kTask candidates: cfg3's 2^20) gets a plan
// of several levels, whose tasks shrink towards the end of the list so that
// the persistent waves finish together (bk_task_plan).  prefix[n_pairs] = task
// count, prefix[n_pairs + 1] = the narrow phase's task counter,
// prefix[n_pairs + 2] = ts, prefix[n_pairs + 3] = the candidate count, then
// the plan's kPlanWords words.
__global__ __launch_bounds__(1024) void range_scan_kernel(const uint32_t* __restrict__ cnt, int n_tiles, int W,
                                                         uint32_t* __restrict__ part, uint32_t* __restrict__ grp,
                                                         int n_groups, int n_pairs, uint32_t* seg_len,
                                                         uint32_t* __restrict__ seg_start,
                                                         uint32_t* __restrict__ prefix, unsigned long long* units,
                                                         uint32_t target_tasks) {
  __shared__ uint2 sums[kSumSlots];
  __shared__ uint32_t wl[16], wt[16], red[16];
  uint32_t* slab = reinterpret_cast<uint32_t*>(sums);  // [1024], after the sums are done with
  const int tid = threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const int C = bk_cols(W);
  if (cnt) range_sum_groups<1024>(cnt, n_tiles, W, part, grp, 0, n_groups, sums);  // ends with a block barrier
  const bool one = C <= 1024;  // one column pass: thread p < n_pairs keeps seg_len[p] in a register
  uint32_t my_len = 0;
  {
    const int CP = min(C, 1024), S = 1024 / CP, per = (n_groups + S - 1) / S;
    const int s = tid / CP, cl = tid % CP;
    for (int c0 = 0; c0 < C; c0 += CP) {
      const int col = c0 + cl;
      const bool act = s < S && col < C;
      const int lo = s * per, hi = act ? min(n_groups, lo + per) : lo;
      const uint32_t i0 = (uint32_t)lo * C + col;  // grp[i0 + k * C], read only for lo + k < hi
      uint32_t v[kScanRegs];
      uint32_t sum = 0;
      if (per <= kScanRegs) {
#pragma unroll
        for (int k = 0; k < kScanRegs; ++k) {
          v[k] = lo + k < hi ? grp[i0 + (uint32_t)k * C] : 0u;
          sum += v[k];
        }
      } else {
        for (int i = lo; i < hi; ++i) sum += grp[i0 + (uint32_t)(i - lo) * C];
      }
      slab[tid] = sum;
      __syncthreads();
      uint32_t run = 0, tot = 0;
      for (int k = 0; k < S; ++k) {
        const uint32_t x = slab[k * CP + cl];
        run += k < s ? x : 0u;
        tot += x;
      }
      if (per <= kScanRegs) {
#pragma unroll
        for (int k = 0; k < kScanRegs; ++k) {
          if (lo + k < hi) grp[i0 + (uint32_t)k * C] = run;
          run += v[k];
        }
      } else {
        for (int i = lo; i < hi; ++i) {
          const uint32_t x = grp[i0 + (uint32_t)(i - lo) * C];
          grp[i0 + (uint32_t)(i - lo) * C] = run;
          run += x;
        }
      }
      if (act && s == 0 && col < n_pairs) {
        seg_len[col] = tot;
        my_len = tot;
      }
      __syncthreads();  // slab is reused; seg_len is read below
    }
  }
  uint32_t psum = 0;
  if (one) psum = my_len;
  else
    for (int p = tid; p < n_pairs; p += 1024) psum += seg_len[p];
  const uint32_t all = block_sum1024(psum, red);
  const TaskPlan plan = bk_task_plan(all, target_tasks, kTaskMin, kTask, kTaperC, kTaperMin);
  uint32_t cl = 0, ct = 0;  // carries over rounds
  for (int p0 = 0; p0 < n_pairs; p0 += 1024) {
    const int p = p0 + tid;
    const uint32_t len = one ? my_len : (p < n_pairs ? seg_len[p] : 0u);
    const uint32_t il = wave_inclusive_scan(len, lane);
    if (lane == 63) wl[wv] = il;
    __syncthreads();
    uint32_t bl = cl, bt = ct;  // candidates / tasks before this wave's pairs
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
      const uint32_t x = wl[k];
      bl += k < wv ? x : 0u;
      cl += x;
    }
    const uint32_t start = bl + il - len;  // the pair's global candidate offset: its tasks follow the plan's levels
    const uint32_t tasks = bk_pair_tasks(start, len, plan);
    const uint32_t it = wave_inclusive_scan(tasks, lane);
    if (lane == 63) wt[wv] = it;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
      const uint32_t x = wt[k];
      bt += k < wv ? x : 0u;
      ct += x;
    }
    if (p < n_pairs) {
      seg_start[p] = start;
      prefix[p] = bt + it - tasks;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    prefix[n_pairs] = ct;
    prefix[n_pairs + 1] = 0;  // narrow-phase task counter
    prefix[n_pairs + 2] = plan.s[0];
    prefix[n_pairs + 3] = cl;  // candidates in all (diagnostics)
    bk_plan_store(plan, prefix + n_pairs + 4);
    if (units) atomicAdd(units, (unsigned long long)cl);  // profiling: narrow-phase candidates
  }
}

// one wave per (survivor word, 64-config tile).  Lane b < 32 holds the slot
// base of pair 32 wd + b in the tile: the pair's segment start + its group's
// base + the range's prefix inside the group + the counts of the range's
// tiles before this one.  Every term is a load of its own, issued together
// with the tile's own counts and its surv word column, so a wave waits for
// memory once.  The surviving pairs are the ballot of count != 0; each one's
// configurations are written at base + rank.
__global__ __launch_bounds__(256) void scatter_kernel(const uint32_t* __restrict__ surv, long long n, long long cap,
                                                     int n_pairs, int W, int n_tiles,
                                                     const uint32_t* __restrict__ cnt,
                                                     const uint32_t* __restrict__ part,
                                                     const uint32_t* __restrict__ grp,
                                                     const uint32_t* __restrict__ seg_start,
                                                     uint32_t* __restrict__ cand) {
  const uint32_t lane = lane_id();
  const long long wid = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (wid >= (long long)n_tiles * W) return;
  const int wd = (int)(wid % W), t = (int)(wid / W);
  const int r = t / kRangeTiles, t0 = bk_range_first(r);
  const int C = bk_cols(W);
  const long long cfg = (long long)t * 64 + lane;
  const uint32_t x = cfg < n ? surv[(long long)wd * cap + cfg] : 0u;
  uint32_t c = 0u, base = 0u;
  if (lane < 32u) {
    const int p = wd * 32 + (int)lane;
    const uint8_t* c8 = reinterpret_cast<const uint8_t*>(cnt) + p;  // column p of the count rows
    c = c8[(long long)t * C];
    uint32_t pre = 0u;
#pragma unroll
    for (int k = 0; k < kRangeTiles - 1; ++k) pre += t0 + k < t ? c8[(long long)(t0 + k) * C] : 0u;
    if (p < n_pairs) base = seg_start[p] + grp[(long long)bk_group_of(r) * C + p] + part[(long long)r * C + p] + pre;
  }
  for (uint32_t m = (uint32_t)__ballot(c != 0u); m; m &= m - 1u) {  // lanes >= 32 hold no count
    const int b = __builtin_ctz(m);
    const uint32_t bit = (x >> b) & 1u;
    const unsigned long long bal = __ballot(bit);
    const uint32_t bs = __builtin_amdgcn_readlane(base, b);
    if (bit)
      cand[bs + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] =
          (uint32_t)cfg;
  }
}

// binary search of the pair whose task range holds task tk: prefix[p] <= tk < prefix[p + 1]
__device__ __forceinline__ int task_pair(const uint32_t* __restrict__ prefix, int n_pairs, uint32_t tk) {
  int lo = 0, hi = n_pairs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= tk) lo = mid;
    else hi = mid;
  }
  return lo;
}

// candidates [t0, t1) of task tk of pair p, local to the pair's list.  The
// plan, the pair's start and its length are read here, per task (wave-uniform
// scalar loads that hit the scalar cache): narrow_kernel keeps none of them
// across its MPR loop, where it has no scalar registers to spare.
__device__ __forceinline__ void task_range(const uint32_t* __restrict__ prefix, const uint32_t* __restrict__ seg_start,
                                           const uint32_t* __restrict__ seg_len, int n_pairs, int p, uint32_t tk,
                                           uint32_t& t0, uint32_t& t1) {
  const TaskPlan plan = bk_plan_load(prefix + n_pairs + 4);
  bk_task_range(seg_start[p], seg_len[p], tk - prefix[p], plan, &t0, &t1);
}

// ---------------------------------------------------------------------------
// Phase B: exact narrow phase.  Each wave takes 64 candidates of ONE pair, so
// every lane scans the same hull (wave-uniform scalar loads of the vertices)
// and only the MPR iteration count diverges.  Poses are rebuilt in fp64 from
// the joint values (chain FK), bit-identical to phase A / the reference.
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// Phase B: exact narrow phase (fp64, bit-identical to the reference).
//
// A wave takes a task of up to kTask candidates of ONE pair, so every lane
// scans the same hull (wave-uniform scalar loads).  libccd's MPR is run as a
// per-lane state machine whose every step is exactly one Minkowski support
// call: all lanes step together through the (uniform) support scan and only
// the cheap portal update diverges.  A lane that finishes takes the next
// candidate of the task; refills are batched (>= 32 idle lanes, or none
// active) so the fp64 chain FK of the refilled lanes runs at high lane
// occupancy too.  Results: atomicOr into the pair mask, flag = 1.
//
// States follow ccdMPRIntersect (libccd 2.1 mpr.c): discoverPortal's v1, v2
// and v3 support points (1, 2, 3), then refinePortal's v4 (4).
// ---------------------------------------------------------------------------
enum : int { MPR_DONE = 0, MPR_V1 = 1, MPR_V2 = 2, MPR_V3 = 3, MPR_V4 = 4 };

__device__ __forceinline__ bool octree_wave(const DevWorld& w, cptr<double> HV, int go, const SE3& TO, int gs,
                                           const SE3& TS);

template <int CLS>
__device__ __forceinline__ unsigned long long walk_wave_eval(const DevWorld& w, cptr<double> HV, int ga, const SE3& TA,
                                                            int gb, const SE3& TB, bool active);

// one pair evaluation of class CLS: closed form, octree walk or BVH mesh
// walk; each class lives in its own kernel instance so the walks' registers
// never lower the other kernels' occupancy
template <int CLS>
__device__ __forceinline__ bool pair_closed_form(int cf, const DevWorld& w, int ga, const SE3& TA, int gb,
                                                 const SE3& TB) {
  if constexpr (CLS == CLS_CLOSED) return closed_form(cf, w, ga, TA, gb, TB);
  if constexpr (CLS == CLS_GJK) return gjk_indep_intersect(w, ga, TA, gb, TB);
  return false;  // octree / mesh pairs: evaluated wave-wide (walk_wave_eval)
}

// FCL closed-form pairs (box-box, sphere-sphere, sphere-box) and octree
// pairs of the candidate lists: one test per candidate.  A kernel of its own so the closed forms'
// registers do not lower the MPR kernel's occupancy.
template <bool FROM_POSES, int CLS>
__global__ __launch_bounds__(256, CLS == CLS_OCTREE ? 2 : 1) void closed_form_kernel(DevWorld w, const double* __restrict__ in,
                                                         const uint32_t* __restrict__ seg_len,
                                                         const uint32_t* __restrict__ seg_start,
                                                         const uint32_t* __restrict__ prefix,
                                                         const uint32_t* __restrict__ cand,
                                                         uint8_t* __restrict__ flags, uint32_t* __restrict__ masks,
                                                         const double* __restrict__ sc) {
  const uint32_t lane = lane_id();
  const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
  const uint32_t total = prefix[w.n_pairs];
  const TaskPlan plan = bk_plan_load(prefix + w.n_pairs + 4);
  for (uint32_t tk = wave; tk < total; tk += n_waves) {
    int lo = 0, hi = w.n_pairs;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (prefix[mid] <= tk) lo = mid;
      else hi = mid;
    }
    const int p = lo;
    const int cf = w.pair_cf[p];
    if (cf == CF_NONE || cf_class(cf) != CLS) continue;
    uint32_t t0, t1;
    bk_task_range(seg_start[p], seg_len[p], tk - prefix[p], plan, &t0, &t1);
    const int a = w.pair_a[p], b = w.pair_b[p];
    const bool am = a < w.n_moving, bm = b < w.n_moving;
    const int ga = am ? w.moving_geom[a] : w.static_geom[a - w.n_moving];
    const int gb = bm ? w.moving_geom[b] : w.static_geom[b - w.n_moving];
    const uint32_t* __restrict__ cl = cand + seg_start[p];
    for (uint32_t base = t0; base < t1; base += 64) {
      const uint32_t idx = base + lane;
      if constexpr (CLS == CLS_OCTREE || CLS == CLS_MESH) {  // the wave walks each candidate together
        const bool active = idx < t1;
        const long long c = active ? cl[idx] : 0;
        SE3 TA = {}, TB = {};
        if (active) {
          TA = am ? moving_tf<FROM_POSES>(w, in, sc, c, a) : load_se3(w.static_T + 12 * (a - w.n_moving));
          TB = bm ? moving_tf<FROM_POSES>(w, in, sc, c, b) : load_se3(w.static_T + 12 * (b - w.n_moving));
        }
        const unsigned long long hits = walk_wave_eval<CLS>(w, w.hull, ga, TA, gb, TB, active);
        if ((hits >> lane) & 1ull) {
          if (masks) atomicOr(&masks[c * w.W + (p >> 5)], 1u << (p & 31));
          flags[c] = 1;
        }
        continue;
      }
      if (idx >= t1) continue;
      const long long c = cl[idx];
      const SE3 TA = am ? moving_tf<FROM_POSES>(w, in, sc, c, a) : load_se3(w.static_T + 12 * (a - w.n_moving));
      const SE3 TB = bm ? moving_tf<FROM_POSES>(w, in, sc, c, b) : load_se3(w.static_T + 12 * (b - w.n_moving));
      if (pair_closed_form<CLS>(cf, w, ga, TA, gb, TB)) {
        if (masks) atomicOr(&masks[c * w.W + (p >> 5)], 1u << (p & 31));
        flags[c] = 1;
      }
    }
  }
}

// One libccd MPR step (ccdMPRIntersect = discoverPortal + refinePortal) for
// a lane whose new Minkowski support point in direction `dir` is `s`.
// States: MPR_V1..V3 discoverPortal (finding v1, v2, v3), MPR_V4 refinePortal.
// Returns 1 = intersect, -1 = separated, 0 = continue with the updated dir.
// The state is copied into locals and written back unconditionally: stores
// under branches through the reference parameters get merged into stores
// through a selected pointer, which keeps the caller's registers on the stack.
__device__ __forceinline__ int mpr_advance(ccd_real mpr_tol, const CV3& s, int& st_io, CV3& v0_io, CV3& v1_io, CV3& v2_io,
                                           CV3& v3_io, CV3& dir_io) {
  int st = st_io;
  CV3 v0 = v0_io, v1 = v1_io, v2 = v2_io, v3 = v3_io, dir = dir_io;
  int res = 0;  // 1 = intersect, -1 = separated
  // Every state ends in one new search direction dir = normalize(a x b);
  // the states only pick (a, b), so the costly normalize (sqrt + divide)
  // runs once per step for all lanes instead of once per state branch.
  const ccd_real dsd = vdot(s, dir);
  CV3 ca, cb;
  bool post_swap = false, post_encl = false;
  if (st == MPR_V4) {  // refinePortal: expand the portal (v1, v2, v3) towards v4 = s
    if (!(is_zero(dsd) || dsd > 0)) {
      res = -1;
    } else {
      const ccd_real dv1 = vdot(v1, dir), dv2 = vdot(v2, dir), dv3 = vdot(v3, dir);
      ccd_real d1 = dsd - dv1;
      const ccd_real dd2 = dsd - dv2, dd3 = dsd - dv3;
      d1 = (d1 < dd2) ? d1 : dd2;  // CCD_FMIN
      d1 = (d1 < dd3) ? d1 : dd3;
      if (ccd_eq(d1, mpr_tol) || d1 < mpr_tol) {
        res = -1;
      } else {
        const CV3 v4v0 = vcross(s, v0);
        if (vdot(v1, v4v0) > 0) {
          if (vdot(v2, v4v0) > 0) v1 = s;
          else v3 = s;
        } else {
          if (vdot(v3, v4v0) > 0) v2 = s;
          else v1 = s;
        }
        ca = vsub(v2, v1);
        cb = vsub(v3, v1);
        post_encl = true;
      }
    }
  } else if (is_zero(dsd) || dsd < 0) {  // discoverPortal: support not past the origin
    res = -1;
  } else if (st == MPR_V1) {
    v1 = s;
    ca = v0;
    cb = v1;
  } else if (st == MPR_V2) {
    v2 = s;
    ca = vsub(v1, v0);
    cb = vsub(v2, v0);
    post_swap = true;
  } else {  // MPR_V3
    v3 = s;
    bool cont = false;
    ccd_real d2 = vdot(vcross(v1, v3), v0);
    if (d2 < 0 && !is_zero(d2)) {
      v2 = v3;
      cont = true;
    }
    if (!cont) {
      d2 = vdot(vcross(v3, v2), v0);
      if (d2 < 0 && !is_zero(d2)) {
        v1 = v3;
        cont = true;
      }
    }
    if (cont) {
      ca = vsub(v1, v0);
      cb = vsub(v2, v0);
    } else {  // portal found: refinePortal starts with (v1, v2, v3)
      ca = vsub(v2, v1);
      cb = vsub(v3, v1);
      post_encl = true;
      st = MPR_V4;
    }
  }
  if (res == 0) {
    const CV3 cr = vcross(ca, cb);
    if (st == MPR_V1 && is_zero(vdot(cr, cr))) {
      res = 1;  // origin on v1 or on segment v0-v1
    } else {
      dir = vnormalize(cr);
      if (st == MPR_V1) {
        st = MPR_V2;
      } else if (post_swap) {
        if (vdot(dir, v0) > 0) {
          const CV3 t = v1;
          v1 = v2;
          v2 = t;
          dir = vscale(dir, ccd_real(-1));
        }
        st = MPR_V3;
      } else if (post_encl) {  // portalEncapsulesOrigin
        const ccd_real d = vdot(dir, v1);
        if (is_zero(d) || d > 0) res = 1;
      }
    }
  }
  st_io = st;
  v0_io = v0;
  v1_io = v1;
  v2_io = v2;
  v3_io = v3;
  dir_io = dir;
  return res;
}

// ccdMPRIntersect's start: findOrigin (v0 = centre difference, nudged off the
// origin) and discoverPortal's first direction
__device__ __forceinline__ void mpr_begin(const CV3& ca, const CV3& cb, int& st, CV3& v0, CV3& dir) {
  v0 = vsub(ca, cb);
  if (vec_is_origin(v0)) v0 = vadd(v0, cv3(kCcdEps * ccd_real(10), 0.0, 0.0));
  dir = vnormalize(vscale(v0, ccd_real(-1)));
  st = MPR_V1;
}

// libccd support of (box with per-lane half sizes h) - (uniform shape b)
__device__ __forceinline__ CV3 msupport_box(const GObj& a, const ccd_real* h, const DevWorld& w, cptr<double> HV,
                                           const GObj& b, const CV3& dir) {
  const CV3 da = quat_rot(dir, a.rot_inv), db = quat_rot(vscale(dir, ccd_real(-1)), b.rot_inv);
  const CV3 la = CV3{(da.x >= 0 ? ccd_real(1) : ccd_real(-1)) * h[0], (da.y >= 0 ? ccd_real(1) : ccd_real(-1)) * h[1],
                     (da.z >= 0 ? ccd_real(1) : ccd_real(-1)) * h[2]};
  const int gb = __builtin_amdgcn_readfirstlane(b.geom), tb = __builtin_amdgcn_readfirstlane(b.type);
  const CV3 lb = support_local(w, HV, gb, tb, db);
  return vsub(vadd(quat_rot(la, a.rot), a.pos), vadd(quat_rot(lb, b.rot), b.pos));
}

// The occupied leaves of octree `go` listed in the grid cells under the box
// [blo, bhi] (octree frame), handed out one per lane: the cells of the range
// 64 at a time (one per lane, loads in parallel), then a wave prefix sum of
// their leaf counts gives the leaves 64 at a time.  leaf_hit(leaf) -> bool;
// true as soon as some lane's leaf hits.  Wave-uniform inputs.  (A leaf in
// several cells may be tested more than once: the answer is an OR.)
template <typename F>
__device__ __forceinline__ bool octree_range_any(const DevWorld& w, int go, const double* blo, const double* bhi,
                                                 F leaf_hit) {
  const cptr<double> og = w.oct_grid + OG_STRIDE * go;
  const double inv = og[OG_INV];
  int c0[3], c1[3], dims[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    dims[i] = (int)og[OG_DIMS + i];
    const double f0 = std::floor((blo[i] - og[OG_ORIGIN + i]) * inv);
    const double f1 = std::floor((bhi[i] - og[OG_ORIGIN + i]) * inv);
    if (f1 < 0.0 || f0 >= (double)dims[i]) return false;
    c0[i] = f0 < 0.0 ? 0 : (int)f0;
    c1[i] = f1 >= (double)dims[i] ? dims[i] - 1 : (int)f1;
  }
  __shared__ int s_k0[4][64], s_end[4][64];  // per wave of the 256-thread block
  const uint32_t lane = lane_id(), wv = threadIdx.x >> 6;
  const int cell0 = (int)og[OG_CELL0];
  const int nx = c1[0] - c0[0] + 1, ny = c1[1] - c0[1] + 1, nz = c1[2] - c0[2] + 1;
  const int ncell = nx * ny * nz;
  for (int cb = 0; cb < ncell; cb += 64) {
    const int ci = cb + (int)lane;
    int k0 = 0, cnt = 0;
    if (ci < ncell) {
      const int z = ci % nz, y = (ci / nz) % ny, x = ci / (nz * ny);
      const int cell = cell0 + ((c0[0] + x) * dims[1] + (c0[1] + y)) * dims[2] + (c0[2] + z);
      k0 = w.oct_cells[cell];
      cnt = w.oct_cells[cell + 1] - k0;
    }
    const uint32_t incl = wave_inclusive_scan((uint32_t)cnt, lane);
    const int total = (int)__builtin_amdgcn_readlane(incl, 63);
    s_k0[wv][lane] = k0;
    s_end[wv][lane] = (int)incl;
    __builtin_amdgcn_wave_barrier();
    for (int ib = 0; ib < total; ib += 64) {
      const int j = ib + (int)lane;
      bool hit = false;
      if (j < total) {
        int lo = 0, hi = 63;  // first cell slot whose inclusive end exceeds j
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_end[wv][mid] > j) hi = mid;
          else lo = mid + 1;
        }
        const int start = lo > 0 ? s_end[wv][lo - 1] : 0;
        hit = leaf_hit(w.oct_list[s_k0[wv][lo] + (j - start)]);
      }
      if (__ballot(hit) != 0) return true;
    }
    __builtin_amdgcn_wave_barrier();
  }
  return false;
}

// One lane's (shape, octree) pair: fcl OcTreeSolver::OcTreeShapeIntersectRecurse
// [ext FCL 0.7.0] reduced to its result -- some occupied leaf whose OBB
// overlaps the shape's OBB (computeBV(shape, I) -> convertBV(., tf), then
// obbDisjoint) and whose box intersects the shape: shapeIntersect(box,
// box_tf, shape, tf) with the leaf box first (box-box / box-sphere closed
// forms, otherwise libccd MPR).  An ancestor's OBB contains its leaves', so
// the recursion's pruning never hides a leaf this test would accept.  Leaves
// come from the octree's grid cells under the shape's box in the octree frame
// widened exactly as obbDisjoint's first three axes (|R| + 1e-6): a leaf
// outside it fails those axes.  Inputs are wave-uniform: the whole wave
// walks one candidate.
__device__ __forceinline__ bool octree_wave(const DevWorld& w, cptr<double> HV, int go, const SE3& TO, int gs,
                                           const SE3& TS) {
  const cptr<double> grs = w.geom_rec + G_STRIDE * gs;
  const int ts = w.geom_type[gs];
  double sc[3], se[3], Rl[9], cl[3], hq[3];
#pragma unroll
  // FCL's exact computeBV extents: with float libccd behind the gate, a leaf
  // the gate passes only by a widening could become an MPR hit
  for (int i = 0; i < 3; ++i) se[i] = grs[G_AABB_E + i];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    sc[i] = ((TS.R[3 * i] * grs[G_OBB_C] + TS.R[3 * i + 1] * grs[G_OBB_C + 1]) + TS.R[3 * i + 2] * grs[G_OBB_C + 2]) +
            TS.p[i];
  const double dsc[3] = {sc[0] - TO.p[0], sc[1] - TO.p[1], sc[2] - TO.p[2]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    cl[i] = (TO.R[i] * dsc[0] + TO.R[3 + i] * dsc[1]) + TO.R[6 + i] * dsc[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) Rl[3 * i + j] = (TO.R[i] * TS.R[j] + TO.R[3 + i] * TS.R[3 + j]) + TO.R[6 + i] * TS.R[6 + j];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
    hq[i] = ((std::fabs(Rl[3 * i]) + 1e-6) * se[0] + (std::fabs(Rl[3 * i + 1]) + 1e-6) * se[1] +
             (std::fabs(Rl[3 * i + 2]) + 1e-6) * se[2]) * (1.0 + 1e-12) + 1e-12;
  // tighter: the shape's own extent along the octree axes (its support in
  // +-axis), padded; a leaf beyond it on an octree axis is separated from
  // the shape, so every leaf test on it fails
  double blo[3], bhi[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double ax[3] = {TO.R[i], TO.R[3 + i], TO.R[6 + i]};
    const V3 dl = v3((TS.R[0] * ax[0] + TS.R[3] * ax[1]) + TS.R[6] * ax[2],
                     (TS.R[1] * ax[0] + TS.R[4] * ax[1]) + TS.R[7] * ax[2],
                     (TS.R[2] * ax[0] + TS.R[5] * ax[1]) + TS.R[8] * ax[2]);
    const V3 sp = support_local_exact(w, HV, gs, ts, dl), sn = support_local_exact(w, HV, gs, ts, vscale(dl, -1.0));
    double ep = 0.0, en = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double lp = (k == 0 ? sp.x : k == 1 ? sp.y : sp.z), ln = (k == 0 ? sn.x : k == 1 ? sn.y : sn.z);
      ep += ax[0] * TS.R[k] * lp + ax[1] * TS.R[3 + k] * lp + ax[2] * TS.R[6 + k] * lp;
      en += ax[0] * TS.R[k] * ln + ax[1] * TS.R[3 + k] * ln + ax[2] * TS.R[6 + k] * ln;
    }
    const double base = (ax[0] * (TS.p[0] - TO.p[0]) + ax[1] * (TS.p[1] - TO.p[1])) + ax[2] * (TS.p[2] - TO.p[2]);
    // libccd MPR can report a leaf within kCcdFalseHitReach of the shape as
    // touching (mpg_math.h): keep every such leaf
    const double pad = kCcdFalseHitReach * (1.0 + 1e-3) + 1e-5 + 1e-5 * (std::fabs(base) + std::fabs(ep) + std::fabs(en));
    blo[i] = fmax(cl[i] - hq[i], base + en - pad);
    bhi[i] = fmin(cl[i] + hq[i], base + ep + pad);
    if (blo[i] > bhi[i]) return false;
  }
  GObj A, B;  // A: the leaf box (rotation of the octree, per-leaf centre), B: the shape
  A.rot = gjk_rot_from_matrix(TO.R);
  A.rot_inv = quat_invert2(A.rot);
  A.geom = go;
  A.type = MPG_GEOM_BOX;
  B.rot = gjk_rot_from_matrix(TS.R);
  B.rot_inv = quat_invert2(B.rot);
  B.pos = cv3(TS.p[0], TS.p[1], TS.p[2]);
  B.geom = gs;
  B.type = ts;
  // one candidate per wave: the leaves listed in the cells under the box
  // are queued 64 at a time (one per lane) and tested side by side
  auto leaf_hit = [&](int leaf) -> bool {
    const cptr<double> L = w.oct_leaf + 6 * (size_t)leaf;
    bool out = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) out |= L[i] > bhi[i] || L[3 + i] < blo[i];
    if (out) return false;
    // leaf OBB: axes TO.R, centre TO * c, extent (max - min) * 0.5
    double c[3], cw[3], a[3], side[3], T[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      c[i] = (L[i] + L[3 + i]) * 0.5;
      side[i] = L[3 + i] - L[i];
      a[i] = side[i] * 0.5;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) cw[i] = ((TO.R[3 * i] * c[0] + TO.R[3 * i + 1] * c[1]) + TO.R[3 * i + 2] * c[2]) + TO.p[i];
    const double t[3] = {sc[0] - cw[0], sc[1] - cw[1], sc[2] - cw[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) T[i] = (TO.R[i] * t[0] + TO.R[3 + i] * t[1]) + TO.R[6 + i] * t[2];
    if (obb_disjoint(Rl, T, a, se)) return false;
    SE3 TL;  // box_tf = tf * Translation(centre)
#pragma unroll
    for (int i = 0; i < 9; ++i) TL.R[i] = TO.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) TL.p[i] = cw[i];
    if (ts == MPG_GEOM_BOX) {
      const double sb[3] = {grs[G_PARAM], grs[G_PARAM + 1], grs[G_PARAM + 2]};
      return box_box_intersect(side, TL, sb, TS);
    }
    if (ts == MPG_GEOM_SPHERE) return sphere_box_intersect(grs[G_PARAM], TS, side, TL);
    GObj A1 = A;
    A1.pos = cv3(cw[0], cw[1], cw[2]);
    const ccd_real h[3] = {(ccd_real)(side[0] / 2.0), (ccd_real)(side[1] / 2.0), (ccd_real)(side[2] / 2.0)};  // boxToGJK
    int st;
    CV3 v0, v1, v2, v3_, dir;
    mpr_begin(A1.pos, center(w, B), st, v0, dir);
    int res = 0;
    while (res == 0) {
      const CV3 sp = msupport_box(A1, h, w, HV, B, dir);
      res = mpr_advance(w.mpr_tol, sp, st, v0, v1, v2, v3_, dir);
    }
    return res > 0;
  };
  return octree_range_any(w, go, blo, bhi, leaf_hit);
}

// fcl OcTreeSolver::OcTreeIntersectRecurse [ext FCL 0.7.0] without contacts
// or costs, reduced to its result: some occupied leaf of tree 1 (the pair's
// o1) whose OBB overlaps some occupied leaf's OBB of tree 2 -- no box test
// (oracle octree_octree_intersect).  The wave takes tree 1's leaves 64 at a
// time, one per lane; a lane lists tree 2's leaves in the grid cells under
// the box obbDisjoint's tree-2 axis tests leave open (centre R2^T (c1 - p2),
// half extents sum_i (|R_ik| + 1e-6) a_i, padded far above rounding) and
// runs obbDisjoint(R1^T R2, R1^T (c2 - c1), a1, a2) on each.  Wave-uniform
// inputs.
__device__ bool octree_octree_wave(const DevWorld& w, int g1, const SE3& T1, int g2, const SE3& T2) {
  const cptr<double> r1 = w.geom_rec + G_STRIDE * g1;
  const long long l0 = (long long)r1[G_PARAM], l1 = l0 + (long long)r1[G_PARAM + 1];
  double R[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (T1.R[i] * T2.R[j] + T1.R[3 + i] * T2.R[3 + j]) + T1.R[6 + i] * T2.R[6 + j];
  const cptr<double> og = w.oct_grid + OG_STRIDE * g2;
  const double inv = og[OG_INV];
  const int dims[3] = {(int)og[OG_DIMS], (int)og[OG_DIMS + 1], (int)og[OG_DIMS + 2]};
  const int cell0 = (int)og[OG_CELL0];
  for (long long base = l0; base < l1; base += 64) {
    const long long la = base + (long long)lane_id();
    bool hit = false;
    if (la < l1) {
      const cptr<double> L = w.oct_leaf + 6 * (size_t)la;
      double a[3], cw[3];
      {
        double c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          c[k] = (L[k] + L[3 + k]) * 0.5;
          a[k] = (L[3 + k] - L[k]) * 0.5;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) cw[i] = ((T1.R[3 * i] * c[0] + T1.R[3 * i + 1] * c[1]) + T1.R[3 * i + 2] * c[2]) + T1.p[i];
      }
      const double dq[3] = {cw[0] - T2.p[0], cw[1] - T2.p[1], cw[2] - T2.p[2]};
      double blo[3], bhi[3];
      int c0[3], c1[3];
      bool empty = false;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double q = (T2.R[k] * dq[0] + T2.R[3 + k] * dq[1]) + T2.R[6 + k] * dq[2];
        const double h = ((std::fabs(R[k]) + 1e-6) * a[0] + (std::fabs(R[3 + k]) + 1e-6) * a[1] +
                          (std::fabs(R[6 + k]) + 1e-6) * a[2]) * (1.0 + 1e-9) + 1e-9 * (1.0 + std::fabs(q));
        blo[k] = q - h;
        bhi[k] = q + h;
        const double f0 = std::floor((blo[k] - og[OG_ORIGIN + k]) * inv);
        const double f1 = std::floor((bhi[k] - og[OG_ORIGIN + k]) * inv);
        empty |= f1 < 0.0 || f0 >= (double)dims[k];
        c0[k] = f0 < 0.0 ? 0 : (int)fmin(f0, (double)(dims[k] - 1));
        c1[k] = f1 >= (double)dims[k] ? dims[k] - 1 : (f1 < 0.0 ? 0 : (int)f1);
      }
      for (int x = c0[0]; !empty && !hit && x <= c1[0]; ++x)
        for (int y = c0[1]; !hit && y <= c1[1]; ++y)
          for (int z = c0[2]; !hit && z <= c1[2]; ++z) {
            const int cell = cell0 + (x * dims[1] + y) * dims[2] + z;
            for (int k = w.oct_cells[cell], ke = w.oct_cells[cell + 1]; k < ke && !hit; ++k) {
              const cptr<double> K = w.oct_leaf + 6 * (size_t)w.oct_list[k];
              bool out = false;
#pragma unroll
              for (int i = 0; i < 3; ++i) out |= K[i] > bhi[i] || K[3 + i] < blo[i];
              if (out) continue;
              double b[3], d[3], t[3], T[3];
#pragma unroll
              for (int i = 0; i < 3; ++i) {
                d[i] = (K[i] + K[3 + i]) * 0.5;
                b[i] = (K[3 + i] - K[i]) * 0.5;
              }
#pragma unroll
              for (int i = 0; i < 3; ++i)
                t[i] = (((T2.R[3 * i] * d[0] + T2.R[3 * i + 1] * d[1]) + T2.R[3 * i + 2] * d[2]) + T2.p[i]) - cw[i];
#pragma unroll
              for (int i = 0; i < 3; ++i) T[i] = (T1.R[i] * t[0] + T1.R[3 + i] * t[1]) + T1.R[6 + i] * t[2];
              hit = !obb_disjoint(R, T, a, b);
            }
          }
    }
    if (__ballot(hit) != 0) return true;
  }
  return false;
}

// ---------------------------------------------------------------------------
// BVH meshes (fcl::BVHModel<OBBRSS>, load_mesh_as_BVH src/urdf_utils.cpp:
// 136-155).  fcl::collide's BVH traversal only prunes triangle (pairs) whose
// bounding volumes are disjoint, so the boolean answer is "some leaf test
// succeeds"; the wave walks one candidate's triangles at a time (64 lanes
// side by side) behind a conservative AABB test in the mesh frame (widened
// by 1e-9, far above rounding: a pruned triangle is genuinely separated).  Leaf tests as FCL 0.7.0 runs them:
//   mesh-mesh   Intersect::intersect_Triangle(p, q, R, T), R = R1^T R2,
//               T = R1^T (t2 - t1), q' = R q + T
//   shape-mesh  shapeTriangleIntersect(shape, tf, P1, P2, P3, tf_mesh): shape
//               first; sphereTriangleIntersect for spheres, else libccd MPR
//               on the triangle GJK object (triCreateGJKObject)
// Same operation order as the oracle (oracle/collide_oracle.c).
// ---------------------------------------------------------------------------
constexpr double kMeshPad = 1e-9;
// shape-triangle pairs run libccd MPR: a triangle it can report as touching
// lies within kCcdFalseHitReach of the shape (mpg_math.h)
constexpr double kMeshShapePad = kCcdFalseHitReach * (1.0 + 1e-3) + 1e-5;

__device__ __forceinline__ double d3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void c3(double* o, const double* a, const double* b) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// Intersect::project6
__device__ __forceinline__ bool project6(const double* ax, const double* p2, const double* p3, const double* q1,
                                         const double* q2, const double* q3) {
  const double P1 = (ax[0] * 0.0 + ax[1] * 0.0) + ax[2] * 0.0;  // p1 = 0
  const double P2 = d3(ax, p2), P3 = d3(ax, p3), Q1 = d3(ax, q1), Q2 = d3(ax, q2), Q3 = d3(ax, q3);
  const double mx1 = fmax(P1, fmax(P2, P3)), mn1 = fmin(P1, fmin(P2, P3));
  const double mx2 = fmax(Q1, fmax(Q2, Q3)), mn2 = fmin(Q1, fmin(Q2, Q3));
  return !(mn1 > mx2) && !(mn2 > mx1);
}

// Intersect::intersect_Triangle without contact output: n1, m1, the nine
// edge cross products, g1..g3, h1..h3
__device__ __forceinline__ bool tri_tri_intersect(const double* P, const double* Q) {
  double p2[3], p3[3], q1[3], q2[3], q3[3], e[3][3], f[3][3], n1[3], m1[3], ax[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p2[k] = P[3 + k] - P[k];
    p3[k] = P[6 + k] - P[k];
    q1[k] = Q[k] - P[k];
    q2[k] = Q[3 + k] - P[k];
    q3[k] = Q[6 + k] - P[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    e[0][k] = p2[k] - 0.0;
    e[1][k] = p3[k] - p2[k];
    e[2][k] = 0.0 - p3[k];
    f[0][k] = q2[k] - q1[k];
    f[1][k] = q3[k] - q2[k];
    f[2][k] = q1[k] - q3[k];
  }
  c3(n1, e[0], e[1]);
  c3(m1, f[0], f[1]);
  if (!project6(n1, p2, p3, q1, q2, q3)) return false;
  if (!project6(m1, p2, p3, q1, q2, q3)) return false;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      c3(ax, e[i], f[j]);
      if (!project6(ax, p2, p3, q1, q2, q3)) return false;
    }
  for (int i = 0; i < 3; ++i) {
    c3(ax, e[i], n1);
    if (!project6(ax, p2, p3, q1, q2, q3)) return false;
  }
  for (int i = 0; i < 3; ++i) {
    c3(ax, f[i], m1);
    if (!project6(ax, p2, p3, q1, q2, q3)) return false;
  }
  return true;
}

// segmentSqrDistance (sphere_triangle-inl.h)
__device__ __forceinline__ double segment_sqr_distance(const double* from, const double* to, const double* p) {
  double diff[3], v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    diff[k] = p[k] - from[k];
    v[k] = to[k] - from[k];
  }
  double t = d3(v, diff);
  if (t > 0) {
    const double vv = d3(v, v);
    if (t < vv) {
      t /= vv;
#pragma unroll
      for (int k = 0; k < 3; ++k) diff[k] -= v[k] * t;
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) diff[k] -= v[k];
    }
  }
  return d3(diff, diff);
}

// sphereTriangleIntersect (sphere_triangle-inl.h), boolean part; W = world
// triangle (tf_mesh * P), c = sphere centre
__device__ __forceinline__ bool sphere_triangle_intersect(double radius, const double* c, const double* W) {
  double a[3], b[3], n[3], pc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = W[3 + k] - W[k];
    b[k] = W[6 + k] - W[k];
  }
  c3(n, a, b);
  const double z = d3(n, n);
  if (z > 0) {
    const double s = std::sqrt(z);
    n[0] /= s;
    n[1] /= s;
    n[2] /= s;
  }
  const double rt = radius + DBL_EPSILON;
#pragma unroll
  for (int k = 0; k < 3; ++k) pc[k] = c[k] - W[k];
  double dist = d3(pc, n);
  if (dist < 0) {
    dist *= -1;
    n[0] *= -1;
    n[1] *= -1;
    n[2] *= -1;
  }
  if (!(dist < rt)) return false;
  {  // projectInTriangle
    double e1[3], e2[3], e3[3], u[3], v[3], x[3], en[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      e1[k] = W[3 + k] - W[k];
      e2[k] = W[6 + k] - W[3 + k];
      e3[k] = W[k] - W[6 + k];
      u[k] = c[k] - W[k];
      v[k] = c[k] - W[3 + k];
      x[k] = c[k] - W[6 + k];
    }
    c3(en, e1, n);
    const double r1 = d3(en, u);
    c3(en, e2, n);
    const double r2 = d3(en, v);
    c3(en, e3, n);
    const double r3 = d3(en, x);
    if ((r1 > 0 && r2 > 0 && r3 > 0) || (r1 <= 0 && r2 <= 0 && r3 <= 0)) return true;
  }
  const double r2 = rt * rt;
  if (segment_sqr_distance(W, W + 3, c) < r2) return true;
  if (segment_sqr_distance(W + 3, W + 6, c) < r2) return true;
  if (segment_sqr_distance(W + 6, W, c) < r2) return true;
  return false;
}

// libccd support of (uniform shape a) - (per-lane triangle b: vertices P in
// the mesh frame, centroid tc): supportTriangle picks argmax dir . (p - c)
__device__ __forceinline__ CV3 msupport_tri(const DevWorld& w, cptr<double> HV, const GObj& a, const GObj& b,
                                            const CV3* P, const CV3& tc, const CV3& dir) {
  const CV3 da = quat_rot(dir, a.rot_inv), db = quat_rot(vscale(dir, ccd_real(-1)), b.rot_inv);
  const int ga = __builtin_amdgcn_readfirstlane(a.geom), ta = __builtin_amdgcn_readfirstlane(a.type);
  const CV3 la = support_local(w, HV, ga, ta, da);
  ccd_real maxdot = -FLT_MAX;
  CV3 lb = P[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const CV3 pc = vsub(P[i], tc);
    const ccd_real dot = vdot(db, pc);
    if (dot > maxdot) {
      lb = P[i];
      maxdot = dot;
    }
  }
  return vsub(vadd(quat_rot(la, a.rot), a.pos), vadd(quat_rot(lb, b.rot), b.pos));
}

// One (config, pair) at a time per wave, the 64 lanes split the triangle
// loops.  Inputs are wave-uniform (broadcast from the lane that owns the
// candidate).
__device__ __forceinline__ double bcast(double v, int k) {
  const unsigned long long u = __double_as_longlong(v);
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, k), hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), k);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ SE3 bcast_se3(const SE3& T, int k) {
  SE3 o;
#pragma unroll
  for (int i = 0; i < 9; ++i) o.R[i] = bcast(T.R[i], k);
#pragma unroll
  for (int i = 0; i < 3; ++i) o.p[i] = bcast(T.p[i], k);
  return o;
}

// ---------------------------------------------------------------------------
// FCL's BVH traversal gates.  fcl::collide on a BVHModel<OBBRSS> runs a leaf
// test only when every bounding-volume test on its way down the tree passed
// (collisionRecurse; BVTesting = !overlap(R0, T0, bv1, bv2), OBB-inl.h).  The
// device finds the intersecting triangles (pairs) with its own pruning (which
// only drops triangles that cannot hit); fcl_gate_* then replays the OBB tests
// of FCL's path to that leaf (pair), so a hit counts only where FCL would have
// reached it.  Oracle: the traversal itself (oracle/collide_oracle.c
// bvh_shape_walk / bvh_mesh_walk).
// ---------------------------------------------------------------------------
// overlap(R0, T0, a, b): R = a.axis^T (R0 b.axis), T = (R0 b.To + T0 - a.To)^T a.axis
__device__ __forceinline__ bool fcl_overlap(const double* R0, const double* T0, const double* aA, const double* aT,
                                            const double* aE, cptr<double> b) {
  double R0b[9], R[9], Tt[3], T[3], bE[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      R0b[3 * i + j] = (R0[3 * i] * b[FB_AXIS + j] + R0[3 * i + 1] * b[FB_AXIS + 3 + j]) + R0[3 * i + 2] * b[FB_AXIS + 6 + j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (aA[i] * R0b[j] + aA[3 + i] * R0b[3 + j]) + aA[6 + i] * R0b[6 + j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    Tt[i] = (((R0[3 * i] * b[FB_TO] + R0[3 * i + 1] * b[FB_TO + 1]) + R0[3 * i + 2] * b[FB_TO + 2]) + T0[i]) - aT[i];
#pragma unroll
  for (int j = 0; j < 3; ++j) T[j] = (Tt[0] * aA[j] + Tt[1] * aA[3 + j]) + Tt[2] * aA[6 + j];
#pragma unroll
  for (int k = 0; k < 3; ++k) bE[k] = b[FB_EXT + k];
  return !obb_disjoint(R, T, aE, bE);
}

// the shape's OBB in the world (computeBV<OBB>(shape, tf): convex / box /
// capsule / cylinder axis = R axis_local, sphere axis I; To = R To_local + T)
__device__ __forceinline__ void fcl_shape_obb_world(const DevWorld& w, int gs, int ts, const SE3& TS, double* A,
                                                    double* To, double* E) {
  const cptr<double> o = w.sobb + FB_STRIDE * gs;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      A[3 * i + j] = ts == MPG_GEOM_SPHERE ? o[FB_AXIS + 3 * i + j]
                                           : (TS.R[3 * i] * o[FB_AXIS + j] + TS.R[3 * i + 1] * o[FB_AXIS + 3 + j]) +
                                                 TS.R[3 * i + 2] * o[FB_AXIS + 6 + j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    To[i] = ((TS.R[3 * i] * o[FB_TO] + TS.R[3 * i + 1] * o[FB_TO + 1]) + TS.R[3 * i + 2] * o[FB_TO + 2]) + TS.p[i];
#pragma unroll
  for (int k = 0; k < 3; ++k) E[k] = o[FB_EXT + k];
}

// MeshShape: the path from the root to triangle t's leaf (t: index in the
// mesh), every node's OBB against the shape's (world) under (TM.R, TM.p).
// mpg_world_create refuses trees deeper than kFclMaxDepth, so every descent
// reaches its leaf inside the loop; the trailing `return true` (the hit
// stands) is only there so that no bound can turn a hit into a miss.
constexpr int kFclMaxDepth = 255;
__device__ __forceinline__ bool fcl_gate_shape(const DevWorld& w, int gm, const SE3& TM, const double* sA,
                                               const double* sT, const double* sE, int t) {
  const int pos = w.tri_pos[(int)w.geom_rec[G_STRIDE * gm + G_PARAM] + t];
  int node = w.fb_root[gm];
  for (int depth = 0; depth <= kFclMaxDepth; ++depth) {
    if (!fcl_overlap(TM.R, TM.p, sA, sT, sE, w.fb_box + FB_STRIDE * node)) return false;
    const int c = w.fb_link[3 * node];
    if (c < 0) return true;
    node = pos < w.fb_link[3 * c + 1] + w.fb_link[3 * c + 2] ? c : c + 1;
  }
  return true;
}

__device__ __forceinline__ double fcl_obb_size(cptr<double> b) {
  return (b[FB_EXT] * b[FB_EXT] + b[FB_EXT + 1] * b[FB_EXT + 1]) + b[FB_EXT + 2] * b[FB_EXT + 2];
}

// MeshMesh: FCL's descent to the leaf pair (ta in A, tb in B) -- the first
// tree is descended when the second node is a leaf or the first is not and
// is larger (firstOverSecond); key (optional) collects the left / right
// choices, whose lexicographic order is FCL's visit order of leaf pairs
__device__ __forceinline__ bool fcl_gate_mesh(const DevWorld& w, int ga, int gb, const double* R, const double* T,
                                              int ta, int tb, uint64_t* key = nullptr) {
  const int pa = w.tri_pos[(int)w.geom_rec[G_STRIDE * ga + G_PARAM] + ta];
  const int pb = w.tri_pos[(int)w.geom_rec[G_STRIDE * gb + G_PARAM] + tb];
  int a = w.fb_root[ga], b = w.fb_root[gb], nk = 0;
  for (int depth = 0; depth <= 2 * kFclMaxDepth; ++depth) {
    const cptr<double> ba = w.fb_box + FB_STRIDE * a;
    double aA[9], aT[3], aE[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) aA[k] = ba[FB_AXIS + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      aT[k] = ba[FB_TO + k];
      aE[k] = ba[FB_EXT + k];
    }
    const cptr<double> bb = w.fb_box + FB_STRIDE * b;
    if (!fcl_overlap(R, T, aA, aT, aE, bb)) return false;
    const int ca = w.fb_link[3 * a], cb = w.fb_link[3 * b];
    if (ca < 0 && cb < 0) return true;
    bool right;
    if (cb < 0 || (ca >= 0 && fcl_obb_size(ba) > fcl_obb_size(bb))) {
      right = !(pa < w.fb_link[3 * ca + 1] + w.fb_link[3 * ca + 2]);
      a = right ? ca + 1 : ca;
    } else {
      right = !(pb < w.fb_link[3 * cb + 1] + w.fb_link[3 * cb + 2]);
      b = right ? cb + 1 : cb;
    }
    if (key && nk < 128) {
      if (right) key[nk >> 6] |= 1ull << (63 - (nk & 63));
      ++nk;
    }
  }
  return true;
}

// MeshOcTree: OcTreeMeshIntersectRecurse's descent to the (occupied leaf l,
// triangle t) pair [ext FCL 0.7.0; oracle octmesh_rec].  Every node pair is
// tested as two world OBBs: the octree node's AABB under TO (To = TO centre,
// axis = R, half sizes) against the mesh node's OBBRSS under TM (To = TM To,
// axis = R axis).  The octree node is split (its child on l's path, oct_path)
// when the mesh node is a leaf or the octree node is not and its AABB size
// (full width squared) exceeds the OBB's (half extents squared); else the mesh
// node (left / right by t's position).  key (optional) collects the octree
// child indices (3 bits) and the mesh choices (1 bit); at the first point two
// descents differ they take the same kind of step, so the lexicographic order
// of keys is the traversal's visit order (children 0..7, left before right).
__device__ __forceinline__ bool fcl_overlap_world(const SE3& TO, const double* lo, const double* hi, const SE3& TM,
                                                  cptr<double> b) {
  double ctr[3], E1[3], To1[3], To2[3], ax2[9], t[3], T[3], R[9], E2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ctr[k] = (lo[k] + hi[k]) * 0.5;
    E1[k] = (hi[k] - lo[k]) * 0.5;
    E2[k] = b[FB_EXT + k];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    To1[i] = ((TO.R[3 * i] * ctr[0] + TO.R[3 * i + 1] * ctr[1]) + TO.R[3 * i + 2] * ctr[2]) + TO.p[i];
    To2[i] = ((TM.R[3 * i] * b[FB_TO] + TM.R[3 * i + 1] * b[FB_TO + 1]) + TM.R[3 * i + 2] * b[FB_TO + 2]) + TM.p[i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      ax2[3 * i + j] = (TM.R[3 * i] * b[FB_AXIS + j] + TM.R[3 * i + 1] * b[FB_AXIS + 3 + j]) + TM.R[3 * i + 2] * b[FB_AXIS + 6 + j];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = To2[k] - To1[k];
#pragma unroll
  for (int i = 0; i < 3; ++i) T[i] = (TO.R[i] * t[0] + TO.R[3 + i] * t[1]) + TO.R[6 + i] * t[2];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (TO.R[i] * ax2[j] + TO.R[3 + i] * ax2[3 + j]) + TO.R[6 + i] * ax2[6 + j];
  return !obb_disjoint(R, T, E1, E2);
}

constexpr int kOctKeyWords = 5;  // 16 octree levels x 3 bits + 2 x kFclMaxDepth mesh bits
__device__ __forceinline__ bool fcl_gate_octree_mesh(const DevWorld& w, int go, const SE3& TO, int gm, const SE3& TM,
                                                     int l, int t, uint64_t* key = nullptr) {
  const double delta = (double)(1 << 16) * w.geom_rec[G_STRIDE * go + G_PARAM + 2] / 2;
  double lo[3] = {-delta, -delta, -delta}, hi[3] = {delta, delta, delta};
  const uint64_t path = w.oct_path[l];
  const int od = w.oct_depth[l];
  const int pos = w.tri_pos[(int)w.geom_rec[G_STRIDE * gm + G_PARAM] + t];
  int lev = 0, node = w.fb_root[gm], nk = 0;
  auto put = [&](unsigned v, int bits) {
    if (!key) return;
    for (int b = bits - 1; b >= 0; --b, ++nk)
      if (((v >> b) & 1u) && nk < 64 * kOctKeyWords) key[nk >> 6] |= 1ull << (63 - (nk & 63));
  };
  for (int step = 0; step <= 16 + kFclMaxDepth; ++step) {
    const cptr<double> bb = w.fb_box + FB_STRIDE * node;
    if (!fcl_overlap_world(TO, lo, hi, TM, bb)) return false;
    const bool oleaf = lev == od;
    const int c = w.fb_link[3 * node];
    if (oleaf && c < 0) return true;
    const double d0 = hi[0] - lo[0], d1 = hi[1] - lo[1], d2 = hi[2] - lo[2];
    if (c < 0 || (!oleaf && ((d0 * d0 + d1 * d1) + d2 * d2) > fcl_obb_size(bb))) {
      const unsigned ci = (unsigned)(path >> (3 * (od - 1 - lev))) & 7u;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double mid = (lo[k] + hi[k]) * 0.5;
        if ((ci >> k) & 1u) lo[k] = mid;
        else hi[k] = mid;
      }
      ++lev;
      put(ci, 3);
    } else {
      const bool right = !(pos < w.fb_link[3 * c + 1] + w.fb_link[3 * c + 2]);
      node = right ? c + 1 : c;
      put(right ? 1u : 0u, 1);
    }
  }
  return true;
}

__device__ __forceinline__ bool mesh_mesh_wave(const DevWorld& w, int ga, const SE3& TA, int gb, const SE3& TB) {
  // lanes take 64 of B's triangles into A's frame; each one that meets A's
  // box is then broadcast, A's cluster boxes are tested one per lane, and
  // the triangles of up to 8 overlapping clusters are tested at once (8
  // lanes per cluster)
  const uint32_t lane = lane_id();
  const cptr<double> gra = w.geom_rec + G_STRIDE * ga, grb = w.geom_rec + G_STRIDE * gb;
  const int b0 = (int)grb[G_PARAM], b1 = b0 + (int)grb[G_PARAM + 1];
  const int c0 = w.mesh_tree[2 * ga], c1 = c0 + w.mesh_tree[2 * ga + 1];
  double R[9], T[3], alo[3], ahi[3];
  const double dt[3] = {TB.p[0] - TA.p[0], TB.p[1] - TA.p[1], TB.p[2] - TA.p[2]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (TA.R[i] * TB.R[j] + TA.R[3 + i] * TB.R[3 + j]) + TA.R[6 + i] * TB.R[6 + j];
    T[i] = (TA.R[i] * dt[0] + TA.R[3 + i] * dt[1]) + TA.R[6 + i] * dt[2];
    alo[i] = gra[G_OBB_C + i] - gra[G_OBB_E + i];
    ahi[i] = gra[G_OBB_C + i] + gra[G_OBB_E + i];
  }
  for (int j0 = b0; j0 < b1; j0 += 64) {
    const int j = j0 + (int)lane;
    bool keep = j < b1;
    const cptr<double> rq = w.mesh_tri + TR_STRIDE * (size_t)(keep ? j : b0);
    double Q[9], qlo[3], qhi[3];
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
      for (int i = 0; i < 3; ++i)
        Q[3 * v + i] = ((R[3 * i] * rq[3 * v] + R[3 * i + 1] * rq[3 * v + 1]) + R[3 * i + 2] * rq[3 * v + 2]) + T[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      qlo[i] = fmin(Q[i], fmin(Q[3 + i], Q[6 + i])) - kMeshPad;
      qhi[i] = fmax(Q[i], fmax(Q[3 + i], Q[6 + i])) + kMeshPad;
      keep &= !(qlo[i] > ahi[i] || qhi[i] < alo[i]);
    }
    unsigned long long todo = __ballot(keep);
    while (todo) {
      const int k = __builtin_ctzll(todo);
      todo &= todo - 1;
      double Qk[9], lk[3], hk[3];
#pragma unroll
      for (int i = 0; i < 9; ++i) Qk[i] = bcast(Q[i], k);
      const int tbk = (int)bcast(rq[TR_ID], k);  // B's triangle (read while every lane is active)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        lk[i] = bcast(qlo[i], k);
        hk[i] = bcast(qhi[i], k);
      }
      for (int cb = c0; cb < c1; cb += 64) {
        const int c = cb + (int)lane;
        bool ov = c < c1;
        if (ov) {
          const cptr<double> bx = w.mesh_node + 6 * (size_t)c;
#pragma unroll
          for (int i = 0; i < 3; ++i) ov &= !(bx[i] > hk[i] || bx[3 + i] < lk[i]);
        }
        unsigned long long m = __ballot(ov);
        while (m) {
          int myc = -1;  // cluster of this lane's group of 8
          for (int g = 0; g < 8 && m; ++g) {
            const int cc = __builtin_ctzll(m);
            m &= m - 1;
            if (g == (int)(lane >> 3)) myc = cb + cc;
          }
          bool hit = false;
          if (myc >= 0) {
            const int t1 = w.mesh_link[2 * myc] + w.mesh_link[2 * myc + 1];
            for (int t = w.mesh_link[2 * myc] + (int)(lane & 7); t < t1 && !hit; t += 8) {
              const cptr<double> rp = w.mesh_tri + TR_STRIDE * (size_t)t;
              bool o2 = false;
#pragma unroll
              for (int i = 0; i < 3; ++i) o2 |= rp[TR_LO + i] > hk[i] || rp[TR_HI + i] < lk[i];
              if (o2) continue;
              double P[9];
#pragma unroll
              for (int q = 0; q < 9; ++q) P[q] = rp[TR_P + q];
              hit = tri_tri_intersect(P, Qk) && fcl_gate_mesh(w, ga, gb, R, T, (int)rp[TR_ID], tbk);
            }
          }
          if (__ballot(hit) != 0) return true;
        }
      }
    }
  }
  return false;
}

__device__ __forceinline__ bool mesh_shape_wave(const DevWorld& w, cptr<double> HV, int gm, const SE3& TM, int gs,
                                             const SE3& TS) {
  const uint32_t lane = lane_id();
  const cptr<double> grm = w.geom_rec + G_STRIDE * gm, grs = w.geom_rec + G_STRIDE * gs;
  const int ts = w.geom_type[gs];
  const int t0 = (int)grm[G_PARAM], t1 = t0 + (int)grm[G_PARAM + 1];
  double sc[3], cl[3], Rl[9], hq[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    sc[i] = ((TS.R[3 * i] * grs[G_OBB_C] + TS.R[3 * i + 1] * grs[G_OBB_C + 1]) + TS.R[3 * i + 2] * grs[G_OBB_C + 2]) + TS.p[i];
  const double dsc[3] = {sc[0] - TM.p[0], sc[1] - TM.p[1], sc[2] - TM.p[2]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    cl[i] = (TM.R[i] * dsc[0] + TM.R[3 + i] * dsc[1]) + TM.R[6 + i] * dsc[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) Rl[3 * i + j] = (TM.R[i] * TS.R[j] + TM.R[3 + i] * TS.R[3 + j]) + TM.R[6 + i] * TS.R[6 + j];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
    hq[i] = ((std::fabs(Rl[3 * i]) * grs[G_OBB_E] + std::fabs(Rl[3 * i + 1]) * grs[G_OBB_E + 1]) +
             std::fabs(Rl[3 * i + 2]) * grs[G_OBB_E + 2]) * (1.0 + 1e-9) +
            kMeshShapePad * (1.0 + std::fabs(TS.p[0]) + std::fabs(TS.p[1]) + std::fabs(TS.p[2]) + std::fabs(TM.p[0]) +
                             std::fabs(TM.p[1]) + std::fabs(TM.p[2]));
  GObj A, B;
  A.rot = gjk_rot_from_matrix(TS.R);
  A.rot_inv = quat_invert2(A.rot);
  A.pos = cv3(TS.p[0], TS.p[1], TS.p[2]);
  A.geom = gs;
  A.type = ts;
  B.rot = gjk_rot_from_matrix(TM.R);
  B.rot_inv = quat_invert2(B.rot);
  B.pos = cv3(TM.p[0], TM.p[1], TM.p[2]);
  B.geom = gm;
  B.type = MPG_GEOM_MESH;
  const CV3 ca = center(w, A);
  double sA[9], sT[3], sE[3];  // FCL's OBB of the shape (the traversal's BV tests)
  fcl_shape_obb_world(w, gs, ts, TS, sA, sT, sE);
  for (int b = t0; b < t1; b += 64) {
    const int t = b + (int)lane;
    bool cand = t < t1;
    const cptr<double> rec = w.mesh_tri + TR_STRIDE * (size_t)(cand ? t : t0);
#pragma unroll
    for (int i = 0; i < 3; ++i) cand &= !(rec[TR_LO + i] > cl[i] + hq[i] || rec[TR_HI + i] < cl[i] - hq[i]);
    if (__ballot(cand) == 0) continue;
    bool hit = false;
    if (cand) {
      double P[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) P[k] = rec[TR_P + k];
      if (ts == MPG_GEOM_SPHERE) {
        double W[9];
#pragma unroll
        for (int v = 0; v < 3; ++v)
#pragma unroll
          for (int i = 0; i < 3; ++i)
            W[3 * v + i] = ((TM.R[3 * i] * P[3 * v] + TM.R[3 * i + 1] * P[3 * v + 1]) + TM.R[3 * i + 2] * P[3 * v + 2]) + TM.p[i];
        hit = sphere_triangle_intersect(grs[G_PARAM], TS.p, W);
      } else {
        // triCreateGJKObject: centre in fp64, then vertices and centre as ccd_real
        const CV3 tc = cv3((P[0] + P[3] + P[6]) / 3, (P[1] + P[4] + P[7]) / 3, (P[2] + P[5] + P[8]) / 3);
        const CV3 TP[3] = {cv3(P[0], P[1], P[2]), cv3(P[3], P[4], P[5]), cv3(P[6], P[7], P[8])};
        int st;
        CV3 v0, v1, v2, v3_, dir;
        mpr_begin(ca, vadd(quat_rot(tc, B.rot), B.pos), st, v0, dir);
        int res = 0;
        while (res == 0) {
          const CV3 sp = msupport_tri(w, HV, A, B, TP, tc, dir);
          res = mpr_advance(w.mpr_tol, sp, st, v0, v1, v2, v3_, dir);
        }
        hit = res > 0;
      }
      hit = hit && fcl_gate_shape(w, gm, TM, sA, sT, sE, (int)rec[TR_ID]);
    }
    if (__ballot(hit) != 0) return true;
  }
  return false;
}

// libccd support of (box, per-lane half sizes h) - (triangle, per-lane: its
// vertices P and centroid tc in the mesh frame, rotation/position of b)
__device__ __forceinline__ CV3 msupport_box_tri(const GObj& a, const ccd_real* h, const GObj& b, const CV3* P,
                                                const CV3& tc, const CV3& dir) {
  const CV3 da = quat_rot(dir, a.rot_inv), db = quat_rot(vscale(dir, ccd_real(-1)), b.rot_inv);
  const CV3 la = CV3{(da.x >= 0 ? ccd_real(1) : ccd_real(-1)) * h[0], (da.y >= 0 ? ccd_real(1) : ccd_real(-1)) * h[1],
                     (da.z >= 0 ? ccd_real(1) : ccd_real(-1)) * h[2]};
  ccd_real maxdot = -FLT_MAX;
  CV3 lb = P[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const ccd_real dot = vdot(db, vsub(P[i], tc));
    if (dot > maxdot) {
      lb = P[i];
      maxdot = dot;
    }
  }
  return vsub(vadd(quat_rot(la, a.rot), a.pos), vadd(quat_rot(lb, b.rot), b.pos));
}

// fcl::collide(mesh, OcTree) in either order [ext FCL 0.7.0 OcTreeSolver::
// OcTreeMeshIntersectRecurse; MeshOcTreeIntersect passes the tree first]:
// some (occupied leaf, triangle) whose shapeTriangleIntersect(Box(leaf),
// box_tf, P1, P2, P3, tf_mesh) -- libccd MPR, leaf box first, triangle GJK
// object second -- reports a hit (oracle mesh_octree_intersect).  The
// traversal's BV tests only prune genuinely separated pairs, so every pair
// within libccd's false-hit reach is run.  Leaves: the octree grid cells under
// the mesh's box (octree frame, padded), one leaf per lane; each lane walks
// the mesh's cluster boxes and triangle boxes against its leaf's box in the
// mesh frame (padded) and runs MPR on the survivors.  Wave-uniform inputs.
__device__ __forceinline__ bool mesh_octree_wave(const DevWorld& w, int gm, const SE3& TM, int go, const SE3& TO) {
  const cptr<double> grm = w.geom_rec + G_STRIDE * gm;
  const double pad = kMeshShapePad * (1.0 + std::fabs(TO.p[0]) + std::fabs(TO.p[1]) + std::fabs(TO.p[2]) +
                                      std::fabs(TM.p[0]) + std::fabs(TM.p[1]) + std::fabs(TM.p[2]));
  double Rm[9], Ro[9];  // Rm = TO.R^T TM.R (mesh axes in the octree frame), Ro = Rm^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Rm[3 * i + j] = (TO.R[i] * TM.R[j] + TO.R[3 + i] * TM.R[3 + j]) + TO.R[6 + i] * TM.R[6 + j];
      Ro[3 * j + i] = Rm[3 * i + j];
    }
  // the mesh's local box (G_OBB) in the octree frame, padded
  double mcw[3], blo[3], bhi[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    mcw[i] = ((TM.R[3 * i] * grm[G_OBB_C] + TM.R[3 * i + 1] * grm[G_OBB_C + 1]) + TM.R[3 * i + 2] * grm[G_OBB_C + 2]) +
             TM.p[i];
  const double dmo[3] = {mcw[0] - TO.p[0], mcw[1] - TO.p[1], mcw[2] - TO.p[2]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double c = (TO.R[i] * dmo[0] + TO.R[3 + i] * dmo[1]) + TO.R[6 + i] * dmo[2];
    const double e = ((std::fabs(Rm[3 * i]) * grm[G_OBB_E] + std::fabs(Rm[3 * i + 1]) * grm[G_OBB_E + 1]) +
                      std::fabs(Rm[3 * i + 2]) * grm[G_OBB_E + 2]) * (1.0 + 1e-9) + 1e-9 + pad;
    blo[i] = c - e;
    bhi[i] = c + e;
  }
  GObj A, B;  // A: the leaf box (octree rotation, per-leaf centre), B: the mesh frame of the triangles
  A.rot = gjk_rot_from_matrix(TO.R);
  A.rot_inv = quat_invert2(A.rot);
  A.geom = go;
  A.type = MPG_GEOM_BOX;
  B.rot = gjk_rot_from_matrix(TM.R);
  B.rot_inv = quat_invert2(B.rot);
  B.pos = cv3(TM.p[0], TM.p[1], TM.p[2]);
  B.geom = gm;
  B.type = MPG_GEOM_MESH;
  const int c0 = w.mesh_tree[2 * gm], c1 = c0 + w.mesh_tree[2 * gm + 1];
  auto leaf_hit = [&](int leaf) -> bool {
    const cptr<double> L = w.oct_leaf + 6 * (size_t)leaf;
    bool out = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) out |= L[i] > bhi[i] || L[3 + i] < blo[i];
    if (out) return false;
    double c[3], side[3], cw[3], cm[3], hm[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      c[i] = (L[i] + L[3 + i]) * 0.5;
      side[i] = L[3 + i] - L[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) cw[i] = ((TO.R[3 * i] * c[0] + TO.R[3 * i + 1] * c[1]) + TO.R[3 * i + 2] * c[2]) + TO.p[i];
    const double dm[3] = {cw[0] - TM.p[0], cw[1] - TM.p[1], cw[2] - TM.p[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // the leaf box in the mesh frame: centre, padded half extents
      cm[i] = (TM.R[i] * dm[0] + TM.R[3 + i] * dm[1]) + TM.R[6 + i] * dm[2];
      hm[i] = ((std::fabs(Ro[3 * i]) * side[0] + std::fabs(Ro[3 * i + 1]) * side[1]) + std::fabs(Ro[3 * i + 2]) * side[2]) *
                  0.5 * (1.0 + 1e-9) + 1e-9 + pad;
    }
    GObj A1 = A;
    A1.pos = cv3(cw[0], cw[1], cw[2]);
    const ccd_real h[3] = {(ccd_real)(side[0] / 2.0), (ccd_real)(side[1] / 2.0), (ccd_real)(side[2] / 2.0)};  // boxToGJK
    for (int cl = c0; cl < c1; ++cl) {
      const cptr<double> bx = w.mesh_node + 6 * (size_t)cl;
      bool away = false;
#pragma unroll
      for (int i = 0; i < 3; ++i) away |= bx[i] > cm[i] + hm[i] || bx[3 + i] < cm[i] - hm[i];
      if (away) continue;
      const int t1 = w.mesh_link[2 * cl] + w.mesh_link[2 * cl + 1];
      for (int t = w.mesh_link[2 * cl]; t < t1; ++t) {
        const cptr<double> rec = w.mesh_tri + TR_STRIDE * (size_t)t;
        bool o2 = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) o2 |= rec[TR_LO + i] > cm[i] + hm[i] || rec[TR_HI + i] < cm[i] - hm[i];
        if (o2) continue;
        double P[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) P[k] = rec[TR_P + k];
        // triCreateGJKObject: centre in fp64, then vertices and centre as ccd_real
        const CV3 tc = cv3((P[0] + P[3] + P[6]) / 3, (P[1] + P[4] + P[7]) / 3, (P[2] + P[5] + P[8]) / 3);
        const CV3 TP[3] = {cv3(P[0], P[1], P[2]), cv3(P[3], P[4], P[5]), cv3(P[6], P[7], P[8])};
        int st;
        CV3 v0, v1, v2, v3_, dir;
        mpr_begin(A1.pos, vadd(quat_rot(tc, B.rot), B.pos), st, v0, dir);
        int res = 0;
        while (res == 0) {
          const CV3 sp = msupport_box_tri(A1, h, B, TP, tc, dir);
          res = mpr_advance(w.mpr_tol, sp, st, v0, v1, v2, v3_, dir);
        }
        if (res > 0 && fcl_gate_octree_mesh(w, go, TO, gm, TM, leaf, (int)rec[TR_ID])) return true;
      }
    }
    return false;
  };
  return octree_range_any(w, go, blo, bhi, leaf_hit);
}

// every active lane's (TA, TB) candidate of the (wave-uniform) mesh or
// octree pair (ga, gb), one after the other with the whole wave; bit k =
// lane k's hit
template <int CLS>
__device__ __forceinline__ unsigned long long walk_wave_eval(const DevWorld& w, cptr<double> HV, int ga, const SE3& TA,
                                                            int gb, const SE3& TB, bool active) {
  const int tga = w.geom_type[ga], tgb = w.geom_type[gb];
  if constexpr (CLS == CLS_OCTREE) {
    unsigned long long todo = __ballot(active), hits = 0;
    while (todo) {
      const int k = __builtin_ctzll(todo);
      todo &= todo - 1;
      const SE3 A = bcast_se3(TA, k), B = bcast_se3(TB, k);
      const bool h = tga == MPG_GEOM_OCTREE && tgb == MPG_GEOM_OCTREE ? octree_octree_wave(w, ga, A, gb, B)
                     : tga == MPG_GEOM_OCTREE                         ? octree_wave(w, HV, ga, A, gb, B)
                                                                      : octree_wave(w, HV, gb, B, ga, A);
      if (h) hits |= 1ull << k;
    }
    return hits;
  } else {
    const bool am = tga == MPG_GEOM_MESH, bm = tgb == MPG_GEOM_MESH;
    unsigned long long todo = __ballot(active), hits = 0;
    while (todo) {
      const int k = __builtin_ctzll(todo);
      todo &= todo - 1;
      const SE3 A = bcast_se3(TA, k), B = bcast_se3(TB, k);
      if (w.dbg(am && bm ? 5 : 6)) continue;
      bool h;
      if (am && bm) h = mesh_mesh_wave(w, ga, A, gb, B);
      else if (tgb == MPG_GEOM_OCTREE) h = mesh_octree_wave(w, ga, A, gb, B);
      else if (tga == MPG_GEOM_OCTREE) h = mesh_octree_wave(w, gb, B, ga, A);
      else if (am) h = mesh_shape_wave(w, HV, ga, A, gb, B);
      else h = mesh_shape_wave(w, HV, gb, B, ga, A);
      if (h) hits |= 1ull << k;
    }
    return hits;
  }
}



// Refill idle lanes once at least this many are idle.  A refill hands out
// candidates whose GJK objects and MPR start were staged in LDS beforehand
// (all 64 lanes compute the chain FK of the next 64 candidates at once), so
// it costs a few LDS reads and can run every few steps.
#ifndef MPG_REFILL_MIN
#define MPG_REFILL_MIN 8
#endif
// take the next task early once the current one is handed out and this many
// lanes are idle: a task of the same pair continues without a drain
#ifndef MPG_STEAL_MIN
#define MPG_STEAL_MIN 64
#endif

// staged candidate of the narrow phase: per moving object its GJK rotation,
// inverse rotation and position (11 floats), then the MPR start v0 and dir
enum { STG_A = 0, STG_B = 11, STG_V0 = 22, STG_DIR = 25, STG_N = 28 };

__device__ __forceinline__ void stage_obj(float (*stg)[64], int c0, uint32_t slot, const GObj& o) {
  stg[c0 + 0][slot] = o.rot.x;
  stg[c0 + 1][slot] = o.rot.y;
  stg[c0 + 2][slot] = o.rot.z;
  stg[c0 + 3][slot] = o.rot.w;
  stg[c0 + 4][slot] = o.rot_inv.x;
  stg[c0 + 5][slot] = o.rot_inv.y;
  stg[c0 + 6][slot] = o.rot_inv.z;
  stg[c0 + 7][slot] = o.rot_inv.w;
  stg[c0 + 8][slot] = o.pos.x;
  stg[c0 + 9][slot] = o.pos.y;
  stg[c0 + 10][slot] = o.pos.z;
}

__device__ __forceinline__ void unstage_obj(float (*stg)[64], int c0, uint32_t slot, GObj& o) {
  o.rot = CQ4{stg[c0 + 0][slot], stg[c0 + 1][slot], stg[c0 + 2][slot], stg[c0 + 3][slot]};
  o.rot_inv = CQ4{stg[c0 + 4][slot], stg[c0 + 5][slot], stg[c0 + 6][slot], stg[c0 + 7][slot]};
  o.pos = CV3{stg[c0 + 8][slot], stg[c0 + 9][slot], stg[c0 + 10][slot]};
}

template <bool FROM_POSES>
// 3 waves per SIMD: the kernel sits at the 168-VGPR edge of that occupancy
// (a few registers more, e.g. an inlined rare path, would drop it to 2 and
// cost ~40 % of its throughput)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void narrow_kernel(DevWorld w, const double* __restrict__ in,
                                                    const uint32_t* __restrict__ seg_len,
                                                    const uint32_t* __restrict__ seg_start,
                                                    const uint32_t* __restrict__ prefix,
                                                    const uint32_t* __restrict__ cand,
                                                    uint8_t* __restrict__ flags, uint32_t* __restrict__ masks,
                                                    uint32_t* __restrict__ task_ctr, const double* __restrict__ sc) {
  // hull reads are wave-uniform: scalar loads through the constant cache
  // (staging the hulls in LDS measured slower: +60 VGPRs, occupancy 4 -> 3)
  const cptr<double> HV = w.hull;
  const uint32_t lane = lane_id();
  const uint32_t total = prefix[w.n_pairs];
  __shared__ float s_stage[4][STG_N][64];
  __shared__ uint32_t s_cfg[4][64];
  float (*stg)[64] = s_stage[threadIdx.x >> 6];
  uint32_t* scfg = s_cfg[threadIdx.x >> 6];
  // dynamic task queue: waves that drew cheap tasks take more.
  // The first task of every wave is its wave index (the counter starts past
  // them): half the atomics on the one counter, which a small batch's waves
  // otherwise all hit at once.  (A relaxed load to skip the atomic once the
  // queue is drained measured 2x slower on cfg3: keep atomics out of the loop.)
  const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
  auto fetch = [&]() {
    uint32_t t = 0;
    if (lane == 0) t = n_waves + atomicAdd(task_ctr, 1u);
    return (uint32_t)__builtin_amdgcn_readfirstlane(t);
  };
  uint32_t tk = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  while (tk < total) {
    const int p = task_pair(prefix, w.n_pairs, tk);
    if (w.pair_cf[p] != CF_NONE) {  // closed-form pairs: closed_form_kernel
      tk = fetch();
      continue;
    }
    uint32_t next, t1;  // wave-uniform cursor into the pair's candidates and the task's end
    task_range(prefix, seg_start, seg_len, w.n_pairs, p, tk, next, t1);
    uint32_t pend = 0xffffffffu;  // a task of another pair, taken early: runs after this one
    bool more = true;             // the queue may still hold tasks
    const uint32_t* __restrict__ cl = cand + seg_start[p];
    const int a = w.pair_a[p], b = w.pair_b[p];
    const bool am = a < w.n_moving, bm = b < w.n_moving;
    const uint32_t bit = 1u << (p & 31);
    int st = MPR_DONE;
    long long cfg = 0;
    GObj A, B;
    if (!am) A = static_obj(w, a - w.n_moving);
    if (!bm) B = static_obj(w, b - w.n_moving);
    if (am) {
      A.geom = w.moving_geom[a];
      A.type = w.geom_type[A.geom];
    }
    if (bm) {
      B.geom = w.moving_geom[b];
      B.type = w.geom_type[B.geom];
    }
    CV3 v0, v1, v2, v3, dir;
    uint32_t sh = 0, sn = 0;  // staged candidates: [sh, sn) not yet handed out
#ifdef MPG_STATS
    int nsteps = 0;
#endif
    for (;;) {
      const unsigned long long idle = __ballot(st == MPR_DONE);
      const uint32_t n_idle = (uint32_t)__popcll(idle);
      if (next >= t1 && sh == sn && pend == 0xffffffffu && more && n_idle >= MPG_STEAL_MIN) {
        const uint32_t t2 = fetch();
        if (t2 >= total) {
          more = false;
        } else if (task_pair(prefix, w.n_pairs, t2) == p) {  // same pair: continue without draining
          task_range(prefix, seg_start, seg_len, w.n_pairs, p, t2, next, t1);
        } else {
          pend = t2;
        }
      }
#ifdef MPG_STATS
      const unsigned long long c0 = __builtin_amdgcn_s_memtime();
#endif
      if ((sh < sn || next < t1) && (n_idle >= MPG_REFILL_MIN || n_idle == 64)) {
        if (sh == sn) {  // stage the next <= 64 candidates: chain FK and MPR start with every lane
          const uint32_t cnt = min(64u, t1 - next);
          if (lane < cnt) {
            const long long c = cl[next + lane];
            GObj sa = A, sb = B;
            if (am) sa = moving_obj<FROM_POSES>(w, in, sc, c, a);
            if (bm) sb = moving_obj<FROM_POSES>(w, in, sc, c, b);
            int s0;
            CV3 w0, d0;
            mpr_begin(center(w, sa), center(w, sb), s0, w0, d0);
            scfg[lane] = (uint32_t)c;
            if (am) stage_obj(stg, STG_A, lane, sa);
            if (bm) stage_obj(stg, STG_B, lane, sb);
            stg[STG_V0][lane] = w0.x;
            stg[STG_V0 + 1][lane] = w0.y;
            stg[STG_V0 + 2][lane] = w0.z;
            stg[STG_DIR][lane] = d0.x;
            stg[STG_DIR + 1][lane] = d0.y;
            stg[STG_DIR + 2][lane] = d0.z;
          }
          wave_lds_sync();
          sh = 0;
          sn = cnt;
          next += cnt;
        }
        if (st == MPR_DONE) {  // hand the staged candidates to the idle lanes
          const uint32_t rank =
              __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
          if (rank < sn - sh) {
            const uint32_t k = sh + rank;
            cfg = scfg[k];
            if (am) unstage_obj(stg, STG_A, k, A);
            if (bm) unstage_obj(stg, STG_B, k, B);
            v0 = CV3{stg[STG_V0][k], stg[STG_V0 + 1][k], stg[STG_V0 + 2][k]};
            dir = CV3{stg[STG_DIR][k], stg[STG_DIR + 1][k], stg[STG_DIR + 2][k]};
            st = MPR_V1;
#ifdef MPG_STATS
            nsteps = 0;
#endif
          }
        }
        sh = min(sn, sh + n_idle);
        wave_lds_sync();  // every read done before the next staging overwrites
      }
#ifdef MPG_STATS
      const unsigned long long c1 = __builtin_amdgcn_s_memtime();
      const unsigned long long n_act = (unsigned long long)__popcll(__ballot(st != MPR_DONE));
      if (w.stats && lane_id() == 0) {
        atomicAdd(&w.stats[3], c1 - c0);
        atomicAdd(&w.stats[6], n_act);
        atomicAdd(&w.stats[7], 1ull);
      }
#endif
      if (__ballot(st != MPR_DONE) == 0) {
        if (next >= t1 && sh == sn && (pend != 0xffffffffu || !more)) break;
        continue;
      }
#ifdef MPG_STATS
      unsigned long long c2 = 0;
#endif
      if (st != MPR_DONE) {
        const CV3 s = msupport(w, HV, A, B, dir);
#ifdef MPG_STATS
        ++nsteps;
        c2 = __builtin_amdgcn_s_memtime();
#endif
        const int res = mpr_advance(w.mpr_tol, s, st, v0, v1, v2, v3, dir);
        if (res != 0) {
          if (res > 0) {
            if (masks) atomicOr(&masks[cfg * w.W + (p >> 5)], bit);
            flags[cfg] = 1;
          }
          st = MPR_DONE;
#ifdef MPG_STATS
          if (w.stats) {
            atomicAdd(&w.stats[res > 0 ? 0 : 1], (unsigned long long)nsteps);
            atomicAdd(&w.stats[res > 0 ? 2 : 8], 1ull);
          }
#endif
        }
      }
#ifdef MPG_STATS
      {
        const unsigned long long c3 = __builtin_amdgcn_s_memtime();
        unsigned long long c2m = c2 ? c2 : ~0ull;  // earliest support end over the active lanes
        for (int off = 32; off > 0; off >>= 1) {
          const unsigned long long o = ((unsigned long long)__shfl_xor((unsigned)(c2m >> 32), off) << 32) |
                                       (unsigned)__shfl_xor((unsigned)c2m, off);
          c2m = o < c2m ? o : c2m;
        }
        if (w.stats && lane_id() == 0 && c2m != ~0ull) {
          atomicAdd(&w.stats[4], c2m - c1);
          atomicAdd(&w.stats[5], c3 - c2m);
        }
      }
#endif
    }
    tk = pend != 0xffffffffu ? pend : (more ? fetch() : total);
  }
}

// ---------------------------------------------------------------------------
// Latency path for small batches (the planner's regime: a few to a few
// thousand states per call, one round trip each).  The two-phase pipeline
// costs six dependent launches and a lane-serial cull whose critical path
// alone is ~60 us; here ONE launch covers the batch with parallelism over
// (pair x configuration): one wave per (pair, 64-configuration tile), the
// pair wave-uniform as the MPR support scans need.  Per lane: exact fp64 FK of
// the pair's two objects (sincos inline), a bounding-sphere separation test
// (margin kSmallMargin >> MPR tolerance + fp64 FK error, so a skipped pair
// cannot intersect), then the FCL closed form or libccd MPR -- the same
// mpr_advance / support code as narrow_kernel, so every bit matches it.
// Output: hit bytes [n_pairs][n], each written exactly once (no
// initialisation, safe in host-mapped memory); the host folds them into
// flags and pair masks.
// ---------------------------------------------------------------------------
constexpr double kSmallMargin = 1e-4;

// the latency path's joint sin/cos: one lane per (configuration, move-group
// dof), shared by every pair's wave of the following small_kernel
__global__ __launch_bounds__(256) void small_sincos_kernel(DevWorld w, const double* __restrict__ in, long long n,
                                                          double* __restrict__ sc) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * w.dof) return;
  const long long r = i / w.dof;
  const int src = (int)(i - r * w.dof);
  for (int j = 0; j < w.nj; ++j) {
    if (w.joint_q_source[j] != src || !joint_is_revolute(w.joint_type[j])) continue;
    double sv, cv;
    mpg_sincos(in[r * w.dof + src], &sv, &cv);
    sc[(r * w.dof + src) * 2] = sv;
    sc[(r * w.dof + src) * 2 + 1] = cv;
    return;
  }
}

// INLINE_SC: each lane computes its configuration's exact joint sin/cos itself
// (one launch per validity batch -- the planner's round trip) into its own LDS
// row, kLatScGroup independent evaluations at a time so that their table loads
// overlap (evaluated inside the chain walk they serialise: two objects' chains
// of up to nine joints, each waiting on its table reads); otherwise they come
// from small_sincos_kernel (larger batches, where the P-fold recomputation
// costs more than the extra launch)
constexpr int kLatScDof = 16;   // move-group dof the inline path holds (host: more -> small_sincos_kernel)
constexpr int kLatScGroup = 4;

// The latency kernel's joint table, staged per wave in LDS by one round of
// parallel loads (lane j: joint j; lanes 0..31 / 32..63: the two objects'
// chains): the chain walk then reads LDS instead of waiting, joint after
// joint, on dependent scalar loads of the chain list and the joint records.
struct LatJoints {
  double place[kMaxJoints][12];
  double axis[kMaxJoints][3];
  double qc[kMaxJoints];
  int type[kMaxJoints], src[kMaxJoints];
  int chain[2][kMaxJoints];
};

__device__ __forceinline__ void stage_lat_joints(const DevWorld& w, LatJoints& J, uint32_t lane, int la, int lb) {
  if ((int)lane < w.nj) {
    const int j = (int)lane;
#pragma unroll
    for (int i = 0; i < 12; ++i) J.place[j][i] = w.joint_place[12 * j + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) J.axis[j][i] = w.joint_axis[3 * j + i];
    J.qc[j] = w.joint_q_const[j];
    J.type[j] = w.joint_type[j];
    J.src[j] = w.joint_q_source[j];
  }
  const int s = lane >> 5, k = (int)(lane & 31u), l = s ? lb : la;
  if (l >= 0 && k < w.link_chain_len[l]) J.chain[s][k] = w.chain_joints[w.link_chain_start[l] + k];
  wave_lds_sync();
}

// chain_oMi on the staged table: the same products in the same order
__device__ __forceinline__ SE3 chain_oMi_lat(const DevWorld& w, const LatJoints& J, int s, int l,
                                             const double* __restrict__ qrow, const double* screw) {
  const int cl = w.link_chain_len[l];
  SE3 T;
  se3_identity(T);
  for (int k = 0; k < cl; ++k) {
    const int j = J.chain[s][k];
    const int src = J.src[j - 1];
    const int type = J.type[j - 1];
    const bool pre = src >= 0 && joint_is_revolute(type);
    const double v = pre ? 0.0 : src >= 0 ? qrow[src] : J.qc[j - 1];
    const SE3 M = joint_motion(type, J.axis[j - 1], v, pre ? screw + 2 * src : nullptr);
    SE3 P;
#pragma unroll
    for (int i = 0; i < 9; ++i) P.R[i] = J.place[j - 1][i];
    P.p[0] = J.place[j - 1][9];
    P.p[1] = J.place[j - 1][10];
    P.p[2] = J.place[j - 1][11];
    const SE3 li = se3_mul(P, M);
    T = k == 0 ? li : se3_mul(T, li);
  }
  return T;
}
// World transform of one side of a latency record (LS_* layout: chain of
// joints, link placement, moving offset; a static side holds its world
// transform at LS_OFF): chain_oMi + link_from_oMi + the moving offset, the
// same products in the same order
__device__ __forceinline__ SE3 rec_side_tf(const double* S, bool moving, const double* qrow, const double* sc_row) {
  if (!moving) return load_se3(S + LS_OFF);
  const int cl = (int)S[LS_CL];
  SE3 T;
  se3_identity(T);
  for (int k = 0; k < cl; ++k) {
    const double* J = S + LS_J + LJ_STRIDE * k;
    const int type = (int)J[0], srcq = (int)J[1];
    const bool pre = srcq >= 0 && joint_is_revolute(type);
    const double qv = pre ? 0.0 : srcq >= 0 ? qrow[srcq] : J[2];
    const SE3 M = joint_motion(type, J + 3, qv, pre ? sc_row + 2 * srcq : nullptr);
    const SE3 li = se3_mul(load_se3(J + 6), M);
    T = k == 0 ? li : se3_mul(T, li);
  }
  const SE3 L = se3_mul(T, load_se3(S + LS_LINKPL));
  double qw, qxyz[3];
  mat_to_quat(L.R, &qw, qxyz);
  SE3 Lr;
  quat_to_mat(qw, qxyz[0], qxyz[1], qxyz[2], Lr.R);
  Lr.p[0] = L.p[0];
  Lr.p[1] = L.p[1];
  Lr.p[2] = L.p[2];
  return se3_mul(Lr, load_se3(S + LS_OFF));
}

// The latency paths' second bounding test (after the spheres): the two
// objects' oriented boxes (local AABBs, world rotation) in fp64, every bound
// widened by `margin` (the latency margin: at least libccd's false-hit reach,
// as the cull's fp32 test), so a separated pair cannot be an MPR hit.  R:
// row-major world rotation (column j = box axis j), c: world centre, e: half
// extents.
__device__ __forceinline__ bool dobb_separated(const double* RA, const double* ca, const double* ea, const double* RB,
                                               const double* cb, const double* eb, double margin) {
  const double d[3] = {cb[0] - ca[0], cb[1] - ca[1], cb[2] - ca[2]};
  double Rm[3][3], Ab[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Rm[i][j] = RA[i] * RB[j] + RA[3 + i] * RB[3 + j] + RA[6 + i] * RB[6 + j];
      Ab[i][j] = std::fabs(Rm[i][j]) + 1e-12;
    }
  double t[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = d[0] * RA[i] + d[1] * RA[3 + i] + d[2] * RA[6 + i];
  bool sep = false;
#pragma unroll
  for (int i = 0; i < 3; ++i) sep |= std::fabs(t[i]) > ea[i] + (eb[0] * Ab[i][0] + eb[1] * Ab[i][1] + eb[2] * Ab[i][2]) + margin;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double ra = ea[0] * Ab[0][j] + ea[1] * Ab[1][j] + ea[2] * Ab[2][j];
    sep |= std::fabs(t[0] * Rm[0][j] + t[1] * Rm[1][j] + t[2] * Rm[2][j]) > ra + eb[j] + margin;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      const double ra = ea[i1] * Ab[i2][j] + ea[i2] * Ab[i1][j];
      const double rb = eb[j1] * Ab[i][j2] + eb[j2] * Ab[i][j1];
      sep |= std::fabs(t[i2] * Rm[i1][j] - t[i1] * Rm[i2][j]) > ra + rb + margin;
    }
  }
  return sep;
}

// The smallest batches' rows by value in the kernel arguments (which the
// launch writes to device memory anyway): row c = q[dof], then sin/cos
// [2 dof] (revolute sources only), no read of host memory from the kernel
constexpr int kLatIn = 256;  // 12 states of a 7-dof group
struct LatIn {
  double d[kLatIn];
};
static_assert(sizeof(DevWorld) + sizeof(LatIn) + 64 <= 4096, "small_kernel arguments exceed the kernarg limit");

__device__ __forceinline__ double dbl_xor32(double v) {  // lane ^ 32's value
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)u, 32), hi = (unsigned)__shfl_xor((int)(unsigned)(u >> 32), 32);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// SCM (joint sin/cos source): 0 = sc buffer (device), chain FK from the
// snapshot; 1 = computed inline per lane, joints staged in LDS; 2 = sc rows
// in host-mapped memory (computed on the host), copied to LDS in one round of
// loads, FK on the pair's record; 3 = as 2 with the rows in the kernel
// arguments (LatIn)
template <bool FROM_POSES, int CLS, int SCM = 0>
__global__ __launch_bounds__(256) void small_kernel(DevWorld w, const double* __restrict__ in, long long n, int n_tiles,
                                                   uint8_t* __restrict__ hits, const double* __restrict__ sc, LatIn args) {
  constexpr bool INLINE_SC = SCM == 1, STAGED = SCM >= 1, REC = SCM >= 2 && !FROM_POSES;
  if (w.dbg(10)) return;  // diagnostics: the launch alone
  // MPG_STATS: per-wave phase times (s_memrealtime, 100 MHz) into stats[24..31]
  const uint64_t ts0 = w.stats ? __builtin_amdgcn_s_memrealtime() : 0;
  uint64_t tm[6] = {ts0, ts0, ts0, ts0, ts0, ts0};  // phase ends (pre, record, fk, spheres, narrow, store)
  auto tmark = [&](int k, uint64_t&) {
    if (w.stats) tm[k] = __builtin_amdgcn_s_memrealtime();
  };
  uint64_t tlast = ts0;
  const cptr<double> HV = w.hull;
  const uint32_t lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  const int p = wave / n_tiles;
  if (p >= w.n_pairs) return;
  if (cf_class(w.pair_cf[p]) != CLS) return;  // octree / mesh pairs: their own instances
  const long long cfg = (long long)(wave - p * n_tiles) * 64 + lane;
  const bool live = cfg < n;
  const long long c = live ? cfg : n - 1;
  uint8_t hit = 0;
  const int a = w.pair_a[p], b = w.pair_b[p];
  const bool am = a < w.n_moving, bm = b < w.n_moving;
  const int cf = w.pair_cf[p];
  if (!w.pair_allowed[p]) {  // ACM-allowed pairs are never reported (filterCollisions)
    const double* sc_row = FROM_POSES ? nullptr : sc + c * w.dof * 2;
    if constexpr (INLINE_SC && !FROM_POSES) {
      __shared__ double lat_sc[4][64][2 * kLatScDof];
      double* mine = lat_sc[threadIdx.x >> 6][lane];
      const double* qrow = in + c * w.dof;
      if ((am || bm) && w.dof > 0) {  // dof 0: no row (q may be null), every joint is a constant
        // the row first, in one round of loads (it may sit in host memory)
        double qv[kLatScDof];
#pragma unroll
        for (int k = 0; k < kLatScDof; ++k) qv[k] = qrow[min(k, w.dof - 1)];
#pragma unroll
        for (int k = 0; k < kLatScDof; ++k)
          if (k < w.dof) mine[2 * k] = qv[k];
        for (int k0 = 0; k0 < w.dof; k0 += kLatScGroup) {
          double sv[kLatScGroup], cv[kLatScGroup];
#pragma unroll
          for (int i = 0; i < kLatScGroup; ++i) mpg_sincos(mine[2 * min(k0 + i, w.dof - 1)], &sv[i], &cv[i]);
#pragma unroll
          for (int i = 0; i < kLatScGroup; ++i)
            if (k0 + i < w.dof) {
              mine[2 * (k0 + i)] = sv[i];
              mine[2 * (k0 + i) + 1] = cv[i];
            }
        }
      }
      sc_row = mine;
    }
    double* sc2_wave = nullptr;
    if constexpr (SCM == 2 && !FROM_POSES) {
      __shared__ double lat_sc2[4][64][2 * kLatScDof];
      sc2_wave = lat_sc2[threadIdx.x >> 6][0];
      double* mine = lat_sc2[threadIdx.x >> 6][lane];
      if ((am || bm) && w.dof > 0) {
        double v[2 * kLatScDof];
#pragma unroll
        for (int k = 0; k < 2 * kLatScDof; ++k) v[k] = sc_row[min(k, 2 * w.dof - 1)];
#pragma unroll
        for (int k = 0; k < 2 * kLatScDof; ++k)
          if (k < 2 * w.dof) mine[k] = v[k];
      }
      sc_row = mine;
    }
    SE3 TA, TB;
    const double* LRec = nullptr;  // SCM 2/3: the pair's record in LDS
    if constexpr (REC) {
      // the pair's record in LDS: one round of loads (every lane a slice)
      __shared__ double lat_r[4][LR_STRIDE];
      double* R = lat_r[threadIdx.x >> 6];
      LRec = R;
      tmark(0, tlast);  // kernel entry -> before the record loads
      const cptr<double> src = w.lat_rec + (size_t)LR_STRIDE * p;
      constexpr int kPer = (LR_STRIDE + 63) / 64;
      double v[kPer];
#pragma unroll
      for (int i = 0; i < kPer; ++i) v[i] = (int)lane + 64 * i < LR_STRIDE ? src[lane + 64 * i] : 0.0;
      const double* qrow = in + c * w.dof;
      // half waves: with at most 32 states, lanes 0-31 run side A's chain and
      // lanes 32-63 side B's for state lane & 31, then swap (the products are
      // the same, each computed once)
      const bool split = n <= 32;
      const int cs = split ? (int)min((long long)(lane & 31), n - 1) : (int)c;
      if constexpr (SCM == 3) {
        __shared__ double lat_in[4][kLatIn];
        double* I = lat_in[threadIdx.x >> 6];
        const int nin = (int)n * 3 * w.dof;
        for (int i = (int)lane; i < nin; i += 64) I[i] = args.d[i];
        sc_row = I + (size_t)cs * 3 * w.dof + w.dof;
        qrow = I + (size_t)cs * 3 * w.dof;
      } else if (split) {  // state cs's rows: lane cs's LDS copy
        sc_row = sc2_wave + (size_t)cs * 2 * kLatScDof;
        qrow = in + (size_t)cs * w.dof;
      }
#pragma unroll
      for (int i = 0; i < kPer; ++i)
        if ((int)lane + 64 * i < LR_STRIDE) R[lane + 64 * i] = v[i];
      wave_lds_sync();
      auto tf = [&](int sd) {
        return rec_side_tf(R + LR_SIDE + LS_STRIDE * sd, R[sd ? LR_BM : LR_AM] != 0.0, qrow, sc_row);
      };
      tmark(1, tlast);  // the record in LDS
      if (split) {
        const int sd = (int)(lane >> 5);
        const SE3 T = tf(sd);
        SE3 O;
#pragma unroll
        for (int i = 0; i < 9; ++i) O.R[i] = dbl_xor32(T.R[i]);
#pragma unroll
        for (int i = 0; i < 3; ++i) O.p[i] = dbl_xor32(T.p[i]);
        TA = sd ? O : T;
        TB = sd ? T : O;
      } else {
        TA = tf(0);
        TB = tf(1);
      }
      tmark(2, tlast);  // FK of both objects
    } else if constexpr (STAGED && !FROM_POSES) {
      __shared__ LatJoints lat_j[4];
      LatJoints& J = lat_j[threadIdx.x >> 6];
      const int la = am ? w.moving_link[a] : -1, lb = bm ? w.moving_link[b] : -1;
      stage_lat_joints(w, J, lane, la, lb);
      const double* qrow = in + c * w.dof;
      auto tf = [&](int id, int s, int l) {
        const SE3 L = link_from_oMi(w, chain_oMi_lat(w, J, s, l, qrow, sc_row), l, nullptr);
        return se3_mul(L, load_se3(w.moving_offset + 12 * id));
      };
      TA = am ? tf(a, 0, la) : load_se3(w.static_T + 12 * (a - w.n_moving));
      TB = bm ? tf(b, 1, lb) : load_se3(w.static_T + 12 * (b - w.n_moving));
    } else {
      TA = am ? moving_tf_row<FROM_POSES>(w, in, sc_row, c, a) : load_se3(w.static_T + 12 * (a - w.n_moving));
      TB = bm ? moving_tf_row<FROM_POSES>(w, in, sc_row, c, b) : load_se3(w.static_T + 12 * (b - w.n_moving));
    }
    int ga, gb;
    double oa[3], ob[3], rsum;
    if (REC) {
      ga = __builtin_amdgcn_readfirstlane((int)LRec[LR_GA]);
      gb = __builtin_amdgcn_readfirstlane((int)LRec[LR_GB]);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        oa[i] = LRec[LR_SIDE + LS_OBBC + i];
        ob[i] = LRec[LR_SIDE + LS_STRIDE + LS_OBBC + i];
      }
      rsum = LRec[LR_RA] + LRec[LR_RB];
    } else {
      ga = am ? w.moving_geom[a] : w.static_geom[a - w.n_moving];
      gb = bm ? w.moving_geom[b] : w.static_geom[b - w.n_moving];
      const cptr<double> ra = w.geom_rec + G_STRIDE * ga, rb = w.geom_rec + G_STRIDE * gb;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        oa[i] = ra[G_OBB_C + i];
        ob[i] = rb[G_OBB_C + i];
      }
      rsum = ra[G_RADIUS] + rb[G_RADIUS];
    }
    double d2 = 0.0, wc[2][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double ci = ((TA.R[3 * i] * oa[0] + TA.R[3 * i + 1] * oa[1]) + TA.R[3 * i + 2] * oa[2]) + TA.p[i];
      const double cj = ((TB.R[3 * i] * ob[0] + TB.R[3 * i + 1] * ob[1]) + TB.R[3 * i + 2] * ob[2]) + TB.p[i];
      wc[0][i] = ci;
      wc[1][i] = cj;
      d2 += (ci - cj) * (ci - cj);
    }
    const double rr = rsum + w.small_margin;
    bool near = live && d2 <= rr * rr && !w.dbg(3) && !(w.dbg(7) && d2 >= 0.0);
    if ((CLS == CLS_CLOSED || CLS == CLS_GJK) && __ballot(near) != 0ull) {  // the boxes next (MPR / closed forms)
      const cptr<double> ra = w.geom_rec + G_STRIDE * ga, rb = w.geom_rec + G_STRIDE * gb;
      const double ea[3] = {ra[G_OBB_E], ra[G_OBB_E + 1], ra[G_OBB_E + 2]};
      const double eb[3] = {rb[G_OBB_E], rb[G_OBB_E + 1], rb[G_OBB_E + 2]};
      if (near && dobb_separated(TA.R, wc[0], ea, TB.R, wc[1], eb, w.small_margin)) near = false;
    }
    tmark(3, tlast);  // bounding spheres
    if constexpr (CLS == CLS_OCTREE || CLS == CLS_MESH) {
      hit = (walk_wave_eval<CLS>(w, HV, ga, TA, gb, TB, near) >> lane) & 1ull;
    } else if (cf != CF_NONE) {
      if (near && pair_closed_form<CLS>(cf, w, ga, TA, gb, TB)) hit = 1;
    } else if (__ballot(near) != 0) {
      GObj A, B;
      A.rot = gjk_rot_from_matrix(TA.R);
      A.rot_inv = quat_invert2(A.rot);
      A.pos = cv3(TA.p[0], TA.p[1], TA.p[2]);
      A.geom = ga;
      A.type = w.geom_type[ga];
      B.rot = gjk_rot_from_matrix(TB.R);
      B.rot_inv = quat_invert2(B.rot);
      B.pos = cv3(TB.p[0], TB.p[1], TB.p[2]);
      B.geom = gb;
      B.type = w.geom_type[gb];
      int st = MPR_DONE;
      CV3 v0, v1, v2, v3, dir;
      if (near) mpr_begin(center(w, A), center(w, B), st, v0, dir);
      while (__ballot(st != MPR_DONE) != 0) {
        if (st != MPR_DONE) {
          const CV3 s = msupport(w, HV, A, B, dir);
          const int res = mpr_advance(w.mpr_tol, s, st, v0, v1, v2, v3, dir);
          if (res != 0) {
            hit = res > 0 ? 1 : 0;
            st = MPR_DONE;
          }
        }
      }
    }
    tmark(4, tlast);  // narrow test
  }
  if (live) hits[(size_t)p * n + cfg] = hit;
  if (w.stats) {
    tmark(5, tlast);  // hit store issued
    // phases that did not run (other kernel paths) took no time
    for (int k = 1; k < 6; ++k) tm[k] = tm[k] < tm[k - 1] ? tm[k - 1] : tm[k];
    if (lane_id() == 0) {
      uint64_t prev = ts0;
      for (int k = 0; k < 6; ++k) {
        atomicAdd(&w.stats[24 + k], tm[k] - prev);
        atomicMax(&w.stats[32 + k], tm[k] - prev);
        prev = tm[k];
      }
      atomicAdd(&w.stats[30], tm[5] - ts0);
      atomicMax(&w.stats[38], tm[5] - ts0);
      atomicMax(&w.stats[31], ((tm[4] - tm[3]) << 12) | (uint64_t)p);  // the slowest narrow test's pair
    }
  }
}

// ---------------------------------------------------------------------------
// Latency server: one resident workgroup that serves the smallest host
// batches without a kernel launch each.  The host writes the rows (q, then
// the joint sin/cos it computed) into host-mapped memory and bumps `seq`;
// thread 0 polls it (system-scope loads, s_sleep between polls) and the
// workgroup then runs one batch: FK per (state, moving object) from the
// objects' records in LDS, the bounding-sphere test per (pair, state), the
// near pairs' closed forms / MPR one pair per wave with lanes = states (the
// code small_kernel runs), pair-mask words written with system-scope stores,
// one barrier, ONE system-scope release store of `done` = seq.  It returns
// after idle_ticks (s_memrealtime, 100 MHz) without a request, or when the
// host sets `quit`: every path through the poll loop ends.
// ---------------------------------------------------------------------------
constexpr int kSrvN = 32;        // states per served batch (at most)
constexpr int kSrvMaxG = 8;      // workgroups (pair p belongs to workgroup p % G)
constexpr int kSrvMaxW = 16;     // pair-mask words per state (512 pairs)
constexpr int kSrvThreads = 512;
constexpr int kSrvPT = 24;       // pair-table doubles per pair
struct SrvCtl {
  unsigned long long seq, quit, pad[6];
  unsigned long long done[kSrvMaxG];   // per workgroup: the last batch it published
  unsigned long long gone[kSrvMaxG];   // per workgroup: 1 once it has left (idle or quit)
  unsigned long long phase[8];         // workgroup 0's s_memrealtime at the batch's phase ends (diagnostics)
  double rows[kSrvN * 3 * kLatScDof];  // per state: q[dof], then (sin, cos)[dof]
  uint32_t out[kSrvMaxG][kSrvN * kSrvMaxW];  // per workgroup, per state: its pairs' mask words
};

__device__ __forceinline__ unsigned long long sys_load(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

constexpr int kSrvJT = 20;   // joint table: type, source, constant, parent, axis[3], pad, placement[12]
constexpr int kSrvOB = 25;   // object table: link placement[12], moving offset[12], the link's parent joint
// one element of se3_mul(A, B) (lane e: row e / 4, column e % 4 of the 3x4
// [R | p]), by se3_mul's formula; se3_slot: where it lives in the 12 doubles
__device__ __forceinline__ int se3_slot(int e) { return (e & 3) < 3 ? 3 * (e >> 2) + (e & 3) : 9 + (e >> 2); }
__device__ __forceinline__ double se3_elem(const double* A, const double* B, int e) {
  const int i = e >> 2, j = e & 3;
  const double* a = A + 3 * i;
  if (j < 3) return (a[0] * B[j] + a[1] * B[3 + j]) + a[2] * B[6 + j];
  return ((a[0] * B[9] + a[1] * B[10]) + a[2] * B[11]) + A[9 + i];
}
// LDS carve-up (doubles, then 32-bit words): joint table, object table,
// static rotations, pair table, rows, joint frames per state, object
// transforms per state, near masks, near-pair list, hit masks
__host__ __device__ inline size_t srv_lds_bytes(int M, int P, int dof, int W, int nj, int ns) {
  const size_t dbl = (size_t)nj * kSrvJT + (size_t)M * kSrvOB + (size_t)ns * 9 + (size_t)P * kSrvPT +
                     (size_t)kSrvN * 3 * dof + (size_t)2 * kSrvN * nj * 12 + (size_t)kSrvN * M * 12;
  return dbl * 8 + ((size_t)2 * P + (size_t)kSrvN * W) * 4;
}

__global__ __launch_bounds__(kSrvThreads) void lat_server_kernel(DevWorld w, SrvCtl* ctl, unsigned long long idle_ticks,
                                                                 int phases) {
  extern __shared__ double srv_lds[];
  const int M = w.n_moving, P = w.n_pairs, dof = w.dof, W = w.W, nj = w.nj, NS = w.n_static;
  double* JT = srv_lds;
  double* OBJ = JT + (size_t)nj * kSrvJT;
  double* SROT = OBJ + (size_t)M * kSrvOB;
  double* PT = SROT + (size_t)NS * 9;
  double* ROWS = PT + (size_t)P * kSrvPT;
  double* OMI = ROWS + (size_t)kSrvN * 3 * dof;
  double* LI = OMI + (size_t)kSrvN * nj * 12;
  double* TT = LI + (size_t)kSrvN * nj * 12;
  uint32_t* NEAR = reinterpret_cast<uint32_t*>(TT + (size_t)kSrvN * M * 12);
  int* NLIST = reinterpret_cast<int*>(NEAR + P);
  uint32_t* HM = reinterpret_cast<uint32_t*>(NLIST + P);
  __shared__ unsigned long long s_cmd;
  __shared__ int s_nl;
  const int t = (int)threadIdx.x, g = (int)blockIdx.x, G = (int)gridDim.x;
  const int PG = P > g ? (P - g + G - 1) / G : 0;  // this workgroup's pairs: g, g + G, ...
  const cptr<double> HV = w.hull;
  unsigned long long last = sys_load(&ctl->done[g]);  // batches up to it are published
  unsigned long long ph[6];  // thread 0's phase stamps
  auto stamp = [&](int k) {
    if (t == 0) ph[k] = __builtin_amdgcn_s_memrealtime();
  };
  // once per residency: joint, object, static-rotation and pair tables
  for (int j = t; j < nj; j += kSrvThreads) {
    double* J = JT + (size_t)kSrvJT * j;
    J[0] = w.joint_type[j];
    J[1] = w.joint_q_source[j];
    J[2] = w.joint_q_const[j];
    J[3] = w.joint_parent[j];
    for (int i = 0; i < 3; ++i) J[4 + i] = w.joint_axis[3 * j + i];
    for (int i = 0; i < 12; ++i) J[8 + i] = w.joint_place[12 * j + i];
  }
  for (int m = t; m < M; m += kSrvThreads) {
    double* O = OBJ + (size_t)kSrvOB * m;
    const int l = w.moving_link[m];
    for (int i = 0; i < 12; ++i) O[i] = w.link_place[12 * l + i];
    for (int i = 0; i < 12; ++i) O[12 + i] = w.moving_offset[12 * m + i];
    O[24] = w.link_parent[l];
  }
  for (int i = t; i < NS * 9; i += kSrvThreads) SROT[i] = w.static_T[12 * (i / 9) + i % 9];
  int probe_cb = -1;  // MPG_STATS probe: the first walk hull's cell records
  if (w.stats && g == 0 && t == 0)
    for (int gg = 0; gg < w.n_geoms && probe_cb < 0; ++gg)
      if (w.geom_nbr[gg] >= 0 && w.geom_cbase[gg] >= 0) probe_cb = w.geom_cbase[gg];
  if (probe_cb >= 0) {
    // shader clocks of 16 dependent loads through one hull's walk cell
    // records, first pass and again (the same addresses)
    const int nrec = kCellsPerHull;
    for (int pass = 0; pass < 2; ++pass) {
      int idx = 7;
      const unsigned long long c0 = __builtin_amdgcn_s_memtime();
      for (int k = 0; k < 16; ++k) {
        const double v = w.wcell_rec[kCellRec * (size_t)(probe_cb + (idx * 97 + k * 131) % nrec) + 9];
        idx = (int)v & 1023;  // the next address depends on this load
      }
      asm volatile("" ::"v"(idx));  // the chain has completed before the clock is read
      const unsigned long long c1 = __builtin_amdgcn_s_memtime();
      atomicAdd(&w.stats[40 + pass], (c1 - c0) + (idx == -1 ? 1ull : 0ull));
      atomicAdd(&w.stats[42 + pass], 16ull);
    }
  }
  for (int p = t; p < P; p += kSrvThreads) {
    const cptr<double> R = w.lat_rec + (size_t)LR_STRIDE * p;
    double* E = PT + (size_t)kSrvPT * p;
    E[0] = R[LR_ALLOWED];
    E[1] = R[LR_CF];
    E[2] = R[LR_GA];
    E[3] = R[LR_GB];
    E[4] = w.pair_a[p];
    E[5] = w.pair_b[p];
    E[6] = R[LR_RA] + R[LR_RB];
    for (int i = 0; i < 3; ++i) {  // half extents of the boxes
      E[13 + i] = w.geom_rec[G_STRIDE * (int)R[LR_GA] + G_OBB_E + i];
      E[16 + i] = w.geom_rec[G_STRIDE * (int)R[LR_GB] + G_OBB_E + i];
    }
    for (int sd = 0; sd < 2; ++sd) {
      const cptr<double> S = R + LR_SIDE + LS_STRIDE * sd;
      const double o0 = S[LS_OBBC], o1 = S[LS_OBBC + 1], o2 = S[LS_OBBC + 2];
      if (R[sd ? LR_BM : LR_AM] != 0.0) {  // moving: the centre in its own frame
        E[7 + 3 * sd] = o0;
        E[8 + 3 * sd] = o1;
        E[9 + 3 * sd] = o2;
      } else {  // static: its world centre, as small_kernel computes it
        const SE3 T = load_se3(S + LS_OFF);
        for (int i = 0; i < 3; ++i)
          E[7 + 3 * sd + i] = ((T.R[3 * i] * o0 + T.R[3 * i + 1] * o1) + T.R[3 * i + 2] * o2) + T.p[i];
      }
    }
  }
  __syncthreads();
  for (;;) {
    if (t == 0) {
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      unsigned long long cmd = 0;
      for (;;) {
        const unsigned long long sq = sys_load(&ctl->seq);
        if (sq != last) {
          // The host stores the rows, then seq with release (x86: in order).
          // The rows are read below with system-coherent loads (sys_load: sc0
          // sc1, past L1 and L2), issued only after this value returned (the
          // branch waits on it), so they see the host's row stores.  The
          // compiler fence keeps them after this load in the program; a
          // system-scope acquire would add an L2 invalidate per batch, which
          // measured +1.8 us on the one-state round trip
          // (profiles/r05a/server_acquire.txt) and protects nothing here.
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
          cmd = sq;
          break;
        }
        if (sys_load(&ctl->quit) != 0ull) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > idle_ticks) break;
        __builtin_amdgcn_s_sleep(2);
      }
      s_cmd = cmd;  // the batch size rides in the low byte of seq
      s_nl = 0;
    }
    __syncthreads();
    const unsigned long long cmd = s_cmd;
    if (cmd == 0ull) {  // idle or quit: the whole workgroup leaves together
      if (t == 0) __hip_atomic_store(&ctl->gone[g], 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
    last = cmd;
    stamp(0);
    const int n = (int)min(cmd & 255ull, (unsigned long long)kSrvN);
    for (int i = t; i < n * 3 * dof; i += kSrvThreads)
      ROWS[i] = __longlong_as_double((long long)sys_load(reinterpret_cast<const unsigned long long*>(&ctl->rows[i])));
    for (int i = t; i < P; i += kSrvThreads) NEAR[i] = 0u;
    for (int i = t; i < n * W; i += kSrvThreads) HM[i] = 0u;
    __syncthreads();
    stamp(1);
    // FK, first the joint frames (forward_kinematics: oMi[j] = oMi[parent] *
    // (placement * M(q)), the products chain_oMi forms for every link), one
    // SE3 element per lane (se3_elem: se3_mul's formula for that element):
    // every joint's placement * M(q) at once ...
    for (int k = t; k < n * nj * 12; k += kSrvThreads) {
      const int e = k % 12, cj = k / 12, c = cj / nj, j = cj - c * nj;
      const double* row = ROWS + (size_t)c * 3 * dof;
      const double* J = JT + (size_t)kSrvJT * j;
      const int type = (int)J[0], srcq = (int)J[1];
      const bool pre = srcq >= 0 && joint_is_revolute(type);
      const double qv = pre ? 0.0 : srcq >= 0 ? row[srcq] : J[2];
      const SE3 Mq = joint_motion(type, J + 4, qv, pre ? row + dof + 2 * srcq : nullptr);
      const int jc = e & 3;  // the column of M(q) this element reads
      const double b0 = jc == 0 ? Mq.R[0] : jc == 1 ? Mq.R[1] : jc == 2 ? Mq.R[2] : Mq.p[0];
      const double b1 = jc == 0 ? Mq.R[3] : jc == 1 ? Mq.R[4] : jc == 2 ? Mq.R[5] : Mq.p[1];
      const double b2 = jc == 0 ? Mq.R[6] : jc == 1 ? Mq.R[7] : jc == 2 ? Mq.R[8] : Mq.p[2];
      const double* a = J + 8 + 3 * (e >> 2);
      const double v = jc < 3 ? (a[0] * b0 + a[1] * b1) + a[2] * b2 : ((a[0] * b0 + a[1] * b1) + a[2] * b2) + J[8 + 9 + (e >> 2)];
      LI[(size_t)cj * 12 + se3_slot(e)] = v;
    }
    __syncthreads();
    // ... then the chain, joint after joint, twelve lanes per state (five
    // states per wave, the group never straddles a wave)
    {
      const int g = lane_id() / 12, e = (int)lane_id() - 12 * g;
      const int c = (t >> 6) * 5 + g;
      if (g < 5 && c < n) {
        double* om = OMI + (size_t)c * nj * 12;
        const double* lic = LI + (size_t)c * nj * 12;
        for (int j = 0; j < nj; ++j) {
          const int par = (int)JT[(size_t)kSrvJT * j + 3];
          const double v = par > 0 ? se3_elem(om + 12 * (par - 1), lic + 12 * j, e) : lic[12 * j + se3_slot(e)];
          om[12 * j + se3_slot(e)] = v;
          wave_lds_sync();
        }
      }
    }
    __syncthreads();
    // ... then one (state, moving object) per thread: link_from_oMi and the
    // moving offset, as rec_side_tf
    for (int k = t; k < n * M; k += kSrvThreads) {
      const int c = k / M, m = k - c * M;
      const double* O = OBJ + (size_t)kSrvOB * m;
      const int jl = (int)O[24];
      SE3 P0;
      if (jl > 0) P0 = load_se3(OMI + ((size_t)c * nj + jl - 1) * 12);
      else se3_identity(P0);
      const SE3 L = se3_mul(P0, load_se3(O));
      double qw, qxyz[3];
      mat_to_quat(L.R, &qw, qxyz);
      SE3 Lr;
      quat_to_mat(qw, qxyz[0], qxyz[1], qxyz[2], Lr.R);
      Lr.p[0] = L.p[0];
      Lr.p[1] = L.p[1];
      Lr.p[2] = L.p[2];
      const SE3 T = se3_mul(Lr, load_se3(O + 12));
      double* o = TT + ((size_t)c * M + m) * 12;
#pragma unroll
      for (int i = 0; i < 9; ++i) o[i] = T.R[i];
      o[9] = T.p[0];
      o[10] = T.p[1];
      o[11] = T.p[2];
    }
    __syncthreads();
    stamp(2);
    // bounding spheres: one (pair, state) per thread
    for (int k = t; k < PG * n; k += kSrvThreads) {
      const int p = g + G * (k / n), c = k % n;
      const double* E = PT + (size_t)kSrvPT * p;
      if (E[0] != 0.0) continue;  // ACM-allowed
      double ce[2][3];
      const double* Rs[2];
      for (int sd = 0; sd < 2; ++sd) {
        const int id = (int)E[4 + sd];
        const double* oc = E + 7 + 3 * sd;
        if (id < M) {
          const double* T = TT + ((size_t)c * M + id) * 12;
          Rs[sd] = T;
#pragma unroll
          for (int i = 0; i < 3; ++i) ce[sd][i] = ((T[3 * i] * oc[0] + T[3 * i + 1] * oc[1]) + T[3 * i + 2] * oc[2]) + T[9 + i];
        } else {
          Rs[sd] = nullptr;
#pragma unroll
          for (int i = 0; i < 3; ++i) ce[sd][i] = oc[i];
        }
      }
      double d2 = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) d2 += (ce[0][i] - ce[1][i]) * (ce[0][i] - ce[1][i]);
      const double rr = E[6] + w.small_margin;
      if (!(d2 <= rr * rr)) continue;
      for (int sd = 0; sd < 2; ++sd)  // static sides: their world rotation
        if (!Rs[sd]) Rs[sd] = SROT + 9 * ((int)E[4 + sd] - M);
      if (!dobb_separated(Rs[0], ce[0], E + 13, Rs[1], ce[1], E + 16, w.small_margin)) atomicOr(&NEAR[p], 1u << c);
    }
    __syncthreads();
    for (int p = g + G * t; p < P; p += G * kSrvThreads)
      if (NEAR[p]) NLIST[atomicAdd(&s_nl, 1)] = p;
    __syncthreads();
    stamp(3);
    // narrow: one near pair per wave at a time, lanes = states.  With at most
    // 32 states both half-waves run every state's MPR (lane and lane ^ 32
    // carry the same state) and split each support: one half a's, the other
    // b's (msupport_split), which halves the support's dependent chain
    const int wv = t >> 6, lane = t & 63, nl = s_nl;
    const bool split = n <= 32;
    const int sl = split ? (lane & 31) : lane;  // the state this lane carries
    for (int k = wv; k < nl; k += kSrvThreads / 64) {
      const int p = __builtin_amdgcn_readfirstlane(NLIST[k]);
      const double* E = PT + (size_t)kSrvPT * p;
      const int cf = __builtin_amdgcn_readfirstlane((int)E[1]);
      const int ga = __builtin_amdgcn_readfirstlane((int)E[2]), gb = __builtin_amdgcn_readfirstlane((int)E[3]);
      const int a = __builtin_amdgcn_readfirstlane((int)E[4]), b = __builtin_amdgcn_readfirstlane((int)E[5]);
      const bool near = sl < n && ((NEAR[p] >> sl) & 1u);
      const int c = sl < n ? sl : 0;
      const SE3 TA = a < M ? load_se3(TT + ((size_t)c * M + a) * 12) : load_se3(w.static_T + 12 * (a - M));
      const SE3 TB = b < M ? load_se3(TT + ((size_t)c * M + b) * 12) : load_se3(w.static_T + 12 * (b - M));
      bool hit = false;
      if (cf != CF_NONE) {
        if (near && pair_closed_form<CLS_CLOSED>(cf, w, ga, TA, gb, TB)) hit = true;
      } else {
        GObj A, B;
        A.rot = gjk_rot_from_matrix(TA.R);
        A.rot_inv = quat_invert2(A.rot);
        A.pos = cv3(TA.p[0], TA.p[1], TA.p[2]);
        A.geom = ga;
        A.type = w.geom_type[ga];
        B.rot = gjk_rot_from_matrix(TB.R);
        B.rot_inv = quat_invert2(B.rot);
        B.pos = cv3(TB.p[0], TB.p[1], TB.p[2]);
        B.geom = gb;
        B.type = w.geom_type[gb];
        int st = MPR_DONE;
        CV3 v0, v1, v2, v3, dir;
        if (near) mpr_begin(center(w, A), center(w, B), st, v0, dir);
        unsigned long long t_sup = 0, t_adv = 0, n_it = 0;  // MPG_STATS: MPR step costs (shader clocks)
        while (__ballot(st != MPR_DONE) != 0) {
          const unsigned long long c0 = w.stats ? __builtin_amdgcn_s_memtime() : 0ull;
          if (st != MPR_DONE) {
            const CV3 sp = split ? msupport_split(w, HV, A, B, dir, lane >= 32) : msupport(w, HV, A, B, dir);
            const unsigned long long c1 = w.stats ? __builtin_amdgcn_s_memtime() : 0ull;
            const int res = mpr_advance(w.mpr_tol, sp, st, v0, v1, v2, v3, dir);
            if (res != 0) {
              hit = res > 0;
              st = MPR_DONE;
            }
            if (w.stats) {
              t_sup += c1 - c0;
              t_adv += __builtin_amdgcn_s_memtime() - c1;
            }
          }
          ++n_it;
        }
        if (w.stats && lane == 0 && n_it > 0) {
          atomicAdd(&w.stats[20], n_it);
          atomicAdd(&w.stats[21], t_sup);
          atomicAdd(&w.stats[22], t_adv);
          atomicMax(&w.stats[23], n_it);
        }
      }
      if (hit && (!split || lane < 32)) atomicOr(&HM[c * W + (p >> 5)], 1u << (p & 31));
    }
    __syncthreads();
    stamp(4);
    // publish: wave 0 writes every pair-mask word, then its lane 0 releases
    // `done` at system scope (the release waits for the whole wave's stores)
    if (t < 64) {
      for (int i = t; i < n * W; i += 64) __hip_atomic_store(&ctl->out[g][i], HM[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (t == 0 && g == 0 && phases) {  // MPG_STATS only: six more stores for the release to wait on
        ph[5] = __builtin_amdgcn_s_memrealtime();
        for (int k = 0; k < 6; ++k) __hip_atomic_store(&ctl->phase[k], ph[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      __builtin_amdgcn_s_waitcnt(0);
      if (t == 0) __hip_atomic_store(&ctl->done[g], cmd, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// ---------------------------------------------------------------------------
// Diagnostics: fcl::collide of two posed geometries of the world, n pose
// pairs at a time (one lane each; the geometries are the same for the whole
// launch, as the narrow phase's wave-uniform support scans need): the exact
// dispatch collide() uses -- FCL closed form, octree or BVH-mesh walk, or
// libccd MPR.  Lets tests compare the narrow phase with the oracle directly,
// without forward kinematics (mpg_debug_collide_pairs).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void debug_pairs_kernel(DevWorld w, int ga, int gb, int cf, long long n,
                                                         const double* __restrict__ Ta, const double* __restrict__ Tb,
                                                         uint8_t* __restrict__ hit) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;
  const long long c = live ? i : n - 1;
  const SE3 TA = load_se3(Ta + 12 * c), TB = load_se3(Tb + 12 * c);
  bool h = false;
  if (cf == CF_OCTREE) {
    h = (walk_wave_eval<CLS_OCTREE>(w, w.hull, ga, TA, gb, TB, live) >> lane_id()) & 1ull;
  } else if (cf == CF_MESH) {
    h = (walk_wave_eval<CLS_MESH>(w, w.hull, ga, TA, gb, TB, live) >> lane_id()) & 1ull;
  } else if (cf != CF_NONE) {
    h = live && closed_form(cf, w, ga, TA, gb, TB);
  } else {
    GObj A, B;
    A.rot = gjk_rot_from_matrix(TA.R);
    A.rot_inv = quat_invert2(A.rot);
    A.pos = cv3(TA.p[0], TA.p[1], TA.p[2]);
    A.geom = ga;
    A.type = w.geom_type[ga];
    B.rot = gjk_rot_from_matrix(TB.R);
    B.rot_inv = quat_invert2(B.rot);
    B.pos = cv3(TB.p[0], TB.p[1], TB.p[2]);
    B.geom = gb;
    B.type = w.geom_type[gb];
    int st = MPR_DONE;
    CV3 v0, v1, v2, v3, dir;
    if (live) mpr_begin(center(w, A), center(w, B), st, v0, dir);
    while (__ballot(st != MPR_DONE) != 0) {
      if (st != MPR_DONE) {
        const CV3 s = msupport(w, w.hull, A, B, dir);
        const int res = mpr_advance(w.mpr_tol, s, st, v0, v1, v2, v3, dir);
        if (res != 0) {
          h = res > 0;
          st = MPR_DONE;
        }
      }
    }
  }
  if (live) hit[i] = h ? 1 : 0;
}

// ---------------------------------------------------------------------------
// Batched distance (PlanningWorld::distanceSelf / distanceOthers,
// src/planning_world.cpp:493-720): exact fp64 object poses once per
// configuration (pose_kernel), then per configuration every non-allowed pair
// in order with a bounding-sphere lower bound against the running minimum,
// GJK distance on the FCL support mappings (-1 for penetrating pairs, as
// fcl::distance with DistanceRequest() reports), strict '<' keeps the first
// minimum.  Same algorithm as the oracle (oracle/collide_oracle.c
// gjk_distance); the north star's bar vs FCL's GJK is 1e-5.
// ---------------------------------------------------------------------------
constexpr int kPoseStride = 20;  // rot xyzw, pos xyz, world OBB centre xyz, fp64 rotation (mesh pairs), pad

template <bool FROM_POSES>
__global__ __launch_bounds__(128) void pose_kernel(DevWorld w, const double* __restrict__ in, long long n,
                                                   double* __restrict__ poses, double* __restrict__ save64) {
  const long long cfg = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (cfg >= n) return;
  auto store = [&](int m, const SE3& T) {
    const CQ4 r = gjk_rot_from_matrix(T.R);
    double* g = poses + ((size_t)m * kPoseStride) * n + cfg;  // [m][field][cfg]
    g[0 * n] = r.x;
    g[1 * n] = r.y;
    g[2 * n] = r.z;
    g[3 * n] = r.w;
    g[4 * n] = T.p[0];
    g[5 * n] = T.p[1];
    g[6 * n] = T.p[2];
    const cptr<double> gr = w.geom_rec + G_STRIDE * w.moving_geom[m];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      g[(7 + i) * n] = ((T.R[3 * i] * gr[G_OBB_C] + T.R[3 * i + 1] * gr[G_OBB_C + 1]) + T.R[3 * i + 2] * gr[G_OBB_C + 2]) +
                       T.p[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) g[(10 + i) * n] = T.R[i];
  };
  if (FROM_POSES) {
    for (int m = 0; m < w.n_moving; ++m)
      store(m, se3_mul(link_from_pose7(in + (cfg * w.n_links + w.moving_link[m]) * 7), load_se3(w.moving_offset + 12 * m)));
    return;
  }
  // oMi[j] = oMi[parent] * (jointPlacement_j * M_j(q)); branch frames spilled
  const double* qrow = in + cfg * w.dof;
  SE3 cur;
  se3_identity(cur);
  for (int j = 0; j <= w.nj; ++j) {
    if (j > 0) {
      const int jj = j - 1;
      const int src = w.joint_q_source[jj];
      const double v = src >= 0 ? qrow[src] : w.joint_q_const[jj];
      const SE3 li = se3_mul(load_se3(w.joint_place + 12 * jj), joint_motion(w.joint_type[jj], w.joint_axis + 3 * jj, v));
      const int sidx = w.bp.jsrc[jj];
      if (sidx < 0) {
        cur = li;
      } else if (sidx > 0) {
        SE3 P;
        const double* sp = save64 + (size_t)(sidx - 1) * 12 * n + cfg;
        for (int i = 0; i < 9; ++i) P.R[i] = sp[i * n];
        for (int i = 0; i < 3; ++i) P.p[i] = sp[(9 + i) * n];
        cur = se3_mul(P, li);
      } else {
        cur = se3_mul(cur, li);
      }
      const int sv = w.bp.jsave[jj];
      if (sv >= 0) {
        double* sp = save64 + (size_t)sv * 12 * n + cfg;
        for (int i = 0; i < 9; ++i) sp[i * n] = cur.R[i];
        for (int i = 0; i < 3; ++i) sp[(9 + i) * n] = cur.p[i];
      }
    }
    for (int k = w.bp.link_start[j]; k < w.bp.link_start[j + 1]; ++k) {
      const int l = w.bp.link_order[k];
      const int o0 = w.bp.obj_start[l], o1 = w.bp.obj_start[l + 1];
      if (o0 == o1) continue;
      SE3 root;
      se3_identity(root);
      const SE3 L = link_from_oMi(w, j == 0 ? root : cur, l, nullptr);
      for (int o = o0; o < o1; ++o) {
        const int m = w.bp.obj_order[o];
        store(m, se3_mul(L, load_se3(w.moving_offset + 12 * m)));
      }
    }
  }
}

__device__ __forceinline__ double d3dot(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// ---------------------------------------------------------------------------
// FCL 0.7.0 shape distance: GJKDistance / GJKSignedDistance on float libccd
// (mpg_ccd_dist.h, the twin of oracle/fcl_gjk_dist.h), the closed forms of
// GJKSolver_libccd::shapeDistance, and the support mappings they run on.
// ---------------------------------------------------------------------------
#include "mpg_ccd_dist.h"

// __ccdSupport of (uniform shape a) - (uniform shape b), both points kept
__device__ __forceinline__ ccdx::Sup csup(const DevWorld& w, cptr<double> HV, const GObj& a, const GObj& b,
                                         const CV3& dir) {
  const CV3 da = quat_rot(dir, a.rot_inv), db = quat_rot(vscale(dir, ccd_real(-1)), b.rot_inv);
  const int ga = __builtin_amdgcn_readfirstlane(a.geom), ta = __builtin_amdgcn_readfirstlane(a.type);
  const int gb = __builtin_amdgcn_readfirstlane(b.geom), tb = __builtin_amdgcn_readfirstlane(b.type);
  const CV3 la = support_local(w, HV, ga, ta, da), lb = support_local(w, HV, gb, tb, db);
  ccdx::Sup s;
  s.v1 = vadd(quat_rot(la, a.rot), a.pos);
  s.v2 = vadd(quat_rot(lb, b.rot), b.pos);
  s.v = vsub(s.v1, s.v2);
  return s;
}

// boxToGJK support with per-lane half sizes h (an octree leaf box)
__device__ __forceinline__ CV3 box_support_world(const GObj& a, const ccd_real* h, const CV3& dir) {
  const CV3 da = quat_rot(dir, a.rot_inv);
  const CV3 la = CV3{(da.x >= 0 ? ccd_real(1) : ccd_real(-1)) * h[0], (da.y >= 0 ? ccd_real(1) : ccd_real(-1)) * h[1],
                     (da.z >= 0 ? ccd_real(1) : ccd_real(-1)) * h[2]};
  return vadd(quat_rot(la, a.rot), a.pos);
}

// (leaf box a) - (uniform shape b)
__device__ __forceinline__ ccdx::Sup csup_box(const GObj& a, const ccd_real* h, const DevWorld& w, cptr<double> HV,
                                              const GObj& b, const CV3& dir) {
  ccdx::Sup s;
  s.v1 = box_support_world(a, h, dir);
  const CV3 db = quat_rot(vscale(dir, ccd_real(-1)), b.rot_inv);
  const int gb = __builtin_amdgcn_readfirstlane(b.geom), tb = __builtin_amdgcn_readfirstlane(b.type);
  s.v2 = vadd(quat_rot(support_local(w, HV, gb, tb, db), b.rot), b.pos);
  s.v = vsub(s.v1, s.v2);
  return s;
}

__device__ __forceinline__ CV3 tri_support(const GObj& b, const CV3* P, const CV3& tc, const CV3& dir);

// (uniform shape a) - (triangle b: vertices P and centroid tc in the mesh frame)
__device__ __forceinline__ ccdx::Sup csup_tri(const DevWorld& w, cptr<double> HV, const GObj& a, const GObj& b,
                                              const CV3* P, const CV3& tc, const CV3& dir) {
  ccdx::Sup s;
  const CV3 da = quat_rot(dir, a.rot_inv);
  const int ga = __builtin_amdgcn_readfirstlane(a.geom), ta = __builtin_amdgcn_readfirstlane(a.type);
  s.v1 = vadd(quat_rot(support_local(w, HV, ga, ta, da), a.rot), a.pos);
  s.v2 = tri_support(b, P, tc, vscale(dir, ccd_real(-1)));
  s.v = vsub(s.v1, s.v2);
  return s;
}

// (leaf box a) - (triangle b)
__device__ __forceinline__ ccdx::Sup csup_box_tri(const GObj& a, const ccd_real* h, const GObj& b, const CV3* P,
                                                  const CV3& tc, const CV3& dir) {
  ccdx::Sup s;
  s.v1 = box_support_world(a, h, dir);
  s.v2 = tri_support(b, P, tc, vscale(dir, ccd_real(-1)));
  s.v = vsub(s.v1, s.v2);
  return s;
}

// ccdx status -> the pair-index sentinel the distance outputs carry
constexpr int kDistThrow = MPG_DISTANCE_FCL_THROWS, kDistOverflow = MPG_DISTANCE_EPA_CAPACITY;

// ---- closed-form shape distances (GJKSolver_libccd::shapeDistance's
// specialisations [ext FCL 0.7.0]; oracle/fcl_gjk_dist.h cf_*, same order)
__device__ __forceinline__ void cf_tf_point(const SE3& T, const double* p, double* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = ((T.R[3 * i] * p[0] + T.R[3 * i + 1] * p[1]) + T.R[3 * i + 2] * p[2]) + T.p[i];
}
__device__ __forceinline__ double cf_norm(const double* v) { return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
// X_FO.inverse() * X_FS: the sphere centre in the other shape's frame
__device__ __forceinline__ void cf_centre_in_frame(const SE3& TS, const SE3& TO, double* c) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double inv_t = -((TO.R[i] * TO.p[0] + TO.R[3 + i] * TO.p[1]) + TO.R[6 + i] * TO.p[2]);
    c[i] = ((TO.R[i] * TS.p[0] + TO.R[3 + i] * TS.p[1]) + TO.R[6 + i] * TS.p[2]) + inv_t;
  }
}

__device__ double cf_sphere_sphere(double r1, const SE3& T1, double r2, const SE3& T2, double* p1, double* p2) {
  const double diff[3] = {T1.p[0] - T2.p[0], T1.p[1] - T2.p[1], T1.p[2] - T2.p[2]};
  const double len = cf_norm(diff);
  if (len > r1 + r2) {
    for (int i = 0; i < 3; ++i) {
      p1[i] = T1.p[i] - diff[i] * (r1 / len);
      p2[i] = T2.p[i] + diff[i] * (r2 / len);
    }
    return len - (r1 + r2);
  }
  return -1.0;
}

__device__ double cf_sphere_capsule(double r1, const SE3& TS, double r2, double lz, const SE3& TC, double* p1,
                                    double* p2) {
  const double a[3] = {0.0, 0.0, 0.5 * lz}, b[3] = {0.0, 0.0, -0.5 * lz};
  double pos1[3], pos2[3], sp[3];
  cf_tf_point(TC, a, pos1);
  cf_tf_point(TC, b, pos2);
  const double* sc = TS.p;
  const double v[3] = {pos2[0] - pos1[0], pos2[1] - pos1[1], pos2[2] - pos1[2]};
  const double wv[3] = {sc[0] - pos1[0], sc[1] - pos1[1], sc[2] - pos1[2]};
  const double c1 = (wv[0] * v[0] + wv[1] * v[1]) + wv[2] * v[2];
  const double c2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  if (c1 <= 0) {
    for (int i = 0; i < 3; ++i) sp[i] = pos1[i];
  } else if (c2 <= c1) {
    for (int i = 0; i < 3; ++i) sp[i] = pos2[i];
  } else {
    const double bb = c1 / c2;
    for (int i = 0; i < 3; ++i) sp[i] = pos1[i] + v[i] * bb;
  }
  double diff[3] = {sc[0] - sp[0], sc[1] - sp[1], sc[2] - sp[2]};
  const double distance = cf_norm(diff) - r1 - r2;
  if (distance <= 0) return -1.0;
  const double n = cf_norm(diff);
  for (int i = 0; i < 3; ++i) diff[i] /= n;
  for (int i = 0; i < 3; ++i) {
    p1[i] = sc[i] - diff[i] * r1;
    p2[i] = sp[i] + diff[i] * r2;
  }
  return distance;
}

__device__ double cf_sphere_box(double r, const SE3& TS, const double* side, const SE3& TB, double* pS, double* pB) {
  double c[3], nq[3];
  cf_centre_in_frame(TS, TB, c);
  bool clamped = false;
  for (int i = 0; i < 3; ++i) {
    const double h = side[i] / 2;
    nq[i] = c[i];
    if (c[i] < -h) {
      clamped = true;
      nq[i] = -h;
    }
    if (c[i] > h) {
      clamped = true;
      nq[i] = h;
    }
  }
  if (clamped) {
    const double nc[3] = {c[0] - nq[0], c[1] - nq[1], c[2] - nq[2]};
    const double sq = (nc[0] * nc[0] + nc[1] * nc[1]) + nc[2] * nc[2];
    if (sq > r * r) {
      const double d = std::sqrt(sq);
      double pSb[3];
      for (int i = 0; i < 3; ++i) pSb[i] = (nc[i] / d) * (d - r) + nq[i];
      cf_tf_point(TB, nq, pB);
      cf_tf_point(TB, pSb, pS);
      return d - r;
    }
  }
  return -1.0;
}

__device__ double cf_sphere_cylinder(double r, const SE3& TS, double rc, double lz, const SE3& TC, double* pS,
                                     double* pC) {
  double c[3], n[3];
  cf_centre_in_frame(TS, TC, c);
  const double h = lz / 2;
  bool clamped = false;
  n[0] = c[0];
  n[1] = c[1];
  n[2] = c[2];
  if (c[2] > h) {
    n[2] = h;
    clamped = true;
  } else if (c[2] < -h) {
    n[2] = -h;
    clamped = true;
  }
  const double rd2 = c[0] * c[0] + c[1] * c[1];
  if (rd2 > rc * rc) {
    const double scale = rc / std::sqrt(rd2);
    n[0] = c[0] * scale;
    n[1] = c[1] * scale;
    clamped = true;
  }
  if (clamped) {
    const double nc[3] = {c[0] - n[0], c[1] - n[1], c[2] - n[2]};
    const double sq = (nc[0] * nc[0] + nc[1] * nc[1]) + nc[2] * nc[2];
    if (sq > r * r) {
      const double d = std::sqrt(sq);
      double pSc[3];
      for (int i = 0; i < 3; ++i) pSc[i] = (nc[i] / d) * (d - r) + n[i];
      cf_tf_point(TC, n, pC);
      cf_tf_point(TC, pSc, pS);
      return d - r;
    }
  }
  return -1.0;
}

__device__ __forceinline__ double cf_clamp01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

__device__ double cf_capsule_capsule(double r1, double lz1, const SE3& T1, double r2, double lz2, const SE3& T2,
                                     double* p1, double* p2) {
  const double eps = 0x1.6a09e667f3bcdp-46, eps2 = eps * eps;  // constants<double>::eps_78() = pow(DBL_EPSILON, 7/8)
  double P1[3], Q1[3], P2[3], Q2[3];
  for (int i = 0; i < 3; ++i) {
    const double h1 = (lz1 / 2) * T1.R[3 * i + 2], h2 = (lz2 / 2) * T2.R[3 * i + 2];
    P1[i] = T1.p[i] + h1;
    Q1[i] = T1.p[i] - h1;
    P2[i] = T2.p[i] + h2;
    Q2[i] = T2.p[i] - h2;
  }
  double d1[3], d2[3], rr[3];
  for (int i = 0; i < 3; ++i) {
    d1[i] = Q1[i] - P1[i];
    d2[i] = Q2[i] - P2[i];
    rr[i] = P1[i] - P2[i];
  }
  const double a = (d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2];
  const double e = (d2[0] * d2[0] + d2[1] * d2[1]) + d2[2] * d2[2];
  const double f = (d2[0] * rr[0] + d2[1] * rr[1]) + d2[2] * rr[2];
  double s, t;
  if (a <= eps2 && e <= eps2) {
    s = t = 0.0;
  } else if (a <= eps2) {
    s = 0.0;
    t = cf_clamp01(f / e);
  } else {
    const double c = (d1[0] * rr[0] + d1[1] * rr[1]) + d1[2] * rr[2];
    if (e <= eps2) {
      t = 0.0;
      s = cf_clamp01(-c / a);
    } else {
      const double b = (d1[0] * d2[0] + d1[1] * d2[1]) + d1[2] * d2[2];
      const double den0 = a * e - b * b, denom = den0 > 0.0 ? den0 : 0.0;
      s = denom > eps2 ? cf_clamp01((b * f - c * e) / denom) : 0.0;
      t = (b * s + f) / e;
      if (t < 0.0) {
        t = 0.0;
        s = cf_clamp01(-c / a);
      } else if (t > 1.0) {
        t = 1.0;
        s = cf_clamp01((b - c) / a);
      }
    }
  }
  double N1[3], N2[3], v[3];
  for (int i = 0; i < 3; ++i) {
    N1[i] = P1[i] + d1[i] * s;
    N2[i] = P2[i] + d2[i] * t;
    v[i] = N2[i] - N1[i];
  }
  const double seg = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  double vh[3];
  if (seg > eps) {
    for (int i = 0; i < 3; ++i) vh[i] = v[i] / seg;
  } else {
    double n[3] = {d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]};
    double nl = cf_norm(n);
    if (!(nl > eps)) {
      const double ax[3] = {std::fabs(d1[0]) < std::fabs(d1[1]) ? 1.0 : 0.0,
                            std::fabs(d1[0]) < std::fabs(d1[1]) ? 0.0 : 1.0, 0.0};
      n[0] = d1[1] * ax[2] - d1[2] * ax[1];
      n[1] = d1[2] * ax[0] - d1[0] * ax[2];
      n[2] = d1[0] * ax[1] - d1[1] * ax[0];
      nl = cf_norm(n);
    }
    for (int i = 0; i < 3; ++i) vh[i] = nl > 0.0 ? n[i] / nl : (i == 2 ? 1.0 : 0.0);
  }
  for (int i = 0; i < 3; ++i) {
    p1[i] = N1[i] + vh[i] * r1;
    p2[i] = N2[i] - vh[i] * r2;
  }
  return seg - r1 - r2;
}

// 1 if (ta, tb) has a closed form; d and the points (zeros for -1)
__device__ bool cf_shape_distance(const DevWorld& w, int ga, int ta, const SE3& Ta, int gb, int tb, const SE3& Tb,
                                  double& d, V3& q1, V3& q2) {
  const cptr<double> pa = w.geom_rec + G_STRIDE * ga + G_PARAM, pb = w.geom_rec + G_STRIDE * gb + G_PARAM;
  double p1[3] = {0, 0, 0}, p2[3] = {0, 0, 0};
  if (ta == MPG_GEOM_SPHERE && tb == MPG_GEOM_SPHERE) {
    d = cf_sphere_sphere(pa[0], Ta, pb[0], Tb, p1, p2);
  } else if (ta == MPG_GEOM_SPHERE && tb == MPG_GEOM_CAPSULE) {
    d = cf_sphere_capsule(pa[0], Ta, pb[0], pb[1], Tb, p1, p2);
  } else if (ta == MPG_GEOM_CAPSULE && tb == MPG_GEOM_SPHERE) {
    d = cf_sphere_capsule(pb[0], Tb, pa[0], pa[1], Ta, p2, p1);
  } else if (ta == MPG_GEOM_SPHERE && tb == MPG_GEOM_BOX) {
    const double side[3] = {pb[0], pb[1], pb[2]};
    d = cf_sphere_box(pa[0], Ta, side, Tb, p1, p2);
  } else if (ta == MPG_GEOM_BOX && tb == MPG_GEOM_SPHERE) {
    const double side[3] = {pa[0], pa[1], pa[2]};
    d = cf_sphere_box(pb[0], Tb, side, Ta, p2, p1);
  } else if (ta == MPG_GEOM_SPHERE && tb == MPG_GEOM_CYLINDER) {
    d = cf_sphere_cylinder(pa[0], Ta, pb[0], pb[1], Tb, p1, p2);
  } else if (ta == MPG_GEOM_CYLINDER && tb == MPG_GEOM_SPHERE) {
    d = cf_sphere_cylinder(pb[0], Tb, pa[0], pa[1], Ta, p2, p1);
  } else if (ta == MPG_GEOM_CAPSULE && tb == MPG_GEOM_CAPSULE) {
    d = cf_capsule_capsule(pa[0], pa[1], Ta, pb[0], pb[1], Tb, p1, p2);
  } else {
    return false;
  }
  if (d == -1.0) p1[0] = p1[1] = p1[2] = p2[0] = p2[1] = p2[2] = 0.0;
  q1 = V3{p1[0], p1[1], p1[2]};
  q2 = V3{p2[0], p2[1], p2[2]};
  return true;
}

// Project<S>::projectLine / projectTriangle and sphereTriangleDistance with
// points (oracle cf_project_line / cf_project_triangle / cf_sphere_triangle)
struct CfProj {
  double param[4], sqr_distance;
};
__device__ CfProj cf_project_line(const double* a, const double* b, const double* p) {
  CfProj r = {{0, 0, 0, 0}, -1.0};
  const double d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const double l = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  if (l > 0) {
    const double pa[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const double t = (pa[0] * d[0] + pa[1] * d[1]) + pa[2] * d[2];
    r.param[1] = (t >= l) ? 1 : ((t <= 0) ? 0 : (t / l));
    r.param[0] = 1 - r.param[1];
    double v[3];
    if (t >= l) {
      for (int i = 0; i < 3; ++i) v[i] = p[i] - b[i];
    } else if (t <= 0) {
      for (int i = 0; i < 3; ++i) v[i] = p[i] - a[i];
    } else {
      for (int i = 0; i < 3; ++i) v[i] = (a[i] + d[i] * r.param[1]) - p[i];
    }
    r.sqr_distance = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  }
  return r;
}
__device__ __forceinline__ void cf_cross(double* o, const double* a, const double* b) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ CfProj cf_project_triangle(const double* a, const double* b, const double* c, const double* p) {
  CfProj r = {{0, 0, 0, 0}, -1.0};
  const double* vt[3] = {a, b, c};
  double dl[3][3], n[3];
  for (int i = 0; i < 3; ++i) {
    dl[0][i] = a[i] - b[i];
    dl[1][i] = b[i] - c[i];
    dl[2][i] = c[i] - a[i];
  }
  cf_cross(n, dl[0], dl[1]);
  const double l = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  if (l > 0) {
    double mindist = -1;
    for (int i = 0; i < 3; ++i) {
      double vp[3], dn[3];
      for (int k = 0; k < 3; ++k) vp[k] = vt[i][k] - p[k];
      cf_cross(dn, dl[i], n);
      if ((vp[0] * dn[0] + vp[1] * dn[1]) + vp[2] * dn[2] > 0) {
        const int j = i == 2 ? 0 : i + 1;
        const CfProj rl = cf_project_line(vt[i], vt[j], p);
        if (mindist < 0 || rl.sqr_distance < mindist) {
          mindist = rl.sqr_distance;
          r.param[i] = rl.param[0];
          r.param[j] = rl.param[1];
          r.param[j == 2 ? 0 : j + 1] = 0;
        }
      }
    }
    if (mindist < 0) {
      const double ap[3] = {a[0] - p[0], a[1] - p[1], a[2] - p[2]};
      const double d = (ap[0] * n[0] + ap[1] * n[1]) + ap[2] * n[2];
      const double s = std::sqrt(l);
      double pp[3], t1[3], t2[3], x[3];
      for (int k = 0; k < 3; ++k) pp[k] = n[k] * (d / l);
      mindist = (pp[0] * pp[0] + pp[1] * pp[1]) + pp[2] * pp[2];
      for (int k = 0; k < 3; ++k) t1[k] = (b[k] - p[k]) - pp[k];
      cf_cross(x, dl[1], t1);
      r.param[0] = cf_norm(x) / s;
      for (int k = 0; k < 3; ++k) t2[k] = (c[k] - p[k]) - pp[k];
      cf_cross(x, dl[2], t2);
      r.param[1] = cf_norm(x) / s;
      r.param[2] = 1 - r.param[0] - r.param[1];
    }
    r.sqr_distance = mindist;
  }
  return r;
}
// W: the triangle's world vertices [3][3]
__device__ double cf_sphere_triangle(double radius, const double* o, const double* W, double* pS, double* pT) {
  const CfProj r = cf_project_triangle(W, W + 3, W + 6, o);
  if (r.sqr_distance > radius * radius) {
    double pp[3], dir[3];
    for (int k = 0; k < 3; ++k) pp[k] = (W[k] * r.param[0] + W[3 + k] * r.param[1]) + W[6 + k] * r.param[2];
    for (int k = 0; k < 3; ++k) dir[k] = o[k] - pp[k];
    const double n = cf_norm(dir);
    for (int k = 0; k < 3; ++k) dir[k] /= n;
    for (int k = 0; k < 3; ++k) {
      pS[k] = o[k] - dir[k] * radius;
      pT[k] = pp[k];
    }
    return std::sqrt(r.sqr_distance) - radius;
  }
  return -1.0;
}

// lower-bound pruning slack (oracle mesh_dist_slack): a pair / leaf / triangle
// is skipped only when its bounding-volume lower bound is above the running
// minimum by more than the float support rounding of libccd's GJK objects
__device__ __forceinline__ double dist_slack(const double* pa, const double* pb) {
  return 1e-5 * (1.0 + std::fabs(pa[0]) + std::fabs(pa[1]) + std::fabs(pa[2]) + std::fabs(pb[0]) + std::fabs(pb[1]) +
                 std::fabs(pb[2]));
}

// fcl::distance(shape, OcTree) [ext FCL 0.7.0 OcTreeShapeDistanceRecurse]:
// shapeDistance(leaf box, box_tf, shape, tf) per occupied leaf in FCL's DFS
// order (Box-Sphere closed form, else GJKDistance), strict '<' -> the first
// minimum; points (leaf box, shape).  Leaves whose bounding sphere cannot be
// below `bound` (the group's running minimum) by the slack are skipped.
// Returns the pair's minimum (DBL_MAX if every leaf was skipped) or a
// kDist* sentinel status in st.
__device__ double octree_distance(const DevWorld& w, cptr<double> HV, int go, const SE3& TO, const GObj& S,
                                  const SE3& TS, const V3& cs, double rs, double bound, ccd_real tol, V3& pb, V3& ps,
                                  int& st) {
  const cptr<double> go_rec = w.geom_rec + G_STRIDE * go;
  const int l0 = (int)go_rec[G_PARAM], ln = (int)go_rec[G_PARAM + 1];
  const bool sphere = S.type == MPG_GEOM_SPHERE;
  const double rsph = w.geom_rec[G_STRIDE * S.geom + G_PARAM];
  const double slack = dist_slack(TO.p, TS.p);
  GObj A;
  A.rot = gjk_rot_from_matrix(TO.R);
  A.rot_inv = quat_invert2(A.rot);
  A.geom = go;
  A.type = MPG_GEOM_BOX;
  double best = DBL_MAX;
  pb = ps = V3{0, 0, 0};
  for (int l = l0; l < l0 + ln && best != -1.0; ++l) {
    const cptr<double> L = w.oct_leaf + 6 * (size_t)l;
    double c[3], side[3], cw[3];
    for (int i = 0; i < 3; ++i) {
      c[i] = (L[i] + L[3 + i]) * 0.5;
      side[i] = L[3 + i] - L[i];
    }
    for (int i = 0; i < 3; ++i) cw[i] = ((TO.R[3 * i] * c[0] + TO.R[3 * i + 1] * c[1]) + TO.R[3 * i + 2] * c[2]) + TO.p[i];
    const double dx = cw[0] - cs.x, dy = cw[1] - cs.y, dz = cw[2] - cs.z;
    const double rl = 0.5 * std::sqrt((side[0] * side[0] + side[1] * side[1]) + side[2] * side[2]) * (1.0 + 1e-9) + 1e-9;
    if (std::sqrt(dx * dx + dy * dy + dz * dz) - rs - rl > fmin(best, bound) + slack) continue;
    double d;
    V3 qb{0, 0, 0}, qs{0, 0, 0};
    if (sphere) {
      SE3 TL;
      for (int k = 0; k < 9; ++k) TL.R[k] = TO.R[k];
      for (int k = 0; k < 3; ++k) TL.p[k] = cw[k];
      double a1[3], a2[3];
      d = cf_sphere_box(rsph, TS, side, TL, a2, a1);
      if (d != -1.0) {
        qb = V3{a1[0], a1[1], a1[2]};
        qs = V3{a2[0], a2[1], a2[2]};
      }
    } else {
      GObj A1 = A;
      A1.pos = cv3(cw[0], cw[1], cw[2]);
      const ccd_real h[3] = {(ccd_real)(side[0] / 2.0), (ccd_real)(side[1] / 2.0), (ccd_real)(side[2] / 2.0)};
      auto sup = [&](const CV3& dir) { return csup_box(A1, h, w, HV, S, dir); };
      ccd_real df;
      CV3 c1, c2;
      const int r = ccdx::gjk_distance<false>(sup, tol, (ccdx::Polytope*)nullptr, df, c1, c2);
      if (r != ccdx::kOk) {
        st = r == ccdx::kThrow ? kDistThrow : kDistOverflow;
        return DBL_MAX;
      }
      d = df;
      qb = to_v3(c1);
      qs = to_v3(c2);
    }
    if (d < best) {
      best = d;
      pb = qb;
      ps = qs;
    }
  }
  return best;
}

__device__ __forceinline__ GObj pose_obj(const DevWorld& w, const double* __restrict__ poses, long long n, long long cfg,
                                         int id, V3& c) {
  if (id < w.n_moving) {
    const double* g = poses + ((size_t)id * kPoseStride) * n + cfg;
    GObj o;
    o.rot = CQ4{(ccd_real)g[0], (ccd_real)g[n], (ccd_real)g[2 * n], (ccd_real)g[3 * n]};
    o.rot_inv = quat_invert2(o.rot);
    o.pos = cv3(g[4 * n], g[5 * n], g[6 * n]);
    o.geom = w.moving_geom[id];
    o.type = w.geom_type[o.geom];
    c = v3(g[7 * n], g[8 * n], g[9 * n]);
    return o;
  }
  const int sid = id - w.n_moving;
  const cptr<double> r = w.static_rec + S_STRIDE * sid;
  c = v3(r[S_OBBC], r[S_OBBC + 1], r[S_OBBC + 2]);
  return static_obj(w, sid);
}

// fp64 transform of object `id` for configuration cfg (pose_kernel fields)
__device__ __forceinline__ SE3 pose_se3(const DevWorld& w, const double* __restrict__ poses, long long n, long long cfg,
                                        int id) {
  if (id >= w.n_moving) return load_se3(w.static_T + 12 * (id - w.n_moving));
  const double* g = poses + ((size_t)id * kPoseStride) * n + cfg;
  SE3 T;
#pragma unroll
  for (int i = 0; i < 9; ++i) T.R[i] = g[(10 + i) * n];
#pragma unroll
  for (int i = 0; i < 3; ++i) T.p[i] = g[(4 + i) * n];
  return T;
}

// ---------------------------------------------------------------------------
// Distance with BVH meshes (fcl::distance on BVHModel<OBBRSS>, FCL 0.7.0):
//   mesh-shape   MeshShapeDistanceTraversalNodeOBBRSS: min over triangles of
//                shapeTriangleDistance(shape, tf, P1, P2, P3, tf_mesh) (GJK,
//                shape first; -1 once one intersects)
//   mesh-mesh    MeshDistanceTraversalNodeOBBRSS: min of triDistance over the
//                triangle pairs, B's triangles in A's frame (0 if one pair
//                intersects)
//   mesh-OcTree  OcTreeMeshDistanceRecurse: min over (leaf box, triangle) of
//                shapeTriangleDistance(box, box_tf, ...), box first
// The traversal only skips what cannot lower the running minimum; here the
// cluster and triangle boxes are skipped when their lower bound exceeds the
// running minimum by more than the float support rounding (dist_slack).  One
// lane per configuration, as distance_kernel.
// ---------------------------------------------------------------------------

// distance from point c to the box [lo, hi]
__device__ __forceinline__ double point_box_distance(const double* c, const double* lo, const double* hi) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double e = fmax(fmax(lo[i] - c[i], c[i] - hi[i]), 0.0);
    s += e * e;
  }
  return std::sqrt(s);
}

// PQP TriDist as FCL's TriangleDistance::segPoints / triDistance (oracle
// seg_points / tri_face_case / tri_distance, same operation order)
__device__ void seg_points(const double* P, const double* A, const double* Q, const double* B, double* VEC, double* X,
                           double* Y) {
  double T[3], TMP[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) T[k] = Q[k] - P[k];
  const double AA = d3(A, A), BB = d3(B, B), AB = d3(A, B), AT = d3(A, T), BT = d3(B, T);
  const double denom = AA * BB - AB * AB;
  double t = (AT * BB - BT * AB) / denom;
  if (t < 0 || std::isnan(t)) t = 0;
  else if (t > 1) t = 1;
  const double u = (t * AB - BT) / BB;
  if (u <= 0 || std::isnan(u)) {
    for (int k = 0; k < 3; ++k) Y[k] = Q[k];
    t = AT / AA;
    if (t <= 0 || std::isnan(t)) {
      for (int k = 0; k < 3; ++k) {
        X[k] = P[k];
        VEC[k] = Q[k] - P[k];
      }
    } else if (t >= 1) {
      for (int k = 0; k < 3; ++k) {
        X[k] = P[k] + A[k];
        VEC[k] = Q[k] - X[k];
      }
    } else {
      for (int k = 0; k < 3; ++k) X[k] = P[k] + A[k] * t;
      c3(TMP, T, A);
      c3(VEC, A, TMP);
    }
  } else if (u >= 1) {
    for (int k = 0; k < 3; ++k) Y[k] = Q[k] + B[k];
    t = (AB + AT) / AA;
    if (t <= 0 || std::isnan(t)) {
      for (int k = 0; k < 3; ++k) {
        X[k] = P[k];
        VEC[k] = Y[k] - P[k];
      }
    } else if (t >= 1) {
      for (int k = 0; k < 3; ++k) {
        X[k] = P[k] + A[k];
        VEC[k] = Y[k] - X[k];
      }
    } else {
      for (int k = 0; k < 3; ++k) {
        X[k] = P[k] + A[k] * t;
        T[k] = Y[k] - P[k];
      }
      c3(TMP, T, A);
      c3(VEC, A, TMP);
    }
  } else {
    for (int k = 0; k < 3; ++k) Y[k] = Q[k] + B[k] * u;
    if (t <= 0 || std::isnan(t)) {
      for (int k = 0; k < 3; ++k) X[k] = P[k];
      c3(TMP, T, B);
      c3(VEC, B, TMP);
    } else if (t >= 1) {
      for (int k = 0; k < 3; ++k) {
        X[k] = P[k] + A[k];
        T[k] = Q[k] - X[k];
      }
      c3(TMP, T, B);
      c3(VEC, B, TMP);
    } else {
      for (int k = 0; k < 3; ++k) X[k] = P[k] + A[k] * t;
      c3(VEC, A, B);
      if (d3(VEC, T) < 0)
        for (int k = 0; k < 3; ++k) VEC[k] = -VEC[k];
    }
  }
}

// Pf: the projection of T's closest vertex on S's face, Qf: that vertex
__device__ bool tri_face_case(const double* S, const double* Sv, const double* T, bool& disjoint, double& dist,
                              double* Pf, double* Qf) {
  double Sn[3], V[3], Z[3], Tp[3];
  c3(Sn, Sv, Sv + 3);
  const double Snl = d3(Sn, Sn);
  if (!(Snl > 1e-15)) return false;
  for (int i = 0; i < 3; ++i) {
    for (int k = 0; k < 3; ++k) V[k] = S[k] - T[3 * i + k];
    Tp[i] = d3(V, Sn);
  }
  int point = -1;
  if (Tp[0] > 0 && Tp[1] > 0 && Tp[2] > 0) {
    point = Tp[0] < Tp[1] ? 0 : 1;
    if (Tp[2] < Tp[point]) point = 2;
  } else if (Tp[0] < 0 && Tp[1] < 0 && Tp[2] < 0) {
    point = Tp[0] > Tp[1] ? 0 : 1;
    if (Tp[2] > Tp[point]) point = 2;
  }
  if (point < 0) return false;
  disjoint = true;
  for (int e = 0; e < 3; ++e) {
    for (int k = 0; k < 3; ++k) V[k] = T[3 * point + k] - S[3 * e + k];
    c3(Z, Sn, Sv + 3 * e);
    if (!(d3(V, Z) > 0)) return false;
  }
  double D[3];
  const double s = Tp[point] / Snl;
  for (int k = 0; k < 3; ++k) {
    Pf[k] = T[3 * point + k] + Sn[k] * s;
    Qf[k] = T[3 * point + k];
    D[k] = Pf[k] - Qf[k];
  }
  dist = std::sqrt(d3(D, D));
  return true;
}

// TriangleDistance::triDistance(S, T, P, Q) (oracle tri_distance_pq); S, T:
// 3 vertices each, row-major [3][3]; P, Q zero when they intersect
__device__ double tri_distance_pq(const double* S, const double* T, double* P, double* Q) {
  double Sv[9], Tv[9], VEC[3], Pc[3], Qc[3], V[3], Z[3], minP[3] = {0, 0, 0}, minQ[3] = {0, 0, 0};
  for (int k = 0; k < 3; ++k) {
    Sv[k] = S[3 + k] - S[k];
    Sv[3 + k] = S[6 + k] - S[3 + k];
    Sv[6 + k] = S[k] - S[6 + k];
    Tv[k] = T[3 + k] - T[k];
    Tv[3 + k] = T[6 + k] - T[3 + k];
    Tv[6 + k] = T[k] - T[6 + k];
    P[k] = 0.0;
    Q[k] = 0.0;
  }
  bool shown_disjoint = false;
  for (int k = 0; k < 3; ++k) V[k] = S[k] - T[k];
  double mindd = d3(V, V) + 1;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      seg_points(S + 3 * i, Sv + 3 * i, T + 3 * j, Tv + 3 * j, VEC, Pc, Qc);
      for (int k = 0; k < 3; ++k) V[k] = Qc[k] - Pc[k];
      const double dd = d3(V, V);
      if (dd <= mindd) {
        for (int k = 0; k < 3; ++k) {
          minP[k] = Pc[k];
          minQ[k] = Qc[k];
        }
        mindd = dd;
        const int i2 = (i + 2) % 3, j2 = (j + 2) % 3;
        for (int k = 0; k < 3; ++k) Z[k] = S[3 * i2 + k] - Pc[k];
        double a = d3(Z, VEC);
        for (int k = 0; k < 3; ++k) Z[k] = T[3 * j2 + k] - Qc[k];
        double b = d3(Z, VEC);
        if (a <= 0 && b >= 0) {
          for (int k = 0; k < 3; ++k) {
            P[k] = Pc[k];
            Q[k] = Qc[k];
          }
          return std::sqrt(dd);
        }
        const double p = d3(V, VEC);
        if (a < 0) a = 0;
        if (b > 0) b = 0;
        if (p - a + b > 0) shown_disjoint = true;
      }
    }
  double d;
  if (tri_face_case(S, Sv, T, shown_disjoint, d, P, Q)) return d;
  if (tri_face_case(T, Tv, S, shown_disjoint, d, Q, P)) return d;
  if (shown_disjoint) {
    for (int k = 0; k < 3; ++k) {
      P[k] = minP[k];
      Q[k] = minQ[k];
    }
    return std::sqrt(mindd);
  }
  return 0.0;
}

__device__ __forceinline__ GObj mesh_frame_obj(int gm, const SE3& TM) {
  GObj B;
  B.rot = gjk_rot_from_matrix(TM.R);
  B.rot_inv = quat_invert2(B.rot);
  B.pos = cv3(TM.p[0], TM.p[1], TM.p[2]);
  B.geom = gm;
  B.type = MPG_GEOM_MESH;
  return B;
}

// point p (world) in the frame T
__device__ __forceinline__ void to_frame(const SE3& T, const double* p, double* o) {
  const double d[3] = {p[0] - T.p[0], p[1] - T.p[1], p[2] - T.p[2]};
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = (T.R[i] * d[0] + T.R[3 + i] * d[1]) + T.R[6 + i] * d[2];
}

// mesh-shape (MeshShapeDistanceTraversalNodeOBBRSS leaf): the minimum over
// the triangles of shapeTriangleDistance(shape, tf, P1, P2, P3, tf_mesh)
// (sphereTriangleDistance for spheres, else GJKDistance with the shape first),
// points (mesh, shape).  Triangles are met in cluster order; ties go to the
// lower triangle index, as the oracle's index-order scan with strict '<'.
// Clusters / triangles whose lower bound is above min(own minimum, bound) by
// the slack are skipped.  DBL_MAX when everything was skipped.
__device__ double mesh_shape_distance_lane(const DevWorld& w, cptr<double> HV, int gm, const SE3& TM, const GObj& S,
                                           const SE3& TS, double bound, ccd_real tol, V3& pm, V3& ps, int& st) {
  const cptr<double> grs = w.geom_rec + G_STRIDE * S.geom;
  double cs[3], csm[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    cs[i] = ((TS.R[3 * i] * grs[G_OBB_C] + TS.R[3 * i + 1] * grs[G_OBB_C + 1]) + TS.R[3 * i + 2] * grs[G_OBB_C + 2]) + TS.p[i];
  to_frame(TM, cs, csm);
  const double rs = grs[G_RADIUS], slack = dist_slack(TM.p, TS.p);
  const bool sphere = S.type == MPG_GEOM_SPHERE;
  const GObj B = mesh_frame_obj(gm, TM);
  const int c0 = w.mesh_tree[2 * gm], c1 = c0 + w.mesh_tree[2 * gm + 1];
  double best = DBL_MAX;
  int best_id = INT_MAX;
  pm = ps = V3{0, 0, 0};
  for (int cl = c0; cl < c1 && best != -1.0; ++cl) {
    const cptr<double> bx = w.mesh_node + 6 * (size_t)cl;
    const double lo[3] = {bx[0], bx[1], bx[2]}, hi[3] = {bx[3], bx[4], bx[5]};
    if (point_box_distance(csm, lo, hi) - rs > fmin(best, bound) + slack) continue;
    const int t1 = w.mesh_link[2 * cl] + w.mesh_link[2 * cl + 1];
    for (int t = w.mesh_link[2 * cl]; t < t1 && best != -1.0; ++t) {
      const cptr<double> rec = w.mesh_tri + TR_STRIDE * (size_t)t;
      const double tlo[3] = {rec[TR_LO], rec[TR_LO + 1], rec[TR_LO + 2]}, thi[3] = {rec[TR_HI], rec[TR_HI + 1], rec[TR_HI + 2]};
      if (point_box_distance(csm, tlo, thi) - rs > fmin(best, bound) + slack) continue;
      const int id = (int)rec[TR_ID];
      double P[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) P[k] = rec[TR_P + k];
      double d;
      V3 qm{0, 0, 0}, qs{0, 0, 0};
      if (sphere) {
        double W[9], a1[3], a2[3];
        for (int v = 0; v < 3; ++v)
          for (int i = 0; i < 3; ++i)
            W[3 * v + i] = ((TM.R[3 * i] * P[3 * v] + TM.R[3 * i + 1] * P[3 * v + 1]) + TM.R[3 * i + 2] * P[3 * v + 2]) + TM.p[i];
        d = cf_sphere_triangle(grs[G_PARAM], TS.p, W, a1, a2);
        if (d != -1.0) {
          qs = V3{a1[0], a1[1], a1[2]};
          qm = V3{a2[0], a2[1], a2[2]};
        }
      } else {
        const CV3 tc = cv3((P[0] + P[3] + P[6]) / 3, (P[1] + P[4] + P[7]) / 3, (P[2] + P[5] + P[8]) / 3);
        const CV3 TP[3] = {cv3(P[0], P[1], P[2]), cv3(P[3], P[4], P[5]), cv3(P[6], P[7], P[8])};
        auto sup = [&](const CV3& dir) { return csup_tri(w, HV, S, B, TP, tc, dir); };
        ccd_real df;
        CV3 c1, c2;
        const int r = ccdx::gjk_distance<false>(sup, tol, (ccdx::Polytope*)nullptr, df, c1, c2);
        if (r != ccdx::kOk) {
          st = r == ccdx::kThrow ? kDistThrow : kDistOverflow;
          return DBL_MAX;
        }
        d = df;
        qs = to_v3(c1);
        qm = to_v3(c2);
      }
      if (d < best || (d == best && id < best_id)) {
        best = d;
        best_id = id;
        pm = qm;
        ps = qs;
      }
    }
  }
  return best;
}

// mesh-mesh (MeshDistanceTraversalNodeOBBRSS): the minimum of triDistance
// over the triangle pairs, B's triangles in A's frame; 0 once a pair
// intersects (zero points); points (A, B) in A's frame -> world.  Ties go to
// the lexicographically lower (A index, B index), the oracle's scan order.
__device__ double mesh_mesh_distance_lane(const DevWorld& w, int ga, const SE3& TA, int gb, const SE3& TB, double bound,
                                          V3& pa, V3& pb) {
  double R[9], T[3];
  const double dt[3] = {TB.p[0] - TA.p[0], TB.p[1] - TA.p[1], TB.p[2] - TA.p[2]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (TA.R[i] * TB.R[j] + TA.R[3 + i] * TB.R[3 + j]) + TA.R[6 + i] * TB.R[6 + j];
    T[i] = (TA.R[i] * dt[0] + TA.R[3 + i] * dt[1]) + TA.R[6 + i] * dt[2];
  }
  const double slack = dist_slack(TA.p, TB.p);
  const int a0 = w.mesh_tree[2 * ga], a1 = a0 + w.mesh_tree[2 * ga + 1];
  const int b0 = w.mesh_tree[2 * gb], b1 = b0 + w.mesh_tree[2 * gb + 1];
  double best = DBL_MAX, bP[3] = {0, 0, 0}, bQ[3] = {0, 0, 0};
  long long best_key = LLONG_MAX;
  for (int cb = b0; cb < b1 && best != 0.0; ++cb) {
    const cptr<double> bb = w.mesh_node + 6 * (size_t)cb;
    double cc[3], cca[3], e2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      cc[k] = (bb[k] + bb[3 + k]) * 0.5;
      e2 += (bb[3 + k] - bb[k]) * (bb[3 + k] - bb[k]);
    }
    const double rb = 0.5 * std::sqrt(e2) * (1.0 + 1e-9) + 1e-9;
#pragma unroll
    for (int i = 0; i < 3; ++i) cca[i] = ((R[3 * i] * cc[0] + R[3 * i + 1] * cc[1]) + R[3 * i + 2] * cc[2]) + T[i];
    for (int ca = a0; ca < a1 && best != 0.0; ++ca) {
      const cptr<double> ba = w.mesh_node + 6 * (size_t)ca;
      const double lo[3] = {ba[0], ba[1], ba[2]}, hi[3] = {ba[3], ba[4], ba[5]};
      if (point_box_distance(cca, lo, hi) - rb > fmin(best, bound) + slack) continue;
      const int tb1 = w.mesh_link[2 * cb] + w.mesh_link[2 * cb + 1];
      for (int tb = w.mesh_link[2 * cb]; tb < tb1 && best != 0.0; ++tb) {
        const cptr<double> rq = w.mesh_tri + TR_STRIDE * (size_t)tb;
        double Q[9], qc[3], qr = 0.0;
#pragma unroll
        for (int v = 0; v < 3; ++v)
#pragma unroll
          for (int i = 0; i < 3; ++i)
            Q[3 * v + i] = ((R[3 * i] * rq[3 * v] + R[3 * i + 1] * rq[3 * v + 1]) + R[3 * i + 2] * rq[3 * v + 2]) + T[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) qc[i] = (Q[i] + Q[3 + i] + Q[6 + i]) / 3.0;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          const double dx = Q[3 * v] - qc[0], dy = Q[3 * v + 1] - qc[1], dz = Q[3 * v + 2] - qc[2];
          qr = fmax(qr, dx * dx + dy * dy + dz * dz);
        }
        qr = std::sqrt(qr) * (1.0 + 1e-9) + 1e-9;
        if (point_box_distance(qc, lo, hi) - qr > fmin(best, bound) + slack) continue;
        const long long idb = (long long)rq[TR_ID];
        const int ta1 = w.mesh_link[2 * ca] + w.mesh_link[2 * ca + 1];
        for (int ta = w.mesh_link[2 * ca]; ta < ta1; ++ta) {
          const cptr<double> rp = w.mesh_tri + TR_STRIDE * (size_t)ta;
          const double tlo[3] = {rp[TR_LO], rp[TR_LO + 1], rp[TR_LO + 2]}, thi[3] = {rp[TR_HI], rp[TR_HI + 1], rp[TR_HI + 2]};
          if (point_box_distance(qc, tlo, thi) - qr > fmin(best, bound) + slack) continue;
          double P[9], Pp[3], Qq[3];
#pragma unroll
          for (int k = 0; k < 9; ++k) P[k] = rp[TR_P + k];
          const double d = tri_distance_pq(P, Q, Pp, Qq);
          const long long key = ((long long)rp[TR_ID] << 32) | idb;
          if (d < best || (d == best && key < best_key)) {
            best = d;
            best_key = key;
            for (int k = 0; k < 3; ++k) {
              bP[k] = Pp[k];
              bQ[k] = Qq[k];
            }
          }
          if (best == 0.0) break;
        }
      }
    }
  }
  double wa[3], wb[3];
  cf_tf_point(TA, bP, wa);
  cf_tf_point(TA, bQ, wb);
  pa = V3{wa[0], wa[1], wa[2]};
  pb = V3{wb[0], wb[1], wb[2]};
  return best;
}

// mesh-OcTree (OcTreeMeshDistanceRecurse): the minimum over (occupied leaf,
// triangle) of shapeTriangleDistance(Box(leaf), box_tf, triangle) (GJK, leaf
// box first); points (box, triangle); ties to the earlier leaf, then the
// lower triangle index, as the oracle's leaf-major scan
__device__ double mesh_octree_distance_lane(const DevWorld& w, int gm, const SE3& TM, int go, const SE3& TO, double bound,
                                            ccd_real tol, V3& pbox, V3& ptri, int& st) {
  const cptr<double> grm = w.geom_rec + G_STRIDE * gm, go_rec = w.geom_rec + G_STRIDE * go;
  const int l0 = (int)go_rec[G_PARAM], ln = (int)go_rec[G_PARAM + 1];
  double mcw[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    mcw[i] = ((TM.R[3 * i] * grm[G_OBB_C] + TM.R[3 * i + 1] * grm[G_OBB_C + 1]) + TM.R[3 * i + 2] * grm[G_OBB_C + 2]) + TM.p[i];
  const double rm = grm[G_RADIUS], slack = dist_slack(TM.p, TO.p);
  const GObj B = mesh_frame_obj(gm, TM);
  GObj A;
  A.rot = gjk_rot_from_matrix(TO.R);
  A.rot_inv = quat_invert2(A.rot);
  A.geom = go;
  A.type = MPG_GEOM_BOX;
  const int c0 = w.mesh_tree[2 * gm], c1 = c0 + w.mesh_tree[2 * gm + 1];
  double best = DBL_MAX;
  int best_id = INT_MAX;
  pbox = ptri = V3{0, 0, 0};
  for (int l = l0; l < l0 + ln && best != -1.0; ++l) {
    const cptr<double> L = w.oct_leaf + 6 * (size_t)l;
    double c[3], side[3], cw[3], cm[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      c[i] = (L[i] + L[3 + i]) * 0.5;
      side[i] = L[3 + i] - L[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) cw[i] = ((TO.R[3 * i] * c[0] + TO.R[3 * i + 1] * c[1]) + TO.R[3 * i + 2] * c[2]) + TO.p[i];
    const double rl = 0.5 * std::sqrt((side[0] * side[0] + side[1] * side[1]) + side[2] * side[2]) * (1.0 + 1e-9) + 1e-9;
    const double dx = cw[0] - mcw[0], dy = cw[1] - mcw[1], dz = cw[2] - mcw[2];
    if (std::sqrt(dx * dx + dy * dy + dz * dz) - rl - rm > fmin(best, bound) + slack) continue;
    to_frame(TM, cw, cm);
    GObj A1 = A;
    A1.pos = cv3(cw[0], cw[1], cw[2]);
    const ccd_real h[3] = {(ccd_real)(side[0] / 2.0), (ccd_real)(side[1] / 2.0), (ccd_real)(side[2] / 2.0)};
    const double leaf_best = best;  // a later leaf wins only when strictly below the earlier leaves
    for (int cl = c0; cl < c1 && best != -1.0; ++cl) {
      const cptr<double> bx = w.mesh_node + 6 * (size_t)cl;
      const double lo[3] = {bx[0], bx[1], bx[2]}, hi[3] = {bx[3], bx[4], bx[5]};
      if (point_box_distance(cm, lo, hi) - rl > fmin(best, bound) + slack) continue;
      const int t1 = w.mesh_link[2 * cl] + w.mesh_link[2 * cl + 1];
      for (int t = w.mesh_link[2 * cl]; t < t1 && best != -1.0; ++t) {
        const cptr<double> rec = w.mesh_tri + TR_STRIDE * (size_t)t;
        const double tlo[3] = {rec[TR_LO], rec[TR_LO + 1], rec[TR_LO + 2]}, thi[3] = {rec[TR_HI], rec[TR_HI + 1], rec[TR_HI + 2]};
        if (point_box_distance(cm, tlo, thi) - rl > fmin(best, bound) + slack) continue;
        const int id = (int)rec[TR_ID];
        double P[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) P[k] = rec[TR_P + k];
        const CV3 tc = cv3((P[0] + P[3] + P[6]) / 3, (P[1] + P[4] + P[7]) / 3, (P[2] + P[5] + P[8]) / 3);
        const CV3 TP[3] = {cv3(P[0], P[1], P[2]), cv3(P[3], P[4], P[5]), cv3(P[6], P[7], P[8])};
        auto sup = [&](const CV3& dir) { return csup_box_tri(A1, h, B, TP, tc, dir); };
        ccd_real df;
        CV3 q1, q2;
        const int r = ccdx::gjk_distance<false>(sup, tol, (ccdx::Polytope*)nullptr, df, q1, q2);
        if (r != ccdx::kOk) {
          st = r == ccdx::kThrow ? kDistThrow : kDistOverflow;
          return DBL_MAX;
        }
        const double d = df;
        // within this leaf: the lower triangle index among equals; against
        // earlier leaves: strictly below
        if (d < leaf_best && (d < best || (d == best && id < best_id))) {
          best = d;
          best_id = id;
          pbox = to_v3(q1);
          ptri = to_v3(q2);
        }
      }
    }
  }
  return best;
}

// (MODE bit) PTS: write the nearest points; SIGNED: enable_signed_distance;
// NP: enable_nearest_points (mesh-mesh points, the (shape, mesh) swap)
// INDEP: DistanceRequest(gjk_solver_type=GST_INDEP), unsigned shape pairs only
constexpr int MPG_DIST_POINTS = 1, MPG_DIST_SIGNED = 2, MPG_DIST_NP = 4, MPG_DIST_INDEP = 8;
constexpr int kBigPool = 16;  // big EPA polytopes per world (distance_redo_kernel)

// Per configuration, every non-allowed pair in order with the group's strict
// '<' (planning_world.cpp:513): fcl::distance with DistanceRequest's options
// (oracle/collide_oracle.c pair_distance: which algorithm each pair kind runs
// and which point is which).  Shape pairs whose bounding spheres are apart
// by more than the running minimum plus the slack are skipped (their GJK
// value cannot be below it).  A configuration on which FCL throws
// (p = kDistThrow) or whose EPA outgrows the polytope arrays (p =
// kDistOverflow) gets NaN distances in both groups.
// PT: the signed instances' EPA polytope type; ptp its storage (private in
// distance_kernel, a global pool slot in distance_redo_kernel).
template <int MODE, class PT>
__device__ __forceinline__ void distance_config(const DevWorld& w, const double* __restrict__ poses, long long n,
                                                long long cfg, bool live, int n_self, ccd_real tol, double dtol,
                                                PT* ptp, double* __restrict__ d_self, int32_t* __restrict__ p_self,
                                                double* __restrict__ d_others, int32_t* __restrict__ p_others,
                                                double* __restrict__ pts_self, double* __restrict__ pts_others) {
  constexpr bool SIGNED = (MODE & MPG_DIST_SIGNED) != 0;
  constexpr bool PTS = (MODE & MPG_DIST_POINTS) != 0;
  constexpr bool NP = (MODE & MPG_DIST_NP) != 0;
  constexpr bool INDEP = (MODE & MPG_DIST_INDEP) != 0;
  static_assert(!(INDEP && SIGNED), "GST_INDEP signed distance (FCL's EPA) is not restated");
  const cptr<double> HV = w.hull;
  double best[2] = {DBL_MAX, DBL_MAX};
  int bp[2] = {-1, -1};
  V3 bpt[2][2] = {{{0, 0, 0}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}};
  int st = 0;
  for (int p = 0; p < w.n_pairs && !st; ++p) {
    if (w.pair_allowed[p]) continue;  // ACM before distance (planning_world.cpp:509-510)
    const int g = p < n_self ? 0 : 1;
    const int a = w.pair_a[p], b = w.pair_b[p];
    V3 ca, cb;
    const GObj A = pose_obj(w, poses, n, cfg, a, ca);
    const GObj B = pose_obj(w, poses, n, cfg, b, cb);
    const double ra = w.geom_rec[G_STRIDE * A.geom + G_RADIUS], rb = w.geom_rec[G_STRIDE * B.geom + G_RADIUS];
    double d = DBL_MAX;
    V3 q1{0, 0, 0}, q2{0, 0, 0};
    if (w.pair_cf[p] == CF_MESH) {  // mesh pairs report unsigned values, never below -1
      if (!live || best[g] <= -1.0) continue;
      const SE3 TA = pose_se3(w, poses, n, cfg, a), TB = pose_se3(w, poses, n, cfg, b);
      if (A.type == MPG_GEOM_MESH && B.type == MPG_GEOM_MESH) {
        d = mesh_mesh_distance_lane(w, A.geom, TA, B.geom, TB, best[g], q1, q2);
        if (!NP) q1 = q2 = V3{0, 0, 0};
      } else if (A.type == MPG_GEOM_OCTREE) {
        d = mesh_octree_distance_lane(w, B.geom, TB, A.geom, TA, best[g], tol, q1, q2, st);
      } else if (B.type == MPG_GEOM_OCTREE) {
        d = mesh_octree_distance_lane(w, A.geom, TA, B.geom, TB, best[g], tol, q1, q2, st);
      } else if (A.type == MPG_GEOM_MESH) {
        d = mesh_shape_distance_lane(w, HV, A.geom, TA, B, TB, best[g], tol, q1, q2, st);
      } else {
        V3 pm, ps;
        d = mesh_shape_distance_lane(w, HV, B.geom, TB, A, TA, best[g], tol, pm, ps, st);
        q1 = NP ? ps : pm;  // distance() swaps the points back with enable_nearest_points
        q2 = NP ? pm : ps;
      }
    } else if (w.pair_cf[p] == CF_OCTREE) {  // leaf box first whatever the order; unsigned
      if (!live || best[g] <= -1.0) continue;
      const bool oa = A.type == MPG_GEOM_OCTREE;
      const SE3 TO = pose_se3(w, poses, n, cfg, oa ? a : b);  // static, or riding on a link / attached body
      const SE3 TS = pose_se3(w, poses, n, cfg, oa ? b : a);
      d = oa ? octree_distance(w, HV, A.geom, TO, B, TS, cb, rb, best[g], tol, q1, q2, st)
             : octree_distance(w, HV, B.geom, TO, A, TS, ca, ra, best[g], tol, q1, q2, st);
    } else {
      if (!live) continue;
      const V3 dc = vsub(cb, ca);
      const double lb = std::sqrt(d3dot(dc, dc)) - ra - rb - 1e-9;
      const double slack = dist_slack(&ca.x, &cb.x);
      // with signed distances a pair is skipped only when its shapes are
      // apart: an intersecting pair reaches EPA, which can throw
      // (FCL_THROW_FAILED_AT_THIS_CONFIGURATION) however deep the running
      // minimum already is, and FCL runs every pair (planning_world.cpp:509-537)
      if (lb > best[g] + slack && (!SIGNED || lb > slack)) continue;
      bool done = false;
      if constexpr (!SIGNED) {
        const SE3 TA = pose_se3(w, poses, n, cfg, a), TB = pose_se3(w, poses, n, cfg, b);
        done = cf_shape_distance(w, A.geom, A.type, TA, B.geom, B.type, TB, d, q1, q2);
        if constexpr (INDEP) {  // FCL's own GJK in double (the same closed forms first)
          if (!done) d = gjk_indep_distance(w, HV, A.geom, TA, B.geom, TB, dtol, q1, q2);
          done = true;
        }
      }
      if (!done) {
        auto sup = [&](const CV3& dir) { return csup(w, HV, A, B, dir); };
        ccd_real df;
        CV3 c1, c2;
        const int r = ccdx::gjk_distance<SIGNED>(sup, tol, ptp, df, c1, c2);
        if (r != ccdx::kOk) st = r == ccdx::kThrow ? kDistThrow : kDistOverflow;
        d = df;
        q1 = to_v3(c1);
        q2 = to_v3(c2);
      }
    }
    if (st) break;
    if (d < best[g]) {
      best[g] = d;
      bp[g] = p;
      if constexpr (PTS) {
        bpt[g][0] = q1;
        bpt[g][1] = q2;
      }
    }
  }
  if (!live) return;
  if (st) {
    best[0] = best[1] = __longlong_as_double(0x7ff8000000000000ll);
    bp[0] = bp[1] = st;
  }
  d_self[cfg] = best[0];
  p_self[cfg] = bp[0];
  d_others[cfg] = best[1];
  p_others[cfg] = bp[1];
  if constexpr (PTS) {
    for (int g = 0; g < 2; ++g) {
      double* o = (g ? pts_others : pts_self) + 6 * cfg;
      o[0] = bpt[g][0].x;
      o[1] = bpt[g][0].y;
      o[2] = bpt[g][0].z;
      o[3] = bpt[g][1].x;
      o[4] = bpt[g][1].y;
      o[5] = bpt[g][1].z;
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(128) void distance_kernel(DevWorld w, const double* __restrict__ poses, long long n,
                                                       int n_self, ccd_real tol, double dtol,
                                                       double* __restrict__ d_self, int32_t* __restrict__ p_self,
                                                       double* __restrict__ d_others, int32_t* __restrict__ p_others,
                                                       double* __restrict__ pts_self, double* __restrict__ pts_others) {
  constexpr bool SIGNED = (MODE & MPG_DIST_SIGNED) != 0;
  const long long cfg0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = cfg0 < n;
  const long long cfg = live ? cfg0 : n - 1;
  struct NoPolytope {};
  std::conditional_t<SIGNED, ccdx::Polytope, NoPolytope> polytope;
  ccdx::Polytope* ptp = nullptr;
  if constexpr (SIGNED) ptp = &polytope;
  distance_config<MODE>(w, poses, n, cfg, live, n_self, tol, dtol, ptp, d_self, p_self, d_others, p_others, pts_self,
                        pts_others);
}

// Signed instances only: the configurations distance_kernel left at
// kDistOverflow (an EPA past kPtV vertices; rare -- 29 at most on the parity
// batches, 124 for a sphere deep in a sphere) are listed (overflow_list_kernel:
// list[0] = count, ids after it; the count zeroed by the host), then evaluated
// again from the start by kBigPool lanes, lane k with the k-th kBigPtV-vertex
// polytope of `pool`, taking every kBigPool-th listed configuration.
__global__ __launch_bounds__(256) void overflow_list_kernel(const int32_t* __restrict__ p_self, long long n,
                                                            unsigned* __restrict__ list) {
  const long long cfg = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (cfg < n && p_self[cfg] == kDistOverflow) list[1 + atomicAdd(&list[0], 1u)] = (unsigned)cfg;
}

template <int MODE>
__global__ __launch_bounds__(64) void distance_redo_kernel(DevWorld w, const double* __restrict__ poses, long long n,
                                                           int n_self, ccd_real tol, double dtol,
                                                           double* __restrict__ d_self,
                                                           int32_t* __restrict__ p_self, double* __restrict__ d_others,
                                                           int32_t* __restrict__ p_others,
                                                           double* __restrict__ pts_self,
                                                           double* __restrict__ pts_others,
                                                           ccdx::BigPolytope* __restrict__ pool,
                                                           const unsigned* __restrict__ list) {
  const unsigned k = threadIdx.x, count = list[0];
  for (unsigned i = k; i < count; i += kBigPool)
    distance_config<MODE>(w, poses, n, (long long)list[1 + i], true, n_self, tol, dtol, pool + k, d_self, p_self,
                          d_others, p_others, pts_self, pts_others);
}

// ---------------------------------------------------------------------------
// Contacts: CollisionRequest(enable_contact=True) -> FCL GJKCollide ->
// libccd 2.1 ccdMPRPenetration (discoverPortal, refinePortal, findPenetr /
// findPenetrTouch / findPenetrSegment, findPos; max_iterations 500), the same
// restatement as oracle/collide_oracle.c mpr_penetration.  Runs after the
// collide pipeline on the pairs it reported, one lane per candidate; the
// portal keeps each vertex's per-object support points (v1, v2) for findPos.
// ---------------------------------------------------------------------------
struct SupP {
  CV3 v, v1, v2;
};

__device__ __forceinline__ SupP msupport3(const DevWorld& w, cptr<double> HV, const GObj& a, const GObj& b,
                                          const CV3& dir) {
  SupP s;
  s.v1 = support(w, HV, a, dir);
  s.v2 = support(w, HV, b, vscale(dir, ccd_real(-1)));
  s.v = vsub(s.v1, s.v2);
  return s;
}

__device__ __forceinline__ CV3 portal_dir3(const SupP P[4]) {
  return vnormalize(vcross(vsub(P[2].v, P[1].v), vsub(P[3].v, P[1].v)));
}

__device__ __forceinline__ bool reach_tol(const SupP P[4], const CV3& v4, const CV3& dir, ccd_real tol) {
  const ccd_real dv1 = vdot(P[1].v, dir), dv2 = vdot(P[2].v, dir), dv3 = vdot(P[3].v, dir), dv4 = vdot(v4, dir);
  ccd_real d1 = dv4 - dv1;
  const ccd_real d2 = dv4 - dv2, d3 = dv4 - dv3;
  d1 = (d1 < d2) ? d1 : d2;
  d1 = (d1 < d3) ? d1 : d3;
  return ccd_eq(d1, tol) || d1 < tol;
}

__device__ __forceinline__ void expand3(SupP P[4], const SupP& v4) {
  const CV3 v4v0 = vcross(v4.v, P[0].v);
  if (vdot(P[1].v, v4v0) > 0.0) {
    if (vdot(P[2].v, v4v0) > 0.0) P[1] = v4;
    else P[3] = v4;
  } else {
    if (vdot(P[3].v, v4v0) > 0.0) P[2] = v4;
    else P[1] = v4;
  }
}

__device__ __forceinline__ ccd_real seg_dist2(const CV3& x0, const CV3& b, CV3& wit) {
  const CV3 d = vsub(b, x0), a = x0;  // P = origin
  ccd_real t = -1.0 * vdot(a, d);
  t /= vdot(d, d);
  if (t < 0.0 || is_zero(t)) {
    wit = x0;
  } else if (t > 1.0 || ccd_eq(t, 1.0)) {
    wit = b;
  } else {
    wit = vadd(vscale(d, t), x0);
  }
  return vdot(wit, wit);
}

// ccdVec3PointTriDist2(origin, x0, B, C, witness)
__device__ __forceinline__ ccd_real tri_dist2(const CV3& x0, const CV3& B, const CV3& C, CV3& wit) {
  const CV3 d1 = vsub(B, x0), d2 = vsub(C, x0), a = x0;
  const ccd_real v = vdot(d1, d1), w_ = vdot(d2, d2), p = vdot(a, d1), q = vdot(a, d2), r = vdot(d1, d2);
  const ccd_real d = w_ * v - r * r;
  ccd_real s, t;
  if (is_zero(d)) {
    s = t = -1.0;
  } else {
    s = (q * r - w_ * p) / d;
    t = (-s * r - q) / w_;
  }
  if ((is_zero(s) || s > 0.0) && (ccd_eq(s, 1.0) || s < 1.0) && (is_zero(t) || t > 0.0) && (ccd_eq(t, 1.0) || t < 1.0) &&
      (ccd_eq(t + s, 1.0) || t + s < 1.0)) {
    wit = vadd(vadd(x0, vscale(d1, s)), vscale(d2, t));
    return vdot(wit, wit);
  }
  CV3 w2;
  ccd_real dist = seg_dist2(x0, B, wit);
  ccd_real dist2 = seg_dist2(x0, C, w2);
  if (dist2 < dist) {
    dist = dist2;
    wit = w2;
  }
  dist2 = seg_dist2(B, C, w2);
  if (dist2 < dist) {
    dist = dist2;
    wit = w2;
  }
  return dist;
}

__device__ __forceinline__ CV3 find_pos3(const SupP P[4]) {
  const CV3 dir = portal_dir3(P);
  ccd_real b[4];
  b[0] = vdot(vcross(P[1].v, P[2].v), P[3].v);
  b[1] = vdot(vcross(P[3].v, P[2].v), P[0].v);
  b[2] = vdot(vcross(P[0].v, P[1].v), P[3].v);
  b[3] = vdot(vcross(P[2].v, P[1].v), P[0].v);
  ccd_real sum = b[0] + b[1] + b[2] + b[3];
  if (is_zero(sum) || sum < 0.0) {
    b[0] = 0.0;
    b[1] = vdot(vcross(P[2].v, P[3].v), dir);
    b[2] = vdot(vcross(P[3].v, P[1].v), dir);
    b[3] = vdot(vcross(P[1].v, P[2].v), dir);
    sum = b[1] + b[2] + b[3];
  }
  const ccd_real inv = ccd_real(1) / sum;
  CV3 p1{0, 0, 0}, p2{0, 0, 0};
  for (int i = 0; i < 4; ++i) {
    p1 = vadd(p1, vscale(P[i].v1, b[i]));
    p2 = vadd(p2, vscale(P[i].v2, b[i]));
  }
  p1 = vscale(p1, inv);
  p2 = vscale(p2, inv);
  return vscale(vadd(p1, p2), ccd_real(0.5));
}

// ccdMPRPenetration: true if penetrating (depth, dir, pos set); sup(dir)
// gives the Minkowski support with both objects' points, c1 / c2 the centres
template <typename Sup3>
__device__ bool mpr_penetration_core(ccd_real tol, const CV3& c1, const CV3& c2, Sup3 msup, ccd_real& depth,
                                     CV3& dir_out, CV3& pos_out) {
  SupP P[4];
  P[0].v1 = c1;
  P[0].v2 = c2;
  P[0].v = vsub(P[0].v1, P[0].v2);
  if (vec_is_origin(P[0].v)) P[0].v = vadd(P[0].v, cv3(kCcdEps * ccd_real(10), 0.0, 0.0));
  CV3 dir = vnormalize(vscale(P[0].v, ccd_real(-1)));
  P[1] = msup(dir);
  ccd_real dot = vdot(P[1].v, dir);
  if (is_zero(dot) || dot < 0.0) return false;
  dir = vcross(P[0].v, P[1].v);
  if (is_zero(vdot(dir, dir))) {
    pos_out = vscale(vadd(P[1].v1, P[1].v2), ccd_real(0.5));
    if (vec_is_origin(P[1].v)) {  // findPenetrTouch
      depth = 0.0;
      dir_out = cv3(0.0, 0.0, 0.0);
    } else {  // findPenetrSegment
      dir_out = P[1].v;
      depth = std::sqrt(vdot(dir_out, dir_out));
      dir_out = vnormalize(dir_out);
    }
    return true;
  }
  dir = vnormalize(dir);
  P[2] = msup(dir);
  dot = vdot(P[2].v, dir);
  if (is_zero(dot) || dot < 0.0) return false;
  dir = vnormalize(vcross(vsub(P[1].v, P[0].v), vsub(P[2].v, P[0].v)));
  if (vdot(dir, P[0].v) > 0.0) {
    const SupP t = P[1];
    P[1] = P[2];
    P[2] = t;
    dir = vscale(dir, ccd_real(-1));
  }
  for (;;) {
    P[3] = msup(dir);
    dot = vdot(P[3].v, dir);
    if (is_zero(dot) || dot < 0.0) return false;
    bool cont = false;
    ccd_real d2 = vdot(vcross(P[1].v, P[3].v), P[0].v);
    if (d2 < 0.0 && !is_zero(d2)) {
      P[2] = P[3];
      cont = true;
    }
    if (!cont) {
      d2 = vdot(vcross(P[3].v, P[2].v), P[0].v);
      if (d2 < 0.0 && !is_zero(d2)) {
        P[1] = P[3];
        cont = true;
      }
    }
    if (!cont) break;
    dir = vnormalize(vcross(vsub(P[1].v, P[0].v), vsub(P[2].v, P[0].v)));
  }
  // refinePortal
  for (;;) {
    dir = portal_dir3(P);
    const ccd_real d = vdot(dir, P[1].v);
    if (is_zero(d) || d > 0.0) break;
    const SupP v4 = msup(dir);
    const ccd_real dv4 = vdot(v4.v, dir);
    if (!(is_zero(dv4) || dv4 > 0.0) || reach_tol(P, v4.v, dir, tol)) return false;
    expand3(P, v4);
  }
  // findPenetr
  for (unsigned long it = 0;; ++it) {
    dir = portal_dir3(P);
    const SupP v4 = msup(dir);
    if (reach_tol(P, v4.v, dir, tol) || it > 500UL) {
      CV3 wit;
      depth = std::sqrt(tri_dist2(P[1].v, P[2].v, P[3].v, wit));
      dir_out = is_zero(depth) ? cv3(0.0, 0.0, 0.0) : vnormalize(wit);
      pos_out = find_pos3(P);
      return true;
    }
    expand3(P, v4);
  }
}

__device__ bool mpr_penetration_ccd(const DevWorld& w, cptr<double> HV, const GObj& A, const GObj& B, ccd_real& depth,
                                    CV3& dir_out, CV3& pos_out) {
  return mpr_penetration_core(w.mpr_tol, center(w, A), center(w, B),
                              [&](const CV3& d) { return msupport3(w, HV, A, B, d); }, depth, dir_out, pos_out);
}

// FCL reads the contact back into fp64 (Contact<double>)
__device__ bool mpr_penetration(const DevWorld& w, cptr<double> HV, const GObj& A, const GObj& B, double& depth,
                                V3& dir_out, V3& pos_out) {
  ccd_real d = 0;
  CV3 n{0, 0, 0}, ps{0, 0, 0};
  const bool hit = mpr_penetration_ccd(w, HV, A, B, d, n, ps);
  if (hit) {
    depth = d;
    dir_out = to_v3(n);
    pos_out = to_v3(ps);
  }
  return hit;
}

// ---------------------------------------------------------------------------
// FCL closed-form contacts (CollisionRequest(enable_contact=True) on box-box,
// sphere-sphere, sphere-box, sphere-capsule, sphere-cylinder pairs, both orders): the contacts FCL 0.7.0's
// GJKSolver_libccd::shapeIntersect specialisations emit, reduced to the one
// ShapeShapeCollide keeps for num_max_contacts = 1 (partial_sort by
// descending penetration_depth, first of equals).  Same operation order as
// oracle/collide_oracle.c box_box_contact & co (parity unpinned: FCL's
// contact code is not under /root/reference).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void cf_keep(int& n, double pd, const double* nrm, const double* p, double& depth, V3& nd,
                                        V3& ps) {
  if (n == 0 || pd > depth) {
    depth = pd;
    nd = v3(nrm[0], nrm[1], nrm[2]);
    ps = v3(p[0], p[1], p[2]);
  }
  ++n;
}

// ODE intersectRectQuad (box_box-inl.h intersectRectQuad2)
__device__ int cf_rect_quad(const double h[2], double p[8], double ret[16]) {
  int nq = 4, nr = 0;
  double buffer[16];
  double* q = p;
  double* r = ret;
  for (int dir = 0; dir <= 1; ++dir) {
    for (int sign = -1; sign <= 1; sign += 2) {
      double* pq = q;
      double* pr = r;
      nr = 0;
      for (int i = nq; i > 0; --i) {
        if (sign * pq[dir] < h[dir]) {
          pr[0] = pq[0];
          pr[1] = pq[1];
          pr += 2;
          nr++;
          if (nr & 8) {
            q = r;
            goto done;
          }
        }
        double* nextq = (i > 1) ? pq + 2 : q;
        if ((sign * pq[dir] < h[dir]) ^ (sign * nextq[dir] < h[dir])) {
          pr[1 - dir] = pq[1 - dir] + (nextq[1 - dir] - pq[1 - dir]) / (nextq[dir] - pq[dir]) * (sign * h[dir] - pq[dir]);
          pr[dir] = sign * h[dir];
          pr += 2;
          nr++;
          if (nr & 8) {
            q = r;
            goto done;
          }
        }
        pq += 2;
      }
      q = r;
      r = (q == ret) ? buffer : ret;
      nq = nr;
    }
  }
done:
  if (q != ret)
    for (int i = 0; i < 2 * nr; ++i) ret[i] = q[i];
  return nr;
}

// ODE cullPoints (box_box-inl.h cullPoints2)
__device__ void cf_cull_points(int n, const double* p, int m, int i0, int* iret) {
  double a, cx, cy, q;
  if (n == 1) {
    cx = p[0];
    cy = p[1];
  } else if (n == 2) {
    cx = 0.5 * (p[0] + p[2]);
    cy = 0.5 * (p[1] + p[3]);
  } else {
    a = 0;
    cx = 0;
    cy = 0;
    for (int i = 0; i < n - 1; ++i) {
      q = p[i * 2] * p[i * 2 + 3] - p[i * 2 + 2] * p[i * 2 + 1];
      a += q;
      cx += q * (p[i * 2] + p[i * 2 + 2]);
      cy += q * (p[i * 2 + 1] + p[i * 2 + 3]);
    }
    q = p[n * 2 - 2] * p[1] - p[0] * p[n * 2 - 1];
    if (std::fabs(a + q) > DBL_EPSILON) a = 1 / (3 * (a + q));
    else a = (double)1e18f;
    cx = a * (cx + q * (p[n * 2 - 2] + p[0]));
    cy = a * (cy + q * (p[n * 2 - 1] + p[1]));
  }
  double A[8];
  int avail[8];
  for (int i = 0; i < n; ++i) {
    A[i] = std::atan2(p[i * 2 + 1] - cy, p[i * 2] - cx);
    avail[i] = 1;
  }
  avail[i0] = 0;
  iret[0] = i0;
  const double pi = 3.14159265358979323846;
  for (int j = 1; j < m; ++j) {
    a = j * (2 * pi / m) + A[i0];
    if (a > pi) a -= 2 * pi;
    double maxdiff = 1e9, diff;
    iret[j] = i0;
    for (int i = 0; i < n; ++i) {
      if (avail[i]) {
        diff = std::fabs(A[i] - a);
        if (diff > pi) diff = 2 * pi - diff;
        if (diff < maxdiff) {
          maxdiff = diff;
          iret[j] = i;
        }
      }
    }
    avail[iret[j]] = 0;
  }
}

// detail::boxBox2 with contacts (maxc 4) -> the kept contact
__device__ bool box_box_contact(const double* side1, const SE3& T1, const double* side2, const SE3& T2, double& dout,
                                V3& nout, V3& pout) {
#define R1_(i, j) T1.R[3 * (i) + (j)]
#define R2_(i, j) T2.R[3 * (i) + (j)]
  int nc = 0;
  const double p[3] = {T2.p[0] - T1.p[0], T2.p[1] - T1.p[1], T2.p[2] - T1.p[2]};
  double pp[3], A[3], B[3], R[3][3], Q[3][3];
  for (int i = 0; i < 3; ++i) pp[i] = (R1_(0, i) * p[0] + R1_(1, i) * p[1]) + R1_(2, i) * p[2];
  for (int i = 0; i < 3; ++i) {
    A[i] = side1[i] * 0.5;
    B[i] = side2[i] * 0.5;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      R[i][j] = (R1_(0, i) * R2_(0, j) + R1_(1, i) * R2_(1, j)) + R1_(2, i) * R2_(2, j);
      Q[i][j] = std::fabs(R[i][j]);
    }
  double s = -DBL_MAX, s2, tmp, normalC[3] = {0, 0, 0};
  int code = 0, best_col = -1, normal_r2 = 0, invert = 0;
  for (int i = 0; i < 3; ++i) {
    tmp = pp[i];
    s2 = std::fabs(tmp) - (((Q[i][0] * B[0] + Q[i][1] * B[1]) + Q[i][2] * B[2]) + A[i]);
    if (s2 > 0) return false;
    if (s2 > s) {
      s = s2;
      best_col = i;
      normal_r2 = 0;
      invert = tmp < 0;
      code = 1 + i;
    }
  }
  for (int j = 0; j < 3; ++j) {
    tmp = (R2_(0, j) * p[0] + R2_(1, j) * p[1]) + R2_(2, j) * p[2];
    s2 = std::fabs(tmp) - (((Q[0][j] * A[0] + Q[1][j] * A[1]) + Q[2][j] * A[2]) + B[j]);
    if (s2 > 0) return false;
    if (s2 > s) {
      s = s2;
      best_col = j;
      normal_r2 = 1;
      invert = tmp < 0;
      code = 4 + j;
    }
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Q[i][j] += 1.0e-6;
  const double eps = DBL_EPSILON, fudge = 1.05;
  auto edge = [&](double t, double rad, double n0, double n1, double n2, int c) -> bool {
    tmp = t;
    s2 = std::fabs(tmp) - rad;
    if (s2 > eps) return true;
    const double l = std::sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    if (l > eps) {
      s2 /= l;
      if (s2 * fudge > s) {
        s = s2;
        best_col = -1;
        invert = tmp < 0;
        code = c;
        normalC[0] = n0 / l;
        normalC[1] = n1 / l;
        normalC[2] = n2 / l;
      }
    }
    return false;
  };
  if (edge(pp[2] * R[1][0] - pp[1] * R[2][0], ((A[1] * Q[2][0] + A[2] * Q[1][0]) + B[1] * Q[0][2]) + B[2] * Q[0][1], 0,
           -R[2][0], R[1][0], 7)) return false;
  if (edge(pp[2] * R[1][1] - pp[1] * R[2][1], ((A[1] * Q[2][1] + A[2] * Q[1][1]) + B[0] * Q[0][2]) + B[2] * Q[0][0], 0,
           -R[2][1], R[1][1], 8)) return false;
  if (edge(pp[2] * R[1][2] - pp[1] * R[2][2], ((A[1] * Q[2][2] + A[2] * Q[1][2]) + B[0] * Q[0][1]) + B[1] * Q[0][0], 0,
           -R[2][2], R[1][2], 9)) return false;
  if (edge(pp[0] * R[2][0] - pp[2] * R[0][0], ((A[0] * Q[2][0] + A[2] * Q[0][0]) + B[1] * Q[1][2]) + B[2] * Q[1][1],
           R[2][0], 0, -R[0][0], 10)) return false;
  if (edge(pp[0] * R[2][1] - pp[2] * R[0][1], ((A[0] * Q[2][1] + A[2] * Q[0][1]) + B[0] * Q[1][2]) + B[2] * Q[1][0],
           R[2][1], 0, -R[0][1], 11)) return false;
  if (edge(pp[0] * R[2][2] - pp[2] * R[0][2], ((A[0] * Q[2][2] + A[2] * Q[0][2]) + B[0] * Q[1][1]) + B[1] * Q[1][0],
           R[2][2], 0, -R[0][2], 12)) return false;
  if (edge(pp[1] * R[0][0] - pp[0] * R[1][0], ((A[0] * Q[1][0] + A[1] * Q[0][0]) + B[1] * Q[2][2]) + B[2] * Q[2][1],
           -R[1][0], R[0][0], 0, 13)) return false;
  if (edge(pp[1] * R[0][1] - pp[0] * R[1][1], ((A[0] * Q[1][1] + A[1] * Q[0][1]) + B[0] * Q[2][2]) + B[2] * Q[2][0],
           -R[1][1], R[0][1], 0, 14)) return false;
  if (edge(pp[1] * R[0][2] - pp[0] * R[1][2], ((A[0] * Q[1][2] + A[1] * Q[0][2]) + B[0] * Q[2][1]) + B[1] * Q[2][0],
           -R[1][2], R[0][2], 0, 15)) return false;
  if (!code) return false;
  double normal[3];
  if (best_col != -1) {
    const double* Rm = normal_r2 ? T2.R : T1.R;
    for (int i = 0; i < 3; ++i) normal[i] = Rm[3 * i + best_col];
  } else {
    for (int i = 0; i < 3; ++i) normal[i] = (R1_(i, 0) * normalC[0] + R1_(i, 1) * normalC[1]) + R1_(i, 2) * normalC[2];
  }
  if (invert)
    for (int i = 0; i < 3; ++i) normal[i] = -normal[i];
  const double depth = -s;
  if (code > 6) {  // edge-edge: the closest point of box 2's edge
    double pa[3] = {T1.p[0], T1.p[1], T1.p[2]}, pb[3] = {T2.p[0], T2.p[1], T2.p[2]}, sign;
    for (int j = 0; j < 3; ++j) {
      sign = (((R1_(0, j) * normal[0] + R1_(1, j) * normal[1]) + R1_(2, j) * normal[2]) > 0) ? 1 : -1;
      for (int i = 0; i < 3; ++i) pa[i] += R1_(i, j) * (A[j] * sign);
    }
    for (int j = 0; j < 3; ++j) {
      sign = (((R2_(0, j) * normal[0] + R2_(1, j) * normal[1]) + R2_(2, j) * normal[2]) > 0) ? -1 : 1;
      for (int i = 0; i < 3; ++i) pb[i] += R2_(i, j) * (B[j] * sign);
    }
    const int ca = (code - 7) / 3, cb = (code - 7) % 3;
    const double ua[3] = {R1_(0, ca), R1_(1, ca), R1_(2, ca)}, ub[3] = {R2_(0, cb), R2_(1, cb), R2_(2, cb)};
    // lineClosestApproach (ODE dLineClosestApproach); only beta is used
    const double d0 = pb[0] - pa[0], d1 = pb[1] - pa[1], d2 = pb[2] - pa[2];
    const double uaub = (ua[0] * ub[0] + ua[1] * ub[1]) + ua[2] * ub[2];
    const double q1 = (ua[0] * d0 + ua[1] * d1) + ua[2] * d2;
    const double q2 = -((ub[0] * d0 + ub[1] * d1) + ub[2] * d2);
    double dd = 1 - uaub * uaub, beta = 0;
    if (!(dd <= (double)0.0001f)) {
      dd = 1 / dd;
      beta = (uaub * q1 + q2) * dd;
    }
    for (int i = 0; i < 3; ++i) pb[i] += ub[i] * beta;
    cf_keep(nc, -depth, normal, pb, dout, nout, pout);
    return true;
  }
  // face-something: reference face on box a, incident box b
  const double* Ra = code <= 3 ? T1.R : T2.R;
  const double* Rb = code <= 3 ? T2.R : T1.R;
  const double* pa = code <= 3 ? T1.p : T2.p;
  const double* pb = code <= 3 ? T2.p : T1.p;
  const double* Sa = code <= 3 ? A : B;
  const double* Sb = code <= 3 ? B : A;
#define RA(i, j) Ra[3 * (i) + (j)]
#define RB(i, j) Rb[3 * (i) + (j)]
  double normal2[3], nr[3], anr[3];
  for (int i = 0; i < 3; ++i) normal2[i] = code <= 3 ? normal[i] : -normal[i];
  for (int j = 0; j < 3; ++j) {
    nr[j] = (RB(0, j) * normal2[0] + RB(1, j) * normal2[1]) + RB(2, j) * normal2[2];
    anr[j] = std::fabs(nr[j]);
  }
  int lanr, a1, a2;
  if (anr[1] > anr[0]) {
    if (anr[1] > anr[2]) { a1 = 0; lanr = 1; a2 = 2; }
    else { a1 = 0; a2 = 1; lanr = 2; }
  } else {
    if (anr[0] > anr[2]) { lanr = 0; a1 = 1; a2 = 2; }
    else { a1 = 0; a2 = 1; lanr = 2; }
  }
  double center[3];
  for (int i = 0; i < 3; ++i)
    center[i] = nr[lanr] < 0 ? (pb[i] - pa[i]) + RB(i, lanr) * Sb[lanr] : (pb[i] - pa[i]) - RB(i, lanr) * Sb[lanr];
  const int codeN = code <= 3 ? code - 1 : code - 4;
  const int code1 = codeN == 0 ? 1 : 0, code2 = codeN == 2 ? 1 : 2;
  const double c1 = (RA(0, code1) * center[0] + RA(1, code1) * center[1]) + RA(2, code1) * center[2];
  const double c2 = (RA(0, code2) * center[0] + RA(1, code2) * center[1]) + RA(2, code2) * center[2];
  double m11 = (RB(0, a1) * RA(0, code1) + RB(1, a1) * RA(1, code1)) + RB(2, a1) * RA(2, code1);
  double m12 = (RB(0, a2) * RA(0, code1) + RB(1, a2) * RA(1, code1)) + RB(2, a2) * RA(2, code1);
  double m21 = (RB(0, a1) * RA(0, code2) + RB(1, a1) * RA(1, code2)) + RB(2, a1) * RA(2, code2);
  double m22 = (RB(0, a2) * RA(0, code2) + RB(1, a2) * RA(1, code2)) + RB(2, a2) * RA(2, code2);
  double quad[8];
  {
    const double k1 = m11 * Sb[a1], k2 = m21 * Sb[a1], k3 = m12 * Sb[a2], k4 = m22 * Sb[a2];
    quad[0] = c1 - k1 - k3;
    quad[1] = c2 - k2 - k4;
    quad[2] = c1 - k1 + k3;
    quad[3] = c2 - k2 + k4;
    quad[4] = c1 + k1 + k3;
    quad[5] = c2 + k2 + k4;
    quad[6] = c1 + k1 - k3;
    quad[7] = c2 + k2 - k4;
  }
  const double rect[2] = {Sa[code1], Sa[code2]};
  double ret[16];
  const int n_intersect = cf_rect_quad(rect, quad, ret);
  if (n_intersect < 1) return true;  // collision without a contact point
  double points[8][3], dep[8];
  const double det1 = 1.f / (m11 * m22 - m12 * m21);
  m11 *= det1;
  m12 *= det1;
  m21 *= det1;
  m22 *= det1;
  int cnum = 0;
  for (int j = 0; j < n_intersect; ++j) {
    const double k1 = m22 * (ret[j * 2] - c1) - m12 * (ret[j * 2 + 1] - c2);
    const double k2 = -m21 * (ret[j * 2] - c1) + m11 * (ret[j * 2 + 1] - c2);
    for (int i = 0; i < 3; ++i) points[cnum][i] = (center[i] + RB(i, a1) * k1) + RB(i, a2) * k2;
    dep[cnum] = Sa[codeN] - ((normal2[0] * points[cnum][0] + normal2[1] * points[cnum][1]) + normal2[2] * points[cnum][2]);
    if (dep[cnum] >= 0) {
      ret[cnum * 2] = ret[j * 2];
      ret[cnum * 2 + 1] = ret[j * 2 + 1];
      cnum++;
    }
  }
  if (cnum < 1) return true;
  int iret[8];
  if (cnum <= 4) {
    for (int j = 0; j < cnum; ++j) iret[j] = j;
  } else {
    int i1 = 0;
    double maxdepth = dep[0];
    for (int i = 1; i < cnum; ++i)
      if (dep[i] > maxdepth) {
        maxdepth = dep[i];
        i1 = i;
      }
    cf_cull_points(cnum, ret, 4, i1, iret);
    cnum = 4;
  }
  for (int j = 0; j < cnum; ++j) {
    const int k = iret[j];
    double wpt[3];
    for (int i = 0; i < 3; ++i) wpt[i] = code < 4 ? points[k][i] + pa[i] : (points[k][i] + pa[i]) - normal[i] * dep[k];
    cf_keep(nc, -dep[k], normal, wpt, dout, nout, pout);
  }
#undef RA
#undef RB
#undef R1_
#undef R2_
  return true;
}

// detail::sphereSphereIntersect with its contact
__device__ bool sphere_sphere_contact(double r1, const SE3& T1, double r2, const SE3& T2, double& depth, V3& nd,
                                      V3& ps) {
  const double d0 = T2.p[0] - T1.p[0], d1 = T2.p[1] - T1.p[1], d2 = T2.p[2] - T1.p[2];
  const double len = std::sqrt((d0 * d0 + d1 * d1) + d2 * d2);
  if (len > r1 + r2) return false;
  nd = len > 0 ? v3(d0 / len, d1 / len, d2 / len) : v3(d0, d1, d2);
  ps = v3(T1.p[0] + d0 * r1 / (r1 + r2), T1.p[1] + d1 * r1 / (r1 + r2), T1.p[2] + d2 * r1 / (r1 + r2));
  depth = r1 + r2 - len;
  return true;
}

// detail::sphereBoxIntersect with its contact (normal from the sphere into the box)
__device__ bool sphere_box_contact(double r, const SE3& TS, const double* side, const SE3& TB, double& depth, V3& nd,
                                   V3& ps) {
  double c[3], d[3];
  bool clamped = false;
  for (int i = 0; i < 3; ++i) {
    const double inv_t = -((TB.R[i] * TB.p[0] + TB.R[3 + i] * TB.p[1]) + TB.R[6 + i] * TB.p[2]);
    c[i] = ((TB.R[i] * TS.p[0] + TB.R[3 + i] * TS.p[1]) + TB.R[6 + i] * TS.p[2]) + inv_t;
    const double h = side[i] / 2;
    double nq = c[i];
    if (c[i] < -h) {
      clamped = true;
      nq = -h;
    }
    if (c[i] > h) {
      clamped = true;
      nq = h;
    }
    d[i] = c[i] - nq;
  }
  const double dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  if (clamped && dd > r * r) return false;
  double n[3] = {0, 0, 0}, dep;
  if (clamped) {
    const double dist = std::sqrt(dd);
    for (int i = 0; i < 3; ++i) n[i] = -d[i] / dist;
    dep = r - dist;
  } else {
    double min_d = INFINITY;
    int ax = 0;
    for (int i = 0; i < 3; ++i) {
      const double di = side[i] / 2 - std::fabs(c[i]);
      if (di < min_d) {
        min_d = di;
        ax = i;
      }
    }
    n[ax] = c[ax] >= 0 ? -1 : 1;
    dep = min_d + r;
  }
  double pc[3], nw[3], pw[3];
  for (int i = 0; i < 3; ++i) pc[i] = c[i] + n[i] * (r - dep / 2);
  for (int i = 0; i < 3; ++i) {
    nw[i] = (TB.R[3 * i] * n[0] + TB.R[3 * i + 1] * n[1]) + TB.R[3 * i + 2] * n[2];
    pw[i] = ((TB.R[3 * i] * pc[0] + TB.R[3 * i + 1] * pc[1]) + TB.R[3 * i + 2] * pc[2]) + TB.p[i];
  }
  nd = v3(nw[0], nw[1], nw[2]);
  ps = v3(pw[0], pw[1], pw[2]);
  depth = dep;
  return true;
}

// detail::sphereCapsuleIntersect with its contact (oracle sphere_capsule_contact)
__device__ bool sphere_capsule_contact(double r1, const SE3& TS, double r2, double lz, const SE3& TC, double& depth,
                                       V3& nd, V3& ps) {
  double c[3];
  centre_in_frame(TS, TC, c);
  const double s1z = 0.5 * lz, s2z = -s1z;
  const double vz = s2z - s1z;
  const double w2 = c[2] - s1z;
  const double c1 = (c[0] * 0.0 + c[1] * 0.0) + w2 * vz;
  const double c2 = (0.0 * 0.0 + 0.0 * 0.0) + vz * vz;
  double spz;
  if (c1 <= 0) spz = s1z;
  else if (c2 <= c1) spz = s2z;
  else spz = s1z + vz * (c1 / c2);
  const double d[3] = {c[0], c[1], c[2] - spz};
  const double sq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  const double dist = std::sqrt(sq) - r1 - r2;
  if (dist > 0) return false;
  const double nn = std::sqrt(sq);
  double ln[3], lp[3], nw[3], pw[3];
  for (int i = 0; i < 3; ++i) ln[i] = sq > 0 ? -(d[i] / nn) : -d[i];
  lp[0] = 0.0 + ln[0] * dist;
  lp[1] = 0.0 + ln[1] * dist;
  lp[2] = spz + ln[2] * dist;
  for (int i = 0; i < 3; ++i) {
    nw[i] = (TC.R[3 * i] * ln[0] + TC.R[3 * i + 1] * ln[1]) + TC.R[3 * i + 2] * ln[2];
    pw[i] = ((TC.R[3 * i] * lp[0] + TC.R[3 * i + 1] * lp[1]) + TC.R[3 * i + 2] * lp[2]) + TC.p[i];
  }
  nd = v3(nw[0], nw[1], nw[2]);
  ps = v3(pw[0], pw[1], pw[2]);
  depth = -dist;
  return true;
}

// detail::sphereCylinderIntersect with its contact (oracle sphere_cylinder_contact)
__device__ bool sphere_cylinder_contact(double r, const SE3& TS, double rc, double lz, const SE3& TC, double& depth,
                                        V3& nd, V3& ps) {
  double c[3], q[3];
  centre_in_frame(TS, TC, c);
  const double h = lz / 2;
  bool clamped = false;
  q[0] = c[0];
  q[1] = c[1];
  q[2] = c[2];
  if (c[2] > h) {
    q[2] = h;
    clamped = true;
  } else if (c[2] < -h) {
    q[2] = -h;
    clamped = true;
  }
  const double rd2 = c[0] * c[0] + c[1] * c[1];
  if (rd2 > rc * rc) {
    const double scale = rc / std::sqrt(rd2);
    q[0] = c[0] * scale;
    q[1] = c[1] * scale;
    clamped = true;
  }
  const double d[3] = {q[0] - c[0], q[1] - c[1], q[2] - c[2]};
  const double dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  if (clamped && dd > r * r) return false;
  double n[3] = {0, 0, 0}, dep;
  if (clamped) {
    const double dist = std::sqrt(dd);
    for (int i = 0; i < 3; ++i) n[i] = d[i] / dist;
    dep = r - dist;
  } else {
    const double face = h - std::fabs(c[2]);
    const double rad = std::sqrt(rd2);
    const double barrel = rc - rad;
    if (face <= barrel) {
      n[2] = c[2] >= 0 ? -1 : 1;
      dep = face + r;
    } else {
      if (rad > 0) {
        n[0] = -(c[0] / rad);
        n[1] = -(c[1] / rad);
      } else {
        n[0] = -1;
      }
      dep = barrel + r;
    }
  }
  double pc[3], nw[3], pw[3];
  for (int i = 0; i < 3; ++i) pc[i] = c[i] + n[i] * (r - dep / 2);
  for (int i = 0; i < 3; ++i) {
    nw[i] = (TC.R[3 * i] * n[0] + TC.R[3 * i + 1] * n[1]) + TC.R[3 * i + 2] * n[2];
    pw[i] = ((TC.R[3 * i] * pc[0] + TC.R[3 * i + 1] * pc[1]) + TC.R[3 * i + 2] * pc[2]) + TC.p[i];
  }
  nd = v3(nw[0], nw[1], nw[2]);
  ps = v3(pw[0], pw[1], pw[2]);
  depth = dep;
  return true;
}

// CollisionRequest(enable_contact=True) on a (shape, OcTree) pair
// [ext FCL 0.7.0 OcTreeShapeIntersectRecurse with contacts]: the first
// occupied leaf in traversal order (the leaf list's order) whose OBB
// overlaps the shape's and whose box intersects it; its contact from
// shapeIntersect(leaf box, shape): the tree is the contact's o1, the normal
// points from the leaf into the shape (oracle octree_contact).  One lane
// walks the whole leaf list: contacts are a scalar-API path.
__device__ bool octree_first_contact(const DevWorld& w, cptr<double> HV, int go, const SE3& TO, int gs, const SE3& TS,
                                     double& depth, V3& nd, V3& ps) {
  const cptr<double> grs = w.geom_rec + G_STRIDE * gs;
  const int ts = w.geom_type[gs];
  double sc[3], se[3], Rl[9];
  for (int i = 0; i < 3; ++i) se[i] = grs[G_AABB_E + i];
  for (int i = 0; i < 3; ++i)
    sc[i] = ((TS.R[3 * i] * grs[G_OBB_C] + TS.R[3 * i + 1] * grs[G_OBB_C + 1]) + TS.R[3 * i + 2] * grs[G_OBB_C + 2]) +
            TS.p[i];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Rl[3 * i + j] = (TO.R[i] * TS.R[j] + TO.R[3 + i] * TS.R[3 + j]) + TO.R[6 + i] * TS.R[6 + j];
  GObj B;
  B.rot = gjk_rot_from_matrix(TS.R);
  B.rot_inv = quat_invert2(B.rot);
  B.pos = cv3(TS.p[0], TS.p[1], TS.p[2]);
  B.geom = gs;
  B.type = ts;
  GObj A;
  A.rot = gjk_rot_from_matrix(TO.R);
  A.rot_inv = quat_invert2(A.rot);
  A.geom = go;
  A.type = MPG_GEOM_BOX;
  const double sb[3] = {grs[G_PARAM], grs[G_PARAM + 1], grs[G_PARAM + 2]};
  const cptr<double> gor = w.geom_rec + G_STRIDE * go;
  const int l0 = (int)gor[G_PARAM], ln = (int)gor[G_PARAM + 1];
  for (int l = l0; l < l0 + ln; ++l) {
    const cptr<double> L = w.oct_leaf + 6 * (size_t)l;
    double c[3], cw[3], a[3], side[3], t[3], T[3];
    for (int i = 0; i < 3; ++i) {
      c[i] = (L[i] + L[3 + i]) * 0.5;
      side[i] = L[3 + i] - L[i];
      a[i] = side[i] * 0.5;
    }
    for (int i = 0; i < 3; ++i) cw[i] = ((TO.R[3 * i] * c[0] + TO.R[3 * i + 1] * c[1]) + TO.R[3 * i + 2] * c[2]) + TO.p[i];
    for (int i = 0; i < 3; ++i) t[i] = sc[i] - cw[i];
    for (int i = 0; i < 3; ++i) T[i] = (TO.R[i] * t[0] + TO.R[3 + i] * t[1]) + TO.R[6 + i] * t[2];
    if (obb_disjoint(Rl, T, a, se)) continue;
    SE3 TL;
    for (int i = 0; i < 9; ++i) TL.R[i] = TO.R[i];
    for (int i = 0; i < 3; ++i) TL.p[i] = cw[i];
    depth = 0.0;
    nd = v3(0, 0, 0);
    ps = v3(0, 0, 0);
    bool hit;
    if (ts == MPG_GEOM_BOX) {
      hit = box_box_contact(side, TL, sb, TS, depth, nd, ps);
    } else if (ts == MPG_GEOM_SPHERE) {
      hit = sphere_box_contact(sb[0], TS, side, TL, depth, nd, ps);
      nd = v3(-nd.x, -nd.y, -nd.z);  // flipNormal
    } else {
      GObj A1 = A;
      A1.pos = cv3(cw[0], cw[1], cw[2]);
      const ccd_real h[3] = {(ccd_real)(side[0] / 2.0), (ccd_real)(side[1] / 2.0), (ccd_real)(side[2] / 2.0)};
      ccd_real dc = 0;
      CV3 n{0, 0, 0}, pc{0, 0, 0};
      hit = mpr_penetration_core(
          w.mpr_tol, A1.pos, center(w, B),
          [&](const CV3& d) {
            SupP sp;
            const CV3 da = quat_rot(d, A1.rot_inv);
            const CV3 la = CV3{(da.x >= 0 ? ccd_real(1) : ccd_real(-1)) * h[0], (da.y >= 0 ? ccd_real(1) : ccd_real(-1)) * h[1],
                               (da.z >= 0 ? ccd_real(1) : ccd_real(-1)) * h[2]};
            sp.v1 = vadd(quat_rot(la, A1.rot), A1.pos);
            sp.v2 = support(w, HV, B, vscale(d, ccd_real(-1)));
            sp.v = vsub(sp.v1, sp.v2);
            return sp;
          },
          dc, n, pc);
      if (hit) {
        depth = dc;
        nd = to_v3(n);
        ps = to_v3(pc);
      }
    }
    if (hit) return true;
  }
  depth = 0.0;
  nd = v3(0, 0, 0);
  ps = v3(0, 0, 0);
  return false;
}

__host__ __device__ __forceinline__ bool cf_has_contact(int cf) {
  return cf != CF_NONE && cf != CF_OCTREE && cf != CF_MESH;
}

__device__ bool closed_form_contact(int cf, const DevWorld& w, int ga, const SE3& TA, int gb, const SE3& TB,
                                    double& depth, V3& nd, V3& ps) {
  const cptr<double> pa = w.geom_rec + G_STRIDE * ga + G_PARAM, pb = w.geom_rec + G_STRIDE * gb + G_PARAM;
  const double sa[3] = {pa[0], pa[1], pa[2]}, sb[3] = {pb[0], pb[1], pb[2]};
  switch (cf) {
    case CF_BOX_BOX: return box_box_contact(sa, TA, sb, TB, depth, nd, ps);
    case CF_SPHERE_SPHERE: return sphere_sphere_contact(sa[0], TA, sb[0], TB, depth, nd, ps);
    case CF_SPHERE_BOX: return sphere_box_contact(sa[0], TA, sb, TB, depth, nd, ps);
    case CF_SPHERE_CAPSULE: return sphere_capsule_contact(sa[0], TA, sb[0], sb[1], TB, depth, nd, ps);
    case CF_SPHERE_CYLINDER: return sphere_cylinder_contact(sa[0], TA, sb[0], sb[1], TB, depth, nd, ps);
    default: break;
  }
  // the shape-sphere orders: the sphere first, then flipNormal
  bool h;
  if (cf == CF_CAPSULE_SPHERE) h = sphere_capsule_contact(sb[0], TB, sa[0], sa[1], TA, depth, nd, ps);
  else if (cf == CF_CYLINDER_SPHERE) h = sphere_cylinder_contact(sb[0], TB, sa[0], sa[1], TA, depth, nd, ps);
  else h = sphere_box_contact(sb[0], TB, sa, TA, depth, nd, ps);  // CF_BOX_SPHERE
  nd = v3(-nd.x, -nd.y, -nd.z);
  return h;
}

// ---------------------------------------------------------------------------
// Contacts on BVH-mesh pairs (CollisionRequest(enable_contact=True)), one lane
// per reported (configuration, pair), the lane alone -- the same restatement
// as oracle/collide_oracle.c mesh_contact [ext FCL 0.7.0, parity unpinned]:
// the first hit in FCL's traversal order (the reachable hit whose descent key
// -- fcl_gate_shape's leaf position, fcl_gate_mesh's left / right choices,
// fcl_gate_octree_mesh's octree children and mesh choices -- is smallest),
// then
//   mesh-mesh    intersect_Triangle's contact branch (computeDeepestPoints
//                of each triangle against the other's plane), o1's frame ->
//                world;
//   shape-mesh   sphereTriangleIntersect's contact for spheres, libccd MPR
//                penetration of (shape, triangle GJK object) otherwise; the
//                mesh-first order negates the normal;
//   mesh-OcTree  MPR penetration of (leaf box, triangle) of the first hit in
//                OcTreeMeshIntersectRecurse's visit order.
// The AABB prefilters only skip separated triangles and the gates replay
// FCL's descent, so the first hit is the one the oracle's recursion finds.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void tri_plane(const double* v1, const double* v2, const double* v3, double* n, double& t) {
  double a[3], b[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = v2[k] - v1[k];
    b[k] = v3[k] - v1[k];
  }
  c3(n, a, b);
  const double z = d3(n, n);
  if (!(z > 0)) {
    n[0] = n[1] = n[2] = 0.0;
    t = 0.0;
    return;
  }
  const double r = std::sqrt(z);
#pragma unroll
  for (int k = 0; k < 3; ++k) n[k] /= r;
  t = d3(n, v1);
}

// Intersect::computeDeepestPoints: depth and the first deepest vertex
__device__ __forceinline__ int deepest_points(const double* T, const double* n, double t, double& pen, double* first) {
  double max_depth = -DBL_MAX;
  int num = 0, num_neg = 0, num_pos = 0, num_zero = 0;
  for (int i = 0; i < 3; ++i) {
    const double dist = -(d3(n, T + 3 * i) - t);
    if (dist > 1e-5) num_pos++;
    else if (dist < -1e-5) num_neg++;
    else num_zero++;
    if (dist > max_depth) {
      max_depth = dist;
      num = 1;
      first[0] = T[3 * i];
      first[1] = T[3 * i + 1];
      first[2] = T[3 * i + 2];
    } else if (dist + 1e-6 >= max_depth) {
      num++;
    }
  }
  if (max_depth < -1e-5) num = 0;
  if (num_zero == 0 && (num_neg == 0 || num_pos == 0)) num = 0;
  pen = max_depth;
  return num;
}

__device__ int tri_tri_contact(const double* P, const double* Q, double* point, double* normal, double& depth) {
  double n1[3], n2[3], t1, t2, d1[3] = {0, 0, 0}, d2[3] = {0, 0, 0}, pen1, pen2;
  tri_plane(P, P + 3, P + 6, n1, t1);
  tri_plane(Q, Q + 3, Q + 6, n2, t2);
  const int k2 = deepest_points(Q, n1, t1, pen2, d2);
  const int k1 = deepest_points(P, n2, t2, pen1, d1);
  if (pen1 > pen2) {
    for (int k = 0; k < 3; ++k) {
      point[k] = d2[k];
      normal[k] = -n1[k];
    }
    depth = pen2;
    return min(k2, 2);
  }
  for (int k = 0; k < 3; ++k) {
    point[k] = d1[k];
    normal[k] = n2[k];
  }
  depth = pen1;
  return min(k1, 2);
}

__device__ __forceinline__ double seg_sqr_dist_nearest(const double* from, const double* to, const double* p,
                                                       double* nearest) {
  double diff[3], v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    diff[k] = p[k] - from[k];
    v[k] = to[k] - from[k];
  }
  double t = d3(v, diff);
  if (t > 0) {
    const double vv = d3(v, v);
    if (t < vv) {
      t /= vv;
#pragma unroll
      for (int k = 0; k < 3; ++k) diff[k] -= v[k] * t;
    } else {
      t = 1;
#pragma unroll
      for (int k = 0; k < 3; ++k) diff[k] -= v[k];
    }
  } else {
    t = 0;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) nearest[k] = from[k] + v[k] * t;
  return d3(diff, diff);
}

// sphereTriangleIntersect with its contact (W = world triangle)
__device__ bool sphere_triangle_contact(double radius, const double* c, const double* W, double& depth, V3& nd,
                                        V3& ps) {
  double a[3], b[3], n[3], pc[3], cp[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = W[3 + k] - W[k];
    b[k] = W[6 + k] - W[k];
  }
  c3(n, a, b);
  const double z = d3(n, n);
  if (z > 0) {
    const double s = std::sqrt(z);
    n[0] /= s;
    n[1] /= s;
    n[2] /= s;
  }
  const double rt = radius + DBL_EPSILON;
#pragma unroll
  for (int k = 0; k < 3; ++k) pc[k] = c[k] - W[k];
  double dist = d3(pc, n);
  if (dist < 0) {
    dist *= -1;
    n[0] *= -1;
    n[1] *= -1;
    n[2] *= -1;
  }
  bool has = false;
  if (dist < rt) {
    double e1[3], e2[3], e3[3], u[3], v[3], x[3], en[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      e1[k] = W[3 + k] - W[k];
      e2[k] = W[6 + k] - W[3 + k];
      e3[k] = W[k] - W[6 + k];
      u[k] = c[k] - W[k];
      v[k] = c[k] - W[3 + k];
      x[k] = c[k] - W[6 + k];
    }
    c3(en, e1, n);
    const double r1 = d3(en, u);
    c3(en, e2, n);
    const double r2 = d3(en, v);
    c3(en, e3, n);
    const double r3 = d3(en, x);
    if ((r1 > 0 && r2 > 0 && r3 > 0) || (r1 <= 0 && r2 <= 0 && r3 <= 0)) {
      has = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) cp[k] = c[k] - n[k] * dist;
    } else {
      const double rr = rt * rt;
      double ne[3];
      if (seg_sqr_dist_nearest(W, W + 3, c, ne) < rr) {
        has = true;
        cp[0] = ne[0]; cp[1] = ne[1]; cp[2] = ne[2];
      }
      if (seg_sqr_dist_nearest(W + 3, W + 6, c, ne) < rr) {
        has = true;
        cp[0] = ne[0]; cp[1] = ne[1]; cp[2] = ne[2];
      }
      if (seg_sqr_dist_nearest(W + 6, W, c, ne) < rr) {
        has = true;
        cp[0] = ne[0]; cp[1] = ne[1]; cp[2] = ne[2];
      }
    }
  }
  if (!has) return false;
  const double cc[3] = {cp[0] - c[0], cp[1] - c[1], cp[2] - c[2]};
  const double d2 = d3(cc, cc);
  if (!(d2 < rt * rt)) return false;
  if (d2 > 0) {
    const double d = std::sqrt(d2);
    nd = v3(cc[0] / d, cc[1] / d, cc[2] / d);
    depth = -(radius - d);
  } else {
    nd = v3(-n[0], -n[1], -n[2]);
    depth = -radius;
  }
  ps = v3(cp[0], cp[1], cp[2]);
  return true;
}

// triangle GJK object support (supportTriangle) in world coordinates
__device__ __forceinline__ CV3 tri_support(const GObj& b, const CV3* P, const CV3& tc, const CV3& dir) {
  const CV3 db = quat_rot(dir, b.rot_inv);
  ccd_real maxdot = -FLT_MAX;
  CV3 lb = P[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const ccd_real dot = vdot(db, vsub(P[i], tc));
    if (dot > maxdot) {
      lb = P[i];
      maxdot = dot;
    }
  }
  return vadd(quat_rot(lb, b.rot), b.pos);
}

// MPR penetration of (object a, triangle of record rec in b's frame); a is a
// shape (h == nullptr) or a box with half sizes h
__device__ bool tri_mpr_penetration(const DevWorld& w, cptr<double> HV, const GObj& a, const ccd_real* h,
                                    const GObj& b, cptr<double> rec, double& depth, V3& nd, V3& ps) {
  double P[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) P[k] = rec[TR_P + k];
  const CV3 tc = cv3((P[0] + P[3] + P[6]) / 3, (P[1] + P[4] + P[7]) / 3, (P[2] + P[5] + P[8]) / 3);
  const CV3 TP[3] = {cv3(P[0], P[1], P[2]), cv3(P[3], P[4], P[5]), cv3(P[6], P[7], P[8])};
  ccd_real dc = 0;
  CV3 n{0, 0, 0}, pc{0, 0, 0};
  const CV3 ca = h ? a.pos : center(w, a);
  const bool hit = mpr_penetration_core(
      w.mpr_tol, ca, vadd(quat_rot(tc, b.rot), b.pos),
      [&](const CV3& d) {
        SupP sp;
        if (h) {
          const CV3 da = quat_rot(d, a.rot_inv);
          const CV3 la = CV3{(da.x >= 0 ? ccd_real(1) : ccd_real(-1)) * h[0], (da.y >= 0 ? ccd_real(1) : ccd_real(-1)) * h[1],
                             (da.z >= 0 ? ccd_real(1) : ccd_real(-1)) * h[2]};
          sp.v1 = vadd(quat_rot(la, a.rot), a.pos);
        } else {
          sp.v1 = support(w, HV, a, d);
        }
        sp.v2 = tri_support(b, TP, tc, vscale(d, ccd_real(-1)));
        sp.v = vsub(sp.v1, sp.v2);
        return sp;
      },
      dc, n, pc);
  if (hit) {
    depth = dc;
    nd = to_v3(n);
    ps = to_v3(pc);
  }
  return hit;
}

__device__ __forceinline__ GObj posed_obj(const SE3& T, int g, int type) {
  GObj o;
  o.rot = gjk_rot_from_matrix(T.R);
  o.rot_inv = quat_invert2(o.rot);
  o.pos = cv3(T.p[0], T.p[1], T.p[2]);
  o.geom = g;
  o.type = type;
  return o;
}

__device__ bool mesh_shape_first_contact(const DevWorld& w, cptr<double> HV, int gm, const SE3& TM, int gs,
                                         const SE3& TS, bool mesh_first, double& depth, V3& nd, V3& ps) {
  const cptr<double> grm = w.geom_rec + G_STRIDE * gm, grs = w.geom_rec + G_STRIDE * gs;
  const int ts = w.geom_type[gs];
  const int t0 = (int)grm[G_PARAM], t1 = t0 + (int)grm[G_PARAM + 1];
  double sc[3], cl[3], Rl[9], hq[3];  // the shape's box in the mesh frame, as mesh_shape_wave
  for (int i = 0; i < 3; ++i)
    sc[i] = ((TS.R[3 * i] * grs[G_OBB_C] + TS.R[3 * i + 1] * grs[G_OBB_C + 1]) + TS.R[3 * i + 2] * grs[G_OBB_C + 2]) + TS.p[i];
  const double dsc[3] = {sc[0] - TM.p[0], sc[1] - TM.p[1], sc[2] - TM.p[2]};
  for (int i = 0; i < 3; ++i) {
    cl[i] = (TM.R[i] * dsc[0] + TM.R[3 + i] * dsc[1]) + TM.R[6 + i] * dsc[2];
    for (int j = 0; j < 3; ++j) Rl[3 * i + j] = (TM.R[i] * TS.R[j] + TM.R[3 + i] * TS.R[3 + j]) + TM.R[6 + i] * TS.R[6 + j];
  }
  for (int i = 0; i < 3; ++i)
    hq[i] = ((std::fabs(Rl[3 * i]) * grs[G_OBB_E] + std::fabs(Rl[3 * i + 1]) * grs[G_OBB_E + 1]) +
             std::fabs(Rl[3 * i + 2]) * grs[G_OBB_E + 2]) * (1.0 + 1e-9) +
            kMeshShapePad * (1.0 + std::fabs(TS.p[0]) + std::fabs(TS.p[1]) + std::fabs(TS.p[2]) + std::fabs(TM.p[0]) +
                             std::fabs(TM.p[1]) + std::fabs(TM.p[2]));
  const GObj A = posed_obj(TS, gs, ts), B = posed_obj(TM, gm, MPG_GEOM_MESH);
  double sA[9], sT[3], sE[3];
  fcl_shape_obb_world(w, gs, ts, TS, sA, sT, sE);
  // FCL's traversal visits the leaves left to right: the first hit is the
  // reachable (gated) hit of smallest leaf position
  int best = INT_MAX;
  double bd = 0.0;
  V3 bn{0, 0, 0}, bp{0, 0, 0};
  for (int t = t0; t < t1; ++t) {
    const cptr<double> rec = w.mesh_tri + TR_STRIDE * (size_t)t;
    const int id = w.tri_pos[t0 + (int)rec[TR_ID]];  // leaf position
    if (id >= best) continue;
    bool out = false;
    for (int i = 0; i < 3; ++i) out |= rec[TR_LO + i] > cl[i] + hq[i] || rec[TR_HI + i] < cl[i] - hq[i];
    if (out) continue;
    double dp = 0.0;
    V3 n{0, 0, 0}, p{0, 0, 0};
    bool hit;
    if (ts == MPG_GEOM_SPHERE) {
      double W[9];
      for (int v = 0; v < 3; ++v)
        for (int i = 0; i < 3; ++i)
          W[3 * v + i] = ((TM.R[3 * i] * rec[3 * v] + TM.R[3 * i + 1] * rec[3 * v + 1]) + TM.R[3 * i + 2] * rec[3 * v + 2]) +
                         TM.p[i];
      hit = sphere_triangle_contact(grs[G_PARAM], TS.p, W, dp, n, p);
    } else {
      hit = tri_mpr_penetration(w, HV, A, nullptr, B, rec, dp, n, p);
    }
    if (hit && fcl_gate_shape(w, gm, TM, sA, sT, sE, (int)rec[TR_ID])) {
      best = id;
      bd = dp;
      bn = n;
      bp = p;
    }
  }
  depth = bd;
  nd = mesh_first ? v3(-bn.x, -bn.y, -bn.z) : bn;
  ps = bp;
  return best != INT_MAX;
}

__device__ bool mesh_mesh_first_contact(const DevWorld& w, int ga, const SE3& TA, int gb, const SE3& TB, double& depth,
                                        V3& nd, V3& ps) {
  const cptr<double> gra = w.geom_rec + G_STRIDE * ga, grb = w.geom_rec + G_STRIDE * gb;
  const int b0 = (int)grb[G_PARAM], b1 = b0 + (int)grb[G_PARAM + 1];
  const int c0 = w.mesh_tree[2 * ga], c1 = c0 + w.mesh_tree[2 * ga + 1];
  double R[9], T[3], alo[3], ahi[3];
  const double dt[3] = {TB.p[0] - TA.p[0], TB.p[1] - TA.p[1], TB.p[2] - TA.p[2]};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (TA.R[i] * TB.R[j] + TA.R[3 + i] * TB.R[3 + j]) + TA.R[6 + i] * TB.R[6 + j];
    T[i] = (TA.R[i] * dt[0] + TA.R[3 + i] * dt[1]) + TA.R[6 + i] * dt[2];
    alo[i] = gra[G_OBB_C + i] - gra[G_OBB_E + i];
    ahi[i] = gra[G_OBB_C + i] + gra[G_OBB_E + i];
  }
  // the first hit in FCL's visit order: the reachable intersecting pair whose
  // descent (fcl_gate_mesh's left / right choices) is lexicographically smallest
  uint64_t best[2] = {~0ull, ~0ull};
  int best_a = -1, best_b = -1;
  for (int j = b0; j < b1; ++j) {
    const cptr<double> rq = w.mesh_tri + TR_STRIDE * (size_t)j;
    const long long idb = (long long)rq[TR_ID];
    double Q[9], qlo[3], qhi[3];
    for (int v = 0; v < 3; ++v)
      for (int i = 0; i < 3; ++i)
        Q[3 * v + i] = ((R[3 * i] * rq[3 * v] + R[3 * i + 1] * rq[3 * v + 1]) + R[3 * i + 2] * rq[3 * v + 2]) + T[i];
    bool keep = true;
    for (int i = 0; i < 3; ++i) {
      qlo[i] = fmin(Q[i], fmin(Q[3 + i], Q[6 + i])) - kMeshPad;
      qhi[i] = fmax(Q[i], fmax(Q[3 + i], Q[6 + i])) + kMeshPad;
      keep &= !(qlo[i] > ahi[i] || qhi[i] < alo[i]);
    }
    if (!keep) continue;
    for (int c = c0; c < c1; ++c) {
      const cptr<double> bx = w.mesh_node + 6 * (size_t)c;
      bool ov = true;
      for (int i = 0; i < 3; ++i) ov &= !(bx[i] > qhi[i] || bx[3 + i] < qlo[i]);
      if (!ov) continue;
      const int t1 = w.mesh_link[2 * c] + w.mesh_link[2 * c + 1];
      for (int t = w.mesh_link[2 * c]; t < t1; ++t) {
        const cptr<double> rp = w.mesh_tri + TR_STRIDE * (size_t)t;
        bool o2 = false;
        for (int i = 0; i < 3; ++i) o2 |= rp[TR_LO + i] > qhi[i] || rp[TR_HI + i] < qlo[i];
        if (o2) continue;
        double P[9];
        for (int q = 0; q < 9; ++q) P[q] = rp[TR_P + q];
        if (!tri_tri_intersect(P, Q)) continue;
        uint64_t key[2] = {0ull, 0ull};
        if (!fcl_gate_mesh(w, ga, gb, R, T, (int)rp[TR_ID], (int)idb, key)) continue;
        if (key[0] < best[0] || (key[0] == best[0] && key[1] < best[1])) {
          best[0] = key[0];
          best[1] = key[1];
          best_a = t;
          best_b = j;
        }
      }
    }
  }
  depth = 0.0;
  nd = v3(0, 0, 0);
  ps = v3(0, 0, 0);
  if (best_a < 0) return false;
  double P[9], Q[9], pt[3], nl[3], pen;
  const cptr<double> rp = w.mesh_tri + TR_STRIDE * (size_t)best_a, rq = w.mesh_tri + TR_STRIDE * (size_t)best_b;
  for (int q = 0; q < 9; ++q) P[q] = rp[TR_P + q];
  for (int v = 0; v < 3; ++v)
    for (int i = 0; i < 3; ++i)
      Q[3 * v + i] = ((R[3 * i] * rq[3 * v] + R[3 * i + 1] * rq[3 * v + 1]) + R[3 * i + 2] * rq[3 * v + 2]) + T[i];
  if (tri_tri_contact(P, Q, pt, nl, pen) > 0) {
    double wp[3], wn[3];
    for (int i = 0; i < 3; ++i) {
      wp[i] = ((TA.R[3 * i] * pt[0] + TA.R[3 * i + 1] * pt[1]) + TA.R[3 * i + 2] * pt[2]) + TA.p[i];
      wn[i] = (TA.R[3 * i] * nl[0] + TA.R[3 * i + 1] * nl[1]) + TA.R[3 * i + 2] * nl[2];
    }
    depth = pen;
    nd = v3(wn[0], wn[1], wn[2]);
    ps = v3(wp[0], wp[1], wp[2]);
  }
  return true;
}

__device__ bool mesh_octree_first_contact(const DevWorld& w, int gm, const SE3& TM, int go, const SE3& TO,
                                          double& depth, V3& nd, V3& ps) {
  const cptr<double> grm = w.geom_rec + G_STRIDE * gm;
  const double pad = kMeshShapePad * (1.0 + std::fabs(TO.p[0]) + std::fabs(TO.p[1]) + std::fabs(TO.p[2]) +
                                      std::fabs(TM.p[0]) + std::fabs(TM.p[1]) + std::fabs(TM.p[2]));
  double Rm[9], Ro[9], mcw[3], blo[3], bhi[3];  // as mesh_octree_wave
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      Rm[3 * i + j] = (TO.R[i] * TM.R[j] + TO.R[3 + i] * TM.R[3 + j]) + TO.R[6 + i] * TM.R[6 + j];
      Ro[3 * j + i] = Rm[3 * i + j];
    }
  for (int i = 0; i < 3; ++i)
    mcw[i] = ((TM.R[3 * i] * grm[G_OBB_C] + TM.R[3 * i + 1] * grm[G_OBB_C + 1]) + TM.R[3 * i + 2] * grm[G_OBB_C + 2]) +
             TM.p[i];
  const double dmo[3] = {mcw[0] - TO.p[0], mcw[1] - TO.p[1], mcw[2] - TO.p[2]};
  for (int i = 0; i < 3; ++i) {
    const double c = (TO.R[i] * dmo[0] + TO.R[3 + i] * dmo[1]) + TO.R[6 + i] * dmo[2];
    const double e = ((std::fabs(Rm[3 * i]) * grm[G_OBB_E] + std::fabs(Rm[3 * i + 1]) * grm[G_OBB_E + 1]) +
                      std::fabs(Rm[3 * i + 2]) * grm[G_OBB_E + 2]) * (1.0 + 1e-9) + 1e-9 + pad;
    blo[i] = c - e;
    bhi[i] = c + e;
  }
  GObj A = posed_obj(TO, go, MPG_GEOM_BOX);
  const GObj B = posed_obj(TM, gm, MPG_GEOM_MESH);
  const int c0 = w.mesh_tree[2 * gm], c1 = c0 + w.mesh_tree[2 * gm + 1];
  const cptr<double> gor = w.geom_rec + G_STRIDE * go;
  const int l0 = (int)gor[G_PARAM], ln = (int)gor[G_PARAM + 1];
  // the first hit in OcTreeMeshIntersectRecurse's visit order: the reachable
  // (leaf, triangle) hit whose descent key (fcl_gate_octree_mesh) is smallest
  uint64_t best[kOctKeyWords];
  for (int k = 0; k < kOctKeyWords; ++k) best[k] = ~0ull;
  bool found = false;
  double bd = 0.0;
  V3 bn{0, 0, 0}, bp{0, 0, 0};
  for (int l = l0; l < l0 + ln; ++l) {
    const cptr<double> L = w.oct_leaf + 6 * (size_t)l;
    bool out = false;
    for (int i = 0; i < 3; ++i) out |= L[i] > bhi[i] || L[3 + i] < blo[i];
    if (out) continue;
    double c[3], side[3], cw[3], cm[3], hm[3];
    for (int i = 0; i < 3; ++i) {
      c[i] = (L[i] + L[3 + i]) * 0.5;
      side[i] = L[3 + i] - L[i];
    }
    for (int i = 0; i < 3; ++i) cw[i] = ((TO.R[3 * i] * c[0] + TO.R[3 * i + 1] * c[1]) + TO.R[3 * i + 2] * c[2]) + TO.p[i];
    const double dm[3] = {cw[0] - TM.p[0], cw[1] - TM.p[1], cw[2] - TM.p[2]};
    for (int i = 0; i < 3; ++i) {
      cm[i] = (TM.R[i] * dm[0] + TM.R[3 + i] * dm[1]) + TM.R[6 + i] * dm[2];
      hm[i] = ((std::fabs(Ro[3 * i]) * side[0] + std::fabs(Ro[3 * i + 1]) * side[1]) + std::fabs(Ro[3 * i + 2]) * side[2]) *
                  0.5 * (1.0 + 1e-9) + 1e-9 + pad;
    }
    A.pos = cv3(cw[0], cw[1], cw[2]);
    const ccd_real h[3] = {(ccd_real)(side[0] / 2.0), (ccd_real)(side[1] / 2.0), (ccd_real)(side[2] / 2.0)};
    for (int cl = c0; cl < c1; ++cl) {
      const cptr<double> bx = w.mesh_node + 6 * (size_t)cl;
      bool away = false;
      for (int i = 0; i < 3; ++i) away |= bx[i] > cm[i] + hm[i] || bx[3 + i] < cm[i] - hm[i];
      if (away) continue;
      const int t1 = w.mesh_link[2 * cl] + w.mesh_link[2 * cl + 1];
      for (int t = w.mesh_link[2 * cl]; t < t1; ++t) {
        const cptr<double> rec = w.mesh_tri + TR_STRIDE * (size_t)t;
        const int id = (int)rec[TR_ID];
        bool o2 = false;
        for (int i = 0; i < 3; ++i) o2 |= rec[TR_LO + i] > cm[i] + hm[i] || rec[TR_HI + i] < cm[i] - hm[i];
        if (o2) continue;
        double dp = 0.0;
        V3 n{0, 0, 0}, p{0, 0, 0};
        if (!tri_mpr_penetration(w, w.hull, A, h, B, rec, dp, n, p)) continue;
        uint64_t key[kOctKeyWords] = {0ull, 0ull, 0ull, 0ull, 0ull};
        if (!fcl_gate_octree_mesh(w, go, TO, gm, TM, l, id, key)) continue;
        bool less = false;
        for (int k = 0; k < kOctKeyWords; ++k)
          if (key[k] != best[k]) {
            less = key[k] < best[k];
            break;
          }
        if (!found || less) {
          for (int k = 0; k < kOctKeyWords; ++k) best[k] = key[k];
          found = true;
          bd = dp;
          bn = n;
          bp = p;
        }
      }
    }
  }
  depth = found ? bd : 0.0;
  nd = found ? bn : v3(0, 0, 0);
  ps = found ? bp : v3(0, 0, 0);
  return found;
}

__device__ bool mesh_first_contact(const DevWorld& w, cptr<double> HV, int ga, const SE3& TA, int gb, const SE3& TB,
                                   double& depth, V3& nd, V3& ps) {
  const int ta = w.geom_type[ga], tb = w.geom_type[gb];
  if (ta == MPG_GEOM_MESH && tb == MPG_GEOM_MESH) return mesh_mesh_first_contact(w, ga, TA, gb, TB, depth, nd, ps);
  if (tb == MPG_GEOM_OCTREE) return mesh_octree_first_contact(w, ga, TA, gb, TB, depth, nd, ps);
  if (ta == MPG_GEOM_OCTREE) return mesh_octree_first_contact(w, gb, TB, ga, TA, depth, nd, ps);
  if (ta == MPG_GEOM_MESH) return mesh_shape_first_contact(w, HV, ga, TA, gb, TB, true, depth, nd, ps);
  return mesh_shape_first_contact(w, HV, gb, TB, ga, TA, false, depth, nd, ps);
}

template <bool FROM_POSES>
__global__ __launch_bounds__(256) void contact_kernel(DevWorld w, const double* __restrict__ in,
                                                     const uint32_t* __restrict__ seg_len,
                                                     const uint32_t* __restrict__ seg_start,
                                                     const uint32_t* __restrict__ prefix,
                                                     const uint32_t* __restrict__ cand,
                                                     const uint32_t* __restrict__ masks, const double* __restrict__ sc,
                                                     double* __restrict__ depth, double* __restrict__ normal,
                                                     double* __restrict__ pos) {
  const cptr<double> HV = w.hull;
  const uint32_t lane = lane_id();
  const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
  const uint32_t total = prefix[w.n_pairs];
  const TaskPlan plan = bk_plan_load(prefix + w.n_pairs + 4);
  for (uint32_t tk = wave; tk < total; tk += n_waves) {
    int lo = 0, hi = w.n_pairs;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (prefix[mid] <= tk) lo = mid;
      else hi = mid;
    }
    const int p = lo;
    uint32_t t0, t1;
    bk_task_range(seg_start[p], seg_len[p], tk - prefix[p], plan, &t0, &t1);
    const int a = w.pair_a[p], b = w.pair_b[p];
    for (uint32_t base = t0; base < t1; base += 64) {
      const uint32_t idx = base + lane;
      if (idx >= t1) continue;
      const long long c = cand[seg_start[p] + idx];
      if (!((masks[c * w.W + (p >> 5)] >> (p & 31)) & 1u)) continue;
      double dp = 0.0;
      V3 nd{0, 0, 0}, ps{0, 0, 0};
      if (w.pair_cf[p] == CF_OCTREE) {  // the octree is side b (octree-first pairs are refused on the host)
        const SE3 TA = a < w.n_moving ? moving_tf<FROM_POSES>(w, in, sc, c, a) : load_se3(w.static_T + 12 * (a - w.n_moving));
        const SE3 TB = b < w.n_moving ? moving_tf<FROM_POSES>(w, in, sc, c, b) : load_se3(w.static_T + 12 * (b - w.n_moving));
        const int ga = a < w.n_moving ? w.moving_geom[a] : w.static_geom[a - w.n_moving];
        const int gb = b < w.n_moving ? w.moving_geom[b] : w.static_geom[b - w.n_moving];
        octree_first_contact(w, HV, gb, TB, ga, TA, dp, nd, ps);
      } else if (w.pair_cf[p] == CF_MESH) {
        const SE3 TA = a < w.n_moving ? moving_tf<FROM_POSES>(w, in, sc, c, a) : load_se3(w.static_T + 12 * (a - w.n_moving));
        const SE3 TB = b < w.n_moving ? moving_tf<FROM_POSES>(w, in, sc, c, b) : load_se3(w.static_T + 12 * (b - w.n_moving));
        const int ga = a < w.n_moving ? w.moving_geom[a] : w.static_geom[a - w.n_moving];
        const int gb = b < w.n_moving ? w.moving_geom[b] : w.static_geom[b - w.n_moving];
        mesh_first_contact(w, HV, ga, TA, gb, TB, dp, nd, ps);
      } else if (cf_has_contact(w.pair_cf[p])) {
        const SE3 TA = a < w.n_moving ? moving_tf<FROM_POSES>(w, in, sc, c, a) : load_se3(w.static_T + 12 * (a - w.n_moving));
        const SE3 TB = b < w.n_moving ? moving_tf<FROM_POSES>(w, in, sc, c, b) : load_se3(w.static_T + 12 * (b - w.n_moving));
        const int ga = a < w.n_moving ? w.moving_geom[a] : w.static_geom[a - w.n_moving];
        const int gb = b < w.n_moving ? w.moving_geom[b] : w.static_geom[b - w.n_moving];
        closed_form_contact(w.pair_cf[p], w, ga, TA, gb, TB, dp, nd, ps);
      } else {
        const GObj A = a < w.n_moving ? moving_obj<FROM_POSES>(w, in, sc, c, a) : static_obj(w, a - w.n_moving);
        const GObj B = b < w.n_moving ? moving_obj<FROM_POSES>(w, in, sc, c, b) : static_obj(w, b - w.n_moving);
        mpr_penetration(w, HV, A, B, dp, nd, ps);
      }
      const size_t k = (size_t)c * w.n_pairs + p;
      depth[k] = dp;
      normal[3 * k] = nd.x;
      normal[3 * k + 1] = nd.y;
      normal[3 * k + 2] = nd.z;
      pos[3 * k] = ps.x;
      pos[3 * k + 1] = ps.y;
      pos[3 * k + 2] = ps.z;
    }
  }
}

__global__ void fk_kernel(DevWorld w, const double* __restrict__ q, long long n, double* __restrict__ out) {
  const long long cfg = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (cfg >= n) return;
  FkState st;
  forward_kinematics(w, q + cfg * w.dof, st);
  for (int l = 0; l < w.n_links; ++l) link_transform(w, st, l, out + (cfg * w.n_links + l) * 7);
}

// Worlds with free frames: the link-pose rows their pairs are evaluated from.
// The kinematic links by FK as fk_kernel writes them, the free frames copied
// from free_pose (row cfg * free_stride doubles in; stride 0: one pose set
// shared by the batch) or, when free_pose is NULL, from the world's current
// poses.  A movable object's transform is then the frame's isometry whatever
// the source of the pose.  MAPPED: row cfg takes pose set row_of[cfg] instead
// of cfg (motion validation: the sub-states of an edge share the edge's set;
// row_of is already offset to this pass's first row, free_pose is not).
// One set for every row is read through uniform addresses by each lane; one
// set per row is copied by the block with its lanes along a set's doubles, so
// that loads and stores cover whole 56 * n_free byte runs (a lane per row
// would touch 64 lines per load).
template <bool MAPPED>
__global__ void fk_free_kernel(DevWorld w, const double* __restrict__ q, long long n, double* __restrict__ out,
                               const double* __restrict__ free_pose, long long free_stride,
                               const int32_t* __restrict__ row_of) {
  const long long base = (long long)blockIdx.x * blockDim.x;
  const long long cfg = base + threadIdx.x;
  const int nk = w.n_links - w.n_free;
  const int fr = w.n_free * 7;
  if (cfg < n) {
    FkState st;
    forward_kinematics(w, q + cfg * w.dof, st);
    for (int l = 0; l < nk; ++l) link_transform(w, st, l, out + (cfg * w.n_links + l) * 7);
    if (!free_pose || free_stride == 0) {
      const double* src = free_pose ? free_pose : w.free_cur;
      double* dst = out + (cfg * w.n_links + nk) * 7;
      for (int k = 0; k < fr; ++k) dst[k] = src[k];
    }
  }
  if (!free_pose || free_stride == 0) return;
  const long long left = n - base;  // > 0: the grid covers n rows
  const int tot = (int)(left < (long long)blockDim.x ? left : (long long)blockDim.x) * fr;
  for (int i = threadIdx.x; i < tot; i += blockDim.x) {
    const int r = i / fr, k = i - r * fr;
    const long long row = MAPPED ? (long long)row_of[base + r] : base + r;
    out[((base + r) * w.n_links + nk) * 7 + k] = free_pose[row * free_stride + k];
  }
}

// ---------------------------------------------------------------------------
// Batched motion validation (OMPL DiscreteMotionValidator over the MPlib
// compound state space, src/ompl_planner.cpp:248-293): per edge the segment
// count, the interpolated states, then the per-edge reduction of their flags.
// ---------------------------------------------------------------------------
// ompl::base::SO2StateSpace::distance / RealVectorStateSpace(1)::distance,
// summed with weight 1.0 by CompoundStateSpace::distance
__device__ __forceinline__ double motion_distance(const double* a, const double* b, int dof, uint32_t so2) {
  double d = 0.0;
  for (int i = 0; i < dof; ++i) {
    double di;
    if ((so2 >> i) & 1u) {
      di = std::fabs(a[i] - b[i]);
      di = (di > M_PI) ? 2.0 * M_PI - di : di;
    } else {
      const double diff = a[i] - b[i];
      di = std::sqrt(diff * diff);
    }
    d += 1.0 * di;
  }
  return d;
}

__global__ void motion_count_kernel(const double* __restrict__ from, const double* __restrict__ to, long long n,
                                    int dof, uint32_t so2, double lvs, int32_t* __restrict__ segs) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  // StateSpace::validSegmentCount: factor 1 * (unsigned)ceil(distance / longestValidSegment)
  const unsigned nd = (unsigned)std::ceil(motion_distance(from + e * dof, to + e * dof, dof, so2) / lvs);
  segs[e] = (int32_t)(nd > 1u ? nd : 1u);  // states j/nd, j = 1..nd (s1 is assumed valid)
}

__global__ void motion_states_kernel(const double* __restrict__ from, const double* __restrict__ to, long long n,
                                     int dof, uint32_t so2, const int32_t* __restrict__ segs,
                                     const long long* __restrict__ offs, double* __restrict__ states) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const double* a = from + e * dof;
  const double* b = to + e * dof;
  const int m = segs[e];
  double* out = states + offs[e] * dof;
  for (int j = 1; j <= m; ++j, out += dof) {
    if (j == m) {  // checkMotion tests s2 itself
      for (int i = 0; i < dof; ++i) out[i] = b[i];
      continue;
    }
    const double t = (double)j / (double)m;
    for (int i = 0; i < dof; ++i) {
      if ((so2 >> i) & 1u) {  // SO2StateSpace::interpolate
        double diff = b[i] - a[i];
        double v;
        if (std::fabs(diff) <= M_PI) {
          v = a[i] + diff * t;
        } else {
          diff = diff > 0.0 ? 2.0 * M_PI - diff : -2.0 * M_PI - diff;
          v = a[i] - diff * t;
          if (v > M_PI) v -= 2.0 * M_PI;
          else if (v < -M_PI) v += 2.0 * M_PI;
        }
        out[i] = v;
      } else {  // RealVectorStateSpace::interpolate
        out[i] = a[i] + (b[i] - a[i]) * t;
      }
    }
  }
}

// Per-edge free poses: row_of[i] = the edge that owns sub-state i, the last e
// with offs[e] <= i (offs is the exclusive prefix of segs >= 1, so strictly
// increasing with offs[0] = 0).  One thread per sub-state: neighbouring lanes
// search neighbouring keys (the same few offs lines) and store neighbouring
// words.
__global__ void motion_rowmap_kernel(const long long* __restrict__ offs, long long n_edges, long long total,
                                     int32_t* __restrict__ row_of) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  long long lo = 0, hi = n_edges - 1;  // invariant: offs[lo] <= i, and hi == n_edges - 1 or offs[hi + 1] > i
  while (lo < hi) {
    const long long mid = lo + (hi - lo + 1) / 2;
    if (offs[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  row_of[i] = (int32_t)lo;
}

__global__ void motion_reduce_kernel(const uint8_t* __restrict__ flags, long long n, const int32_t* __restrict__ segs,
                                     const long long* __restrict__ offs, uint8_t* __restrict__ valid,
                                     int32_t* __restrict__ first_invalid) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const uint8_t* f = flags + offs[e];
  int bad = -1;
  for (int j = 0; j < segs[e]; ++j)
    if (f[j]) {
      bad = j + 1;
      break;
    }
  valid[e] = bad < 0 ? 1 : 0;
  if (first_invalid) first_invalid[e] = bad;
}

__global__ void sincos_kernel(const double* __restrict__ x, long long n, double* s, double* c) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  mpg_sincos(x[i], s + i, c + i);
}

// ---------------------------------------------------------------------------
// generate_collision_pair (mplib/planner.py:118-163), batched: random full
// configurations drawn on the device, the pairs collide_full() reports
// counted per pair.
// Sampler: value i (row-major, rows counted from the call's first sample) is
// lo + (hi - lo) * u, u = (splitmix64(seed + (i + 1) * golden) >> 11) * 2^-53
// (mplib_amd/planner.py sample_uniform restates it on the host).
// ---------------------------------------------------------------------------
constexpr int kSampleMaxDof = 64;
struct SampleRange {
  double lo[kSampleMaxDof], hi[kSampleMaxDof];
};

__device__ __forceinline__ double splitmix_u01(uint64_t seed, uint64_t i) {
  uint64_t z = seed + (i + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

__global__ __launch_bounds__(256) void sample_uniform_kernel(SampleRange r, int dof, long long n, uint64_t seed,
                                                            long long row0, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * dof) return;
  const int k = (int)(i % dof);
  const double u = splitmix_u01(seed, (uint64_t)(row0 * dof + i));
  out[i] = r.lo[k] + (r.hi[k] - r.lo[k]) * u;
}

// ---------------------------------------------------------------------------
// Planner.IK's loop (mplib/planner.py:256-350), batched: mpg_ik_batch.  The
// per-row arithmetic is mpg_ik.h's.
// ---------------------------------------------------------------------------
// the seeds of a call without q_init: seed 0 of each goal and every masked
// slot from q_start, the rest row g * rows_per_goal + r of the sampler above
__global__ __launch_bounds__(256) void ik_seed_kernel(IkView iv, int dof, long long n_rows, long long rows_per_goal,
                                                     uint64_t seed, const double* __restrict__ q_start,
                                                     double* __restrict__ q) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows * dof) return;
  const int d = (int)(i % dof);
  const long long r = (i / dof) % rows_per_goal;
  if (r == 0 || iv.frozen[d]) q[i] = q_start[d];
  else q[i] = iv.lo[d] + (iv.hi[d] - iv.lo[d]) * splitmix_u01(seed, (uint64_t)i);
}

// One lane per row, one wave per block, the whole iteration in one launch.
// Rows need some 60 to 1000 iterations, so a lane that has finished its row
// writes it and claims the next unclaimed one from *counter (zeroed on the
// stream before the launch): one atomic per wave and pass for all its claiming
// lanes (ballot + popcount).  A row's arithmetic is its lane's alone, so its
// result does not depend on the lane that ran it.  Each pass of the loop gives
// every lane that holds a row one iteration or its last check, so n_rows *
// (max_iter + 2) passes bound the loop for any input.
// A lane asks for a row only when kIkRefill lanes of its wave are idle (or all
// are): every pass with a claim pays an atomic, the row's loads and the
// previous row's stores, and with lanes finishing at different passes that
// was nearly every pass.
// LDS: the lanes' IkLane state, [chain joint][component][lane], then the
// chain's joint constants (IkJointsTable), filled once per wave.
constexpr int kIkRefill = 16;
__global__ __launch_bounds__(64) void ik_clik_kernel(DevWorld w, IkView iv, const double* __restrict__ goal,
                                                    long long n_rows, long long rows_per_goal, const double* q_in,
                                                    double* q_out, uint8_t* __restrict__ status,
                                                    double* __restrict__ err_out, int32_t* __restrict__ iters_out,
                                                    unsigned long long* __restrict__ counter) {
  extern __shared__ double ik_lds[];
  const int lane = threadIdx.x;
  const IkLane L{ik_lds + lane, 64};
  double* const td = ik_lds + (size_t)iv.cl * kIkSlot * 64;
  int* const ti = reinterpret_cast<int*>(td + (size_t)iv.cl * IKT_DOUBLES);
  for (int k = lane; k < iv.cl; k += 64) {
    const int j0 = w.chain_joints[iv.cs + k] - 1;
    ti[IKT_INTS * k + IKT_TYPE] = w.joint_type[j0];
    ti[IKT_INTS * k + IKT_SRC] = w.joint_q_source[j0];
    ti[IKT_INTS * k + IKT_MOVE] = iv.move[k];
    td[IKT_DOUBLES * k + IKT_QCONST] = w.joint_q_const[j0];
    for (int c = 0; c < 3; ++c) td[IKT_DOUBLES * k + IKT_AXIS + c] = w.joint_axis[3 * j0 + c];
    for (int c = 0; c < 12; ++c) td[IKT_DOUBLES * k + IKT_PLACE + c] = w.joint_place[12 * j0 + c];
  }
  __syncthreads();
  const IkJointsTable jt{td, ti};
  const int dof = w.dof;
  long long row = -1;
  int it = 0;
  bool rows_left = true;
  SE3 Ginv;
  se3_identity(Ginv);
  const long long bound = n_rows * ((long long)iv.max_iter + 2) + 2;
  for (long long pass = 0; pass < bound; ++pass) {
    const bool want = row < 0 && rows_left;
    const unsigned long long wants = __ballot(want);
    if (wants && (__popcll(wants) >= kIkRefill || !__ballot(row >= 0))) {
      const int leader = __ffsll((long long)wants) - 1;
      unsigned long long base = 0;
      if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(wants));
      const unsigned lo32 = __shfl((unsigned)base, leader), hi32 = __shfl((unsigned)(base >> 32), leader);
      base = ((unsigned long long)hi32 << 32) | lo32;
      if (want) {
        const unsigned long long r = base + (unsigned long long)__popcll(wants & ((1ull << lane) - 1ull));
        if (r < (unsigned long long)n_rows) {
          row = (long long)r;
          it = 0;
          const double* g = goal + 7 * (row / rows_per_goal);
          Ginv = se3_mul(load_se3(w.link_place + 12 * iv.link), ik_se3_inverse(ik_pose_se3(g)));
          const double* qi = q_in + row * dof;
          ik_load_row(jt, iv, L, qi);
          if (q_in != q_out)  // the slots outside the chain pass through
            for (int d = 0; d < dof; ++d) q_out[row * dof + d] = qi[d];
        } else {
          rows_left = false;
        }
      }
    }
    if (!__ballot(row >= 0)) break;  // no lane of the wave holds a row: none is left
    if (row >= 0) {
      const SE3 T = ik_fk(jt, iv, L);
      double err[6];
      ik_log6(se3_mul(Ginv, T), err);
      int st = 0;
      bool fin = true;
      if (ik_norm6(err) < iv.eps) st = MPG_IK_CONVERGED;
      else if (it >= iv.max_iter) st = 0;
      else if (!ik_update(jt, iv, L, T, err)) st = MPG_IK_SINGULAR;
      else fin = false;
      if (fin) {
        ik_store_row(jt, iv, L, q_out + row * dof);
        status[row] = (uint8_t)st;
        if (err_out)
          for (int k = 0; k < 6; ++k) err_out[row * 6 + k] = err[k];
        if (iters_out) iters_out[row] = it;
        row = -1;
      } else {
        ++it;
      }
    }
  }
}

// check_joint_limit and the distance_6D bit of every row (steps 2 and 3 of
// mpg_ik_batch, before the collide pass on the wrapped values)
__global__ __launch_bounds__(128) void ik_finish_kernel(DevWorld w, IkView iv, const double* __restrict__ goal,
                                                       long long n_rows, long long rows_per_goal,
                                                       double* __restrict__ q_out, uint8_t* __restrict__ status) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_rows) return;
  status[row] |= (uint8_t)ik_finish_row(w, iv, goal + 7 * (row / rows_per_goal), q_out + row * w.dof);
}

// folds the collide pass's flags into the status bytes
__global__ __launch_bounds__(256) void ik_fold_kernel(const uint8_t* __restrict__ flags, long long n_rows,
                                                     uint8_t* __restrict__ status) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_rows) return;
  if (flags[row] == 0) status[row] |= MPG_IK_COLLISION_FREE;
}

// ---------------------------------------------------------------------------
// Planner.plan_screw's loop (mplib/planner.py:526-671), batched:
// mpg_screw_batch.  The per-row arithmetic is mpg_screw.h's.
// ---------------------------------------------------------------------------
// One lane per row, one wave per block, the whole row in one launch.  A row is
// at most max_waypoints steps of equal cost, so the grid is ceil(rows / 64)
// blocks and no lane claims a second row.  Each lane writes its waypoints to
// path [rows][max_waypoints][dof] as they are accepted and pads the rest.
// LDS: the lanes' IkLane state, [chain joint][component][lane], then the
// chain's joint constants (IkJointsTable), filled once per wave.
__global__ __launch_bounds__(64) void screw_kernel(DevWorld w, ScrewView sv, const double* __restrict__ goal,
                                                  const double* __restrict__ q_start, long long n_rows, double* path,
                                                  int32_t* __restrict__ n_waypoints, uint8_t* __restrict__ status) {
  extern __shared__ double screw_lds[];
  const int lane = threadIdx.x;
  const int cl = sv.iv.cl;
  const IkLane L{screw_lds + lane, 64};
  double* const td = screw_lds + (size_t)cl * kIkSlot * 64;
  int* const ti = reinterpret_cast<int*>(td + (size_t)cl * IKT_DOUBLES);
  for (int k = lane; k < cl; k += 64) {
    const int j0 = w.chain_joints[sv.iv.cs + k] - 1;
    ti[IKT_INTS * k + IKT_TYPE] = w.joint_type[j0];
    ti[IKT_INTS * k + IKT_SRC] = w.joint_q_source[j0];
    ti[IKT_INTS * k + IKT_MOVE] = sv.iv.move[k];
    td[IKT_DOUBLES * k + IKT_QCONST] = w.joint_q_const[j0];
    for (int c = 0; c < 3; ++c) td[IKT_DOUBLES * k + IKT_AXIS + c] = w.joint_axis[3 * j0 + c];
    for (int c = 0; c < 12; ++c) td[IKT_DOUBLES * k + IKT_PLACE + c] = w.joint_place[12 * j0 + c];
  }
  __syncthreads();
  const long long row = (long long)blockIdx.x * 64 + lane;
  if (row >= n_rows) return;
  const IkJointsTable jt{td, ti};
  int count;
  const int st = screw_row(w, jt, sv, L, goal + 7 * row, q_start + row * w.dof,
                           path + row * sv.max_waypoints * w.dof, &count);
  n_waypoints[row] = count;
  status[row] = (uint8_t)st;
}

// folds the collide pass's flags of the padded path into the status bytes:
// waypoints 1 .. count - 1 (the start state is not checked)
__global__ __launch_bounds__(256) void screw_fold_kernel(const uint8_t* __restrict__ flags,
                                                        const int32_t* __restrict__ n_waypoints, long long n_rows,
                                                        int max_waypoints, uint8_t* __restrict__ status,
                                                        int32_t* __restrict__ first_hit) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_rows) return;
  int n = n_waypoints[row];
  n = n < max_waypoints ? n : max_waypoints;
  int hit = -1;
  for (int i = 1; i < n; ++i)
    if (flags[row * max_waypoints + i] != 0) {
      hit = i;
      break;
    }
  if (hit < 0) status[row] |= MPG_SCREW_COLLISION_FREE;
  if (first_hit) first_hit[row] = hit;
}

// ---------------------------------------------------------------------------
// Planner.plan's RRTConnect (ompl_planner.cpp over OMPL's RRTConnect::solve),
// batched: mpg_plan_batch.  The per-row arithmetic is mpg_rrt.h's.  A round is
// rrt_propose_kernel, one collide pass over every row's slot block,
// rrt_commit_kernel; the host loops over the rounds (launch_plan).
// ---------------------------------------------------------------------------
// a call's workspace as the kernels take it (mpg_world::PlanWork), all per row
struct RrtBufs {
  double* nodes;     // [Q][2][max_nodes][dof]
  int32_t* parent;   // [Q][2][max_nodes]
  int32_t* sizes;    // [Q][2]
  int32_t* phase;    // [Q] RRT_EXTEND / RRT_CONNECT / RRT_DONE
  int32_t* added;    // [Q] the node the iteration's extension added
  int32_t* iter;     // [Q] iterations started
  int32_t* prop;     // [Q][RRT_P_INTS] the round's proposal
  double* newstate;  // [Q][dof] the state it would add
  uint64_t* seeds;   // [Q]
  double* slots;     // [Q][block][dof] the states of the round's collide pass ([Q][1 + G][dof] at the start)
  uint8_t* flags;    // their flags
  int32_t* active;   // rows that have not ended
};

// start and goals of every row, packed for the first collide pass
__global__ __launch_bounds__(256) void rrt_gather_kernel(RrtView v, long long Q, const double* __restrict__ start,
                                                        const double* __restrict__ goal, double* __restrict__ slots) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long per = (long long)(1 + v.goals) * v.dof;
  if (i >= Q * per) return;
  const long long row = i / per, k = i % per;
  slots[i] = k < v.dof ? start[row * v.dof + k] : goal[row * (long long)v.goals * v.dof + (k - v.dof)];
}

// a thread per row: the roots, the status of an invalid start / goal set, the
// machine's first state (rrt_init_row); counts the rows that plan
__global__ __launch_bounds__(64) void rrt_init_kernel(RrtView v, long long Q, const double* __restrict__ start,
                                                     const double* __restrict__ goal,
                                                     const uint64_t* __restrict__ row_seed, uint64_t seed, RrtBufs b,
                                                     int32_t* __restrict__ n_waypoints, uint8_t* __restrict__ status) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= Q) return;
  const size_t tree = (size_t)2 * v.max_nodes;
  b.seeds[row] = row_seed ? row_seed[row] : rrt_row_seed(seed, (uint64_t)row);
  const bool plans = rrt_init_row(v, start + row * v.dof, goal + row * (long long)v.goals * v.dof,
                                  b.flags + row * (1 + v.goals), b.nodes + row * tree * v.dof, b.parent + row * tree,
                                  b.sizes + 2 * row, b.phase + row, b.added + row, b.iter + row,
                                  b.prop + RRT_P_INTS * row, n_waypoints + row, status + row);
  if (plans) atomicAdd(b.active, 1);
}

// every row's slot block and path start as copies of its start state, so the
// collide passes and a row without a path see finite states: a thread per
// value (grid-stride), after the first collide pass has read the slots
__global__ __launch_bounds__(256) void rrt_fill_kernel(RrtView v, long long Q, const double* __restrict__ start,
                                                      double* __restrict__ slots, double* __restrict__ path) {
  const long long per = (long long)(v.block + v.max_waypoints) * v.dof, tot = Q * per;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (long long)gridDim.x * blockDim.x) {
    const long long row = i / per, k = i % per;
    *rrt_fill_start(v, k, slots + row * (long long)v.block * v.dof, path + row * (long long)v.max_waypoints * v.dof) =
        start[row * v.dof + k % v.dof];
  }
}

// A workgroup per row.  Thread 0 draws the sample or takes the connect target;
// every thread scans a strided share of the tree (node-major, so the
// workgroup reads contiguous memory) for the first strict minimum of the
// distance, summed in dimension order as on the host; the reduction orders
// (distance, index) lexicographically, which is the serial scan's "first
// strict minimum".  Thread 0 steers, then the threads write the motion's
// states into the row's slot block (the slots past the count repeat slot 0).
// Every loop is bounded by max_nodes, dof or the block size.
__global__ __launch_bounds__(256) void rrt_propose_kernel(RrtView v, RrtBufs b) {
  __shared__ double s_target[kRrtDof], s_ds[kRrtDof], s_bd[4];
  __shared__ int s_bi[4], s_meta[4];  // tree, nearest node, segments, states
  const long long row = blockIdx.x;
  if (b.phase[row] == RRT_DONE) return;  // the whole workgroup
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double* const nodes = b.nodes + (size_t)row * 2 * v.max_nodes * v.dof;
  if (tid == 0)
    s_meta[0] = rrt_target(v, b.seeds[row], b.phase[row], b.iter + row, b.added[row], nodes, s_target);
  __syncthreads();
  const int tree = s_meta[0];
  const double* const tn = rrt_node(v, nodes, tree, 0);
  int n = b.sizes[2 * row + tree];
  n = n < v.max_nodes ? n : v.max_nodes;
  double bd = INFINITY;
  int bi = 0x7fffffff;
  rrt_nearest_scan(v, tn, n, s_target, tid, 256, &bd, &bi);
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(bd, o);
    const int oi = __shfl_xor(bi, o);
    if (rrt_nearer(od, oi, bd, bi)) bd = od, bi = oi;
  }
  if (lane == 0) s_bd[wv] = bd, s_bi[wv] = bi;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < 4; ++k)
      if (rrt_nearer(s_bd[k], s_bi[k], bd, bi)) bd = s_bd[k], bi = s_bi[k];
    if (bi >= n) bi = 0;  // no finite distance: the serial scan's initial answer
    int32_t* const prop = b.prop + RRT_P_INTS * row;
    s_meta[1] = bi;
    s_meta[2] = rrt_steer(v, tree, tn + (size_t)bi * v.dof, bi, s_target, s_ds, prop);
    s_meta[3] = prop[RRT_P_COUNT];
    rrt_copy(v.dof, s_ds, b.newstate + row * v.dof);
  }
  __syncthreads();
  const double* const near = tn + (size_t)s_meta[1] * v.dof;
  const int nd = s_meta[2], count = s_meta[3];
  double* const slots = b.slots + row * (long long)v.block * v.dof;
  for (int s = tid; s < v.block; s += 256)
    rrt_slot_state(v, tree, near, s_ds, nd, s < count ? s : 0, slots + (size_t)s * v.dof);
}

// a thread per row: growTree's answer from the block's flags, the node, the
// next state of the machine and the status of a row that ends (rrt_commit);
// the rows that end leave the count of active rows
__global__ __launch_bounds__(64) void rrt_commit_kernel(RrtView v, long long Q, int round, RrtBufs b,
                                                       uint8_t* __restrict__ status) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= Q) return;
  const size_t tree = (size_t)2 * v.max_nodes;
  const bool ended = rrt_commit(v, round, b.prop + RRT_P_INTS * row, b.newstate + row * v.dof,
                                b.flags + row * (long long)v.block, b.nodes + row * tree * v.dof, b.parent + row * tree,
                                b.sizes + 2 * row, b.phase + row, b.added + row, status + row);
  if (ended) atomicSub(b.active, 1);
}

// after the last round, a wave per row: lane 0 of a solved row walks the two
// parent chains into the waypoints' node indices (LDS; at most max_waypoints
// <= 4096 of them, each walk bounded by max_nodes steps), then the lanes copy
// the path's slots (rrt_finish_row's steps).  A path longer than
// max_waypoints sets MPG_PLAN_TRUNCATED and leaves the count 0.
__global__ __launch_bounds__(64) void rrt_path_kernel(RrtView v, RrtBufs b, double* __restrict__ path,
                                                     int32_t* __restrict__ n_waypoints, uint8_t* __restrict__ status) {
  __shared__ int32_t s_idx[4096];
  __shared__ int s_n;
  const long long row = blockIdx.x;
  if (!(status[row] & MPG_PLAN_SOLVED)) return;  // the whole wave
  const size_t tree = (size_t)2 * v.max_nodes;
  if (threadIdx.x == 0) {
    const int32_t* prop = b.prop + RRT_P_INTS * row;
    s_n = rrt_path_indices(v, b.parent + row * tree, prop[RRT_P_SM], prop[RRT_P_GM], s_idx);
    if (s_n < 0) status[row] |= MPG_PLAN_TRUNCATED;
    else n_waypoints[row] = s_n;
  }
  __syncthreads();
  const int n = s_n;
  if (n < 0) return;
  double* const out = path + row * (long long)v.max_waypoints * v.dof;
  for (int p = threadIdx.x; p < v.max_waypoints; p += 64) rrt_path_slot(v, b.nodes + row * tree * v.dof, s_idx, n, p, out);
}

// ---------------------------------------------------------------------------
// Planner.TOPP (mplib/planner.py:358-375), batched: mpg_topp_batch.  The
// per-row arithmetic is mpg_topp.h's.
// ---------------------------------------------------------------------------
// mpg_topp.h's lane policy for a wave of 64: the minimum is a butterfly, so
// every lane holds it
struct ToppWave {
  static MPG_INLINE int lane() {
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)threadIdx.x;
#else
    return 0;
#endif
  }
  static MPG_INLINE int lanes() { return 64; }
  static MPG_INLINE double wmin(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double u = __shfl_xor(v, o);
      v = u < v ? u : v;
    }
#endif
    return v;
  }
  static MPG_INLINE void sync() {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
  }
};

// One wave per row, one wave per block.  A row is two dependent chains of N
// gridpoints (the controllable sets backwards, the profile forwards), each
// gridpoint a minimum over (2 dof + 1)^2 pairs of constraint rows: the lanes
// split the joints (spline, constraint rows) and the pairs, the minimum is a
// wave reduction, the chain's K_k / x_k / t_k are wave-uniform and lane 0
// stores them.  LDS: the interval's constraint rows.  The workspace M, K, x, t
// is per row (mpg_world::ToppWork).
__global__ __launch_bounds__(64) void topp_row_kernel(ToppView v, const double* __restrict__ path,
                                                     const int32_t* __restrict__ n_waypoints, double* M, double* K,
                                                     double* x, double* t, int32_t* __restrict__ n_samples,
                                                     double* __restrict__ duration, uint8_t* __restrict__ status) {
  __shared__ double s_rows[4 * kToppRows];
  const size_t row = blockIdx.x;
  const size_t pstride = (size_t)v.max_waypoints * v.dof, gstride = (size_t)v.ncap + 1;
  const ToppRowBufs b{M + row * pstride, K + row * gstride, x + row * gstride, t + row * gstride};
  double dur;
  int m;
  const int st = topp_row<ToppWave>(v, path + row * pstride, n_waypoints[row], b, s_rows, &dur, &m);
  if (threadIdx.x == 0) {
    n_samples[row] = m;
    duration[row] = dur;
    status[row] = (uint8_t)st;
  }
}

// One thread per (row, sample slot): a binary search in the row's t, then
// mpg_topp.h's sample.  Neighbouring threads write neighbouring slots.
__global__ __launch_bounds__(256) void topp_sample_kernel(ToppView v, const double* __restrict__ path,
                                                         const int32_t* __restrict__ n_waypoints, long long n_rows,
                                                         const double* __restrict__ M, const double* __restrict__ x,
                                                         const double* __restrict__ t,
                                                         const int32_t* __restrict__ n_samples,
                                                         const double* __restrict__ duration,
                                                         double* __restrict__ times, double* __restrict__ pos,
                                                         double* __restrict__ vel, double* __restrict__ acc) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_rows * v.max_samples) return;
  const size_t row = (size_t)(idx / v.max_samples);
  const int i = (int)(idx - (long long)row * v.max_samples);
  const size_t pstride = (size_t)v.max_waypoints * v.dof, gstride = (size_t)v.ncap + 1;
  const ToppRowBufs b{const_cast<double*>(M) + row * pstride, nullptr, const_cast<double*>(x) + row * gstride,
                      const_cast<double*>(t) + row * gstride};
  topp_sample(v, path + row * pstride, n_waypoints[row], b, duration[row], n_samples[row], i, times + idx,
              pos + (size_t)idx * v.dof, vel + (size_t)idx * v.dof, acc + (size_t)idx * v.dof);
}

// per pair, the configurations whose pair mask has its bit: LDS counters per
// block (atomics on the block's own copy), then one global add per pair
__global__ __launch_bounds__(256) void pair_count_kernel(const uint32_t* __restrict__ masks, long long n, int W,
                                                        int P, unsigned long long* __restrict__ counts) {
  extern __shared__ uint32_t c_lds[];
  for (int p = threadIdx.x; p < P; p += blockDim.x) c_lds[p] = 0u;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    for (int k = 0; k < W; ++k) {
      uint32_t x = masks[i * W + k];
      while (x) {
        atomicAdd(&c_lds[32 * k + __builtin_ctz(x)], 1u);
        x &= x - 1u;
      }
    }
  __syncthreads();
  for (int p = threadIdx.x; p < P; p += blockDim.x)
    if (c_lds[p]) atomicAdd(&counts[p], (unsigned long long)c_lds[p]);
}

// ---------------------------------------------------------------------------
// Host-buffer pipeline (collide_host_pipelined): the pair-mask rows of the
// colliding configurations only, packed in configuration order and written
// straight into pinned host memory.  flags[i] != 0 exactly when row i has a
// bit (collide() == !collideFull().empty(), planning_world.h:248-250), so the
// host rebuilds the full [m, W] mask from the flags and the packed rows.
// Block b covers configurations [b * kPackCfg, (b + 1) * kPackCfg).
// ---------------------------------------------------------------------------
constexpr int kPackCfg = 4096;

__device__ __forceinline__ int block_sum256(int v, int* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const int s = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(256) void flag_count_kernel(const uint8_t* __restrict__ fl, long long m,
                                                         uint32_t* __restrict__ bcnt, uint32_t* __restrict__ bcnt_host) {
  __shared__ int red[4];
  const long long base = (long long)blockIdx.x * kPackCfg;
  int c = 0;
  for (int r = 0; r < kPackCfg / 256; ++r) {
    const long long i = base + r * 256 + threadIdx.x;
    c += (i < m && fl[i]) ? 1 : 0;
  }
  c = block_sum256(c, red);
  if (threadIdx.x == 0) {
    bcnt[blockIdx.x] = (uint32_t)c;
    bcnt_host[blockIdx.x] = (uint32_t)c;
  }
}

// STAGED: the block's packed rows go through LDS (256 * W words), so each
// store instruction writes consecutive words of host memory; otherwise each
// colliding lane writes its own row (wide masks only)
// The flags go to host memory too (fl_out); W = 0: flags only.
template <bool STAGED>
__global__ __launch_bounds__(256) void mask_pack_kernel(const uint8_t* __restrict__ fl, const uint32_t* __restrict__ mk,
                                                        long long m, int W, const uint32_t* __restrict__ bcnt,
                                                        uint32_t* __restrict__ out, uint8_t* __restrict__ fl_out) {
  extern __shared__ uint32_t pk_lds[];
  __shared__ int red[4];
  __shared__ int wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int off = 0;
  for (int b = tid; b < (int)blockIdx.x; b += 256) off += (int)bcnt[b];
  long long run = block_sum256(off, red);
  const long long base = (long long)blockIdx.x * kPackCfg;
  for (int r = 0; r < kPackCfg / 256; ++r) {
    const long long i = base + r * 256 + tid;
    if (base + r * 256 >= m) break;  // block-uniform
    const bool f = i < m && fl[i];
    if (i < m) fl_out[i] = f ? 1 : 0;
    if (W == 0) continue;  // block-uniform
    const unsigned long long bal = __ballot(f);
    const int lpos = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[wv] = __popcll(bal);
    __syncthreads();
    int woff = 0;
    for (int k = 0; k < wv; ++k) woff += wcnt[k];
    const int total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    if constexpr (STAGED) {
      if (f)
        for (int k = 0; k < W; ++k) pk_lds[(woff + lpos) * W + k] = mk[i * W + k];
      __syncthreads();
      uint32_t* o = out + run * W;
      for (int d = tid; d < total * W; d += 256) o[d] = pk_lds[d];
    } else {
      if (f)
        for (int k = 0; k < W; ++k) out[(run + woff + lpos) * W + k] = mk[i * W + k];
    }
    run += total;
    __syncthreads();
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// host side: snapshot build + C ABI
// ---------------------------------------------------------------------------
#include "mpg_devbuf.h"
#include "mpg_world.h"

namespace {

#include "mpg_snapshot_host.h"
#include "mpg_streams_host.h"

}  // namespace

extern "C" {

#include "mpg_abi_world.h"

}  // extern "C"

namespace {

#include "mpg_collide_host.h"

}  // namespace

extern "C" {

#include "mpg_abi_batch.h"

}  // extern "C"
