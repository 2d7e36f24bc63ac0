// mpg_streams_host.h -- per-stream workspaces, stream pinning, launch_collide,
// input staging, the pinned ring and the world scratch, host side (included by
// mpg_kernels.hip in an anonymous namespace, after mpg_snapshot_host.h).
#pragma once

// drops the state kept for caller stream s (its workspace, its side stream
// and the side stream's workspace); the device is synchronised first, so no
// queued kernel still uses the buffers.  Caller holds ws_mu.
void release_stream_locked(mpg_world* w, hipStream_t s) {
  const auto wi = w->ws.find(s);
  const auto si = w->sides.find(s);
  const auto ki = w->ik_ws.find(s);
  const auto ci = w->screw_ws.find(s);
  const auto pi = w->plan_ws.find(s);
  const auto ti = w->topp_ws.find(s);
  if (wi == w->ws.end() && si == w->sides.end() && ki == w->ik_ws.end() && ci == w->screw_ws.end() &&
      pi == w->plan_ws.end() && ti == w->topp_ws.end())
    return;
  hipDeviceSynchronize();
  if (ti != w->topp_ws.end()) w->topp_ws.erase(ti);
  if (pi != w->plan_ws.end()) w->plan_ws.erase(pi);
  if (ki != w->ik_ws.end()) w->ik_ws.erase(ki);
  if (ci != w->screw_ws.end()) w->screw_ws.erase(ci);
  if (wi != w->ws.end()) w->ws.erase(wi);
  if (si != w->sides.end()) {
    w->ws.erase(si->second.side.get());
    w->sides.erase(si);
  }
}

// evicts the least recently used caller stream's state when a new stream
// would exceed kMaxStreamState (side-stream workspaces are owned by their
// caller stream's entry).  Caller holds ws_mu.
void evict_streams_locked(mpg_world* w) {
  std::map<hipStream_t, uint64_t> callers;
  for (auto& kv : w->ws) callers[kv.first] = kv.second.last;
  for (auto& kv : w->sides) {
    callers.erase(kv.second.side.get());
    uint64_t& t = callers[kv.first];
    t = std::max(t, kv.second.last);
  }
  for (auto& kv : w->busy)
    if (kv.second > 0) callers.erase(kv.first);  // in use by a call: not evictable
  size_t pinned = 0;
  for (auto& kv : w->busy) pinned += kv.second > 0;
  while (!callers.empty() && callers.size() + pinned >= mpg_world::kMaxStreamState) {
    auto lru = callers.begin();
    for (auto it = callers.begin(); it != callers.end(); ++it)
      if (it->second < lru->second) lru = it;
    release_stream_locked(w, lru->first);
    callers.erase(lru);
  }
}

// keeps a caller stream's state (workspace, side stream) from eviction for
// the duration of one call
struct StreamPin {
  mpg_world* w;
  hipStream_t s;
  StreamPin(mpg_world* w_, hipStream_t s_) : w(w_), s(s_) {
    std::lock_guard<std::mutex> lk(w->ws_mu);
    ++w->busy[s];
  }
  ~StreamPin() {
    std::lock_guard<std::mutex> lk(w->ws_mu);
    if (--w->busy[s] <= 0) w->busy.erase(s);
  }
};

bool is_side_stream_locked(const mpg_world* w, hipStream_t s) {
  for (auto& kv : w->sides)
    if (kv.second.side.get() == s) return true;
  return false;
}

int get_workspace(mpg_world* w, hipStream_t s, long long want, mpg_world::Workspace** out) {
  std::lock_guard<std::mutex> lk(w->ws_mu);
  if (w->ws.find(s) == w->ws.end() && !is_side_stream_locked(w, s) && w->sides.find(s) == w->sides.end())
    evict_streams_locked(w);
  auto& ws = w->ws[s];
  ws.last = ++w->ws_tick;
  const long long np = std::max(w->dw.n_pairs, 1);
  if (ws.cap < want) {
    ws = mpg_world::Workspace{};  // no wait of its own: freeing device memory waits for the queued work that reads it
    ws.last = w->ws_tick;
    HIP_TRY(ws.surv.reserve((size_t)w->dw.W * want));
    HIP_TRY(ws.cnt.reserve(bk_cnt_words(w->dw.W, want)));
    HIP_TRY(ws.part.reserve(bk_part_words(w->dw.W, want)));
    HIP_TRY(ws.grp.reserve(bk_grp_words(w->dw.W, want)));
    HIP_TRY(ws.seg_len.reserve(np));
    HIP_TRY(ws.seg_start.reserve(np));
    HIP_TRY(ws.prefix.reserve(np + kPrefixTail));
    HIP_TRY(ws.cand.reserve((size_t)np * want));
    HIP_TRY(ws.rq.reserve((size_t)4 * std::max(w->dw.n_moving, 1) * want));
    HIP_TRY(ws.sc.reserve((size_t)2 * std::max(w->dw.dof, 1) * want));
    ws.cap = want;
  }
  *out = &ws;
  return MPG_OK;
}

Event prof_event(mpg_world* w) {  // empty when none could be created
  Event e;
  if (!w->ev_pool.empty()) {
    e = std::move(w->ev_pool.back());
    w->ev_pool.pop_back();
  } else {
    e.create(hipEventDefault);
  }
  return e;
}

// records the start of a stage on `stream` when profiling is on
struct StageTimer {
  mpg_world* w;
  hipStream_t s;
  int stage;
  Event a;
  StageTimer(mpg_world* w_, hipStream_t s_, int st) : w(w_), s(s_), stage(st) {
    if (!w->prof) return;
    std::lock_guard<std::mutex> lk(w->prof_mu);
    a = prof_event(w);
    if (a) hipEventRecord(a.get(), s);
  }
  void stop() {
    if (!a) return;
    std::lock_guard<std::mutex> lk(w->prof_mu);
    Event b = prof_event(w);
    if (!b) return;
    hipEventRecord(b.get(), s);
    w->marks.push_back({stage, std::move(a), std::move(b)});
  }
  ~StageTimer() { stop(); }
};

struct ContactOut {
  double *depth, *normal, *pos;  // [n*P], [n*P*3], [n*P*3]
};

// The words of the cull's lookup grids (NULL: the world has none).  The first
// bulk launch with joint-value input builds them from the plan world creation
// left and uploads them, so creation and the latency path pay nothing; later
// calls only read the flag.
inline int grid_words_for(mpg_world* w, const uint32_t** out) {
  *out = nullptr;
  if (w->dw.n_grid == 0) return MPG_OK;
  if (!w->grid_ready.load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lk(w->grid_mu);
    if (!w->grid_ready.load(std::memory_order_relaxed)) {
      const auto t0 = std::chrono::steady_clock::now();
      std::vector<uint32_t> words;
      bp_grid_fill(w->grid_plan, words);
      HIP_TRY(w->grid_words.reserve(words.size()));
      HIP_TRY(hipMemcpy(w->grid_words.get(), words.data(), sizeof(uint32_t) * words.size(), hipMemcpyHostToDevice));
      w->grid_plan = BpGridPlan();
      w->grid_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (std::getenv("MPG_STATS"))
        std::fprintf(stderr, "[mpg] lookup grids: %zu cells built in %.1f ms\n", words.size(), w->grid_build_ms);
      w->grid_ready.store(true, std::memory_order_release);
    }
  }
  *out = w->grid_words.get();
  return MPG_OK;
}

template <bool FROM_POSES>
int launch_collide(mpg_world* w, const double* in, long long n, uint8_t* flags, uint32_t* masks, hipStream_t stream,
                   const ContactOut* co = nullptr) {
  if (n == 0) return MPG_OK;
  StreamPin pin(w, stream);
  const uint32_t* gwords = nullptr;
  if (!FROM_POSES) {
    const int grc = grid_words_for(w, &gwords);
    if (grc) return grc;
  }
  const long long chunk = std::min<long long>(n, w->max_chunk);
  mpg_world::Workspace* owner = nullptr;
  int rc = get_workspace(w, stream, chunk, &owner);
  if (rc) return rc;
  // the workspace as the kernels take it
  uint32_t *const surv = owner->surv.get(), *const cnt = owner->cnt.get(), *const part = owner->part.get(),
                  *const grp = owner->grp.get(), *const seg_len = owner->seg_len.get(),
                  *const seg_start = owner->seg_start.get(), *const prefix = owner->prefix.get(),
                  *const cand = owner->cand.get();
  float* const rq = owner->rq.get();
  double* const sc = owner->sc.get();
  const long long cap = owner->cap;
  const size_t row = FROM_POSES ? (size_t)w->dw.n_links * 7 : (size_t)w->dw.dof;
  for (long long off = 0; off < n; off += chunk) {
    const long long m = std::min(chunk, n - off);
    const double* qin = in + off * row;
    uint8_t* fl = flags + off;
    uint32_t* mk = masks ? masks + off * w->dw.W : nullptr;
    const unsigned grid = (unsigned)((m + w->block - 1) / w->block);
    const int n_tiles = (int)((m + 63) / 64);
    StageTimer t_cull(w, stream, MPG_STAGE_CULL);
    if (w->prof) w->prof_cfg += m;
    // the cull's histogram path writes every count row whole; the ballot
    // path (more mask words than the histogram holds) writes single bytes
    // and the ablation modes of diagnostic builds leave before the rows
#ifndef MPG_DIAG
    if (w->dw.W * 8 > kQueue)
#endif
      HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(uint32_t) * bk_cnt_words(w->dw.W, m), stream));
    switch (w->block) {
      case 256:
        hipLaunchKernelGGL((cull_kernel<256, FROM_POSES>), dim3(grid), dim3(256), w->lds_bytes, stream, w->dw, qin,
                           m, fl, mk, surv, rq, sc, cap, cnt, n_tiles, gwords);
        break;
      case 128:
        hipLaunchKernelGGL((cull_kernel<128, FROM_POSES>), dim3(grid), dim3(128), w->lds_bytes, stream, w->dw, qin,
                           m, fl, mk, surv, rq, sc, cap, cnt, n_tiles, gwords);
        break;
      default:
        hipLaunchKernelGGL((cull_kernel<64, FROM_POSES>), dim3(grid), dim3(64), w->lds_bytes, stream, w->dw, qin, m,
                           fl, mk, surv, rq, sc, cap, cnt, n_tiles, gwords);
        break;
    }
    HIP_TRY(hipGetLastError());
    t_cull.stop();
    StageTimer t_bucket(w, stream, MPG_STAGE_BUCKET);
    const int n_ranges = bk_ranges(n_tiles), n_groups = bk_groups(n_ranges);
    const long long tw = (long long)n_tiles * w->dw.W;  // one wave per (word, tile)
    const unsigned gb = (unsigned)((tw + 3) / 4);
    // small launches: the scan's block sums the ranges itself (one launch fewer)
    const bool fold = bk_fold_sum(n_ranges, w->dw.W);
    if (!fold) {
      hipLaunchKernelGGL(range_sum_kernel, dim3(n_groups), dim3(256), 0, stream, cnt, n_tiles, w->dw.W, part, grp);
      HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(range_scan_kernel, dim3(1), dim3(1024), 0, stream, fold ? cnt : nullptr, n_tiles, w->dw.W,
                       part, grp, n_groups, w->dw.n_pairs, seg_len, seg_start, prefix,
                       w->prof ? w->prof_units.get() : nullptr, (uint32_t)(4 * w->narrow_blocks));
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(scatter_kernel, dim3(gb), dim3(256), 0, stream, surv, m, cap, w->dw.n_pairs, w->dw.W,
                       n_tiles, cnt, part, grp, seg_start, cand);
    HIP_TRY(hipGetLastError());
    t_bucket.stop();
    StageTimer t_narrow(w, stream, MPG_STAGE_NARROW);
    // persistent narrow phase: enough waves to fill the chip, fewer for tiny batches
    const long long want_waves = (m * std::max(w->dw.n_pairs, 1) + kTaskMin - 1) / kTaskMin;
    const unsigned nb = (unsigned)std::max<long long>(1, std::min<long long>(w->narrow_blocks, (want_waves + 3) / 4));
    hipLaunchKernelGGL((narrow_kernel<FROM_POSES>), dim3(nb), dim3(256), 0, stream, w->dw, qin, seg_len,
                       seg_start, prefix, cand, fl, mk, prefix + w->dw.n_pairs + 1, sc);
    HIP_TRY(hipGetLastError());
    if (w->any_closed_form) {
      hipLaunchKernelGGL((closed_form_kernel<FROM_POSES, CLS_CLOSED>), dim3(w->narrow_blocks), dim3(256), 0, stream,
                         w->dw, qin, seg_len, seg_start, prefix, cand, fl, mk, sc);
      HIP_TRY(hipGetLastError());
    }
    if (w->any_octree) {
      hipLaunchKernelGGL((closed_form_kernel<FROM_POSES, CLS_OCTREE>), dim3(w->narrow_blocks), dim3(256), 0, stream,
                         w->dw, qin, seg_len, seg_start, prefix, cand, fl, mk, sc);
      HIP_TRY(hipGetLastError());
    }
    if (w->any_mesh) {
      hipLaunchKernelGGL((closed_form_kernel<FROM_POSES, CLS_MESH>), dim3(w->narrow_blocks), dim3(256), 0, stream,
                         w->dw, qin, seg_len, seg_start, prefix, cand, fl, mk, sc);
      HIP_TRY(hipGetLastError());
    }
    if (w->any_gjk) {
      hipLaunchKernelGGL((closed_form_kernel<FROM_POSES, CLS_GJK>), dim3(w->narrow_blocks), dim3(256), 0, stream,
                         w->dw, qin, seg_len, seg_start, prefix, cand, fl, mk, sc);
      HIP_TRY(hipGetLastError());
    }
    if (co) {  // penetration info of the reported pairs (enable_contact)
      const size_t P = (size_t)w->dw.n_pairs;
      HIP_TRY(hipMemsetAsync(co->depth + off * P, 0, sizeof(double) * m * P, stream));
      HIP_TRY(hipMemsetAsync(co->normal + off * P * 3, 0, sizeof(double) * m * P * 3, stream));
      HIP_TRY(hipMemsetAsync(co->pos + off * P * 3, 0, sizeof(double) * m * P * 3, stream));
      hipLaunchKernelGGL((contact_kernel<FROM_POSES>), dim3(nb), dim3(256), 0, stream, w->dw, qin, seg_len,
                         seg_start, prefix, cand, mk, sc, co->depth + off * P, co->normal + off * P * 3,
                         co->pos + off * P * 3);
      HIP_TRY(hipGetLastError());
    }
  }
  return MPG_OK;
}

// The staging of one MPG_MEM_HOST call on stream s: grow-only device twins of
// the caller's arrays.  It keeps the call's first error (a failed reserve is
// MPG_E_NOMEM, a failed copy or wait MPG_E_HIP) and does nothing after one: a
// caller checks rc once before it launches and returns finish().  last: the
// world scratch's event (scratch_begin below), waited for before a buffer is
// replaced; the stage structs under host_mu pass none (synchronous calls).
struct HostStage {
  hipStream_t s;
  const char* what;  // "IK", "contact", ...: names the call in the error text
  const Event* last = nullptr;
  int rc = MPG_OK;
  void check(hipError_t e, const char* step) {
    if (!rc && e != hipSuccess)
      rc = set_error(MPG_E_HIP, std::string(what) + " staging, " + step + ": " + hipGetErrorString(e));
  }
  template <class T>
  T* out(DevBuf<T>& buf, size_t count) {  // reserve: the device pointer
    if (!rc && last && *last && buf.get() && buf.cap() < count)
      check(hipEventSynchronize(last->get()), "wait for the previous call");  // the old block's last reader
    if (!rc && buf.reserve(count) != hipSuccess) rc = set_error(MPG_E_NOMEM, std::string(what) + " staging buffers");
    return rc ? nullptr : buf.get();
  }
  template <class T>
  T* in(DevBuf<T>& buf, const T* host, size_t count) {  // reserve, queue the copy in: the device pointer
    T* const d = out(buf, count);
    if (d && count) check(hipMemcpyAsync(d, host, sizeof(T) * count, hipMemcpyHostToDevice, s), "copy in");
    return rc ? nullptr : d;
  }
  template <class T>
  void back(T* host, const T* dev, size_t count) {  // queue the copy out
    if (!rc && count) check(hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, s), "copy out");
  }
  int finish() {  // the results are in the caller's arrays
    if (!rc) check(hipStreamSynchronize(s), "synchronize");
    return rc;
  }
};

// World-owned scratch (distance, motion validation) used by calls on any
// stream: a call's work waits for the previous call's (`last`, whatever its
// stream), and a buffer is freed to grow only after that work has finished,
// so two host threads on two streams never run over the same buffers at once
// (calls on one world are serialised on the device; their enqueueing already
// is, by the world's mutex).  Caller holds the scratch's mutex.
int scratch_begin(Event& last, hipStream_t s) {
  if (!last) HIP_TRY(last.create(hipEventDisableTiming));
  else HIP_TRY(hipStreamWaitEvent(s, last.get(), 0));
  return MPG_OK;
}
template <class T>
int scratch_grow(const Event& last, DevBuf<T>& buf, size_t n) {
  if (buf.get() && buf.cap() < n && last) HIP_TRY(hipEventSynchronize(last.get()));  // the old block's last reader
  HIP_TRY(buf.reserve(n));
  return MPG_OK;
}

// slots of `cap` configurations with `row` input doubles each (grow-only)
int ensure_ring(mpg_world* w, size_t cap, size_t row) {
  auto& R = w->ring;
  if (!R.h2d) {
    HIP_TRY(R.h2d.create(hipStreamNonBlocking));
    HIP_TRY(R.side.create(hipStreamNonBlocking));
    for (int j = 0; j < mpg_world::kRing; ++j) {
      HIP_TRY(R.e_in[j].create(hipEventDisableTiming));
      HIP_TRY(R.e_done[j].create(hipEventDisableTiming));
    }
  }
  const size_t in = cap * std::max<size_t>(row, 1);
  if (cap <= R.cap && in <= R.in_cap) return MPG_OK;
  cap = std::max(cap, R.cap);
  const size_t in_cap = std::max(in, R.in_cap);
  // no wait: the pipeline's calls are synchronous under host_mu.  The slot
  // buffers go, the streams and events stay.
  for (auto& S : R.slot) S = mpg_world::Ring::Slot{};
  R.cap = R.in_cap = 0;
  const size_t W = (size_t)std::max(w->dw.W, 1);
  const size_t blocks = (cap + kPackCfg - 1) / kPackCfg;
  for (auto& S : R.slot) {
    HIP_TRY(S.d_in.reserve(in_cap));
    HIP_TRY(S.d_fl.reserve(cap));
    HIP_TRY(S.d_mk.reserve(W * cap));
    HIP_TRY(S.d_bcnt.reserve(blocks));
    HIP_TRY(S.h_fl.reserve(cap, kPinMapped));
    HIP_TRY(S.h_mk.reserve(W * cap, kPinMapped));
    HIP_TRY(S.h_bcnt.reserve(blocks, kPinMapped));
  }
  R.cap = cap;
  R.in_cap = in_cap;
  return MPG_OK;
}
