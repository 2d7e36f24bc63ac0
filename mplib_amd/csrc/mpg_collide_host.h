// mpg_collide_host.h -- host side of the latency path, the overlapped launch,
// the host pipeline and the free-frame path (included by
// mpg_kernels.hip in an anonymous namespace, after mpg_abi_world.h).
#pragma once

// pinned input rows (ncfg * row doubles: q rows or link poses), hit bytes
// (n_pairs * ncfg) and joint sincos: the input capacity is tracked in doubles,
// since the same buffers serve q rows (dof) and link-pose rows (n_links * 7)
int ensure_small(mpg_world* w, size_t ncfg, size_t row) {
  const size_t want_q = ncfg * std::max<size_t>(row, 1);
  if (ncfg <= w->small_cap && want_q <= w->small_qcap) return MPG_OK;
  ncfg = std::max(ncfg, w->small_cap);
  const size_t qcap = std::max(want_q, w->small_qcap);
  w->small = mpg_world::Small{};  // no wait: the latency path's calls are synchronous under host_mu
  w->small_cap = 0;
  w->small_qcap = 0;
  const size_t P = (size_t)std::max(w->dw.n_pairs, 1);
  auto& S = w->small;
  HIP_TRY(S.h_q.reserve(qcap, kPinCoherent));
  HIP_TRY(S.h_hits.reserve(P * ncfg, kPinCoherent));
  HIP_TRY(S.d_qs.reserve(qcap));
  HIP_TRY(S.d_ssc.reserve(2 * ncfg * std::max<int>(w->dw.dof, 1)));
  HIP_TRY(S.h_ssc.reserve(2 * ncfg * std::max<int>(w->dw.dof, 1), kPinCoherent));
  w->small_cap = ncfg;
  w->small_qcap = qcap;
  return MPG_OK;
}

// (re)start the latency server; it takes `done` as the last batch served
int srv_start(mpg_world* w) {
  if (!w->srv.get()) {
    HIP_TRY(w->srv.reserve(1, kPinCoherent));
    std::memset(w->srv.get(), 0, sizeof(SrvCtl));
    HIP_TRY(w->srv_stream.create(hipStreamNonBlocking));
    HIP_TRY(hipFuncSetAttribute((const void*)lat_server_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)w->srv_lds));
  }
  SrvCtl* const C = w->srv.get();
  for (int k = 0; k < kSrvMaxG; ++k) __atomic_store_n(&C->gone[k], 0ull, __ATOMIC_RELAXED);
  __atomic_store_n(&C->quit, 0ull, __ATOMIC_RELEASE);
  ++w->srv_starts;
  hipLaunchKernelGGL(lat_server_kernel, dim3(w->srv_g), dim3(kSrvThreads), w->srv_lds, w->srv_stream.get(), w->dw,
                     w->srv.dev(), (unsigned long long)w->srv_idle_us * 100ull, w->srv_stats ? 1 : 0);
  HIP_TRY(hipGetLastError());
  w->srv_running = true;
  return MPG_OK;
}

// one batch through the resident server: rows (q, host sin/cos) into the
// control block, seq bumped, the host spins on `done`.  The server may have
// left (idle) before it saw the request: every 50 us the host looks for
// workgroups that have left (`gone`) without answering -- all of them (stream
// complete): start it again; some of them: stop the rest and start all again.
// Workgroups that are only slow (another stream sharing the GPU) are waited
// for.  No answer within 2 s: the server is stopped, MPG_E_HIP (the caller
// launches instead for a while, then tries the server again).
int collide_served(mpg_world* w, const double* q, int64_t n, uint8_t* flags, uint32_t* pair_mask) {
  if (w->srv_running && w->srv_quitting) {  // told to quit after a missed answer
    if (hipStreamQuery(w->srv_stream.get()) != hipSuccess) return set_error(MPG_E_HIP, "latency server has not left yet");
    w->srv_running = false;
    w->srv_quitting = false;
  }
  if (!w->srv_running) {
    const int rc = srv_start(w);
    if (rc) return rc;
  }
  SrvCtl* C = w->srv.get();
  const int dof = w->dw.dof, W = w->dw.W;
  for (int64_t c = 0; c < n; ++c) {
    double* r = C->rows + c * 3 * dof;
    std::memcpy(r, q + c * dof, sizeof(double) * (size_t)dof);
    for (const int src : w->h_rev_src) mpg_sincos(q[c * dof + src], &r[dof + 2 * src], &r[dof + 2 * src + 1]);
  }
  const unsigned long long seq = (++w->srv_seq << 8) | (unsigned long long)n;
  __atomic_store_n(&C->seq, seq, __ATOMIC_RELEASE);
  const auto t0 = std::chrono::steady_clock::now();
  long long next_us = 50;
  bool forced = false;
  auto all_done = [&] {
    for (int k = 0; k < w->srv_g; ++k)
      if (__atomic_load_n(&C->done[k], __ATOMIC_ACQUIRE) != seq) return false;
    return true;
  };
  while (!all_done()) {
    __builtin_ia32_pause();
    const long long us =
        std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    if (us < next_us) continue;
    next_us = us + 50;
    hipError_t e = hipStreamQuery(w->srv_stream.get());
    bool partial = false;  // a workgroup left before this request, others are still resident
    for (int k = 0; k < w->srv_g && e == hipErrorNotReady; ++k)
      partial |= __atomic_load_n(&C->gone[k], __ATOMIC_ACQUIRE) != 0ull &&
                 __atomic_load_n(&C->done[k], __ATOMIC_ACQUIRE) != seq;
    if (partial && !forced) {
      // stop the ones still polling and start all again (once per request);
      // they see quit within one poll, so this wait is short
      __atomic_store_n(&C->quit, 1ull, __ATOMIC_RELEASE);
      e = hipStreamSynchronize(w->srv_stream.get());
      forced = true;
    }
    if (e == hipSuccess) {  // it left before this request: start it again
      w->srv_running = false;
      const int rc = srv_start(w);
      if (rc) return rc;
    } else if (e != hipErrorNotReady || us > 2000000) {
      __atomic_store_n(&C->quit, 1ull, __ATOMIC_RELEASE);
      w->srv_quitting = true;  // not waited for here: the next try checks that it has left
      return set_error(MPG_E_HIP, "latency server did not answer");
    }
  }
  ++w->srv_served;
  if (w->prof) {  // a served batch counts as one narrow-stage "launch" of its post -> done time
    std::lock_guard<std::mutex> lk(w->prof_mu);
    w->prof_ms[MPG_STAGE_NARROW] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    w->prof_n[MPG_STAGE_NARROW] += 1;
    w->prof_cfg += n;
  }
  if (w->srv_stats) {  // MPG_STATS: phase sums (rows, fk, spheres, narrow, publish), us
    w->srv_stat[5] += 1.0;
    for (int k = 0; k < 5; ++k) w->srv_stat[k] += (double)(C->phase[k + 1] - C->phase[k]) / 100.0;
    w->srv_stat[6] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  }
  for (int64_t c = 0; c < n; ++c) {
    uint32_t any = 0;
    for (int k = 0; k < W; ++k) {
      uint32_t v = 0;
      for (int gg = 0; gg < w->srv_g; ++gg) v |= __atomic_load_n(&C->out[gg][c * W + k], __ATOMIC_RELAXED);
      any |= v;
      if (pair_mask) pair_mask[c * W + k] = v;
    }
    flags[c] = any ? 1 : 0;
  }
  return MPG_OK;
}

// folds the latency path's hit bytes h[P][n] into flags and pair masks (both
// cleared by the caller).  The only host loop of that path over n_pairs * n
// elements: a function of its own with a fixed alignment, so that where its
// loops fall in a fetch line does not depend on the code around the call
__attribute__((noinline, aligned(64))) void fold_hits(const uint8_t* h, int P, int64_t n, int W, uint8_t* flags,
                                                      uint32_t* pair_mask) {
  for (int p = 0; p < P; ++p) {
    const uint8_t* hp = h + (size_t)p * n;
    const uint32_t bit = 1u << (p & 31);
    for (int64_t c0 = 0; c0 < n; c0 += 8) {
      const int64_t c1 = std::min<int64_t>(c0 + 8, n);
      if (c1 - c0 == 8) {  // most hit bytes are zero: eight at a time
        uint64_t v;
        std::memcpy(&v, hp + c0, 8);
        if (!v) continue;
      }
      for (int64_t c = c0; c < c1; ++c)
        if (hp[c]) {
          flags[c] = 1;
          if (pair_mask) pair_mask[(size_t)c * W + (p >> 5)] |= bit;
        }
    }
  }
}

// one round trip: input to the device, one small_kernel launch writing hit
// bytes straight into host memory, one synchronisation; the host folds the
// hits into flags / pair masks
// dev_in: the rows are already on the device (link poses assembled there for
// a world with free frames); q is then not read
template <bool FROM_POSES>
int collide_small(mpg_world* w, const double* q, int64_t n, uint8_t* flags, uint32_t* pair_mask, hipStream_t s,
                  const double* dev_in = nullptr) {
  if (!FROM_POSES && w->srv_mode && w->srv_ok && n <= w->srv_max_n && !w->dw.dbg(3) && !w->dw.dbg(7) &&
      (!w->srv_broken || std::chrono::steady_clock::now() >= w->srv_retry_at)) {
    if (collide_served(w, q, n, flags, pair_mask) == MPG_OK) {
      w->srv_broken = false;
      return MPG_OK;
    }
    // the server could not be started or did not answer: launches for the
    // next second, then the server is tried again
    std::fprintf(stderr, "mplib_amd: latency server unavailable (%s); one launch per batch for 1 s\n",
                 g_last_error.c_str());
    w->srv_broken = true;
    ++w->srv_fallbacks;
    w->srv_retry_at = std::chrono::steady_clock::now() + std::chrono::seconds(1);
    (void)hipGetLastError();
  }
  const size_t row = FROM_POSES ? (size_t)w->dw.n_links * 7 : (size_t)w->dw.dof;
  const size_t cap = std::max<size_t>((size_t)n, std::min<size_t>((size_t)w->small_max, 256));
  int rc = ensure_small(w, cap, row);
  if (rc) return rc;
  const int P = w->dw.n_pairs, W = w->dw.W;
  std::memset(flags, 0, (size_t)n);
  if (pair_mask) std::memset(pair_mask, 0, sizeof(uint32_t) * (size_t)n * W);
  if (P == 0) return MPG_OK;
  const auto& S = w->small;
  const double* qin = dev_in ? dev_in : w->small_zero_copy ? S.h_q.dev() : S.d_qs.get();
  if (row && !dev_in) {  // zero-copy: the kernel reads the pinned rows directly, no copy launch
    std::memcpy(S.h_q.get(), q, sizeof(double) * (size_t)n * row);
    if (!w->small_zero_copy)
      HIP_TRY(hipMemcpyAsync(S.d_qs.get(), S.h_q.get(), sizeof(double) * (size_t)n * row, hipMemcpyHostToDevice, s));
  }
  const int n_tiles = (int)((n + 63) / 64);
  const long long waves = (long long)P * n_tiles;
  StageTimer t_small(w, s, MPG_STAGE_NARROW);
  if (w->prof) w->prof_cfg += n;
  // the smallest batches: joint sin/cos on the host (mpg_sincos, the device's
  // own restatement of glibc's, bit for bit) into pinned mapped memory, one
  // launch without the sin/cos work; up to small_inline_sc states: one launch
  // with sin/cos inline; larger: a sin/cos launch first
  const bool host_sc = !FROM_POSES && w->dw.dof > 0 && n <= w->small_host_sc;
  const bool inline_sc = !host_sc && (FROM_POSES || (n <= w->small_inline_sc && w->dw.dof <= kLatScDof));
  double* sc_src = S.d_ssc.get();
  double* const h_ssc = S.h_ssc.get();
  if (host_sc) {
    const int dof = w->dw.dof;
    for (int64_t c = 0; c < n; ++c)
      for (const int src : w->h_rev_src) {
        double sv, cv;
        mpg_sincos(q[c * dof + src], &sv, &cv);
        h_ssc[(c * dof + src) * 2] = sv;
        h_ssc[(c * dof + src) * 2 + 1] = cv;
      }
    sc_src = S.h_ssc.dev();
  }
  if (!inline_sc && !host_sc && w->dw.dof > 0) {
    const long long nt = n * w->dw.dof;
    hipLaunchKernelGGL(small_sincos_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, w->dw, qin,
                       (long long)n, S.d_ssc.get());
    HIP_TRY(hipGetLastError());
  }
  const dim3 grid((unsigned)((waves + 3) / 4));
  const bool host_staged = host_sc && w->dw.dof <= kLatScDof && w->dw.lat_rec_ok;
  // the fewest states: their rows travel in the kernel arguments
  const bool by_args = host_staged && n * 3 * (int64_t)w->dw.dof <= kLatIn && w->small_args;
  LatIn args{};
  if (by_args) {
    const int dof = w->dw.dof;
    for (int64_t c = 0; c < n; ++c) {
      double* r = args.d + c * 3 * dof;
      std::memcpy(r, q + c * dof, sizeof(double) * (size_t)dof);
      std::memcpy(r + dof, h_ssc + c * 2 * dof, sizeof(double) * 2 * (size_t)dof);
    }
  }
  auto launch = [&](auto kern) {  // every class instance reads the same sin/cos source
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, w->dw, qin, (long long)n, n_tiles, S.h_hits.dev(), sc_src, args);
    return hipGetLastError();
  };
  auto pick = [&](auto k0, auto k1, auto k2, auto k3) {
    return inline_sc ? launch(k1) : by_args ? launch(k3) : host_staged ? launch(k2) : launch(k0);
  };
  HIP_TRY(pick(small_kernel<FROM_POSES, CLS_CLOSED, 0>, small_kernel<FROM_POSES, CLS_CLOSED, 1>,
               small_kernel<FROM_POSES, CLS_CLOSED, 2>, small_kernel<FROM_POSES, CLS_CLOSED, 3>));
  if (w->any_octree)
    HIP_TRY(pick(small_kernel<FROM_POSES, CLS_OCTREE, 0>, small_kernel<FROM_POSES, CLS_OCTREE, 1>,
                 small_kernel<FROM_POSES, CLS_OCTREE, 2>, small_kernel<FROM_POSES, CLS_OCTREE, 3>));
  if (w->any_mesh)
    HIP_TRY(pick(small_kernel<FROM_POSES, CLS_MESH, 0>, small_kernel<FROM_POSES, CLS_MESH, 1>,
                 small_kernel<FROM_POSES, CLS_MESH, 2>, small_kernel<FROM_POSES, CLS_MESH, 3>));
  if (w->any_gjk)
    HIP_TRY(pick(small_kernel<FROM_POSES, CLS_GJK, 0>, small_kernel<FROM_POSES, CLS_GJK, 1>,
                 small_kernel<FROM_POSES, CLS_GJK, 2>, small_kernel<FROM_POSES, CLS_GJK, 3>));
  t_small.stop();
  HIP_TRY(hipStreamSynchronize(s));
  fold_hits(S.h_hits.get(), P, n, W, flags, pair_mask);
  return MPG_OK;
}

// stream-ordered for the caller: the side stream waits for everything queued
// on `s` before the call, and `s` waits for the side stream's half
template <bool FROM_POSES>
int launch_collide_overlapped(mpg_world* w, const double* in, long long n, uint8_t* flags, uint32_t* masks,
                              hipStream_t s) {
  StreamPin pin(w, s);
  // one chunk or less runs on the caller's stream alone: its two halves'
  // cull and narrow kernels each fill the chip and are latency-bound, so on a
  // second stream they only time-share the CUs (cfg3, 2^20: single stream
  // +0.7-1.3 %; cfg4, 4 chunks: overlapped +16 %, profiles/r05a/overlap_ab.txt).
  // The 2^20 figure predates the tapered task list (mpg_bucket.h, bk_task_plan),
  // which shortens a half batch's tail too; it has not been measured again.
  if (w->overlap_min <= 0 || n < w->overlap_min || n <= w->max_chunk)
    return launch_collide<FROM_POSES>(w, in, n, flags, masks, s);
  // one side stream and fork/join event pair per caller stream: callers on
  // different streams (one host thread each, include/mpgpu.h) never record
  // into or wait on each other's events, and each side stream has its own
  // workspace (get_workspace keys by stream)
  struct {
    hipStream_t side;
    hipEvent_t fork, join;
  } sd;  // the entry's handles: pinned, so it outlives this call
  {
    std::lock_guard<std::mutex> lk(w->ws_mu);
    auto it = w->sides.find(s);
    if (it == w->sides.end()) {
      if (w->ws.find(s) == w->ws.end()) evict_streams_locked(w);
      mpg_world::Side n;
      HIP_TRY(n.side.create(hipStreamNonBlocking));
      HIP_TRY(n.fork.create(hipEventDisableTiming));
      HIP_TRY(n.join.create(hipEventDisableTiming));
      it = w->sides.emplace(s, std::move(n)).first;
    }
    it->second.last = ++w->ws_tick;
    sd = {it->second.side.get(), it->second.fork.get(), it->second.join.get()};
  }
  const size_t row = FROM_POSES ? (size_t)w->dw.n_links * 7 : (size_t)w->dw.dof;
  // parts alternate between the caller's stream and the side stream
  const int parts = std::max(2, w->overlap_parts);
  const long long step = ((n + parts - 1) / parts + 63) / 64 * 64;
  HIP_TRY(hipEventRecord(sd.fork, s));
  HIP_TRY(hipStreamWaitEvent(sd.side, sd.fork, 0));
  int k = 0;
  for (long long off = 0; off < n; off += step, ++k) {
    const long long m = std::min(step, n - off);
    const int rc = launch_collide<FROM_POSES>(w, in + (size_t)off * row, m, flags + off,
                                              masks ? masks + (size_t)off * w->dw.W : nullptr, (k & 1) ? sd.side : s);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(sd.join, sd.side));
  HIP_TRY(hipStreamWaitEvent(s, sd.join, 0));
  return MPG_OK;
}

// Host buffers above the latency path's sizes (mpg_hostpipe.h): per chunk,
// the rows are copied from the caller's (pageable) buffer on the ring's copy
// stream by the feeder thread; the compute stream waits for them, runs the
// collide pipeline into the slot's device outputs, packs the colliding
// configurations' mask rows straight into pinned host memory and copies the
// flags back; the issuing thread unpacks a finished chunk into the caller's
// buffers while the next chunks are in flight.  PCIe carries the rows in
// (8 * row B per configuration) and 1 + 4W B per colliding configuration
// back instead of 1 + 4W B per configuration.  Caller holds host_mu.
template <bool FROM_POSES>
struct HostPipeOps {
  mpg_world* w;
  const double* q;
  uint8_t* flags;
  uint32_t* pair_mask;
  hipStream_t s;
  size_t row;
  // the first error text of the feeder / issuer threads (g_last_error is per
  // thread); finish() runs on the caller's thread and sets g_last_error itself
  std::mutex err_mu;
  std::string thread_err;
  bool fin_failed = false;

  int thread_fail(int rc, const std::string& msg) {
    std::lock_guard<std::mutex> lk(err_mu);
    if (thread_err.empty()) thread_err = msg;
    return rc;
  }
  int bind_thread() {
    if (hipSetDevice(w->device) != hipSuccess) return thread_fail(MPG_E_HIP, "hipSetDevice failed in a pipeline thread");
    return MPG_OK;
  }
  double t_in = 0, t_issue = 0, t_wait = 0, t_unpack = 0;
  static double us_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  }
  int h2d(int64_t, int j, int64_t start, int64_t m) {
    auto& R = w->ring;
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipSuccess;
    if (row) e = hipMemcpyAsync(R.slot[j].d_in.get(), q + (size_t)start * row, sizeof(double) * (size_t)m * row,
                                hipMemcpyHostToDevice, R.h2d.get());
    if (e == hipSuccess) e = hipEventRecord(R.e_in[j].get(), R.h2d.get());
    t_in += us_since(t0);
    if (e != hipSuccess) return thread_fail(MPG_E_HIP, std::string("host pipeline input copy failed: ") + hipGetErrorString(e));
    return MPG_OK;
  }
  int issue(int64_t k, int j, int64_t start, int64_t m) {
    const int rc = issue_chunk(k, j, start, m);
    return rc ? thread_fail(rc, g_last_error) : MPG_OK;  // g_last_error of this (issuer) thread
  }
  int issue_chunk(int64_t k, int j, int64_t, int64_t m) {
    auto& R = w->ring;
    const auto t0 = std::chrono::steady_clock::now();
    const hipStream_t cs = (w->ring_streams > 1 && (k & 1)) ? R.side.get() : s;
    HIP_TRY(hipStreamWaitEvent(cs, R.e_in[j].get(), 0));
    const auto& S = R.slot[j];
    uint8_t* const d_fl = S.d_fl.get();
    uint32_t *const d_mk = S.d_mk.get(), *const d_bcnt = S.d_bcnt.get();
    const int rc = launch_collide<FROM_POSES>(w, S.d_in.get(), m, d_fl, d_mk, cs);
    if (rc) return rc;
    // results straight into pinned host memory: the flags, and with masks the
    // block counts and the packed rows (no copy launches)
    const int Wp = pair_mask ? w->dw.W : 0;
    const unsigned nb = (unsigned)((m + kPackCfg - 1) / kPackCfg);
    if (Wp > 0) {
      hipLaunchKernelGGL(flag_count_kernel, dim3(nb), dim3(256), 0, cs, d_fl, (long long)m, d_bcnt, S.h_bcnt.dev());
      HIP_TRY(hipGetLastError());
    }
    const size_t lds = sizeof(uint32_t) * 256 * (size_t)Wp;
    if (lds <= 64 * 1024)
      hipLaunchKernelGGL(mask_pack_kernel<true>, dim3(nb), dim3(256), lds, cs, d_fl, d_mk, (long long)m, Wp, d_bcnt,
                         S.h_mk.dev(), S.h_fl.dev());
    else
      hipLaunchKernelGGL(mask_pack_kernel<false>, dim3(nb), dim3(256), 0, cs, d_fl, d_mk, (long long)m, Wp, d_bcnt,
                         S.h_mk.dev(), S.h_fl.dev());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(R.e_done[j].get(), cs));
    t_issue += us_since(t0);
    return MPG_OK;
  }
  int finish(int64_t, int j, int64_t start, int64_t m) {
    auto& R = w->ring;
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = hipEventSynchronize(R.e_done[j].get());
    if (e != hipSuccess) {
      fin_failed = true;
      return set_error(MPG_E_HIP, std::string("host pipeline: ") + hipGetErrorString(e));
    }
    const auto t1 = std::chrono::steady_clock::now();
    t_wait += std::chrono::duration<double, std::micro>(t1 - t0).count();
    const auto& S = R.slot[j];
    mpg_hostpipe::unpack_chunk(w->pool.get(), S.h_fl.get(), S.h_mk.get(), S.h_bcnt.get(), kPackCfg, m, w->dw.W,
                               flags + start,
                               pair_mask && w->dw.W > 0 ? pair_mask + (size_t)start * w->dw.W : nullptr);
    t_unpack += us_since(t1);
    return MPG_OK;
  }
  void drain() {
    hipStreamSynchronize(w->ring.h2d.get());
    hipStreamSynchronize(w->ring.side.get());
    hipStreamSynchronize(s);
  }
};

template <bool FROM_POSES>
int collide_host_pipelined(mpg_world* w, const double* q, int64_t n, uint8_t* flags, uint32_t* pair_mask,
                           hipStream_t s) {
  const mpg_hostpipe::Plan p =
      mpg_hostpipe::plan(n, w->ring_chunk, 1 << 15, mpg_world::kRing, w->ring_head, w->ring_tail);
  const size_t row = FROM_POSES ? (size_t)w->dw.n_links * 7 : (size_t)w->dw.dof;
  int rc = ensure_ring(w, (size_t)p.chunk, row);
  if (rc) return rc;
  if (!w->pool && w->host_threads > 1 && p.chunk >= 2 * kPackCfg)
    w->pool.reset(new mpg_hostpipe::Pool(w->host_threads - 1));
  HostPipeOps<FROM_POSES> ops{w, q, flags, pair_mask, s, row};
  const auto t0 = std::chrono::steady_clock::now();
  rc = mpg_hostpipe::run(p, n, ops);
  if (w->srv_stats) {
    const double v[6] = {1.0, ops.t_in, ops.t_issue, ops.t_wait, ops.t_unpack, HostPipeOps<FROM_POSES>::us_since(t0)};
    for (int k = 0; k < 6; ++k) w->hp_stat[k] += v[k];
  }
  if (rc && !ops.fin_failed) return set_error(rc, ops.thread_err);
  return rc;
}

int collide_free(mpg_world* w, const double* q, const double* free_pose, int64_t free_rows, int64_t n, uint8_t* flags,
                 uint32_t* pair_mask, int mem, void* stream);
// mpg_args_host.h's reasons as the entry points report them
int bad_mem(int mem) { return mpg_args::mem_ok(mem) ? MPG_OK : set_error(MPG_E_INVALID, "bad mem kind"); }
int pose_fault(mpg_args::PoseFault f, const char* what) {
  return f ? set_error(MPG_E_INVALID, mpg_args::pose_message(f, what)) : MPG_OK;
}
// host-memory poses ("free pose", "goal pose"): finite values, unit quaternions within kFreeQuatTol
int check_poses(const double* p7, size_t count, const char* what) {
  return pose_fault(mpg_args::check_pose7(p7, count, kFreeQuatTol), what);
}
// host-memory link-pose rows: the free frames' columns are checked as every host-memory free pose is
int check_free_columns(const mpg_world* w, const double* rows, int64_t n) {
  return pose_fault(mpg_args::check_free_columns(rows, n, w->dw.n_links, w->dw.n_free, kFreeQuatTol), "free pose");
}
int check_free_args(const mpg_world* w, const double* free_pose, int64_t free_rows, int64_t n) {
  const char* why = mpg_args::check_free_args(free_pose, free_rows, n, w->dw.n_free);
  return why ? set_error(MPG_E_INVALID, why) : MPG_OK;
}

template <bool FROM_POSES>
int collide_common(mpg_world* w, const double* q, int64_t n, uint8_t* flags, uint32_t* pair_mask, int mem,
                   void* stream) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  // joint-value rows of a world with free frames: at its current poses
  if (!FROM_POSES && w->dw.n_free) return collide_free(w, q, nullptr, 0, n, flags, pair_mask, mem, stream);
  if (n < 0) return set_error(MPG_E_INVALID, "n < 0");
  const size_t row = FROM_POSES ? (size_t)w->dw.n_links * 7 : (size_t)w->dw.dof;
  // a world without inputs (dof 0) may pass q = NULL
  if (n > 0 && ((!q && row > 0) || !flags)) return set_error(MPG_E_INVALID, "input/flags is NULL");
  if (FROM_POSES && mem == MPG_MEM_HOST)
    if (const int rc = check_free_columns(w, q, n)) return rc;
  HIP_TRY(hipSetDevice(w->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mem == MPG_MEM_DEVICE) return launch_collide_overlapped<FROM_POSES>(w, q, n, flags, pair_mask, s);
  if (const int rc = bad_mem(mem)) return rc;
  std::lock_guard<std::mutex> lk(w->host_mu);
  if (!s && w->own_stream) s = w->own_stream.get();
  if (n == 0) return MPG_OK;
  if (n <= w->small_max) return collide_small<FROM_POSES>(w, q, n, flags, pair_mask, s);
  return collide_host_pipelined<FROM_POSES>(w, q, n, flags, pair_mask, s);
}

// ---------------------------------------------------------------------------
// Worlds with free frames.  Every pair evaluation of such a world runs on
// link-pose rows: fk_free_kernel writes the kinematic links' poses from q and
// copies the free frames' poses next to them (per row, shared, or the world's
// current ones), then the link-pose instances of the cull / narrow / small
// kernels evaluate the rows.  Device calls keep the rows in the caller
// stream's workspace and read the caller's pose array directly: no state in
// the world, no synchronisation.  Worlds without free frames never come here.
// ---------------------------------------------------------------------------
constexpr long long kFreeChunk = 1 << 18;  // rows per pass: n_links * 56 B each

// device buffers; free_pose NULL = current poses; free_stride in doubles.
// row_of (with free_pose and a stride): row i takes pose set row_of[i], not i;
// each pass reads the map from its own first row on, and the pose array from
// its start (the map holds indices into the whole array).
int launch_collide_free(mpg_world* w, const double* q, const double* free_pose, long long free_stride, long long n,
                        uint8_t* flags, uint32_t* masks, hipStream_t s, const ContactOut* co = nullptr,
                        const int32_t* row_of = nullptr) {
  if (n == 0) return MPG_OK;
  StreamPin pin(w, s);
  const long long chunk = std::min<long long>(n, std::min<long long>(kFreeChunk, w->max_chunk));
  mpg_world::Workspace* ws = nullptr;
  int rc = get_workspace(w, s, chunk, &ws);
  if (rc) return rc;
  const size_t lrow = (size_t)w->dw.n_links * 7;
  if (ws->links_cap < chunk) {
    if (ws->links.get()) HIP_TRY(hipStreamSynchronize(s));  // this stream's queued work may still read the old rows
    ws->links_cap = 0;
    HIP_TRY(ws->links.reserve(lrow * (size_t)chunk));
    ws->links_cap = chunk;
  }
  double* const links = ws->links.get();
  const size_t P = (size_t)w->dw.n_pairs;
  for (long long off = 0; off < n; off += chunk) {
    const long long m = std::min(chunk, n - off);
    const double* qoff = q ? q + (size_t)off * w->dw.dof : nullptr;
    if (row_of && free_pose)
      hipLaunchKernelGGL(fk_free_kernel<true>, dim3((unsigned)((m + 127) / 128)), dim3(128), 0, s, w->dw, qoff, m,
                         links, free_pose, free_stride, row_of + off);
    else
      hipLaunchKernelGGL(fk_free_kernel<false>, dim3((unsigned)((m + 127) / 128)), dim3(128), 0, s, w->dw, qoff, m,
                         links, free_pose ? free_pose + (size_t)off * free_stride : nullptr, free_stride,
                         (const int32_t*)nullptr);
    HIP_TRY(hipGetLastError());
    ContactOut sub{};
    if (co) sub = ContactOut{co->depth + off * P, co->normal + off * P * 3, co->pos + off * P * 3};
    rc = launch_collide<true>(w, links, m, flags + off, masks ? masks + (size_t)off * w->dw.W : nullptr, s,
                              co ? &sub : nullptr);
    if (rc) return rc;
  }
  return MPG_OK;
}

// link-pose rows of n configurations: fk_kernel, or with free frames fk_free_kernel at free_pose (NULL: the
// current poses; free_stride doubles per row).  (After launch_collide_free, where fk_free_kernel is first
// used: the order of first uses is the order of the kernels in the code object.)
int launch_fk(mpg_world* w, const double* q, long long n, double* out, hipStream_t s, const double* free_pose = nullptr,
              long long free_stride = 0) {
  const unsigned grid = (unsigned)((n + 127) / 128);
  if (n && w->dw.n_free)
    hipLaunchKernelGGL(fk_free_kernel<false>, dim3(grid), dim3(128), 0, s, w->dw, q, n, out, free_pose, free_stride,
                       (const int32_t*)nullptr);
  else if (n)
    hipLaunchKernelGGL(fk_kernel, dim3(grid), dim3(128), 0, s, w->dw, q, n, out);
  HIP_TRY(hipGetLastError());
  return MPG_OK;
}

// joint-value rows on the device, evaluated at the world's current free poses
int launch_collide_q(mpg_world* w, const double* q, long long n, uint8_t* flags, uint32_t* masks, hipStream_t s,
                     const ContactOut* co = nullptr) {
  if (w->dw.n_free) return launch_collide_free(w, q, nullptr, 0, n, flags, masks, s, co);
  return launch_collide<false>(w, q, n, flags, masks, s, co);
}

// host buffers: rows staged to the device in passes of kFreeChunk; batches up
// to the latency path's size take its one-launch kernel on the assembled rows
int collide_free_host(mpg_world* w, const double* q, const double* free_pose, long long free_rows, int64_t n,
                      uint8_t* flags, uint32_t* pair_mask, hipStream_t s) {
  auto& F = w->free_stage;
  const size_t dof = (size_t)w->dw.dof, frow = (size_t)w->dw.n_free * 7, lrow = (size_t)w->dw.n_links * 7;
  const size_t W = (size_t)w->dw.W;
  const long long chunk = std::min<long long>(n, kFreeChunk);
  HostStage st{s, "free-frame collide"};
  st.out(F.q, std::max<size_t>(1, dof * chunk));
  st.out(F.fp, frow * (free_rows > 1 ? chunk : 1));
  double* const d_links = st.out(F.links, lrow * chunk);
  // the latency kernel reads all n rows at once: only a batch that one pass
  // assembles (small_batch_max may be set above kFreeChunk)
  const bool small = n <= w->small_max && n <= chunk;
  uint8_t* const d_fl = small ? nullptr : st.out(F.fl, (size_t)chunk);
  uint32_t* const d_mk = small ? nullptr : st.out(F.mk, W * chunk);
  const double* d_fp = free_pose && free_rows == 1 ? st.in(F.fp, free_pose, frow) : nullptr;
  for (long long off = 0; off < n; off += chunk) {
    const long long m = std::min<long long>(chunk, n - off);
    const double* d_q = st.in(F.q, q + off * dof, dof * m);
    if (free_pose && free_rows > 1) d_fp = st.in(F.fp, free_pose + off * frow, frow * m);
    if (st.rc) return st.rc;
    int rc = launch_fk(w, d_q, m, d_links, s, d_fp, free_rows > 1 ? (long long)frow : 0ll);
    if (rc) return rc;
    if (small) return collide_small<true>(w, nullptr, n, flags, pair_mask, s, d_links);
    rc = launch_collide<true>(w, d_links, m, d_fl, pair_mask ? d_mk : nullptr, s);
    if (rc) return rc;
    st.back(flags + off, d_fl, (size_t)m);
    if (pair_mask) st.back(pair_mask + off * W, d_mk, W * m);
    if (st.finish()) return st.rc;
  }
  return MPG_OK;
}

int collide_free(mpg_world* w, const double* q, const double* free_pose, int64_t free_rows, int64_t n, uint8_t* flags,
                 uint32_t* pair_mask, int mem, void* stream) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  if (n < 0) return set_error(MPG_E_INVALID, "n < 0");
  if (n > 0 && ((!q && w->dw.dof > 0) || !flags)) return set_error(MPG_E_INVALID, "input/flags is NULL");
  if (const int rc = bad_mem(mem)) return rc;
  if (const int rc = check_free_args(w, free_pose, free_rows, n)) return rc;
  if (w->dw.n_free == 0) return collide_common<false>(w, q, n, flags, pair_mask, mem, stream);
  HIP_TRY(hipSetDevice(w->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long fstride = free_rows > 1 ? (long long)w->dw.n_free * 7 : 0ll;
  if (mem == MPG_MEM_DEVICE) return launch_collide_free(w, q, free_pose, fstride, n, flags, pair_mask, s);
  if (free_pose)
    if (const int rc = check_poses(free_pose, (size_t)free_rows * w->dw.n_free, "free pose")) return rc;
  std::lock_guard<std::mutex> lk(w->host_mu);
  if (!s && w->own_stream) s = w->own_stream.get();
  if (n == 0) return MPG_OK;
  return collide_free_host(w, q, free_pose, free_rows, n, flags, pair_mask, s);
}

// The shards of a multi-world call, a thread per world (shard 0 on the
// caller's): shard(k) returns its code with the error text set on its thread;
// the first failure is reported as "world k: ...".
template <class F>
int run_shards(int n_worlds, F&& shard) {
  std::vector<int> rc(n_worlds, MPG_OK);
  std::vector<std::string> err(n_worlds);
  auto run = [&](int k) {
    rc[k] = shard(k);
    if (rc[k]) err[k] = g_last_error;  // the worker thread's error text
  };
  std::vector<std::thread> th;
  for (int k = 1; k < n_worlds; ++k) th.emplace_back(run, k);
  run(0);
  for (auto& t : th) t.join();
  for (int k = 0; k < n_worlds; ++k)
    if (rc[k]) return set_error(rc[k], "world " + std::to_string(k) + ": " + err[k]);
  return MPG_OK;
}
