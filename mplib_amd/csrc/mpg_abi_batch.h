// mpg_abi_batch.h -- C entry points of include/mpgpu.h: the batch calls
// (collide, distance, contacts, FK, motion, sampling) and the debug entries
// (included by mpg_kernels.hip inside extern "C", after mpg_collide_host.h).
#pragma once

int mpg_release_stream(mpg_world* w, void* stream) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  HIP_TRY(hipSetDevice(w->device));
  std::lock_guard<std::mutex> lk(w->ws_mu);
  const auto b = w->busy.find(static_cast<hipStream_t>(stream));
  if (b != w->busy.end() && b->second > 0) return set_error(MPG_E_INVALID, "stream has a call in progress");
  release_stream_locked(w, static_cast<hipStream_t>(stream));
  return MPG_OK;
}

int mpg_set_small_batch_max(mpg_world* w, int64_t n) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  if (n < 0) return set_error(MPG_E_INVALID, "n < 0");
  std::lock_guard<std::mutex> lk(w->host_mu);
  w->small_max = n;
  return MPG_OK;
}

int mpg_collide_batch(mpg_world* w, const double* q, int64_t n, uint8_t* flags, uint32_t* pair_mask, int mem,
                      void* stream) {
  return collide_common<false>(w, q, n, flags, pair_mask, mem, stream);
}

// the worlds of a multi-world call: none NULL or listed twice, all built from world 0's descriptor
static int check_worlds(mpg_world* const* worlds, int32_t n_worlds) {
  for (int k = 0; k < n_worlds; ++k) {
    const mpg_world *wk = worlds[k], *w0 = worlds[0];
    if (!wk) return set_error(MPG_E_INVALID, "world " + std::to_string(k) + " is NULL");
    if (wk->dw.dof != w0->dw.dof || wk->dw.n_pairs != w0->dw.n_pairs || wk->dw.W != w0->dw.W ||
        wk->dw.n_links != w0->dw.n_links || wk->blob_bytes != w0->blob_bytes || wk->snapshot_hash != w0->snapshot_hash)
      return set_error(MPG_E_INVALID, "world " + std::to_string(k) + " was not built from world 0's descriptor");
    for (int j = 0; j < k; ++j)
      if (worlds[j] == wk) return set_error(MPG_E_INVALID, "a world is listed twice");
  }
  return MPG_OK;
}

int mpg_collide_batch_multi(mpg_world* const* worlds, int32_t n_worlds, const double* q, int64_t n, uint8_t* flags,
                            uint32_t* pair_mask) {
  if (n_worlds <= 0 || !worlds) return set_error(MPG_E_INVALID, "no worlds");
  if (n < 0) return set_error(MPG_E_INVALID, "n < 0");
  if (n > 0 && (!q || !flags)) return set_error(MPG_E_INVALID, "q / flags is NULL");
  if (const int rc = check_worlds(worlds, n_worlds)) return rc;
  const size_t dof = worlds[0]->dw.dof, W = worlds[0]->dw.W;
  return run_shards(n_worlds, [&](int k) -> int {
    int64_t start = 0, count = 0;
    mpg_shard_range(n, k, n_worlds, &start, &count);
    if (count == 0) return MPG_OK;
    return mpg_collide_batch(worlds[k], q + start * dof, count, flags + start,
                             pair_mask ? pair_mask + start * W : nullptr, MPG_MEM_HOST, nullptr);
  });
}

int mpg_shard_range(int64_t n, int32_t k, int32_t n_parts, int64_t* start, int64_t* count) {
  if (n < 0 || n_parts <= 0 || k < 0 || k >= n_parts || !start || !count)
    return set_error(MPG_E_INVALID, "mpg_shard_range: bad arguments");
  // contiguous shards, the first n % n_parts one row longer (mplib_amd.dist.shard_range)
  const int64_t base = n / n_parts, rem = n % n_parts;
  *start = k * base + std::min<int64_t>(k, rem);
  *count = base + (k < rem ? 1 : 0);
  return MPG_OK;
}

int mpg_collide_batch_multi_device(mpg_world* const* worlds, int32_t n_worlds, const double* const* q,
                                   const int64_t* counts, uint8_t* const* flags, uint32_t* const* pair_mask,
                                   void* const* streams, uint8_t* gather_flags, uint32_t* gather_masks) {
  if (n_worlds <= 0 || !worlds) return set_error(MPG_E_INVALID, "no worlds");
  if (!counts || !q || !flags) return set_error(MPG_E_INVALID, "counts / q / flags array is NULL");
  if (gather_masks && !pair_mask) return set_error(MPG_E_INVALID, "gather_masks needs pair_mask");
  if (const int rc = check_worlds(worlds, n_worlds)) return rc;
  const mpg_world* w0 = worlds[0];
  for (int k = 0; k < n_worlds; ++k) {
    if (counts[k] < 0) return set_error(MPG_E_INVALID, "counts[" + std::to_string(k) + "] < 0");
    if (counts[k] > 0 && ((!q[k] && w0->dw.dof > 0) || !flags[k]))
      return set_error(MPG_E_INVALID, "shard " + std::to_string(k) + ": q / flags is NULL");
    if (counts[k] > 0 && gather_masks && !pair_mask[k])
      return set_error(MPG_E_INVALID, "shard " + std::to_string(k) + ": gather_masks needs its pair_mask");
  }
  const int W = w0->dw.W;
  std::vector<int64_t> off(n_worlds + 1, 0);
  for (int k = 0; k < n_worlds; ++k) off[k + 1] = off[k] + counts[k];
  const bool gather = gather_flags || gather_masks;
  if (gather) {  // direct peer copies over xGMI from every other device into device 0
    HIP_TRY(hipSetDevice(w0->device));
    for (int k = 1; k < n_worlds; ++k) {
      if (worlds[k]->device == w0->device) continue;
      int can = 0;
      HIP_TRY(hipDeviceCanAccessPeer(&can, w0->device, worlds[k]->device));
      if (!can) continue;  // hipMemcpyPeerAsync still works, staged by the runtime
      const hipError_t e = hipDeviceEnablePeerAccess(worlds[k]->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
        return set_error(MPG_E_HIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
      (void)hipGetLastError();
    }
  }
  const int rc = run_shards(n_worlds, [&](int k) -> int {
    mpg_world* w = worlds[k];
    hipStream_t s = streams ? static_cast<hipStream_t>(streams[k]) : nullptr;
    uint32_t* mk = pair_mask ? pair_mask[k] : nullptr;
    if (hipSetDevice(w->device) != hipSuccess) return set_error(MPG_E_HIP, "hipSetDevice failed");
    if (counts[k] > 0) {
      const int r = mpg_collide_batch(w, q[k], counts[k], flags[k], mk, MPG_MEM_DEVICE, s);
      if (r) return r;
    }
    if (!gather) return MPG_OK;
    hipError_t e = hipSuccess;
    if (counts[k] > 0 && gather_flags)
      e = hipMemcpyPeerAsync(gather_flags + off[k], w0->device, flags[k], w->device, (size_t)counts[k], s);
    if (e == hipSuccess && counts[k] > 0 && gather_masks)
      e = hipMemcpyPeerAsync(gather_masks + off[k] * W, w0->device, mk, w->device,
                             sizeof(uint32_t) * (size_t)counts[k] * W, s);
    if (e == hipSuccess && k > 0) {
      if (!w->gather_ev) e = w->gather_ev.create(hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventRecord(w->gather_ev.get(), s);
    }
    if (e != hipSuccess) return set_error(MPG_E_HIP, std::string("gather: ") + hipGetErrorString(e));
    return MPG_OK;
  });
  if (rc) return rc;
  if (gather) {  // streams[0] orders after every shard's copies
    HIP_TRY(hipSetDevice(w0->device));
    hipStream_t s0 = streams ? static_cast<hipStream_t>(streams[0]) : nullptr;
    for (int k = 1; k < n_worlds; ++k) HIP_TRY(hipStreamWaitEvent(s0, worlds[k]->gather_ev.get(), 0));
  }
  return MPG_OK;
}

int mpg_collide_link_poses(mpg_world* w, const double* link_pose, int64_t n, uint8_t* flags, uint32_t* pair_mask,
                           int mem, void* stream) {
  return collide_common<true>(w, link_pose, n, flags, pair_mask, mem, stream);
}

int mpg_collide_batch_free(mpg_world* w, const double* q, const double* free_pose, int64_t free_rows, int64_t n,
                           uint8_t* flags, uint32_t* pair_mask, int mem, void* stream) {
  return collide_free(w, q, free_pose, free_rows, n, flags, pair_mask, mem, stream);
}

int mpg_world_set_free_poses(mpg_world* w, const double* pose7) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  if (w->dw.n_free == 0) return set_error(MPG_E_INVALID, "the world has no free frames");
  if (!pose7) return set_error(MPG_E_INVALID, "pose7 is NULL");
  if (const int rc = check_poses(pose7, (size_t)w->dw.n_free, "free pose")) return rc;
  HIP_TRY(hipSetDevice(w->device));
  // calls in flight read the buffer: wait for them, then overwrite it in place
  std::lock_guard<std::mutex> lk(w->host_mu);
  HIP_TRY(hipDeviceSynchronize());
  std::copy(pose7, pose7 + w->free_host.size(), w->free_host.begin());
  HIP_TRY(hipMemcpy(w->free_dev.get(), w->free_host.data(), sizeof(double) * w->free_host.size(), hipMemcpyHostToDevice));
  return MPG_OK;
}

int mpg_world_get_free_info(const mpg_world* w, int32_t* n_free, double* far_radius, double* pose7) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  if (n_free) *n_free = w->dw.n_free;
  if (far_radius) *far_radius = w->dw.far_r;
  if (pose7) std::copy(w->free_host.begin(), w->free_host.end(), pose7);
  return MPG_OK;
}

int mpg_check_motion_batch(mpg_world* w, const double* q_from, const double* q_to, int64_t n, uint32_t so2_mask,
                           double longest_valid_segment, uint8_t* valid, int32_t* first_invalid, int32_t* segments,
                           int mem, void* stream) {
  return mpg_check_motion_batch_free(w, q_from, q_to, nullptr, 0, n, so2_mask, longest_valid_segment, valid,
                                     first_invalid, segments, mem, stream);
}

int mpg_check_motion_batch_free(mpg_world* w, const double* q_from, const double* q_to, const double* free_pose,
                                int64_t free_rows, int64_t n, uint32_t so2_mask, double longest_valid_segment,
                                uint8_t* valid, int32_t* first_invalid, int32_t* segments, int mem, void* stream) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  if (n < 0) return set_error(MPG_E_INVALID, "n < 0");
  if (n > 0 && (!q_from || !q_to || !valid)) return set_error(MPG_E_INVALID, "from/to/valid is NULL");
  if (!(longest_valid_segment > 0.0)) return set_error(MPG_E_INVALID, "longest_valid_segment must be > 0");
  if (const int mrc = bad_mem(mem)) return mrc;
  if (const int frc = check_free_args(w, free_pose, free_rows, n)) return frc;
  if (w->dw.dof > 32) return set_error(MPG_E_UNSUPPORTED, "motion validation supports dof <= 32");
  if (n == 0) return MPG_OK;
  const bool per_edge = free_pose && free_rows > 1;  // free_rows == n: the row map holds int32 edge indices
  if (per_edge && n > (int64_t)INT32_MAX)
    return set_error(MPG_E_UNSUPPORTED, "per-edge free poses support at most 2^31 - 1 edges");
  if (free_pose && mem == MPG_MEM_HOST)
    if (const int frc = check_poses(free_pose, (size_t)free_rows * w->dw.n_free, "free pose")) return frc;
  HIP_TRY(hipSetDevice(w->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(w->motion_mu);
  const int dof = w->dw.dof;
  const size_t eb = sizeof(double) * (size_t)n * dof;
  auto& M = w->motion;
  // scratch_grow waits for M.last (the previous call's work) before it replaces a buffer
  auto grow = [&](auto& buf, size_t count) { return scratch_grow(M.last, buf, count); };
  int rc = scratch_begin(M.last, s);
  if (rc) return rc;
  if ((rc = grow(M.edges, 2 * (size_t)n * dof))) return rc;
  if ((rc = grow(M.segs, n))) return rc;
  if ((rc = grow(M.offs, n))) return rc;
  if ((rc = grow(M.out, (sizeof(int32_t) + 1) * n))) return rc;
  double* const d_edges = M.edges.get();
  int32_t* const d_segs = M.segs.get();
  long long* const d_offs = M.offs.get();
  const double* from = q_from;
  const double* to = q_to;
  const double* fp = free_pose;  // device memory: read where the caller keeps it
  const size_t frow = (size_t)w->dw.n_free * 7;
  if (mem == MPG_MEM_HOST) {
    HIP_TRY(hipMemcpyAsync(d_edges, q_from, eb, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_edges + (size_t)n * dof, q_to, eb, hipMemcpyHostToDevice, s));
    from = d_edges;
    to = d_edges + (size_t)n * dof;
    HostStage st{s, "motion", &M.last};
    if (free_pose && !(fp = st.in(M.fp, free_pose, frow * (size_t)free_rows))) return st.rc;
  }
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(motion_count_kernel, dim3(grid), dim3(256), 0, s, from, to, (long long)n, dof, so2_mask,
                     longest_valid_segment, d_segs);
  HIP_TRY(hipGetLastError());
  // the state count decides the allocation: one synchronisation per call
  std::vector<int32_t> segs((size_t)n);
  HIP_TRY(hipMemcpyAsync(segs.data(), d_segs, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  std::vector<long long> offs((size_t)n);
  long long total = 0;
  for (int64_t e = 0; e < n; ++e) {
    offs[e] = total;
    total += segs[e];
  }
  HIP_TRY(hipMemcpyAsync(d_offs, offs.data(), sizeof(long long) * n, hipMemcpyHostToDevice, s));
  if ((rc = grow(M.states, (size_t)total * dof))) return rc;
  if ((rc = grow(M.flags, (size_t)total))) return rc;
  double* const d_states = M.states.get();
  uint8_t* const d_flags = M.flags.get();
  hipLaunchKernelGGL(motion_states_kernel, dim3(grid), dim3(256), 0, s, from, to, (long long)n, dof, so2_mask, d_segs,
                     d_offs, d_states);
  HIP_TRY(hipGetLastError());
  if (per_edge) {  // every sub-state of edge e with edge e's pose set: a map, not total * n_free poses
    if ((rc = grow(M.row_of, (size_t)total))) return rc;
    hipLaunchKernelGGL(motion_rowmap_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_offs,
                       (long long)n, total, M.row_of.get());
    HIP_TRY(hipGetLastError());
    rc = launch_collide_free(w, d_states, fp, (long long)frow, total, d_flags, nullptr, s, nullptr, M.row_of.get());
  } else if (fp) {
    rc = launch_collide_free(w, d_states, fp, 0ll, total, d_flags, nullptr, s);
  } else {
    rc = launch_collide_q(w, d_states, total, d_flags, nullptr, s);
  }
  if (rc) return rc;
  int32_t* const out_first = reinterpret_cast<int32_t*>(M.out.get());  // first_invalid[n], then valid[n] bytes
  uint8_t* d_valid = mem == MPG_MEM_DEVICE ? valid : reinterpret_cast<uint8_t*>(out_first + n);
  int32_t* d_first = first_invalid ? (mem == MPG_MEM_DEVICE ? first_invalid : out_first) : nullptr;
  hipLaunchKernelGGL(motion_reduce_kernel, dim3(grid), dim3(256), 0, s, d_flags, (long long)n, d_segs, d_offs, d_valid,
                     d_first);
  HIP_TRY(hipGetLastError());
  if (mem == MPG_MEM_HOST) {
    HIP_TRY(hipMemcpyAsync(valid, d_valid, n, hipMemcpyDeviceToHost, s));
    if (first_invalid) HIP_TRY(hipMemcpyAsync(first_invalid, d_first, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (segments) std::memcpy(segments, segs.data(), sizeof(int32_t) * n);
  } else if (segments) {
    HIP_TRY(hipMemcpyAsync(segments, d_segs, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, s));
  }
  HIP_TRY(hipEventRecord(M.last.get(), s));
  return MPG_OK;
}

int mpg_distance_batch(mpg_world* w, const double* q, int64_t n, int32_t n_self_pairs, double* d_self,
                       int32_t* p_self, double* d_others, int32_t* p_others, int mem, void* stream) {
  return mpg_distance_batch_ex(w, q, n, n_self_pairs, 0, d_self, p_self, nullptr, d_others, p_others, nullptr, mem,
                               stream);
}

int mpg_distance_batch_ex(mpg_world* w, const double* q, int64_t n, int32_t n_self_pairs, int32_t flags,
                          double* d_self, int32_t* p_self, double* pts_self, double* d_others, int32_t* p_others,
                          double* pts_others, int mem, void* stream) {
  mpg_distance_request req;
  req.flags = flags;
  req.distance_tolerance = 1e-6;
  return mpg_distance_batch_req(w, q, n, n_self_pairs, &req, d_self, p_self, pts_self, d_others, p_others, pts_others,
                                mem, stream);
}

int mpg_distance_batch_req(mpg_world* w, const double* q, int64_t n, int32_t n_self_pairs,
                           const mpg_distance_request* req, double* d_self, int32_t* p_self, double* pts_self,
                           double* d_others, int32_t* p_others, double* pts_others, int mem, void* stream) {
  return mpg_distance_batch_free(w, q, nullptr, 0, n, n_self_pairs, req, d_self, p_self, pts_self, d_others, p_others,
                                 pts_others, mem, stream);
}

int mpg_distance_batch_free(mpg_world* w, const double* q, const double* free_pose, int64_t free_rows, int64_t n,
                            int32_t n_self_pairs, const mpg_distance_request* req, double* d_self, int32_t* p_self,
                            double* pts_self, double* d_others, int32_t* p_others, double* pts_others, int mem,
                            void* stream) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  if (!req) return set_error(MPG_E_INVALID, "request is NULL");
  if (n < 0) return set_error(MPG_E_INVALID, "n < 0");
  if (n_self_pairs < 0 || n_self_pairs > w->dw.n_pairs) return set_error(MPG_E_INVALID, "bad n_self_pairs");
  if (n > 0 && ((!q && w->dw.dof > 0) || !d_self || !p_self || !d_others || !p_others))
    return set_error(MPG_E_INVALID, "NULL buffer");
  if (const int mrc = bad_mem(mem)) return mrc;
  if (const int frc = check_free_args(w, free_pose, free_rows, n)) return frc;
  const int32_t flags = req->flags;
  if (flags & ~(MPG_DISTANCE_SIGNED | MPG_DISTANCE_NEAREST_POINTS | MPG_DISTANCE_GJK_INDEP))
    return set_error(MPG_E_INVALID, "bad flags");
  if (!(req->distance_tolerance >= 0.0)) return set_error(MPG_E_INVALID, "bad distance_tolerance");
  if (w->has_octree2)
    return set_error(MPG_E_UNSUPPORTED, "distance for a pair of two OcTrees (OcTreeDistanceRecurse) is not implemented");
  const bool indep = (flags & MPG_DISTANCE_GJK_INDEP) != 0;
  if (indep && (flags & MPG_DISTANCE_SIGNED))
    return set_error(MPG_E_UNSUPPORTED, "signed distance with GST_INDEP (FCL's EPA) is not implemented");
  if (indep && (w->has_mesh || w->has_octree))
    return set_error(MPG_E_UNSUPPORTED, "distance with GST_INDEP for an OcTree or BVH mesh pair is not implemented");
  const ccd_real tol = (ccd_real)req->distance_tolerance;  // GJKSolver_libccd::distance_tolerance -> ccd.dist_tolerance
  const double dtol = req->distance_tolerance;              // GJKSolver_indep::gjk_tolerance (distance-inl.h)
  const bool want_pts = pts_self || pts_others;
  const int mode = (want_pts || (flags & (MPG_DISTANCE_SIGNED | MPG_DISTANCE_NEAREST_POINTS)) ? MPG_DIST_POINTS : 0) |
                   (flags & MPG_DISTANCE_SIGNED ? MPG_DIST_SIGNED : 0) |
                   (flags & MPG_DISTANCE_NEAREST_POINTS ? MPG_DIST_NP : 0) | (indep ? MPG_DIST_INDEP : 0);
  if (n == 0) return MPG_OK;
  if (free_pose && mem == MPG_MEM_HOST)
    if (const int frc = check_poses(free_pose, (size_t)free_rows * w->dw.n_free, "free pose")) return frc;
  HIP_TRY(hipSetDevice(w->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(w->dist_mu);
  auto& D = w->dist;
  // scratch_grow waits for D.last (the previous call's work) before it replaces a buffer
  auto grow = [&](auto& buf, size_t count) { return scratch_grow(D.last, buf, count); };
  int rc = scratch_begin(D.last, s);
  if (rc) return rc;
  const size_t nm = std::max(w->dw.n_moving, 1), ns = std::max(w->dw.bp.n_saves, 1);
  if ((rc = grow(D.poses, kPoseStride * nm * n))) return rc;
  if ((rc = grow(D.save64, 12 * ns * n))) return rc;
  double *const d_poses = D.poses.get(), *const d_save64 = D.save64.get();
  const double* qin = q;
  double *ds = d_self, *dd = d_others, *qs = pts_self, *qo = pts_others;
  int32_t *ps = p_self, *po = p_others;
  const size_t out_bytes = (2 * sizeof(double) + 2 * sizeof(int32_t) + (mode ? 12 * sizeof(double) : 0)) * n;
  HostStage st{s, "distance", &D.last};  // host buffers: their device twins, replaced as scratch_grow does
  if (mem == MPG_MEM_HOST) {
    st.out(D.q, (size_t)std::max(w->dw.dof, 1) * n);
    ds = reinterpret_cast<double*>(st.out(D.out, out_bytes));
    qin = st.in(D.q, q, (size_t)w->dw.dof * n);
    if (st.rc) return st.rc;
    dd = ds + n;
    qs = dd + n;
    qo = qs + (mode ? 6 * n : 0);
    ps = reinterpret_cast<int32_t*>(qo + (mode ? 6 * n : 0));
    po = ps + n;
  } else if (mode && (!qs || !qo)) {  // device buffers: scratch for the points nobody asked for
    if ((rc = grow(D.pts, 12 * (size_t)n))) return rc;
    if (!qs) qs = D.pts.get();
    if (!qo) qo = D.pts.get() + 6 * n;
  }
  const unsigned grid = (unsigned)((n + 127) / 128);
  if (w->dw.n_free) {  // link-pose rows with the call's or the current free poses, then the objects' transforms
    if ((rc = grow(D.links, (size_t)7 * w->dw.n_links * n))) return rc;
    const size_t frow = (size_t)w->dw.n_free * 7;
    const double* fp = free_pose;  // device memory: read where the caller keeps it
    if (free_pose && mem == MPG_MEM_HOST && !(fp = st.in(D.fp, free_pose, frow * (size_t)free_rows))) return st.rc;
    if ((rc = launch_fk(w, qin, n, D.links.get(), s, fp, free_rows > 1 ? (long long)frow : 0ll))) return rc;
    hipLaunchKernelGGL((pose_kernel<true>), dim3(grid), dim3(128), 0, s, w->dw, D.links.get(), (long long)n, d_poses,
                       d_save64);
  } else {
    hipLaunchKernelGGL((pose_kernel<false>), dim3(grid), dim3(128), 0, s, w->dw, qin, (long long)n, d_poses, d_save64);
  }
  HIP_TRY(hipGetLastError());
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(128), 0, s, w->dw, d_poses, (long long)n, n_self_pairs, tol, dtol, ds,
                       ps, dd, po, qs, qo);
    return hipGetLastError();
  };
  constexpr int P = MPG_DIST_POINTS, SG = MPG_DIST_SIGNED, NPF = MPG_DIST_NP, IN = MPG_DIST_INDEP;
  switch (mode) {
    case 0: HIP_TRY(launch(distance_kernel<0>)); break;
    case P: HIP_TRY(launch(distance_kernel<P>)); break;
    case P | NPF: HIP_TRY(launch(distance_kernel<P | NPF>)); break;
    case P | SG: HIP_TRY(launch(distance_kernel<P | SG>)); break;
    case P | SG | NPF: HIP_TRY(launch(distance_kernel<P | SG | NPF>)); break;
    case IN: HIP_TRY(launch(distance_kernel<IN>)); break;
    case P | IN: HIP_TRY(launch(distance_kernel<P | IN>)); break;
    default: HIP_TRY(launch(distance_kernel<P | NPF | IN>)); break;
  }
  if (mode & SG) {  // EPAs past the private polytope: again with a big one from the pool
    if ((rc = grow(D.big, kBigPool))) return rc;
    if ((rc = grow(D.list, (size_t)n + 1))) return rc;
    HIP_TRY(hipMemsetAsync(D.list.get(), 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(overflow_list_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ps, (long long)n,
                       D.list.get());
    HIP_TRY(hipGetLastError());
    auto redo = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(1), dim3(kBigPool), 0, s, w->dw, d_poses, (long long)n, n_self_pairs, tol, dtol,
                         ds, ps, dd, po, qs, qo, D.big.get(), D.list.get());
      return hipGetLastError();
    };
    if (mode & NPF) HIP_TRY(redo(distance_redo_kernel<P | SG | NPF>));
    else HIP_TRY(redo(distance_redo_kernel<P | SG>));
  }
  HIP_TRY(hipEventRecord(D.last.get(), s));
  if (mem == MPG_MEM_HOST) {
    st.back(d_self, ds, n);
    st.back(d_others, dd, n);
    st.back(p_self, ps, n);
    st.back(p_others, po, n);
    if (mode && pts_self) st.back(pts_self, qs, 6 * n);
    if (mode && pts_others) st.back(pts_others, qo, 6 * n);
    if (st.finish()) return st.rc;
    for (int64_t i = 0; i < n; ++i) {
      if (p_self[i] == MPG_DISTANCE_FCL_THROWS)
        return set_error(MPG_E_FAILED, "configuration " + std::to_string(i) +
                                           ": FCL's libccd EPA throws here (FCL_THROW_FAILED_AT_THIS_CONFIGURATION)");
      if (p_self[i] == MPG_DISTANCE_EPA_CAPACITY)
        return set_error(MPG_E_UNSUPPORTED, "configuration " + std::to_string(i) +
                                                ": EPA polytope beyond the device capacity (" +
                                                std::to_string(ccdx::kBigPtV) + " vertices)");
    }
  }
  return MPG_OK;
}

int mpg_collide_contacts(mpg_world* w, const double* input, int64_t n, int input_kind, uint8_t* flags,
                         uint32_t* pair_mask, double* depth, double* normal, double* pos, int mem, void* stream) {
  return mpg_collide_contacts_free(w, input, nullptr, 0, n, input_kind, flags, pair_mask, depth, normal, pos, mem,
                                   stream);
}

int mpg_collide_contacts_free(mpg_world* w, const double* input, const double* free_pose, int64_t free_rows, int64_t n,
                              int input_kind, uint8_t* flags, uint32_t* pair_mask, double* depth, double* normal,
                              double* pos, int mem, void* stream) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  if (n < 0) return set_error(MPG_E_INVALID, "n < 0");
  if (input_kind != MPG_INPUT_Q && input_kind != MPG_INPUT_LINK_POSES) return set_error(MPG_E_INVALID, "bad input_kind");
  const bool poses = input_kind == MPG_INPUT_LINK_POSES;
  if (poses && free_pose)
    return set_error(MPG_E_INVALID, "link-pose rows carry the free frames' poses: free_pose must be NULL");
  if (const int frc = check_free_args(w, free_pose, free_rows, n)) return frc;
  const size_t row = poses ? (size_t)w->dw.n_links * 7 : (size_t)w->dw.dof;
  if (n > 0 && ((!input && row > 0) || !flags || !pair_mask || !depth || !normal || !pos))
    return set_error(MPG_E_INVALID, "NULL buffer");
  if (const int mrc = bad_mem(mem)) return mrc;
  if (w->any_gjk)
    return set_error(MPG_E_UNSUPPORTED, "contacts with gjk_solver MPG_GJK_INDEP (FCL's EPA) are not implemented");
  if (w->has_octree2)
    return set_error(MPG_E_UNSUPPORTED, "contacts for a pair of two OcTrees are not implemented");
  if (w->octree_first)  // contact_kernel reports the (shape, octree) order PlanningWorld uses
    return set_error(MPG_E_UNSUPPORTED, "contacts for a pair whose first object is an OcTree are not implemented");
  if (n == 0) return MPG_OK;
  if (poses && mem == MPG_MEM_HOST)
    if (const int crc = check_free_columns(w, input, n)) return crc;
  if (free_pose && mem == MPG_MEM_HOST)
    if (const int frc = check_poses(free_pose, (size_t)free_rows * w->dw.n_free, "free pose")) return frc;
  HIP_TRY(hipSetDevice(w->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t P = (size_t)w->dw.n_pairs, W = (size_t)w->dw.W;
  const size_t frow = (size_t)w->dw.n_free * 7;
  const long long fstride = free_rows > 1 ? (long long)frow : 0ll;
  auto run = [&](const double* in, const double* fp, uint8_t* fl, uint32_t* mk, const ContactOut& co) {  // device buffers
    if (fp) return launch_collide_free(w, in, fp, fstride, n, fl, mk, s, &co);
    return poses ? launch_collide<true>(w, in, n, fl, mk, s, &co) : launch_collide_q(w, in, n, fl, mk, s, &co);
  };
  if (mem == MPG_MEM_DEVICE) return run(input, free_pose, flags, pair_mask, ContactOut{depth, normal, pos});
  std::lock_guard<std::mutex> lk(w->host_mu);
  if (!s && w->own_stream) s = w->own_stream.get();
  auto& C = w->contact;
  HostStage st{s, "contact"};
  st.out(C.in, std::max<size_t>(1, row * n));
  double* const d_out = st.out(C.out, 7 * P * n);
  uint8_t* const d_fl = st.out(C.fl, n);
  uint32_t* const d_mk = st.out(C.mk, W * n);
  const double* const d_fp = free_pose ? st.in(C.fp, free_pose, frow * (size_t)free_rows) : nullptr;
  const double* const d_in = st.in(C.in, input, row * n);
  if (st.rc) return st.rc;
  const ContactOut co{d_out, d_out + P * n, d_out + 4 * P * n};
  if (const int rc = run(d_in, d_fp, d_fl, d_mk, co)) return rc;
  st.back(flags, d_fl, n);
  st.back(pair_mask, d_mk, W * n);
  st.back(depth, co.depth, P * n);
  st.back(normal, co.normal, 3 * P * n);
  st.back(pos, co.pos, 3 * P * n);
  return st.finish();
}

int mpg_fk_batch(mpg_world* w, const double* q, int64_t n, double* link_pose, int mem, void* stream) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  if (n < 0) return set_error(MPG_E_INVALID, "n < 0");
  if (n > 0 && (!q || !link_pose)) return set_error(MPG_E_INVALID, "q/link_pose is NULL");
  HIP_TRY(hipSetDevice(w->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t nout = (size_t)n * w->dw.n_links * 7;
  if (mem == MPG_MEM_DEVICE) return launch_fk(w, q, n, link_pose, s);
  if (const int mrc = bad_mem(mem)) return mrc;
  std::lock_guard<std::mutex> lk(w->host_mu);
  auto& F = w->fk_stage;
  HostStage st{s, "FK"};
  st.out(F.q, std::max<size_t>(1, (size_t)n * std::max(w->dw.dof, 1)));
  double* const d_out = st.out(F.out, std::max<size_t>(nout, 1));
  if (st.rc || n == 0) return st.rc;
  const double* const d_q = st.in(F.q, q, (size_t)n * w->dw.dof);
  if (st.rc) return st.rc;
  if (const int rc = launch_fk(w, d_q, n, d_out, s)) return rc;
  st.back(link_pose, d_out, nout);
  return st.finish();
}

// what mpg_ik_batch and mpg_screw_batch ask of their link
static int check_ik_link(const mpg_world* w, int32_t link) {
  if (link < 0 || link >= w->dw.n_links) return set_error(MPG_E_INVALID, "link index out of range");
  if (link >= w->dw.n_links - w->dw.n_free) return set_error(MPG_E_INVALID, "link is a free frame: no joint moves it");
  return MPG_OK;
}

// device buffers: seeds (q_init NULL), CLIK, limits + threshold, the collide
// pass of the MPG_MEM_DEVICE callers on q_out, its flags folded into status
static int launch_ik(mpg_world* w, const IkView& iv, const double* goal, long long n_goals, long long rpg,
                     const double* q_init, const double* q_start, uint64_t seed, int max_waves, double* q_out,
                     uint8_t* status, double* err, int32_t* iters, hipStream_t s) {
  const long long rows = n_goals * rpg;
  const int dof = w->dw.dof;
  StreamPin pin(w, s);
  mpg_world::IkWork* K = nullptr;
  {
    std::lock_guard<std::mutex> lk(w->ws_mu);
    K = &w->ik_ws[s];
  }
  if (K->flags.get() && K->flags.cap() < (size_t)rows) HIP_TRY(hipStreamSynchronize(s));  // queued work may still read it
  HIP_TRY(K->flags.reserve((size_t)rows));
  HIP_TRY(K->counter.reserve(1));
  HIP_TRY(hipMemsetAsync(K->counter.get(), 0, sizeof(unsigned long long), s));
  const double* q_in = q_init;
  if (!q_init) {
    const long long tot = rows * dof;
    hipLaunchKernelGGL(ik_seed_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, iv, dof, rows, rpg, seed,
                       q_start, q_out);
    HIP_TRY(hipGetLastError());
    q_in = q_out;
  }
  // one wave per block; the grid: the waves the LDS lets be resident, fewer for small batches
  const size_t lds = mpg_args::ik_lds_bytes(iv.cl);
  const long long resident = (long long)w->ik.cus * std::max<long long>(1, std::min<long long>(8, (160 * 1024) / lds));
  long long waves = std::min<long long>((rows + 63) / 64, resident);
  if (max_waves > 0) waves = std::min<long long>(waves, max_waves);
  hipLaunchKernelGGL(ik_clik_kernel, dim3((unsigned)waves), dim3(64), lds, s, w->dw, iv, goal, rows, rpg, q_in, q_out,
                     status, err, iters, K->counter.get());
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ik_finish_kernel, dim3((unsigned)((rows + 127) / 128)), dim3(128), 0, s, w->dw, iv, goal, rows,
                     rpg, q_out, status);
  HIP_TRY(hipGetLastError());
  const int rc = mpg_collide_batch(w, q_out, rows, K->flags.get(), nullptr, MPG_MEM_DEVICE, s);
  if (rc) return rc;
  hipLaunchKernelGGL(ik_fold_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, K->flags.get(), rows,
                     status);
  HIP_TRY(hipGetLastError());
  return MPG_OK;
}

int mpg_ik_batch(mpg_world* w, int32_t link, const double* goal_pose, int64_t n_goals, int64_t rows_per_goal,
                 const double* q_init, const double* q_start, const mpg_ik_options* opt, double* q_out,
                 uint8_t* status, double* err, int32_t* iters, int mem, void* stream) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  if (n_goals < 0 || rows_per_goal < 0) return set_error(MPG_E_INVALID, "n_goals / rows_per_goal < 0");
  if (const int mrc = bad_mem(mem)) return mrc;
  const auto& T = w->ik;
  if (const int lrc = check_ik_link(w, link)) return lrc;
  if (!q_init && !q_start) return set_error(MPG_E_INVALID, "q_init and q_start are both NULL");
  mpg_ik_options o{1e-5, 1000, 0.1, 1e-12, 1e-3, nullptr, 0, 0};
  if (opt) o = *opt;
  if (o.max_iter < 0 || o.max_iter > 100000) return set_error(MPG_E_INVALID, "max_iter outside [0, 100000]");
  if (o.max_waves < 0) return set_error(MPG_E_INVALID, "max_waves < 0");
  const int dof = w->dw.dof;
  if (dof > kIkDof) return set_error(MPG_E_UNSUPPORTED, "mpg_ik_batch supports dof <= 32");
  if (T.chain_len[link] > kIkChain) return set_error(MPG_E_UNSUPPORTED, "mpg_ik_batch supports at most 15 joints above the link");
  if (n_goals > (int64_t)1 << 40 || rows_per_goal > (int64_t)1 << 20 || n_goals * rows_per_goal > (int64_t)1 << 40)
    return set_error(MPG_E_UNSUPPORTED, "mpg_ik_batch supports at most 2^40 rows");
  IkView iv{};
  mpg_args::fill_ik_view(iv, T, link, dof, o.mask);
  iv.max_iter = o.max_iter;
  iv.eps = o.eps;
  iv.dt = o.dt;
  iv.damp = o.damp;
  iv.threshold = o.threshold;
  constexpr double kPi = 3.14159265358979323846;
  for (int d = 0; d < dof; ++d) {
    if (T.continuous[d]) iv.lo[d] = -kPi, iv.hi[d] = kPi;  // its sampling range
    if (!q_init && !iv.frozen[d] && !T.continuous[d] && !iv.bounded[d])
      return set_error(MPG_E_INVALID, "dof slot " + std::to_string(d) +
                                          ": a joint with neither finite limits nor a continuous type cannot be sampled");
  }
  const int64_t rows = n_goals * rows_per_goal;
  if (rows > 0 && (!goal_pose || !q_out || !status)) return set_error(MPG_E_INVALID, "goal_pose / q_out / status is NULL");
  if (mem == MPG_MEM_HOST && rows > 0) {
    if (const int prc = check_poses(goal_pose, (size_t)n_goals, "goal pose")) return prc;
    if (q_init && !finite_all(q_init, (size_t)rows * dof)) return set_error(MPG_E_INVALID, "non-finite q_init");
    if (q_start && !finite_all(q_start, (size_t)dof)) return set_error(MPG_E_INVALID, "non-finite q_start");
  }
  if (rows == 0) return MPG_OK;
  HIP_TRY(hipSetDevice(w->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mem == MPG_MEM_DEVICE)
    return launch_ik(w, iv, goal_pose, n_goals, rows_per_goal, q_init, q_start, o.seed, o.max_waves, q_out, status, err,
                     iters, s);
  std::lock_guard<std::mutex> lk(w->host_mu);
  if (!s && w->own_stream) s = w->own_stream.get();
  auto& S = w->ik_stage;
  const size_t nq = (size_t)rows * dof;
  HostStage st{s, "IK"};
  st.out(S.goal, 7 * (size_t)n_goals);
  double* const d_q = st.out(S.q, (size_t)rows * std::max(dof, 1));
  st.out(S.start, std::max(dof, 1));
  double* const d_err = st.out(S.err, 6 * (size_t)rows);
  uint8_t* const d_status = st.out(S.status, (size_t)rows);
  int32_t* const d_iters = st.out(S.iters, (size_t)rows);
  const double* const d_goal = st.in(S.goal, goal_pose, 7 * (size_t)n_goals);
  if (q_init) st.in(S.q, q_init, nq);
  const double* const d_start = q_start ? st.in(S.start, q_start, (size_t)dof) : nullptr;
  if (st.rc) return st.rc;
  const int rc = launch_ik(w, iv, d_goal, n_goals, rows_per_goal, q_init ? d_q : nullptr, d_start, o.seed, o.max_waves,
                           d_q, d_status, d_err, d_iters, s);
  if (rc) return rc;
  st.back(q_out, d_q, nq);
  st.back(status, d_status, (size_t)rows);
  if (err) st.back(err, d_err, 6 * (size_t)rows);
  if (iters) st.back(iters, d_iters, (size_t)rows);
  return st.finish();
}

// device buffers: every row integrated by screw_kernel, one collide pass over
// the padded path, its flags folded into status / first_hit
static int launch_screw(mpg_world* w, const ScrewView& sv, const double* goal, const double* q_start, long long rows,
                        double* path, int32_t* n_waypoints, uint8_t* status, int32_t* first_hit, hipStream_t s) {
  const long long cfgs = rows * sv.max_waypoints;
  StreamPin pin(w, s);
  mpg_world::ScrewWork* K = nullptr;
  {
    std::lock_guard<std::mutex> lk(w->ws_mu);
    K = &w->screw_ws[s];
  }
  if (K->flags.get() && K->flags.cap() < (size_t)cfgs) HIP_TRY(hipStreamSynchronize(s));  // queued work may still read it
  HIP_TRY(K->flags.reserve((size_t)cfgs));
  // one wave per block, a lane per row
  hipLaunchKernelGGL(screw_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), mpg_args::ik_lds_bytes(sv.iv.cl), s,
                     w->dw, sv, goal, q_start, rows, path, n_waypoints, status);
  HIP_TRY(hipGetLastError());
  const int rc = mpg_collide_batch(w, path, cfgs, K->flags.get(), nullptr, MPG_MEM_DEVICE, s);
  if (rc) return rc;
  hipLaunchKernelGGL(screw_fold_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, K->flags.get(),
                     n_waypoints, rows, sv.max_waypoints, status, first_hit);
  HIP_TRY(hipGetLastError());
  return MPG_OK;
}

int mpg_screw_batch(mpg_world* w, int32_t link, const double* goal, const double* q_start, int64_t rows,
                    const mpg_screw_options* opt, double* path, int32_t* n_waypoints, uint8_t* status,
                    int32_t* first_hit, int mem, void* stream) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  if (rows < 0) return set_error(MPG_E_INVALID, "rows < 0");
  if (const int mrc = bad_mem(mem)) return mrc;
  const auto& T = w->ik;
  if (const int lrc = check_ik_link(w, link)) return lrc;
  mpg_screw_options o{0.1, 64};
  if (opt) o = *opt;
  if (!(o.qpos_step > 0) || !std::isfinite(o.qpos_step)) return set_error(MPG_E_INVALID, "qpos_step must be > 0");
  if (o.max_waypoints < 2 || o.max_waypoints > 4096) return set_error(MPG_E_INVALID, "max_waypoints outside [2, 4096]");
  if (rows > ((int64_t)1 << 31) / o.max_waypoints)
    return set_error(MPG_E_INVALID, "rows * max_waypoints exceeds 2^31");
  const int dof = w->dw.dof;
  if (dof > kIkDof) return set_error(MPG_E_UNSUPPORTED, "mpg_screw_batch supports dof <= 32");
  if (T.chain_len[link] > kIkChain)
    return set_error(MPG_E_UNSUPPORTED, "mpg_screw_batch supports at most 15 joints above the link");
  ScrewView sv{};
  const IkView& iv = sv.iv;
  mpg_args::fill_ik_view(sv.iv, T, link, dof, nullptr);
  sv.qpos_step = o.qpos_step;
  sv.max_waypoints = o.max_waypoints;
  for (int d = 0; d < dof; ++d) sv.offchain[d] = 1;
  int moving = 0;
  for (int k = 0; k < iv.cl; ++k) {
    const int src = T.joint_q_source[T.chain_joints[iv.cs + k] - 1];
    if (src >= 0 && src < dof) {
      sv.offchain[src] = 0;
      ++moving;
    }
  }
  if (moving < 6)
    return set_error(MPG_E_UNSUPPORTED,
                     "mpg_screw_batch needs at least six joints with a dof slot above the link (J J^T is singular)");
  if (rows > 0 && (!goal || !q_start || !path || !n_waypoints || !status))
    return set_error(MPG_E_INVALID, "goal / q_start / path / n_waypoints / status is NULL");
  if (mem == MPG_MEM_HOST && rows > 0) {
    if (const int prc = check_poses(goal, (size_t)rows, "goal pose")) return prc;
    if (!finite_all(q_start, (size_t)rows * dof)) return set_error(MPG_E_INVALID, "non-finite q_start");
  }
  if (rows == 0) return MPG_OK;
  HIP_TRY(hipSetDevice(w->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mem == MPG_MEM_DEVICE) return launch_screw(w, sv, goal, q_start, rows, path, n_waypoints, status, first_hit, s);
  std::lock_guard<std::mutex> lk(w->host_mu);
  if (!s && w->own_stream) s = w->own_stream.get();
  auto& S = w->screw_stage;
  const size_t nq = (size_t)rows * dof, cap_q = (size_t)rows * std::max(dof, 1);
  HostStage st{s, "screw"};
  st.out(S.goal, 7 * (size_t)rows);
  st.out(S.start, cap_q);
  double* const d_path = st.out(S.path, cap_q * (size_t)o.max_waypoints);
  uint8_t* const d_status = st.out(S.status, (size_t)rows);
  int32_t* const d_count = st.out(S.count, (size_t)rows);
  int32_t* const d_hit = st.out(S.first_hit, (size_t)rows);
  const double* const d_goal = st.in(S.goal, goal, 7 * (size_t)rows);
  const double* const d_start = st.in(S.start, q_start, nq);
  if (st.rc) return st.rc;
  const int rc = launch_screw(w, sv, d_goal, d_start, rows, d_path, d_count, d_status, first_hit ? d_hit : nullptr, s);
  if (rc) return rc;
  st.back(path, d_path, nq * (size_t)o.max_waypoints);
  st.back(n_waypoints, d_count, (size_t)rows);
  st.back(status, d_status, (size_t)rows);
  if (first_hit) st.back(first_hit, d_hit, (size_t)rows);
  return st.finish();
}

// what launch_plan queues on s: the roots and the first collide pass, then the
// rounds -- propose, one collide pass over every row's slot block, commit -- as
// plain launches, then the paths of the rows that connected.  Every
// check_every rounds the host reads the count of rows that have not ended (one
// synchronise) and stops at 0.
static int plan_rounds(mpg_world* w, const RrtView& v, const RrtBufs& b, const double* start, const double* goal,
                       long long Q, const uint64_t* row_seed, uint64_t seed, int check_every, double* path,
                       int32_t* n_waypoints, uint8_t* status, int32_t* iterations, int32_t* tree_sizes, hipStream_t s) {
  const size_t q = (size_t)Q;
  const long long first = 1 + v.goals, per_round = v.block;
  HIP_TRY(hipMemsetAsync(b.active, 0, sizeof(int32_t), s));
  const long long vals = Q * first * v.dof;
  if (vals > 0) {
    hipLaunchKernelGGL(rrt_gather_kernel, dim3((unsigned)((vals + 255) / 256)), dim3(256), 0, s, v, Q, start, goal,
                       b.slots);
    HIP_TRY(hipGetLastError());
  }
  if (const int rc = mpg_collide_batch(w, b.slots, Q * first, b.flags, nullptr, MPG_MEM_DEVICE, s)) return rc;
  const unsigned row_blocks = (unsigned)((Q + 63) / 64);
  hipLaunchKernelGGL(rrt_init_kernel, dim3(row_blocks), dim3(64), 0, s, v, Q, start, goal, row_seed, seed, b,
                     n_waypoints, status);
  HIP_TRY(hipGetLastError());
  const long long fill = Q * (per_round + v.max_waypoints) * v.dof;
  if (fill > 0) {
    hipLaunchKernelGGL(rrt_fill_kernel, dim3((unsigned)std::min<long long>((fill + 255) / 256, 1 << 20)), dim3(256), 0,
                       s, v, Q, start, b.slots, path);
    HIP_TRY(hipGetLastError());
  }
  int32_t active = 1;
  for (int round = 0; round < v.max_rounds && active > 0; ++round) {
    hipLaunchKernelGGL(rrt_propose_kernel, dim3((unsigned)Q), dim3(256), 0, s, v, b);
    HIP_TRY(hipGetLastError());
    if (const int rc = mpg_collide_batch(w, b.slots, Q * per_round, b.flags, nullptr, MPG_MEM_DEVICE, s)) return rc;
    hipLaunchKernelGGL(rrt_commit_kernel, dim3(row_blocks), dim3(64), 0, s, v, Q, round, b, status);
    HIP_TRY(hipGetLastError());
    if ((round + 1) % check_every == 0) {
      HIP_TRY(hipMemcpyAsync(&active, b.active, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
    }
  }
  hipLaunchKernelGGL(rrt_path_kernel, dim3((unsigned)Q), dim3(64), 0, s, v, b, path, n_waypoints, status);
  HIP_TRY(hipGetLastError());
  if (iterations) HIP_TRY(hipMemcpyAsync(iterations, b.iter, sizeof(int32_t) * q, hipMemcpyDeviceToDevice, s));
  if (tree_sizes) HIP_TRY(hipMemcpyAsync(tree_sizes, b.sizes, sizeof(int32_t) * 2 * q, hipMemcpyDeviceToDevice, s));
  return MPG_OK;
}

// device buffers: the stream's workspace, the rounds, and one synchronise at
// the end -- after a failure too -- so the workspace is idle when the call
// returns and the next call may replace its buffers.
static int launch_plan(mpg_world* w, const RrtView& v, const double* start, const double* goal, long long Q,
                       const uint64_t* row_seed, uint64_t seed, int check_every, double* path, int32_t* n_waypoints,
                       uint8_t* status, int32_t* iterations, int32_t* tree_sizes, hipStream_t s) {
  StreamPin pin(w, s);
  mpg_world::PlanWork* K = nullptr;
  {
    std::lock_guard<std::mutex> lk(w->ws_mu);
    K = &w->plan_ws[s];
  }
  const size_t dof = (size_t)std::max(v.dof, 1), q = (size_t)Q;
  const size_t slot_rows = q * (size_t)std::max(1 + v.goals, v.block);
  HIP_TRY(K->nodes.reserve(q * 2 * v.max_nodes * dof));
  HIP_TRY(K->parent.reserve(q * 2 * v.max_nodes));
  HIP_TRY(K->newstate.reserve(q * dof));
  HIP_TRY(K->slots.reserve(slot_rows * dof));
  HIP_TRY(K->flags.reserve(slot_rows));
  HIP_TRY(K->sizes.reserve(2 * q));
  HIP_TRY(K->phase.reserve(q));
  HIP_TRY(K->added.reserve(q));
  HIP_TRY(K->iter.reserve(q));
  HIP_TRY(K->prop.reserve(RRT_P_INTS * q));
  HIP_TRY(K->seeds.reserve(q));
  HIP_TRY(K->active.reserve(1));
  const RrtBufs b{K->nodes.get(), K->parent.get(), K->sizes.get(), K->phase.get(),  K->added.get(), K->iter.get(),
                  K->prop.get(),  K->newstate.get(), K->seeds.get(), K->slots.get(), K->flags.get(), K->active.get()};
  const int rc = plan_rounds(w, v, b, start, goal, Q, row_seed, seed, check_every, path, n_waypoints, status, iterations,
                             tree_sizes, s);
  const hipError_t e = hipStreamSynchronize(s);
  if (rc) return rc;
  HIP_TRY(e);
  return MPG_OK;
}

int mpg_plan_batch(mpg_world* w, const double* start, const double* goal, int64_t Q, int32_t G,
                   const uint64_t* row_seed, const mpg_plan_options* opt, double* path, int32_t* n_waypoints,
                   uint8_t* status, int32_t* iterations, int32_t* tree_sizes, int mem, void* stream) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  if (const int mrc = bad_mem(mem)) return mrc;
  mpg_plan_options o{0.0, 20000, 2048, 256, 8, 0, 0};
  if (opt) o = *opt;
  const int dof = w->dw.dof;
  RrtView v{};
  bool unsupported = false;
  const std::string why = mpg_args::fill_rrt_view(v, o, w->ik.lo.data(), w->ik.hi.data(), dof, Q, G, &unsupported);
  if (!why.empty()) return set_error(unsupported ? MPG_E_UNSUPPORTED : MPG_E_INVALID, why);
  if (Q > 0 && (!start || !goal || !path || !n_waypoints || !status))
    return set_error(MPG_E_INVALID, "start / goal / path / n_waypoints / status is NULL");
  if (mem == MPG_MEM_HOST && Q > 0) {
    if (!finite_all(start, (size_t)Q * dof)) return set_error(MPG_E_INVALID, "non-finite start");
    if (!finite_all(goal, (size_t)Q * G * dof)) return set_error(MPG_E_INVALID, "non-finite goal");
  }
  if (Q == 0) return MPG_OK;
  HIP_TRY(hipSetDevice(w->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mem == MPG_MEM_DEVICE)
    return launch_plan(w, v, start, goal, Q, row_seed, o.seed, o.check_every, path, n_waypoints, status, iterations,
                       tree_sizes, s);
  std::lock_guard<std::mutex> lk(w->host_mu);
  if (!s && w->own_stream) s = w->own_stream.get();
  auto& S = w->plan_stage;
  const size_t q = (size_t)Q, nq = q * dof, cap_q = q * std::max(dof, 1);
  HostStage st{s, "plan"};
  st.out(S.start, cap_q);
  st.out(S.goal, cap_q * (size_t)G);
  double* const d_path = st.out(S.path, cap_q * (size_t)o.max_waypoints);
  uint8_t* const d_status = st.out(S.status, q);
  int32_t* const d_count = st.out(S.count, q);
  int32_t* const d_iters = st.out(S.iters, q);
  int32_t* const d_sizes = st.out(S.sizes, 2 * q);
  const double* const d_start = st.in(S.start, start, nq);
  const double* const d_goal = st.in(S.goal, goal, nq * (size_t)G);
  const uint64_t* const d_seed = row_seed ? st.in(S.row_seed, row_seed, q) : nullptr;
  if (st.rc) return st.rc;
  const int rc = launch_plan(w, v, d_start, d_goal, Q, d_seed, o.seed, o.check_every, d_path, d_count, d_status,
                             iterations ? d_iters : nullptr, tree_sizes ? d_sizes : nullptr, s);
  if (rc) return rc;
  st.back(path, d_path, nq * (size_t)o.max_waypoints);
  st.back(n_waypoints, d_count, q);
  st.back(status, d_status, q);
  if (iterations) st.back(iterations, d_iters, q);
  if (tree_sizes) st.back(tree_sizes, d_sizes, 2 * q);
  return st.finish();
}

// device buffers: every row's profile by topp_row_kernel into the stream's
// workspace (x and t straight into grid_x / grid_t where the caller asks for
// them), then the samples.  Launches only; the stream is waited for just where
// a workspace buffer must grow under queued work.
static int launch_topp(mpg_world* w, const ToppView& v, const double* path, const int32_t* n_waypoints, long long rows,
                       double* times, double* position, double* velocity, double* acceleration, int32_t* n_samples,
                       double* duration, uint8_t* status, double* grid_x, double* grid_t, hipStream_t s) {
  StreamPin pin(w, s);
  mpg_world::ToppWork* K = nullptr;
  {
    std::lock_guard<std::mutex> lk(w->ws_mu);
    K = &w->topp_ws[s];
  }
  const size_t nm = (size_t)rows * v.max_waypoints * std::max(v.dof, 1), ng = (size_t)rows * ((size_t)v.ncap + 1);
  const auto grows = [](const DevBuf<double>& b, size_t n) { return b.get() && b.cap() < n; };
  if (grows(K->M, nm) || grows(K->K, ng) || (!grid_x && grows(K->x, ng)) || (!grid_t && grows(K->t, ng)))
    HIP_TRY(hipStreamSynchronize(s));  // queued work may still use it
  HIP_TRY(K->M.reserve(nm));
  HIP_TRY(K->K.reserve(ng));
  if (!grid_x) HIP_TRY(K->x.reserve(ng));
  if (!grid_t) HIP_TRY(K->t.reserve(ng));
  double* const xs = grid_x ? grid_x : K->x.get();
  double* const ts = grid_t ? grid_t : K->t.get();
  hipLaunchKernelGGL(topp_row_kernel, dim3((unsigned)rows), dim3(64), 0, s, v, path, n_waypoints, K->M.get(),
                     K->K.get(), xs, ts, n_samples, duration, status);
  HIP_TRY(hipGetLastError());
  const long long slots = rows * v.max_samples;
  hipLaunchKernelGGL(topp_sample_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, v, path, n_waypoints,
                     rows, K->M.get(), xs, ts, n_samples, duration, times, position, velocity, acceleration);
  HIP_TRY(hipGetLastError());
  return MPG_OK;
}

int mpg_topp_batch(mpg_world* w, const double* path, const int32_t* n_waypoints, int64_t rows, int32_t max_waypoints,
                   const double* vel_limits, const double* acc_limits, const mpg_topp_options* opt, double* times,
                   double* position, double* velocity, double* acceleration, int32_t* n_samples, double* duration,
                   uint8_t* status, double* grid_x, double* grid_t, int mem, void* stream) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  if (const int mrc = bad_mem(mem)) return mrc;
  mpg_topp_options o{0.1, 8, 100, 256};
  if (opt) o = *opt;
  const int dof = w->dw.dof;
  ToppView v{};
  bool unsupported = false;
  const std::string why =
      mpg_args::fill_topp_view(v, o, dof, rows, max_waypoints, vel_limits, acc_limits, &unsupported);
  if (!why.empty()) return set_error(unsupported ? MPG_E_UNSUPPORTED : MPG_E_INVALID, why);
  if (rows > 0 && (!n_waypoints || !times || !n_samples || !duration || !status ||
                   (dof > 0 && (!path || !position || !velocity || !acceleration))))
    return set_error(MPG_E_INVALID,
                     "path / n_waypoints / times / position / velocity / acceleration / n_samples / duration / status "
                     "is NULL");
  if (mem == MPG_MEM_HOST && rows > 0) {
    const std::string bad = mpg_args::check_topp_rows(path, n_waypoints, rows, max_waypoints, dof);
    if (!bad.empty()) return set_error(MPG_E_INVALID, bad);
  }
  if (rows == 0) return MPG_OK;
  HIP_TRY(hipSetDevice(w->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mem == MPG_MEM_DEVICE)
    return launch_topp(w, v, path, n_waypoints, rows, times, position, velocity, acceleration, n_samples, duration,
                       status, grid_x, grid_t, s);
  std::lock_guard<std::mutex> lk(w->host_mu);
  if (!s && w->own_stream) s = w->own_stream.get();
  auto& S = w->topp_stage;
  const size_t r = (size_t)rows, d1 = (size_t)std::max(dof, 1);
  const size_t np = r * max_waypoints * dof, ns = r * o.max_samples, nsd = ns * dof, ng = r * ((size_t)v.ncap + 1);
  HostStage st{s, "TOPP"};
  st.out(S.path, r * max_waypoints * d1);
  double* const d_times = st.out(S.times, ns);
  double* const d_samples = st.out(S.samples, 3 * ns * d1);
  double* const d_dur = st.out(S.dur, r);
  double* const d_grid = st.out(S.grid, (grid_x ? ng : 0) + (grid_t ? ng : 0));
  int32_t* const d_ns = st.out(S.n_samples, r);
  uint8_t* const d_status = st.out(S.status, r);
  const double* const d_path = st.in(S.path, path, np);
  const int32_t* const d_count = st.in(S.count, n_waypoints, r);
  if (st.rc) return st.rc;
  double* const d_gx = grid_x ? d_grid : nullptr;
  double* const d_gt = grid_t ? d_grid + (grid_x ? ng : 0) : nullptr;
  const int rc = launch_topp(w, v, d_path, d_count, rows, d_times, d_samples, d_samples + nsd, d_samples + 2 * nsd, d_ns,
                             d_dur, d_status, d_gx, d_gt, s);
  if (rc) return rc;
  st.back(times, d_times, ns);
  st.back(position, d_samples, nsd);
  st.back(velocity, d_samples + nsd, nsd);
  st.back(acceleration, d_samples + 2 * nsd, nsd);
  st.back(n_samples, d_ns, r);
  st.back(duration, d_dur, r);
  st.back(status, d_status, r);
  if (grid_x) st.back(grid_x, d_gx, ng);
  if (grid_t) st.back(grid_t, d_gt, ng);
  return st.finish();
}

int mpg_debug_collide_pairs(mpg_world* w, int32_t geom_a, int32_t geom_b, int64_t n, const double* Ta,
                            const double* Tb, uint8_t* hit) {
  if (!w || n < 0 || (n > 0 && (!Ta || !Tb || !hit))) return set_error(MPG_E_INVALID, "bad arguments");
  if (geom_a < 0 || geom_b < 0 || geom_a >= w->n_geoms || geom_b >= w->n_geoms)
    return set_error(MPG_E_INVALID, "geometry index out of range");
  if (n == 0) return MPG_OK;
  const int ta = w->geom_type_h[geom_a], tb = w->geom_type_h[geom_b];
  int cf = CF_NONE;
  if (ta == MPG_GEOM_MESH || tb == MPG_GEOM_MESH) cf = CF_MESH;
  else if (ta == MPG_GEOM_OCTREE || tb == MPG_GEOM_OCTREE) cf = CF_OCTREE;
  else if (ta == MPG_GEOM_BOX && tb == MPG_GEOM_BOX) cf = CF_BOX_BOX;
  else if (ta == MPG_GEOM_SPHERE && tb == MPG_GEOM_SPHERE) cf = CF_SPHERE_SPHERE;
  else if (ta == MPG_GEOM_SPHERE && tb == MPG_GEOM_BOX) cf = CF_SPHERE_BOX;
  else if (ta == MPG_GEOM_BOX && tb == MPG_GEOM_SPHERE) cf = CF_BOX_SPHERE;
  else if (ta == MPG_GEOM_SPHERE && tb == MPG_GEOM_CAPSULE) cf = CF_SPHERE_CAPSULE;
  else if (ta == MPG_GEOM_CAPSULE && tb == MPG_GEOM_SPHERE) cf = CF_CAPSULE_SPHERE;
  else if (ta == MPG_GEOM_SPHERE && tb == MPG_GEOM_CYLINDER) cf = CF_SPHERE_CYLINDER;
  else if (ta == MPG_GEOM_CYLINDER && tb == MPG_GEOM_SPHERE) cf = CF_CYLINDER_SPHERE;
  if ((cf == CF_OCTREE && ta == tb) || (cf == CF_MESH && (ta == MPG_GEOM_OCTREE || tb == MPG_GEOM_OCTREE)))
    return set_error(MPG_E_UNSUPPORTED, "geometry pair not supported");
  HIP_TRY(hipSetDevice(w->device));
  // every exit path frees the buffers, then the private stream (a failing
  // path's queued work is waited for when the device memory is freed, which synchronises the device)
  Stream st;
  DevBuf<double> dA, dB;
  DevBuf<uint8_t> dh;
  HIP_TRY(st.create(hipStreamNonBlocking));
  HIP_TRY(dA.reserve(12 * (size_t)n));
  HIP_TRY(dB.reserve(12 * (size_t)n));
  HIP_TRY(dh.reserve((size_t)n));
  HIP_TRY(hipMemcpyAsync(dA.get(), Ta, sizeof(double) * 12 * n, hipMemcpyHostToDevice, st.get()));
  HIP_TRY(hipMemcpyAsync(dB.get(), Tb, sizeof(double) * 12 * n, hipMemcpyHostToDevice, st.get()));
  // (walk_wave_eval finds the octree / mesh argument itself)
  hipLaunchKernelGGL(debug_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st.get(), w->dw, geom_a,
                     geom_b, cf, (long long)n, dA.get(), dB.get(), dh.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(hit, dh.get(), (size_t)n, hipMemcpyDeviceToHost, st.get()));
  HIP_TRY(hipStreamSynchronize(st.get()));
  return MPG_OK;
}

int mpg_debug_task_plan(mpg_world* w, void* stream, int64_t* tasks, int32_t* task_size, int32_t* levels,
                        int64_t* candidates) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  HIP_TRY(hipSetDevice(w->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t* tail = nullptr;
  {
    std::lock_guard<std::mutex> lk(w->ws_mu);
    auto it = w->ws.find(s);
    if (it == w->ws.end() && !s && w->own_stream) it = w->ws.find(s = w->own_stream.get());  // host-buffer calls
    if (it == w->ws.end() || !it->second.prefix.get())
      return set_error(MPG_E_INVALID, "the stream has no workspace: no bulk collide call has run on it");
    tail = it->second.prefix.get() + std::max(w->dw.n_pairs, 0);
  }
  HIP_TRY(hipStreamSynchronize(s));
  uint32_t h[kPrefixTail];
  HIP_TRY(hipMemcpy(h, tail, sizeof(h), hipMemcpyDeviceToHost));
  if (tasks) *tasks = h[0];
  if (task_size) *task_size = (int32_t)h[2];
  if (candidates) *candidates = h[3];
  if (levels) *levels = (int32_t)bk_plan_load(h + 4).n;
  return MPG_OK;
}

int mpg_sample_uniform(const double* lower, const double* upper, int32_t dof, int64_t n, uint64_t seed,
                       int64_t row_offset, double* q, int device) {
  if (dof < 0 || dof > kSampleMaxDof) return set_error(MPG_E_INVALID, "dof out of range [0, 64]");
  if (n < 0 || row_offset < 0 || (n > 0 && dof > 0 && (!lower || !upper || !q)))
    return set_error(MPG_E_INVALID, "bad arguments");
  if (n == 0 || dof == 0) return MPG_OK;
  SampleRange r{};
  if (const char* why = mpg_args::fill_sample_range(r, lower, upper, dof)) return set_error(MPG_E_INVALID, why);
  HIP_TRY(hipSetDevice(device));
  DevBuf<double> d;
  HIP_TRY(d.reserve((size_t)n * dof));
  const long long tot = (long long)n * dof;
  hipLaunchKernelGGL(sample_uniform_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, 0, r, (int)dof,
                     (long long)n, seed, (long long)row_offset, d.get());
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(q, d.get(), sizeof(double) * (size_t)tot, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return set_error(MPG_E_HIP, std::string("mpg_sample_uniform: ") + hipGetErrorString(e));
  return MPG_OK;
}

int mpg_collide_count(mpg_world* w, const double* lower, const double* upper, int64_t n, uint64_t seed,
                      int64_t* counts, void* stream) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  const int dof = w->dw.dof, P = w->dw.n_pairs, W = w->dw.W;
  if (dof > kSampleMaxDof) return set_error(MPG_E_UNSUPPORTED, "mpg_collide_count supports dof <= 64");
  if (n < 0 || (P > 0 && !counts) || (dof > 0 && (!lower || !upper))) return set_error(MPG_E_INVALID, "bad arguments");
  if ((size_t)P * sizeof(uint32_t) > 64 * 1024) return set_error(MPG_E_UNSUPPORTED, "mpg_collide_count supports <= 16384 pairs");
  for (int p = 0; p < P; ++p) counts[p] = 0;
  if (n == 0 || P == 0) return MPG_OK;
  SampleRange r{};
  if (const char* why = mpg_args::fill_sample_range(r, lower, upper, dof)) return set_error(MPG_E_INVALID, why);
  HIP_TRY(hipSetDevice(w->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long chunk = std::min<long long>(n, w->max_chunk);
  // freed on every exit path (freeing device memory synchronises the device: a failing path's queued work is done)
  DevBuf<double> bq;
  DevBuf<uint8_t> bfl;
  DevBuf<uint32_t> bmk;
  DevBuf<unsigned long long> bcnt;
  HIP_TRY(bq.reserve((size_t)chunk * std::max(dof, 1)));
  HIP_TRY(bfl.reserve((size_t)chunk));
  HIP_TRY(bmk.reserve((size_t)chunk * W));
  HIP_TRY(bcnt.reserve(P));
  HIP_TRY(hipMemsetAsync(bcnt.get(), 0, sizeof(unsigned long long) * P, s));
  for (long long off = 0; off < n; off += chunk) {
    const long long m = std::min(chunk, n - off);
    if (dof > 0) {
      const long long tot = m * dof;
      hipLaunchKernelGGL(sample_uniform_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, r, dof, m, seed,
                         off, bq.get());
      HIP_TRY(hipGetLastError());
    }
    const int rc = w->dw.n_free ? launch_collide_q(w, bq.get(), m, bfl.get(), bmk.get(), s)
                                : launch_collide_overlapped<false>(w, bq.get(), m, bfl.get(), bmk.get(), s);
    if (rc) return rc;
    const unsigned grid = (unsigned)std::min<long long>(1024, (m + 255) / 256);
    hipLaunchKernelGGL(pair_count_kernel, dim3(grid), dim3(256), sizeof(uint32_t) * P, s, bmk.get(), m, W, P,
                       bcnt.get());
    HIP_TRY(hipGetLastError());
  }
  std::vector<unsigned long long> h(P);
  HIP_TRY(hipMemcpyAsync(h.data(), bcnt.get(), sizeof(unsigned long long) * P, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int p = 0; p < P; ++p) counts[p] = (int64_t)h[p];
  return MPG_OK;
}

int mpg_debug_sincos(const double* x, int64_t n, double* s, double* c, int device) {
  if (n < 0 || (n > 0 && (!x || !s || !c))) return set_error(MPG_E_INVALID, "bad arguments");
  if (n == 0) return MPG_OK;
  HIP_TRY(hipSetDevice(device));
  DevBuf<double> dx, ds, dc;
  HIP_TRY(dx.reserve(n));
  HIP_TRY(ds.reserve(n));
  HIP_TRY(dc.reserve(n));
  HIP_TRY(hipMemcpy(dx.get(), x, sizeof(double) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(sincos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx.get(), (long long)n,
                     ds.get(), dc.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(s, ds.get(), sizeof(double) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(c, dc.get(), sizeof(double) * n, hipMemcpyDeviceToHost));
  return MPG_OK;
}
