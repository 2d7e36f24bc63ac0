// mpg_abi_world.h -- C entry points of include/mpgpu.h: errors, the BVH build,
// profiles, world creation, destruction and info (included by
// mpg_kernels.hip inside extern "C", after mpg_streams_host.h).
#pragma once

const char* mpg_last_error(void) { return g_last_error.c_str(); }

int mpg_fcl_bvh_build(const double* vertices, int32_t n_vertices, const int32_t* triangles, int32_t n_triangles,
                      double* boxes, int32_t* links, int32_t* leaf_order) {
  if (n_triangles <= 0 || !vertices || !triangles || !boxes || !links || !leaf_order)
    return set_error(MPG_E_INVALID, "mpg_fcl_bvh_build: empty mesh or NULL buffer");
  for (int64_t i = 0; i < 3 * (int64_t)n_triangles; ++i)
    if (triangles[i] < 0 || triangles[i] >= n_vertices) return set_error(MPG_E_INVALID, "triangle vertex out of range");
  FclBvh B;
  B.box.resize(FB_STRIDE);
  B.link.resize(3);
  std::vector<int> prim((size_t)n_triangles);
  for (int t = 0; t < n_triangles; ++t) prim[t] = t;
  fcl_bvh_node(B, vertices, triangles, prim, 0, 0, n_triangles, 0);
  std::copy(B.box.begin(), B.box.end(), boxes);
  std::copy(B.link.begin(), B.link.end(), links);
  std::copy(prim.begin(), prim.end(), leaf_order);
  return (int)(B.link.size() / 3);
}

int mpg_last_error_copy(char* buf, size_t size) {
  const size_t len = g_last_error.size();
  if (buf && size > 0) {
    const size_t k = std::min(len, size - 1);
    std::memcpy(buf, g_last_error.data(), k);
    buf[k] = '\0';
  }
  return (int)std::min<size_t>(len, 0x7fffffff);
}

const char* mpg_version(void) { return "mpgpu 0.3 (gfx950, fp64, libccd-MPR)"; }

int mpg_device_count(int* count) {
  if (!count) return set_error(MPG_E_INVALID, "count is NULL");
  HIP_TRY(hipGetDeviceCount(count));
  return MPG_OK;
}

int mpg_profile_enable(mpg_world* w, int enable) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  HIP_TRY(hipSetDevice(w->device));
  std::lock_guard<std::mutex> lk(w->prof_mu);
  if (enable && !w->prof_units.get()) {
    HIP_TRY(w->prof_units.reserve(1));
    HIP_TRY(hipMemset(w->prof_units.get(), 0, sizeof(unsigned long long)));
  }
  w->prof = enable != 0;
  return MPG_OK;
}

int mpg_profile_read(mpg_world* w, double* ms, int64_t* launches, int64_t* units, int n_stages) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  HIP_TRY(hipSetDevice(w->device));
  std::lock_guard<std::mutex> lk(w->prof_mu);
  unsigned long long cand = 0;
  if (w->prof_units.get()) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&cand, w->prof_units.get(), sizeof(cand), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(w->prof_units.get(), 0, sizeof(cand)));
  }
  const int64_t u[MPG_NUM_STAGES] = {w->prof_cfg, w->prof_cfg, (int64_t)cand};
  w->prof_cfg = 0;
  for (auto& mk : w->marks) {
    HIP_TRY(hipEventSynchronize(mk.b.get()));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, mk.a.get(), mk.b.get()));
    w->prof_ms[mk.stage] += t;
    w->prof_n[mk.stage] += 1;
  }
  for (auto& mk : w->marks) {  // the events go back to the pool once all are read
    w->ev_pool.push_back(std::move(mk.a));
    w->ev_pool.push_back(std::move(mk.b));
  }
  w->marks.clear();
  for (int k = 0; k < MPG_NUM_STAGES; ++k) {
    if (k < n_stages) {
      if (ms) ms[k] = w->prof_ms[k];
      if (launches) launches[k] = w->prof_n[k];
      if (units) units[k] = u[k];
    }
    w->prof_ms[k] = 0.0;
    w->prof_n[k] = 0;
  }
  return MPG_OK;
}

int mpg_latency_server_stats(mpg_world* w, int64_t* served, int64_t* starts, int64_t* fallbacks, int32_t* state) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  if (served) *served = w->srv_served;
  if (starts) *starts = w->srv_starts;
  if (fallbacks) *fallbacks = w->srv_fallbacks;
  if (state) *state = !(w->srv_mode && w->srv_ok) ? 0 : w->srv_broken ? 2 : 1;
  return MPG_OK;
}

int mpg_cull_grid_info(const mpg_world* w, int32_t* objects, int64_t* cells, int32_t* built, double* cell_edge,
                       int32_t cap, int32_t* object, int32_t* partners, double* box) {
  if (!w) return set_error(MPG_E_INVALID, "world is NULL");
  const mpg_world::GridInfo& g = w->grid_info;
  if (objects) *objects = (int32_t)g.object.size();
  if (cells) *cells = g.cells;
  if (built) *built = w->grid_ready.load(std::memory_order_acquire) ? 1 : 0;
  if (cell_edge) *cell_edge = g.h;
  for (int32_t i = 0; i < cap && i < (int32_t)g.object.size(); ++i) {
    if (object) object[i] = g.object[i];
    if (partners) partners[i] = g.partners[i];
    if (box) std::copy(g.box.begin() + 6 * i, g.box.begin() + 6 * i + 6, box + 6 * i);
  }
  return MPG_OK;
}

int mpg_synchronize(int device) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());
  return MPG_OK;
}

int mpg_world_create(const mpg_world_desc* d_in, int device, mpg_world** out) {
  if (!out) return set_error(MPG_E_INVALID, "out is NULL");
  *out = nullptr;
  int rc = validate(d_in);
  if (rc) return rc;
  // free frames: the kinematic build below (chains, broad-phase program,
  // latency records) sees them as links fixed to the universe at their initial
  // pose; what the kernels read for them is the pose input
  mpg_world_desc dd = *d_in;
  std::vector<int32_t> lp_kin(dd.link_parent, dd.link_parent + dd.n_links);
  int n_free = 0;
  for (int32_t& p : lp_kin)
    if (p == MPG_LINK_FREE) {
      p = 0;
      ++n_free;
    }
  if (n_free) dd.link_parent = lp_kin.data();
  const mpg_world_desc* d = &dd;
  std::vector<double> geom_rec((size_t)G_STRIDE * std::max(d->n_geoms, 1), 0.0);
  for (int g = 0; g < d->n_geoms; ++g) geom_record(d, g, geom_rec.data() + (size_t)G_STRIDE * g);
  std::vector<double> obb((size_t)7 * std::max(d->n_geoms, 1), 0.0);
  for (int g = 0; g < d->n_geoms; ++g) {
    const double* r = geom_rec.data() + (size_t)G_STRIDE * g;
    for (int k = 0; k < 3; ++k) obb[7 * g + k] = r[G_OBB_C + k];
    for (int k = 0; k < 3; ++k) obb[7 * g + 3 + k] = r[G_OBB_E + k];
    obb[7 * g + 6] = r[G_RADIUS];
  }
  BpProgram bpp;
  bp_build(d, obb, bpp);
  bp_build_support(d, obb, bpp);
  size_t lds = 0;
  const int W = std::max(1, (d->n_pairs + 31) / 32);
  const int block = choose_block(cull_lds_per_thread(d->n_moving, bpp.n_saves, W), &lds);
  if (block < 0) return set_error(MPG_E_UNSUPPORTED, "world too large for the phase-A LDS budget");
  HIP_TRY(hipSetDevice(device));

  std::vector<double> static_rec((size_t)S_STRIDE * std::max(d->n_static, 1), 0.0);
  for (int s = 0; s < d->n_static; ++s) static_record(d, s, geom_rec.data(), static_rec.data() + (size_t)S_STRIDE * s);
  // hulls in AoSoA-4 groups, padded with copies of the hull's first vertex
  std::vector<int> gstart(std::max(d->n_geoms, 1), 0), ngroups(std::max(d->n_geoms, 1), 0);
  std::vector<double> hull;
  std::vector<int> cbase(std::max(d->n_geoms, 1), -1), geom_nbr(std::max(d->n_geoms, 1), -1), hull_nbr, wcell_end, wcell_end2, wcell_pre;
  std::vector<double> cell_rec, cell_ovf, wcell_rec, wcell_ovf, wcell_aux, nbr_ent;
  const int walk_subk =
      std::getenv("MPG_WALK_SUBK") ? std::max(1, std::min(8, std::atoi(std::getenv("MPG_WALK_SUBK")))) : kSubK;
  int big_words = 0;  // walk hulls above kMaxWalkVerts: the widest visited set
  for (int g = 0; g < d->n_geoms; ++g) {
    if (d->geom_type[g] != MPG_GEOM_CONVEX) continue;
    const double* Vg = d->vertices + 3 * (size_t)d->geom_vertex_start[g];
    const int nvg = d->geom_vertex_count[g];
    // FCL 0.7.0 Convex: neighbour walk for > 32 vertices with valid faces
    std::vector<int> enc;
    const int nf = (int)d->geom_param[4 * g + 1];
    bool walk = nf > 0 && fcl_convex_neighbors(nvg, d->convex_face + (int64_t)d->geom_param[4 * g], nf, enc);
#ifdef MPG_DIAG  // ablation builds only (changes results)
    if (std::getenv("MPG_DEBUG_NO_WALK")) walk = false;
#endif
    if (walk) {
      geom_nbr[g] = (int)(hull_nbr.size() / 2);
      if (nvg > kMaxWalkVerts) big_words = std::max(big_words, (nvg + 63) / 64);  // pooled visited set
      for (int i = 0; i < nvg; ++i) {
        const int st = enc[i], cnt = enc[st];
        hull_nbr.push_back((int)(nbr_ent.size() / 4));
        hull_nbr.push_back(cnt);
        for (int k = 1; k <= cnt; ++k) {
          const int vi = enc[st + k];
          nbr_ent.insert(nbr_ent.end(), {Vg[3 * vi], Vg[3 * vi + 1], Vg[3 * vi + 2], (double)vi});
        }
      }
      const size_t r0 = wcell_rec.size();
      if (build_walk_cells(Vg, nvg, enc.data(), walk_subk, wcell_rec, wcell_ovf, wcell_aux, wcell_end, wcell_end2, wcell_pre))
        cbase[g] = (int)(r0 / kCellRec);
    } else {
      std::vector<uint32_t> cstart;
      std::vector<double> cpts;
      if (build_hull_cells(Vg, nvg, cstart, cpts)) {
        cbase[g] = (int)(cell_rec.size() / kCellRec);
        pack_cell_records(cstart.data(), cpts.data(), cell_rec, cell_ovf);
      }
    }
    const double* V = d->vertices + 3 * (size_t)d->geom_vertex_start[g];
    const int nv = d->geom_vertex_count[g], ng = (nv + 3) / 4;
    gstart[g] = (int)(hull.size() / 12);
    ngroups[g] = ng;
    for (int q = 0; q < ng; ++q)
      for (int k = 0; k < 3; ++k)
        for (int l = 0; l < 4; ++l) {
          const int i = 4 * q + l < nv ? 4 * q + l : 0;
          hull.push_back(V[3 * i + k]);
        }
  }
  for (int g = 0; g < d->n_geoms; ++g) {  // TriangleP: its three vertices as one group (supportTriangle reads them)
    if (d->geom_type[g] != MPG_GEOM_TRIANGLE) continue;
    const double* V = d->vertices + 3 * (size_t)d->geom_vertex_start[g];
    gstart[g] = (int)(hull.size() / 12);
    ngroups[g] = 1;
    for (int k = 0; k < 3; ++k)
      for (int l = 0; l < 4; ++l) hull.push_back(V[3 * (l < 3 ? l : 0) + k]);
  }
  if (hull.empty()) hull.assign(12, 0.0);
  if (cell_rec.empty()) cell_rec.assign(kCellRec, 0.0);
  if (cell_ovf.empty()) cell_ovf.assign(4, 0.0);
  if (hull_nbr.empty()) hull_nbr.assign(2, 0);
  if (nbr_ent.empty()) nbr_ent.assign(4, 0.0);
  if (wcell_rec.empty()) wcell_rec.assign(kCellRec, 0.0);
  if (wcell_ovf.empty()) wcell_ovf.assign(4, 0.0);
  if (wcell_aux.empty()) wcell_aux.assign(kWalkAux, 0.0);
  if (wcell_end.empty()) wcell_end.assign(1, -1);
  if (wcell_end2.empty()) wcell_end2.assign(1, -1);
  if (wcell_pre.empty()) wcell_pre.assign(kWalkPre, 0);
  // octrees: leaf boxes + a uniform grid per octree geometry (cells of at
  // least the largest leaf, <= 64 per axis); a leaf is listed in every cell
  // its box overlaps
  // BVH meshes: per triangle its vertices (mesh frame) and AABB (TR_*), in
  // cluster order
  std::vector<double> mesh_tri((size_t)TR_STRIDE * std::max<int64_t>(d->n_mesh_triangles, 1), 0.0);
  std::vector<double> mesh_node;
  std::vector<int> mesh_link, mesh_tree(2 * (size_t)std::max(d->n_geoms, 1), 0);
  for (int g = 0; g < d->n_geoms; ++g) {
    if (d->geom_type[g] != MPG_GEOM_MESH) continue;
    const double* V = d->vertices + 3 * (size_t)d->geom_vertex_start[g];
    const int64_t t0 = (int64_t)d->geom_param[4 * g], tn = (int64_t)d->geom_param[4 * g + 1];
    std::vector<double> rec((size_t)TR_STRIDE * std::max<int64_t>(tn, 1), 0.0);
    for (int64_t t = 0; t < tn; ++t) {
      double* r = rec.data() + (size_t)TR_STRIDE * t;
      for (int v = 0; v < 3; ++v)
        for (int k = 0; k < 3; ++k) r[TR_P + 3 * v + k] = V[3 * (size_t)d->mesh_triangle[3 * (t0 + t) + v] + k];
      for (int k = 0; k < 3; ++k) {
        r[TR_LO + k] = std::min(r[TR_P + k], std::min(r[TR_P + 3 + k], r[TR_P + 6 + k]));
        r[TR_HI + k] = std::max(r[TR_P + k], std::max(r[TR_P + 3 + k], r[TR_P + 6 + k]));
      }
      r[TR_ID] = (double)t;  // the triangle's index in the mesh (its leaf position: tri_pos)
    }
    std::vector<int> order((size_t)tn);
    for (int64_t t = 0; t < tn; ++t) order[t] = (int)t;
    // clusters of <= max(8, T / 64) triangles: ~64 cluster boxes per mesh
    mesh_tree[2 * g] = (int)(mesh_link.size() / 2);
    mesh_build_clusters(rec, order, 0, (int)tn, std::max<int>(8, (int)((tn + 63) / 64)), (int)t0, mesh_node, mesh_link);
    mesh_tree[2 * g + 1] = (int)(mesh_link.size() / 2) - mesh_tree[2 * g];
    for (int64_t k = 0; k < tn; ++k)
      std::copy(rec.begin() + (size_t)TR_STRIDE * order[k], rec.begin() + (size_t)TR_STRIDE * (order[k] + 1),
                mesh_tri.begin() + (size_t)TR_STRIDE * (t0 + k));
  }
  if (mesh_node.empty()) mesh_node.assign(6, 0.0);
  if (mesh_link.empty()) mesh_link.assign(2, 0);
  // FCL's BVHModel<OBBRSS> trees (the traversal gates of mesh pairs) and the
  // shapes' computeBV OBBs
  FclBvh fbvh;
  std::vector<int> fb_root(std::max(d->n_geoms, 1), -1), tri_pos(std::max<int64_t>(d->n_mesh_triangles, 1), 0);
  std::vector<double> sobb((size_t)FB_STRIDE * std::max(d->n_geoms, 1), 0.0);
  for (int g = 0; g < d->n_geoms; ++g) {
    fcl_shape_obb(d, g, sobb.data() + (size_t)FB_STRIDE * g);
    if (d->geom_type[g] != MPG_GEOM_MESH) continue;
    const int64_t t0 = (int64_t)d->geom_param[4 * g], tn = (int64_t)d->geom_param[4 * g + 1];
    if (tn <= 0) continue;
    const int base = (int)(fbvh.link.size() / 3);
    fb_root[g] = base;
    fbvh.box.resize(fbvh.box.size() + FB_STRIDE);
    fbvh.link.resize(fbvh.link.size() + 3);
    std::vector<int> prim((size_t)tn);
    for (int64_t t = 0; t < tn; ++t) prim[t] = (int)t;
    fbvh.max_depth = 0;
    fcl_bvh_node(fbvh, d->vertices + 3 * (size_t)d->geom_vertex_start[g], d->mesh_triangle + 3 * t0, prim, 0, 0,
                 (int)tn, base);
    if (fbvh.max_depth > kFclMaxDepth)
      return set_error(MPG_E_UNSUPPORTED, "BVH mesh geometry " + std::to_string(g) + ": FCL's mean-split tree is " +
                                              std::to_string(fbvh.max_depth) + " levels deep (the device gates descend at most " +
                                              std::to_string(kFclMaxDepth) + ")");
    for (int64_t k = 0; k < tn; ++k) tri_pos[t0 + prim[k]] = (int)k;
  }
  if (fbvh.box.empty()) {
    fbvh.box.assign(FB_STRIDE, 0.0);
    fbvh.link.assign(3, 0);
  }
  std::vector<double> oct_leaf(6 * (size_t)std::max<int64_t>(d->n_octree_leaves, 1), 0.0);
  if (d->n_octree_leaves > 0) std::copy(d->octree_leaf, d->octree_leaf + 6 * d->n_octree_leaves, oct_leaf.begin());
  // each leaf's path down FCL's octree: getRootBV (delta = 2^16 resolution /
  // 2) halved by computeChildBV until the leaf box (the leaves were cut that
  // way: host octree.cpp collect, octomap's 16 levels)
  std::vector<uint64_t> oct_path(std::max<int64_t>(d->n_octree_leaves, 1), 0);
  std::vector<int> oct_depth(std::max<int64_t>(d->n_octree_leaves, 1), 0);
  for (int g = 0; g < d->n_geoms; ++g) {
    if (d->geom_type[g] != MPG_GEOM_OCTREE) continue;
    const int64_t l0 = (int64_t)d->geom_param[4 * g], ln = (int64_t)d->geom_param[4 * g + 1];
    const double delta = (double)(1 << 16) * d->geom_param[4 * g + 2] / 2;
    for (int64_t l = l0; l < l0 + ln; ++l) {
      const double* L = d->octree_leaf + 6 * l;
      double lo[3] = {-delta, -delta, -delta}, hi[3] = {delta, delta, delta};
      uint64_t code = 0;
      int depth = 0;
      while (!(lo[0] == L[0] && lo[1] == L[1] && lo[2] == L[2] && hi[0] == L[3] && hi[1] == L[4] && hi[2] == L[5])) {
        if (++depth > 16)
          return set_error(MPG_E_INVALID, "octree geometry " + std::to_string(g) + ": leaf " + std::to_string(l - l0) +
                                              " is not a box of FCL's root-BV halving (getRootBV / computeChildBV)");
        int ci = 0;
        for (int k = 0; k < 3; ++k) {
          const double mid = (lo[k] + hi[k]) * 0.5;
          if (L[k] >= mid) {
            ci |= 1 << k;
            lo[k] = mid;
          } else {
            hi[k] = mid;
          }
        }
        code = (code << 3) | (uint64_t)ci;
      }
      oct_path[l] = code;
      oct_depth[l] = depth;
    }
  }
  std::vector<double> oct_grid((size_t)OG_STRIDE * std::max(d->n_geoms, 1), 0.0);
  std::vector<int> oct_cells, oct_list;
  for (int g = 0; g < d->n_geoms; ++g) {
    if (d->geom_type[g] != MPG_GEOM_OCTREE) continue;
    const int64_t l0 = (int64_t)d->geom_param[4 * g], ln = (int64_t)d->geom_param[4 * g + 1];
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, big = 0.0;
    for (int64_t i = l0; i < l0 + ln; ++i)
      for (int k = 0; k < 3; ++k) {
        const double a = d->octree_leaf[6 * i + k], b = d->octree_leaf[6 * i + 3 + k];
        lo[k] = i == l0 ? a : std::min(lo[k], a);
        hi[k] = i == l0 ? b : std::max(hi[k], b);
        big = std::max(big, b - a);
      }
    double ext = 0.0;
    for (int k = 0; k < 3; ++k) ext = std::max(ext, hi[k] - lo[k]);
    const double cell = std::max({big, ext / 64.0, 1e-9});
    int dims[3];
    for (int k = 0; k < 3; ++k) dims[k] = std::max(1, std::min(66, (int)std::ceil((hi[k] - lo[k]) / cell) + 1));
    double* og = oct_grid.data() + (size_t)OG_STRIDE * g;
    for (int k = 0; k < 3; ++k) og[OG_ORIGIN + k] = lo[k];
    og[OG_INV] = 1.0 / cell;
    for (int k = 0; k < 3; ++k) og[OG_DIMS + k] = dims[k];
    og[OG_CELL0] = (double)oct_cells.size();
    const size_t nc = (size_t)dims[0] * dims[1] * dims[2];
    std::vector<std::vector<int>> lists(nc);
    // the same cell arithmetic as the device query, so a leaf is found from
    // every cell a query box overlapping it can touch
    auto cidx = [&](double v, int k) {
      const double f = std::floor((v - lo[k]) * og[OG_INV]);
      return f < 0.0 ? 0 : (f >= dims[k] ? dims[k] - 1 : (int)f);
    };
    for (int64_t i = l0; i < l0 + ln; ++i) {
      const double* L = d->octree_leaf + 6 * i;
      for (int x = cidx(L[0], 0); x <= cidx(L[3], 0); ++x)
        for (int y = cidx(L[1], 1); y <= cidx(L[4], 1); ++y)
          for (int z = cidx(L[2], 2); z <= cidx(L[5], 2); ++z)
            lists[((size_t)x * dims[1] + y) * dims[2] + z].push_back((int)i);
    }
    for (size_t c = 0; c < nc; ++c) {
      oct_cells.push_back((int)oct_list.size());
      oct_list.insert(oct_list.end(), lists[c].begin(), lists[c].end());
    }
  }
  oct_cells.push_back((int)oct_list.size());
  if (oct_list.empty()) oct_list.push_back(0);
  // per link: joints from the root to link_parent (chain FK in phase B)
  std::vector<int> chain_start, chain_len, chain_joints;
  for (int l = 0; l < d->n_links; ++l) {
    std::vector<int> c;
    for (int j = d->link_parent[l]; j > 0; j = d->joint_parent[j - 1]) c.push_back(j);
    std::reverse(c.begin(), c.end());
    chain_start.push_back((int)chain_joints.size());
    chain_len.push_back((int)c.size());
    chain_joints.insert(chain_joints.end(), c.begin(), c.end());
  }
  std::vector<int> allowed(std::max(d->n_pairs, 1), 0);
  for (int p = 0; p < d->n_pairs; ++p) allowed[p] = d->pair_allowed ? (d->pair_allowed[p] != 0) : 0;
  std::vector<int> pair_cf(std::max(d->n_pairs, 1), 0);
  for (int p = 0; p < d->n_pairs; ++p) {
    pair_cf[p] = closed_form_kind(d, d->pair_a[p], d->pair_b[p]);
    // GST_INDEP: the shape pairs without a closed form run FCL's own GJK
    // (GJKSolver_indep keeps the same closed forms as GJKSolver_libccd)
    if (d->gjk_solver == MPG_GJK_INDEP && pair_cf[p] == CF_NONE) pair_cf[p] = CF_GJK;
  }
  // latency pair records (LR_*): one round of loads per wave instead of a
  // chain of dependent snapshot lookups (pair -> object -> link -> chain ->
  // joints -> geometry)
  std::vector<double> lat_rec((size_t)LR_STRIDE * std::max(d->n_pairs, 1), 0.0);
  bool lat_rec_ok = true;
  for (int p = 0; p < d->n_pairs; ++p) {
    double* R = lat_rec.data() + (size_t)LR_STRIDE * p;
    const int ids[2] = {d->pair_a[p], d->pair_b[p]};
    R[LR_ALLOWED] = allowed[p];
    R[LR_CF] = pair_cf[p];
    for (int s2 = 0; s2 < 2; ++s2) {
      const int id = ids[s2];
      const bool mv = id < d->n_moving;
      const int g = mv ? d->moving_geom[id] : d->static_geom[id - d->n_moving];
      R[s2 ? LR_GB : LR_GA] = g;
      R[s2 ? LR_BM : LR_AM] = mv ? 1.0 : 0.0;
      R[s2 ? LR_RB : LR_RA] = geom_rec[G_STRIDE * (size_t)g + G_RADIUS];
      double* S = R + LR_SIDE + LS_STRIDE * s2;
      for (int k = 0; k < 3; ++k) S[LS_OBBC + k] = geom_rec[G_STRIDE * (size_t)g + G_OBB_C + k];
      if (!mv) {
        std::copy(d->static_transform + 12 * (size_t)(id - d->n_moving),
                  d->static_transform + 12 * (size_t)(id - d->n_moving) + 12, S + LS_OFF);
        continue;
      }
      const int l = d->moving_link[id];
      const int cl = chain_len[l];
      if (cl > kLatChain) {
        lat_rec_ok = false;
        continue;
      }
      S[LS_CL] = cl;
      std::copy(d->link_placement + 12 * (size_t)l, d->link_placement + 12 * (size_t)l + 12, S + LS_LINKPL);
      std::copy(d->moving_offset + 12 * (size_t)id, d->moving_offset + 12 * (size_t)id + 12, S + LS_OFF);
      for (int k = 0; k < cl; ++k) {
        const int j = chain_joints[chain_start[l] + k] - 1;
        double* J = S + LS_J + LJ_STRIDE * k;
        J[0] = d->joint_type[j];
        J[1] = d->joint_q_source[j];
        J[2] = d->joint_q_const[j];
        for (int i = 0; i < 3; ++i) J[3 + i] = d->joint_axis[3 * (size_t)j + i];
        for (int i = 0; i < 12; ++i) J[6 + i] = d->joint_placement[12 * (size_t)j + i];
      }
    }
  }
  // phase-A schedule: non-allowed pairs grouped by their lower moving object
  // ---- culling margins: pairs that can reach libccd MPR (directly, on octree
  // leaves or on mesh triangles) keep everything within its false-hit reach.
  // MPR's own tolerance cannot add to that reach: a larger gjk_tolerance only
  // ends refinePortal earlier, with "no intersection" (it never gains a hit).
  // FCL's own GJK (CF_GJK pairs) is the other way round: evaluate() reports
  // Inside as soon as its ray is shorter than gjk_tolerance, and the ray's
  // length bounds the true separation from above, so it reports shapes up to
  // gjk_tolerance apart -- the margins of a world with such a pair cover that
  // too (at the default 1e-6 the libccd reach is the larger one, as before).
  bool may_mpr = false, may_gjk = false;
  for (int p = 0; p < d->n_pairs; ++p) {
    if (allowed[p]) continue;
    const int ta = obj_geom_type(d, d->pair_a[p]), tb = obj_geom_type(d, d->pair_b[p]);
    const bool closed = pair_cf[p] != CF_NONE && cf_class(pair_cf[p]) == CLS_CLOSED;
    const bool mesh_mesh = ta == MPG_GEOM_MESH && tb == MPG_GEOM_MESH;
    may_mpr |= !closed && !mesh_mesh;
    may_gjk |= pair_cf[p] == CF_GJK;
  }
  double reach = kCcdFalseHitReach * (1.0 + 1e-3) + 1e-5;
  if (may_gjk) reach = std::max(reach, d->gjk_tolerance * (1.0 + 1e-3) + 1e-5);
  float bp_margin = may_mpr ? (float)std::max((double)kBpMargin, reach) : kBpMargin;
  // The travel of each prismatic joint: a move-group joint's value bound from
  // its limits (kDefaultTravel when unbounded), a fixed joint's own value.
  // A configuration whose prismatic value exceeds its bound is evaluated with
  // every pair (the cull's coordinate bound below would not hold for it).
  auto sq3 = [](const double* v) { return v[0] * v[0] + v[1] * v[1] + v[2] * v[2]; };
  // prism_bound < 0: not a move-group prismatic joint (a [0, 0] limit is a real bound of 0)
  std::vector<double> travel(std::max(d->n_joints, 1), 0.0), prism_bound(std::max(d->n_joints, 1), -1.0);
  int n_prism = 0;
  for (int j = 0; j < d->n_joints; ++j) {
    const int t = d->joint_type[j];
    if (t < MPG_JOINT_PX || t > MPG_JOINT_PRISMATIC_UNALIGNED) continue;
    const double an = t == MPG_JOINT_PRISMATIC_UNALIGNED ? std::sqrt(sq3(d->joint_axis + 3 * j)) : 1.0;
    if (d->joint_q_source[j] >= 0) {
      double qb = kDefaultTravel;
      if (d->joint_lower && d->joint_upper && std::isfinite(d->joint_lower[j]) && std::isfinite(d->joint_upper[j]))
        qb = std::max(std::fabs(d->joint_lower[j]), std::fabs(d->joint_upper[j]));
      prism_bound[j] = qb;
      ++n_prism;
      travel[j] = qb * an;
    } else {
      travel[j] = std::fabs(d->joint_q_const[j]) * an;
    }
  }
  // the fp32 broad phase's rounding grows with coordinate magnitude: bound
  // every world coordinate the cull computes (the chain's reach -- sum of the
  // placement translations and prismatic travels, revolute joints cannot
  // lengthen it --, moving offsets, static poses, geometry radii) and keep the
  // margin above kFp32CullRel of it (kBpMargin covers a ~2 m world near the
  // origin)
  double reach_x = 0.0, geo_r = 0.0, stat_x = 0.0;
  for (int j = 0; j < d->n_joints; ++j) reach_x += std::sqrt(sq3(d->joint_placement + 12 * j + 9)) + travel[j];
  // (the kinematic links: where a free frame starts says nothing about the chain)
  for (int l = 0; l < d->n_links - n_free; ++l) reach_x += std::sqrt(sq3(d->link_placement + 12 * l + 9));
  double off = 0.0;
  for (int m = 0; m < d->n_moving; ++m) off = std::max(off, std::sqrt(sq3(d->moving_offset + 12 * m + 9)));
  for (int g = 0; g < d->n_geoms; ++g) geo_r = std::max(geo_r, geom_rec[G_STRIDE * g + G_RADIUS] +
                                                                   std::sqrt(sq3(&geom_rec[G_STRIDE * g + G_OBB_C])));
  for (int s2 = 0; s2 < d->n_static; ++s2) stat_x = std::max(stat_x, std::sqrt(sq3(d->static_transform + 12 * s2 + 9)));
  double X = std::max(reach_x + off, stat_x) + geo_r;
  bp_margin = std::max(bp_margin, (float)(kFp32CullRel * X));
  double small_margin = may_mpr ? std::max(kSmallMargin, reach) : kSmallMargin;
  // Movable objects (on free frames).  Every link-borne object lies in the
  // ball of radius link_r around the origin: each coordinate of a link origin
  // is within reach_x (FK keeps the norm there; the link-pose input forces
  // every pair of a row beyond it), then the offset and the geometry.  A
  // movable object whose bounding sphere is outside far_r = link_r + margin +
  // slack (as never_near) is dropped by the cull's exact fp64 far test; one
  // that is not has every coordinate within far_r + 2 geo_r, which X (and so
  // the margin, which in turn moves far_r: a few rounds settle it) covers.
  // The margins also carry the scaling a free pose's quaternion may have
  // (kFreeQuatTol, mpgpu.h).
  double far_r = 0.0;
  if (n_free) {
    const double link_r = std::sqrt(3.0) * reach_x + off + geo_r;
    const float quat_slack = (float)(4.0 * kFreeQuatTol * geo_r);
    bp_margin += quat_slack;
    small_margin += 4.0 * kFreeQuatTol * geo_r;
    for (int it = 0; it < 8; ++it) {
      far_r = (link_r + (double)bp_margin + 1e-6 * (1.0 + X)) * (1.0 + 1e-9);
      X = std::max(X, far_r + 2.0 * geo_r);
      bp_margin = std::max(bp_margin, (float)(kFp32CullRel * X) + quat_slack);
    }
    far_r = (link_r + (double)bp_margin + 1e-6 * (1.0 + X)) * (1.0 + 1e-9);
    X = std::max(X, far_r + 2.0 * geo_r);
  }
  // link poses given directly (mpg_collide_link_poses): a pose beyond the
  // chain's reach falls outside the coordinate bound -> every pair
  const double pose_bound = reach_x;
  // Reach ball of each moving object: its centre stays within radius R of
  // the origin of the first joint of its chain (every later joint origin is
  // a fixed distance from its parent's, plus a prismatic travel; revolute
  // angles cannot lengthen the chain), or is fixed when the chain is empty.
  // A static partner farther than R + the object's radius + the culling
  // margin from that ball can never be a candidate: its schedule entry is
  // kept only for the link-pose input, whose poses are not kinematic.
  std::vector<std::array<double, 4>> ball(std::max(d->n_moving, 1));  // centre, radius (object radius included)
  std::vector<double> ball_rc(std::max(d->n_moving, 1), 0.0);          // the same without it: the centre's reach
  for (int m = 0; m < d->n_moving; ++m) {
    const int l = d->moving_link[m];
    const double* g = geom_rec.data() + G_STRIDE * d->moving_geom[m];
    const double* mo = d->moving_offset + 12 * m;
    const double* lp = d->link_placement + 12 * l;
    double a[3], bpt[3];
    for (int i = 0; i < 3; ++i)
      a[i] = mo[3 * i] * g[G_OBB_C] + mo[3 * i + 1] * g[G_OBB_C + 1] + mo[3 * i + 2] * g[G_OBB_C + 2] + mo[9 + i];
    for (int i = 0; i < 3; ++i) bpt[i] = lp[3 * i] * a[0] + lp[3 * i + 1] * a[1] + lp[3 * i + 2] * a[2] + lp[9 + i];
    const int cs = chain_start[l], cn = chain_len[l];
    double R = g[G_RADIUS];
    if (cn == 0) {
      ball[m] = {bpt[0], bpt[1], bpt[2], R};
      continue;
    }
    const int j1 = chain_joints[cs] - 1;
    const double* p1 = d->joint_placement + 12 * j1 + 9;
    R += travel[j1] + std::sqrt(sq3(bpt));
    for (int k = 1; k < cn; ++k) {
      const int j = chain_joints[cs + k] - 1;
      R += std::sqrt(sq3(d->joint_placement + 12 * j + 9)) + travel[j];
    }
    ball[m] = {p1[0], p1[1], p1[2], R * (1.0 + 1e-9) + 1e-9};
    ball_rc[m] = (R - g[G_RADIUS]) * (1.0 + 1e-9) + 1e-9;
  }
  auto never_near = [&](int m, int sid) {  // exact fp64 distance, reach ball vs the static OBB
    const double* sr = static_rec.data() + (size_t)S_STRIDE * sid;
    const double* gs = geom_rec.data() + G_STRIDE * d->static_geom[sid];
    double e2 = 0.0;
    for (int k = 0; k < 3; ++k) {  // box axis k = column k of S_R
      double t = 0.0;
      for (int i = 0; i < 3; ++i) t += (ball[m][i] - sr[S_OBBC + i]) * sr[S_R + 3 * i + k];
      const double ex = std::max(std::fabs(t) - gs[G_OBB_E + k], 0.0);
      e2 += ex * ex;
    }
    const double slack = 1e-6 * (1.0 + X);
    return std::sqrt(e2) - ball[m][3] > (double)bp_margin + slack;
  };
  // bits of every non-allowed pair (a configuration evaluated with all pairs)
  std::vector<int> all_mask(std::max(W, 1), 0);
  for (int p = 0; p < d->n_pairs; ++p)
    if (!allowed[p]) all_mask[p >> 5] |= (int)(1u << (p & 31));
  // moving-moving pairs by their lower moving object, then the moving-static
  // pairs static-major (one static record serves all its entries), those the
  // object's reach ball can bring near (group 0) before the rest (group 1)
  const int ns = d->n_static;
  std::vector<int> sched_start(d->n_moving + 1, 0), sched_pair, sched_other, st_start(2 * (ns + 1), 0), st_m;
  std::vector<float> st_r;
  for (int m = 0; m < d->n_moving; ++m) {
    sched_start[m] = (int)sched_pair.size();
    for (int p = 0; p < d->n_pairs; ++p) {
      if (allowed[p]) continue;
      const int a = d->pair_a[p], b = d->pair_b[p];
      const int lo = std::min(a, b), hi = std::max(a, b);  // static ids are >= n_moving
      if (lo != m || hi >= d->n_moving) continue;
      sched_pair.push_back(p);
      sched_other.push_back(hi);
      st_m.push_back(0);
      st_r.push_back(0.f);
    }
  }
  sched_start[d->n_moving] = (int)sched_pair.size();
  for (int g = 0; g < 2; ++g) {
    for (int sid = 0; sid < ns; ++sid) {
      st_start[g * (ns + 1) + sid] = (int)sched_pair.size();
      for (int m = 0; m < d->n_moving; ++m)
        for (int p = 0; p < d->n_pairs; ++p) {
          if (allowed[p]) continue;
          const int a = d->pair_a[p], b = d->pair_b[p];
          if (std::min(a, b) != m || std::max(a, b) != d->n_moving + sid) continue;
          if (never_near(m, sid) != (g == 1)) continue;
          sched_pair.push_back(p);
          sched_other.push_back(d->n_moving + sid);
          st_m.push_back(m);
          st_r.push_back(bpp.mobj[BM_STRIDE * m + BM_R]);
        }
    }
    st_start[g * (ns + 1) + ns] = (int)sched_pair.size();
  }
  // Lookup grids of the joint-value cull (mpg_broadphase.h bp_grid_*): a
  // link-borne object with kGridMinPartners..kGridMaxPartners group-0 static partners is a
  // candidate, its box the cube around its reach ball's centre (the centre's
  // reach, without the object's radius, plus the fp32 centre error);
  // bp_grid_choose keeps those that fit the cell budget.  Their group-0
  // entries are repeated object-major after the schedule above, then those of
  // the other objects static-major (gst_start); the link-pose input keeps
  // st_start.  A world where no object has a grid adds nothing, and a world
  // with free frames has none: its joint-value rows go through link poses
  // (launch_collide_free), so the joint-value cull never runs for it.
  BpGridPlan gplan;
  std::vector<int> gst_start, grid_i;
  std::vector<float> grid_f;
  {
    const double slack = kFp32CullRel * X + 1e-6;
    for (int m = 0; m < d->n_moving && n_free == 0; ++m) {
      BpGridObj o;
      o.m = m;
      o.r = (double)bpp.mobj[BM_STRIDE * m + BM_R];
      for (int k = 0; k < 3; ++k) {
        o.lo[k] = ball[m][k] - (ball_rc[m] + slack);
        o.hi[k] = ball[m][k] + (ball_rc[m] + slack);
      }
      for (int sid = 0; sid < ns; ++sid)
        for (int p = 0; p < d->n_pairs; ++p) {
          if (allowed[p]) continue;
          const int a = d->pair_a[p], b = d->pair_b[p];
          if (std::min(a, b) != m || std::max(a, b) != d->n_moving + sid || never_near(m, sid)) continue;
          o.sid.push_back(sid);
          o.pair.push_back(p);
        }
      if (bp_grid_candidate(o.sid.size())) gplan.obj.push_back(std::move(o));
    }
    bp_grid_choose(gplan, X, (double)bp_margin);
  }
  if (!gplan.obj.empty()) {
    std::vector<char> gridded(d->n_moving, 0);
    std::vector<int> E;
    for (const BpGridObj& o : gplan.obj) {
      gridded[o.m] = 1;
      E.push_back((int)sched_pair.size());
      for (size_t k = 0; k < o.sid.size(); ++k) {
        sched_pair.push_back(o.pair[k]);
        sched_other.push_back(d->n_moving + o.sid[k]);
        st_m.push_back(o.m);
        st_r.push_back(bpp.mobj[BM_STRIDE * o.m + BM_R]);
      }
    }
    E.push_back((int)sched_pair.size());
    bp_grid_records(gplan, E, grid_f, grid_i);
    gst_start.assign(ns + 1, 0);
    for (int sid = 0; sid < ns; ++sid) {
      gst_start[sid] = (int)sched_pair.size();
      for (int m = 0; m < d->n_moving; ++m)
        for (int p = 0; p < d->n_pairs && !gridded[m]; ++p) {
          if (allowed[p]) continue;
          const int a = d->pair_a[p], b = d->pair_b[p];
          if (std::min(a, b) != m || std::max(a, b) != d->n_moving + sid || never_near(m, sid)) continue;
          sched_pair.push_back(p);
          sched_other.push_back(d->n_moving + sid);
          st_m.push_back(m);
          st_r.push_back(bpp.mobj[BM_STRIDE * m + BM_R]);
        }
    }
    gst_start[ns] = (int)sched_pair.size();
    gplan.sobb.assign((size_t)15 * ns, 0.0);
    for (int sid = 0; sid < ns; ++sid) {
      const float* r = bpp.sobj.data() + BS_STRIDE * sid;
      double* S = gplan.sobb.data() + 15 * (size_t)sid;
      for (int k = 0; k < 3; ++k) S[k] = r[BS_C + k], S[12 + k] = r[BS_E + k];
      for (int k = 0; k < 9; ++k) S[3 + k] = r[BS_R + k];
    }
  }
  if (sched_pair.empty()) {
    sched_pair.push_back(0);
    sched_other.push_back(0);
    st_m.push_back(0);
    st_r.push_back(0.f);
  }

  BlobBuilder bb;
  const size_t o_jt = bb.add(d->joint_type, d->n_joints);
  const size_t o_jp = bb.add(d->joint_parent, d->n_joints);
  const size_t o_jqs = bb.add(d->joint_q_source, d->n_joints);
  const size_t o_jqc = bb.add(d->joint_q_const, d->n_joints);
  const size_t o_ja = bb.add(d->joint_axis, 3 * (size_t)d->n_joints);
  const size_t o_jpl = bb.add(d->joint_placement, 12 * (size_t)d->n_joints);
  const size_t o_lp = bb.add(d->link_parent, d->n_links);
  const size_t o_lpl = bb.add(d->link_placement, 12 * (size_t)d->n_links);
  const size_t o_gt = bb.add(d->geom_type, d->n_geoms);
  const size_t o_gvs = bb.add(gstart.data(), gstart.size());
  const size_t o_gnv = bb.add(ngroups.data(), ngroups.size());
  std::vector<int> nvert(std::max(d->n_geoms, 1), 0);
  for (int g = 0; g < d->n_geoms; ++g) nvert[g] = d->geom_type[g] == MPG_GEOM_CONVEX ? d->geom_vertex_count[g] : 0;
  const size_t o_gnvt = bb.add(nvert.data(), nvert.size());
  const size_t o_grec = bb.add(geom_rec.data(), geom_rec.size());
  const size_t o_v = bb.add(hull.data(), hull.size());
  const size_t o_cb = bb.add(cbase.data(), cbase.size());
  const size_t o_crec = bb.add(cell_rec.data(), cell_rec.size());
  const size_t o_covf = bb.add(cell_ovf.data(), cell_ovf.size());
  const size_t o_gnb = bb.add(geom_nbr.data(), geom_nbr.size());
  const size_t o_hnb = bb.add(hull_nbr.data(), hull_nbr.size());
  const size_t o_nent = bb.add(nbr_ent.data(), nbr_ent.size());
  const size_t o_wrec = bb.add(wcell_rec.data(), wcell_rec.size());
  const size_t o_wovf = bb.add(wcell_ovf.data(), wcell_ovf.size());
  const size_t o_waux = bb.add(wcell_aux.data(), wcell_aux.size());
  const size_t o_wend = bb.add(wcell_end.data(), wcell_end.size());
  const size_t o_wend2 = bb.add(wcell_end2.data(), wcell_end2.size());
  const size_t o_wpre = bb.add(wcell_pre.data(), wcell_pre.size());
  const size_t o_ml = bb.add(d->moving_link, d->n_moving);
  const size_t o_mg = bb.add(d->moving_geom, d->n_moving);
  const size_t o_mo = bb.add(d->moving_offset, 12 * (size_t)d->n_moving);
  const size_t o_sg = bb.add(d->static_geom, d->n_static);
  const size_t o_srec = bb.add(static_rec.data(), static_rec.size());
  const size_t o_pa = bb.add(d->pair_a, d->n_pairs);
  const size_t o_pb = bb.add(d->pair_b, d->n_pairs);
  const size_t o_al = bb.add(allowed.data(), allowed.size());
  const size_t o_cf = bb.add(pair_cf.data(), pair_cf.size());
  const size_t o_sT = bb.add(d->static_transform, 12 * (size_t)d->n_static);
  const size_t o_cs = bb.add(chain_start.data(), chain_start.size());
  const size_t o_cl = bb.add(chain_len.data(), chain_len.size());
  const size_t o_cj = bb.add(chain_joints.data(), chain_joints.size());
  const size_t o_ss = bb.add(sched_start.data(), sched_start.size());
  const size_t o_sp = bb.add(sched_pair.data(), sched_pair.size());
  const size_t o_so = bb.add(sched_other.data(), sched_other.size());
  const size_t o_sts = bb.add(st_start.data(), st_start.size());
  const size_t o_stm = bb.add(st_m.data(), st_m.size());
  const size_t o_str = bb.add(st_r.data(), st_r.size());
  const size_t o_pbd = bb.add(prism_bound.data(), prism_bound.size());
  const size_t o_amk = bb.add(all_mask.data(), all_mask.size());
  const size_t o_bjs = bb.add(bpp.jsrc.data(), bpp.jsrc.size());
  const size_t o_bjv = bb.add(bpp.jsave.data(), bpp.jsave.size());
  const size_t o_bja = bb.add(bpp.jaxis.data(), bpp.jaxis.size());
  const size_t o_bjp = bb.add(bpp.jplace.data(), bpp.jplace.size());
  const size_t o_bls = bb.add(bpp.link_start.data(), bpp.link_start.size());
  const size_t o_blo = bb.add(bpp.link_order.data(), bpp.link_order.size());
  const size_t o_blp = bb.add(bpp.lplace.data(), bpp.lplace.size());
  const size_t o_bos = bb.add(bpp.obj_start.data(), bpp.obj_start.size());
  const size_t o_boo = bb.add(bpp.obj_order.data(), bpp.obj_order.size());
  const size_t o_bmo = bb.add(bpp.moff.data(), bpp.moff.size());
  const size_t o_bmb = bb.add(bpp.mobj.data(), bpp.mobj.size());
  const size_t o_bsb = bb.add(bpp.sobj.data(), bpp.sobj.size());
  if (bpp.jobj_order.empty()) bpp.jobj_order.push_back(0);
  const size_t o_bjk = bb.add(bpp.jkind.data(), bpp.jkind.size());
  const size_t o_bjo = bb.add(bpp.jobj_start.data(), bpp.jobj_start.size());
  const size_t o_bjr = bb.add(bpp.jobj_order.data(), bpp.jobj_order.size());
  const size_t o_bop = bb.add(bpp.oplace.data(), bpp.oplace.size());
  const size_t o_boq = bb.add(bpp.oquat.data(), bpp.oquat.size());
  const size_t o_boc = bb.add(bpp.ocen.data(), bpp.ocen.size());
  const size_t o_bsh = bb.add(bpp.shtab.data(), bpp.shtab.size());
  std::vector<int> sched_rec(SR_STRIDE * sched_pair.size(), 0);
  for (size_t e = 0; e < sched_pair.size() && d->n_pairs > 0; ++e) {
    const int p = sched_pair[e];
    int* r = sched_rec.data() + SR_STRIDE * e;
    r[SR_P] = p;
    r[SR_A] = d->pair_a[p];
    r[SR_B] = d->pair_b[p];
    r[SR_SH] = (bpp.pair_sh[2 * p] + 2) | ((bpp.pair_sh[2 * p + 1] + 2) << 16);
  }
  const size_t o_srr = bb.add(sched_rec.data(), sched_rec.size());
  const size_t o_olf = bb.add(oct_leaf.data(), oct_leaf.size());
  const size_t o_mtr = bb.add(mesh_tri.data(), mesh_tri.size());
  const size_t o_mnd = bb.add(mesh_node.data(), mesh_node.size());
  const size_t o_mln = bb.add(mesh_link.data(), mesh_link.size());
  const size_t o_mtt = bb.add(mesh_tree.data(), mesh_tree.size());
  const size_t o_lrec = bb.add(lat_rec.data(), lat_rec.size());
  const size_t o_fbb = bb.add(fbvh.box.data(), fbvh.box.size());
  const size_t o_fbl = bb.add(fbvh.link.data(), fbvh.link.size());
  const size_t o_fbr = bb.add(fb_root.data(), fb_root.size());
  const size_t o_tps = bb.add(tri_pos.data(), tri_pos.size());
  const size_t o_sob = bb.add(sobb.data(), sobb.size());
  const size_t o_ogr = bb.add(oct_grid.data(), oct_grid.size());
  const size_t o_oce = bb.add(oct_cells.data(), oct_cells.size());
  const size_t o_oli = bb.add(oct_list.data(), oct_list.size());
  const size_t o_opa = bb.add(oct_path.data(), oct_path.size());
  const size_t o_ode = bb.add(oct_depth.data(), oct_depth.size());
  // free frame k (link n_links - n_free + k) -> its object; worlds without
  // free frames add nothing to the snapshot (their hash stays what it was)
  std::vector<int> free_obj(n_free, 0);
  for (int m = 0; m < d->n_moving; ++m)
    if (d->moving_link[m] >= d->n_links - n_free) free_obj[d->moving_link[m] - (d->n_links - n_free)] = m;
  const size_t o_fob = n_free ? bb.add(free_obj.data(), free_obj.size()) : 0;
  const bool has_grid = !gplan.obj.empty();
  const size_t o_ggf = has_grid ? bb.add(grid_f.data(), grid_f.size()) : 0;
  const size_t o_ggi = has_grid ? bb.add(grid_i.data(), grid_i.size()) : 0;
  const size_t o_gst = has_grid ? bb.add(gst_start.data(), gst_start.size()) : 0;
  std::vector<int> rev_src = revolute_sources(d->joint_type, d->joint_q_source, d->n_joints);
  const int n_rev = (int)rev_src.size();
  if (rev_src.empty()) rev_src.push_back(0);
  const size_t o_rvs = bb.add(rev_src.data(), rev_src.size());

  std::unique_ptr<mpg_world> w(new mpg_world());  // every failure below releases what was built
  w->device = device;
  w->n_geoms = d->n_geoms;
  w->geom_type_h.assign(d->geom_type, d->geom_type + d->n_geoms);
  w->block = block;
  w->lds_bytes = lds;
  w->blob_bytes = bb.bytes.size();
  {  // FNV-1a over the snapshot: worlds built from the same descriptor agree
    uint64_t h = 1469598103934665603ull;
    for (const char c : bb.bytes) h = (h ^ (uint8_t)c) * 1099511628211ull;
    w->snapshot_hash = h;
  }
  HIP_TRY(w->blob.reserve(w->blob_bytes));
  HIP_TRY(hipMemcpy(w->blob.get(), bb.bytes.data(), w->blob_bytes, hipMemcpyHostToDevice));
  char* base = w->blob.get();
  DevWorld& dw = w->dw;
  dw.nj = d->n_joints;
  dw.dof = d->dof;
  dw.n_links = d->n_links;
  dw.n_geoms = d->n_geoms;
  dw.n_moving = d->n_moving;
  dw.n_static = d->n_static;
  dw.n_pairs = d->n_pairs;
  dw.W = W;
  dw.mpr_tol = d->gjk_tolerance;
  dw.bp_margin = bp_margin;
  // the support-height axes' own fp32 evaluation (two rotations, the cell
  // ratios, the interpolation: ~15 dependent operations on values within X),
  // bounded like the rest of the cull's rounding
  dw.sh_margin = bp_margin + (float)(kFp32CullRel * X);
  dw.small_margin = small_margin;
  dw.n_prism = n_prism;
  dw.prism_bound = to_cptr<double>(base + o_pbd);
  dw.pose_bound = pose_bound;
  dw.all_mask = to_cptr<int>(base + o_amk);
  dw.n_free = n_free;
  dw.far_r = far_r;
  dw.free_obj = to_cptr<int>(base + o_fob);
  dw.n_rev = n_rev;
  dw.rev_src = to_cptr<int>(base + o_rvs);
  dw.free_cur = nullptr;
  if (n_free) {  // the current poses start at the frames' link_placement, as (p, wxyz)
    w->free_host.resize((size_t)n_free * 7);
    for (int k = 0; k < n_free; ++k) {
      const double* lp = d->link_placement + 12 * (size_t)(d->n_links - n_free + k);
      double* p7 = w->free_host.data() + 7 * (size_t)k;
      for (int i = 0; i < 3; ++i) p7[i] = lp[9 + i];
      mat_to_quat(lp, &p7[3], &p7[4]);
    }
    HIP_TRY(w->free_dev.reserve(w->free_host.size()));
    HIP_TRY(hipMemcpy(w->free_dev.get(), w->free_host.data(), sizeof(double) * w->free_host.size(),
                      hipMemcpyHostToDevice));
    dw.free_cur = w->free_dev.get();
  }
#ifdef MPG_DIAG  // ablation builds only (changes results)
  if (const char* m = std::getenv("MPG_DEBUG_MARGIN")) {
    dw.bp_margin = (float)std::atof(m);
    dw.sh_margin = dw.bp_margin + (float)(kFp32CullRel * X);
    dw.small_margin = std::atof(m);
  }
#endif
  dw.debug_mode = 0;
#ifdef MPG_DIAG  // ablation builds only (changes results)
  if (const char* e = std::getenv("MPG_DEBUG_CULL")) dw.debug_mode = std::atoi(e);
#endif
  dw.big_vis = nullptr;
  dw.big_busy = nullptr;
  dw.big_slots = 0;
  dw.big_words = big_words;
  if (big_words > 0) {  // one visited set per resident wave at most (256 CUs x 32 waves)
    dw.big_slots = 8192;
    HIP_TRY(w->big_vis.reserve((size_t)dw.big_slots * big_words));
    dw.big_vis = w->big_vis.get();
    HIP_TRY(hipMemset(dw.big_vis, 0, sizeof(unsigned long long) * (size_t)dw.big_slots * big_words));
    HIP_TRY(w->big_busy.reserve((size_t)dw.big_slots));
    dw.big_busy = w->big_busy.get();
    HIP_TRY(hipMemset(dw.big_busy, 0, sizeof(int) * (size_t)dw.big_slots));
  }
  dw.stats = nullptr;
  if (std::getenv("MPG_STATS") && std::atoi(std::getenv("MPG_STATS")) > 0) {
    const size_t n_stats = 64;
    HIP_TRY(w->stats.reserve(n_stats));
    dw.stats = w->stats.get();
    HIP_TRY(hipMemset(dw.stats, 0, n_stats * sizeof(unsigned long long)));
  }
  dw.joint_type = to_cptr<int>(base + o_jt);
  dw.joint_parent = to_cptr<int>(base + o_jp);
  dw.joint_q_source = to_cptr<int>(base + o_jqs);
  dw.joint_q_const = to_cptr<double>(base + o_jqc);
  dw.joint_axis = to_cptr<double>(base + o_ja);
  dw.joint_place = to_cptr<double>(base + o_jpl);
  dw.link_parent = to_cptr<int>(base + o_lp);
  dw.link_place = to_cptr<double>(base + o_lpl);
  dw.geom_type = to_cptr<int>(base + o_gt);
  dw.geom_gstart = to_cptr<int>(base + o_gvs);
  dw.geom_ng = to_cptr<int>(base + o_gnv);
  dw.geom_nvert = to_cptr<int>(base + o_gnvt);
  dw.geom_rec = to_cptr<double>(base + o_grec);
  dw.hull = to_cptr<double>(base + o_v);
  dw.hull_doubles = (int)hull.size();
  dw.geom_cbase = to_cptr<int>(base + o_cb);
  dw.cell_rec = to_cptr<double>(base + o_crec);
  dw.cell_ovf = to_cptr<double>(base + o_covf);
  dw.geom_nbr = to_cptr<int>(base + o_gnb);
  dw.hull_nbr = to_cptr<int>(base + o_hnb);
  dw.nbr_ent = to_cptr<double>(base + o_nent);
  dw.wcell_rec = to_cptr<double>(base + o_wrec);
  dw.wcell_ovf = to_cptr<double>(base + o_wovf);
  dw.wcell_aux = to_cptr<double>(base + o_waux);
  dw.wcell_end = to_cptr<int>(base + o_wend);
  dw.wcell_end2 = to_cptr<int>(base + o_wend2);
  dw.wcell_pre = to_cptr<int>(base + o_wpre);
  dw.walk_subk = walk_subk;
  dw.moving_link = to_cptr<int>(base + o_ml);
  dw.moving_geom = to_cptr<int>(base + o_mg);
  dw.moving_offset = to_cptr<double>(base + o_mo);
  dw.static_geom = to_cptr<int>(base + o_sg);
  dw.static_rec = to_cptr<double>(base + o_srec);
  dw.pair_a = to_cptr<int>(base + o_pa);
  dw.pair_b = to_cptr<int>(base + o_pb);
  dw.pair_allowed = to_cptr<int>(base + o_al);
  dw.pair_cf = to_cptr<int>(base + o_cf);
  for (int p = 0; p < d->n_pairs; ++p) {
    w->has_closed_form |= pair_cf[p] != CF_NONE && !allowed[p];
    w->has_octree |= pair_cf[p] == CF_OCTREE && !allowed[p];
    w->octree_first |= pair_cf[p] == CF_OCTREE && !allowed[p] && obj_geom_type(d, d->pair_a[p]) == MPG_GEOM_OCTREE;
    w->any_closed_form |= pair_cf[p] != CF_NONE && cf_class(pair_cf[p]) == CLS_CLOSED;
    w->any_octree |= pair_cf[p] == CF_OCTREE;
    w->has_mesh |= pair_cf[p] == CF_MESH && !allowed[p];
    w->any_mesh |= pair_cf[p] == CF_MESH;
    w->any_gjk |= pair_cf[p] == CF_GJK;
    w->has_octree2 |= !allowed[p] && obj_geom_type(d, d->pair_a[p]) == MPG_GEOM_OCTREE &&
                      obj_geom_type(d, d->pair_b[p]) == MPG_GEOM_OCTREE;
  }
  dw.static_T = to_cptr<double>(base + o_sT);
  dw.link_chain_start = to_cptr<int>(base + o_cs);
  dw.link_chain_len = to_cptr<int>(base + o_cl);
  dw.chain_joints = to_cptr<int>(base + o_cj);
  auto I = [&](size_t o) { return to_cptr<int>(base + o); };
  dw.sched_start = I(o_ss);
  dw.sched_pair = I(o_sp);
  dw.sched_other = I(o_so);
  dw.sched_rec = I(o_srr);
  dw.st_start = I(o_sts);
  dw.st_m = I(o_stm);
  dw.st_r = to_cptr<float>(base + o_str);
  dw.n_grid = has_grid ? (int)(grid_i.size() / GI_STRIDE) : 0;
  dw.grid_f = to_cptr<float>(base + o_ggf);
  dw.grid_i = I(o_ggi);
  dw.gst_start = I(o_gst);
  for (const BpGridObj& o : gplan.obj) {
    w->grid_info.object.push_back(o.m);
    w->grid_info.partners.push_back((int)o.sid.size());
    for (int k = 0; k < 3; ++k) w->grid_info.box.push_back((double)o.o[k]);
    for (int k = 0; k < 3; ++k) w->grid_info.box.push_back((double)o.o[k] + o.n[k] * gplan.h);
  }
  w->grid_info.cells = has_grid ? gplan.cells : 0;
  w->grid_info.h = has_grid ? gplan.h : 0.0;
  w->grid_plan = std::move(gplan);
  auto F = [&](size_t o) { return to_cptr<float>(base + o); };
  BpView& bp = dw.bp;
  bp.nj = d->n_joints;
  bp.n_links = d->n_links;
  bp.n_moving = d->n_moving;
  bp.n_static = d->n_static;
  bp.n_saves = bpp.n_saves;
  bp.joint_type = dw.joint_type;
  bp.joint_q_source = dw.joint_q_source;
  bp.joint_q_const = dw.joint_q_const;
  bp.jsrc = I(o_bjs);
  bp.jsave = I(o_bjv);
  bp.jaxis = F(o_bja);
  bp.jplace = F(o_bjp);
  bp.link_start = I(o_bls);
  bp.link_order = I(o_blo);
  bp.lplace = F(o_blp);
  bp.obj_start = I(o_bos);
  bp.obj_order = I(o_boo);
  bp.moving_link = dw.moving_link;
  bp.moff = F(o_bmo);
  bp.mobj = F(o_bmb);
  bp.sobj = F(o_bsb);
  bp.jkind = I(o_bjk);
  bp.jobj_start = I(o_bjo);
  bp.jobj_order = I(o_bjr);
  bp.oplace = F(o_bop);
  bp.oquat = F(o_boq);
  bp.ocen = F(o_boc);
  bp.shtab = F(o_bsh);
  dw.oct_leaf = to_cptr<double>(base + o_olf);
  dw.oct_path = to_cptr<uint64_t>(base + o_opa);
  dw.oct_depth = to_cptr<int>(base + o_ode);
  dw.mesh_tri = to_cptr<double>(base + o_mtr);
  dw.mesh_node = to_cptr<double>(base + o_mnd);
  dw.mesh_link = to_cptr<int>(base + o_mln);
  dw.mesh_tree = to_cptr<int>(base + o_mtt);
  dw.fb_box = to_cptr<double>(base + o_fbb);
  dw.fb_link = to_cptr<int>(base + o_fbl);
  dw.fb_root = to_cptr<int>(base + o_fbr);
  dw.tri_pos = to_cptr<int>(base + o_tps);
  dw.sobb = to_cptr<double>(base + o_sob);
  dw.lat_rec = to_cptr<double>(base + o_lrec);
  dw.lat_rec_ok = lat_rec_ok ? 1 : 0;
  dw.oct_grid = to_cptr<double>(base + o_ogr);
  dw.oct_cells = I(o_oce);
  dw.oct_list = I(o_oli);
  int cus = 256;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
  // persistent narrow grid: exactly the resident workgroups
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, narrow_kernel<false>, 256, 0) != hipSuccess || per_cu <= 0)
    per_cu = 2;
  w->narrow_blocks = cus * per_cu;
  // a smaller grid (tests: a few thousand candidates then reach every level of the task plan)
  if (const char* e = std::getenv("MPG_NARROW_BLOCKS"))
    w->narrow_blocks = std::max(1, std::min(w->narrow_blocks, std::atoi(e)));
  // mpg_ik_batch's tables: host copies of the chains and, per dof slot, the
  // kind and limits of the joint behind it
  {
    auto& K = w->ik;
    K.cus = cus;
    K.chain_start = chain_start;
    K.chain_len = chain_len;
    K.chain_joints = chain_joints;
    K.joint_q_source.assign(d->joint_q_source, d->joint_q_source + d->n_joints);
    const size_t nd = (size_t)std::max(d->dof, 0);
    K.lo.assign(nd, -INFINITY);
    K.hi.assign(nd, INFINITY);
    K.kind.assign(nd, IKK_NONE);
    K.continuous.assign(nd, 0);
    for (int j = 0; j < d->n_joints; ++j) {
      const int s = d->joint_q_source[j];
      if (s < 0 || s >= d->dof || K.kind[s] != IKK_NONE) continue;
      K.kind[s] = joint_is_revolute(d->joint_type[j]) ? IKK_REVOLUTE : IKK_PRISMATIC;
      K.continuous[s] = d->joint_type[j] >= MPG_JOINT_RUBX;
      if (d->joint_lower && d->joint_upper) {
        K.lo[s] = d->joint_lower[j];
        K.hi[s] = d->joint_upper[j];
      }
    }
  }
  // bound the candidate lists to 1 GiB: cap * n_pairs * 4 B
  w->max_chunk = std::max<long long>(4096, std::min<long long>(1 << 20, (1ll << 28) / std::max(d->n_pairs, 1)));
  if (const char* e = std::getenv("MPG_SMALL_BATCH_MAX")) w->small_max = std::atoll(e);
  if (const char* e = std::getenv("MPG_SMALL_ZEROCOPY")) w->small_zero_copy = std::atoi(e) != 0;
  if (const char* e = std::getenv("MPG_OVERLAP_MIN")) w->overlap_min = std::atoll(e);
  if (const char* e = std::getenv("MPG_HOST_STREAMS")) w->ring_streams = std::atoi(e) > 1 ? 2 : 1;
  if (const char* e = std::getenv("MPG_HOST_THREADS")) w->host_threads = std::max(1, std::min(64, std::atoi(e)));
  if (const char* e = std::getenv("MPG_HOST_HEAD")) w->ring_head = std::max(0ll, std::atoll(e));
  if (const char* e = std::getenv("MPG_HOST_TAIL")) w->ring_tail = std::max(0ll, std::atoll(e));
  if (const char* e = std::getenv("MPG_HOST_CHUNK"))
    w->ring_chunk = std::max(64ll, std::min((long long)w->max_chunk, (std::atoll(e) + 63) / 64 * 64));
  if (const char* e = std::getenv("MPG_SMALL_INLINE_SC")) w->small_inline_sc = std::atoll(e);
  if (const char* e = std::getenv("MPG_OVERLAP_PARTS")) w->overlap_parts = std::atoi(e);
  if (const char* e = std::getenv("MPG_SMALL_HOST_SC")) w->small_host_sc = std::atoll(e);
  if (const char* e = std::getenv("MPG_SMALL_ARGS")) w->small_args = std::atoi(e) != 0;
  w->h_rev_src.assign(rev_src.begin(), rev_src.begin() + n_rev);
  if (const char* e = std::getenv("MPG_SMALL_SERVER")) w->srv_mode = std::atoi(e);
  w->srv_stats = std::getenv("MPG_STATS") != nullptr;
  if (const char* e = std::getenv("MPG_SMALL_SERVER_IDLE_US")) w->srv_idle_us = std::max(10ll, std::atoll(e));
  if (const char* e = std::getenv("MPG_SMALL_SERVER_WG")) w->srv_g = std::min(kSrvMaxG, std::max(1, std::atoi(e)));
  if (const char* e = std::getenv("MPG_SMALL_SERVER_MAX")) w->srv_max_n = std::min(kSrvN, std::max(1, std::atoi(e)));
  w->srv_lds = srv_lds_bytes(d->n_moving, d->n_pairs, d->dof, w->dw.W, d->n_joints, d->n_static);
  w->srv_ok = lat_rec_ok && !w->any_octree && !w->any_mesh && !w->any_gjk && d->dof > 0 && d->dof <= kLatScDof &&
              d->n_pairs > 0 && w->dw.W <= kSrvMaxW && w->srv_lds <= 144 * 1024 &&  // + ~11 KB static LDS
              n_free == 0;  // the resident server holds a by-value world: it would not see a pose update
  const char* own = std::getenv("MPG_OWN_STREAM");
  if (!own || std::atoi(own) != 0) HIP_TRY(w->own_stream.create(hipStreamNonBlocking));
  *out = w.release();
  return MPG_OK;
}

// the MPG_STATS report of a world that is about to go
static void print_stats(const mpg_world* w) {
  if (w->dw.stats) {
    unsigned long long st[64];
    hipDeviceSynchronize();
    hipMemcpy(st, w->dw.stats, sizeof(st), hipMemcpyDeviceToHost);
    std::fprintf(stderr,
                 "[mpg stats] small_kernel phases (sum over waves / max per wave, us): pre %.1f/%.2f, record %.1f/%.2f, "
                 "fk %.1f/%.2f, spheres %.1f/%.2f, narrow %.1f/%.2f, store %.1f/%.2f, wave %.1f/%.2f\n",
                 st[24] / 100.0, st[32] / 100.0, st[25] / 100.0, st[33] / 100.0, st[26] / 100.0, st[34] / 100.0,
                 st[27] / 100.0, st[35] / 100.0, st[28] / 100.0, st[36] / 100.0, st[29] / 100.0, st[37] / 100.0,
                 st[30] / 100.0, st[38] / 100.0);
    if (st[42])
      std::fprintf(stderr, "[mpg stats] latency server probe: dependent cell-record loads, shader clocks each: "
                   "first pass %.0f, again %.0f\n", (double)st[40] / st[42], (double)st[41] / st[43]);
    if (st[20])
      std::fprintf(stderr, "[mpg stats] latency server MPR steps: %llu (max %llu per pair), shader clocks per step: "
                   "support %.0f, advance %.0f\n", st[20], st[23], (double)st[21] / st[20], (double)st[22] / st[20]);
    if (st[52])
      std::fprintf(stderr, "[mpg stats] walk-hull support phases, shader clocks per hull support (%llu): cell lookup "
                   "%.0f, record load + inline dots %.0f, overflow entries %.0f, tie / trap checks %.0f\n",
                   st[52], (double)st[48] / st[52], (double)st[49] / st[52], (double)st[50] / st[52],
                   (double)st[51] / st[52]);
    std::fprintf(stderr, "[mpg stats] small_kernel slowest narrow test: pair %llu, %.2f us\n",
                 (unsigned long long)(st[31] & 4095), (st[31] >> 12) / 100.0);
    std::fprintf(stderr, "[mpg stats] walk hulls: supports %llu, trap-free fast %llu, verified %llu, full walks %llu, "
                 "certified endpoints %llu; pending: tie %llu, uncertified %llu, resumed %llu; resolve ticks: verify %llu, walk %llu\n",
                 st[10], st[11], st[12], st[13], st[14], st[16], st[17], st[18], st[9], st[15]);
    std::fprintf(stderr,
                 "[mpg stats] narrow: refill %llu, support %llu, update %llu (memtime ticks, summed over waves); "
                 "steps %llu, mean active lanes/step %.1f; hits %llu (%.2f supports each), misses %llu (%.2f)\n",
                 st[3], st[4], st[5], st[7], st[7] ? (double)st[6] / st[7] : 0.0, st[2],
                 st[2] ? (double)st[0] / st[2] : 0.0, st[8], st[8] ? (double)st[1] / st[8] : 0.0);
  }
  if (w->srv_stats && w->srv_stat[5] > 0)
    std::fprintf(stderr, "[mpg stats] latency server, mean us over %.0f batches: rows %.2f, fk %.2f, spheres %.2f, "
                 "narrow %.2f, publish %.2f; host post->done %.2f\n", w->srv_stat[5], w->srv_stat[0] / w->srv_stat[5],
                 w->srv_stat[1] / w->srv_stat[5], w->srv_stat[2] / w->srv_stat[5], w->srv_stat[3] / w->srv_stat[5],
                 w->srv_stat[4] / w->srv_stat[5], w->srv_stat[6] / w->srv_stat[5]);
  if (w->srv_stats && w->hp_stat[0] > 0)
    std::fprintf(stderr, "[mpg stats] host pipeline, mean us over %.0f calls: input copies %.1f, issue %.1f, "
                 "result wait %.1f, unpack %.1f; whole call %.1f\n", w->hp_stat[0], w->hp_stat[1] / w->hp_stat[0],
                 w->hp_stat[2] / w->hp_stat[0], w->hp_stat[3] / w->hp_stat[0], w->hp_stat[4] / w->hp_stat[0],
                 w->hp_stat[5] / w->hp_stat[0]);
}

// what is ordering; the members release everything else (mpg_world.h)
mpg_world::~mpg_world() {
  hipSetDevice(device);
  print_stats(this);  // before the stats buffer goes
  if (srv.get()) {    // the server leaves at its next poll, before its control block or the snapshot goes
    __atomic_store_n(&srv.get()->quit, 1ull, __ATOMIC_RELEASE);
    hipStreamSynchronize(srv_stream.get());
  }
  pool.reset();
}

int mpg_world_destroy(mpg_world* w) {
  delete w;
  return MPG_OK;
}

int mpg_world_get_info(const mpg_world* w, mpg_world_info* info) {
  if (!w || !info) return set_error(MPG_E_INVALID, "NULL argument");
  info->n_pairs = w->dw.n_pairs;
  info->mask_words = w->dw.W;
  info->dof = w->dw.dof;
  info->n_links = w->dw.n_links;
  info->device = w->device;
  info->block_size = w->block;
  info->snapshot_bytes = (int64_t)w->blob_bytes;
  return MPG_OK;
}
