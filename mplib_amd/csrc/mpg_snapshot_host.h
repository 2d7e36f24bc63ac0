// mpg_snapshot_host.h -- snapshot building, plain host C++: descriptor
// validation, geometry records, BlobBuilder, FCL's BVH build (FclBvh), block
// size choice (included by mpg_kernels.hip in an anonymous namespace, after mpg_world.h).
#pragma once

// Spatial clusters of one mesh's triangle records: the leaves of a median
// split (centroids, longest axis) with at most `leaf` triangles each, in
// order; triangle k of the clusters' ranges is rec[order[k]].
void mesh_build_clusters(const std::vector<double>& rec, std::vector<int>& order, int lo, int hi, int leaf, int rec0,
                         std::vector<double>& box, std::vector<int>& link) {
  auto cen = [&](int t, int k) {
    const double* r = rec.data() + (size_t)TR_STRIDE * t;
    return r[TR_LO + k] + r[TR_HI + k];
  };
  if (hi - lo <= leaf) {
    double blo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, bhi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    for (int i = lo; i < hi; ++i) {
      const double* r = rec.data() + (size_t)TR_STRIDE * order[i];
      for (int k = 0; k < 3; ++k) {
        blo[k] = std::min(blo[k], r[TR_LO + k]);
        bhi[k] = std::max(bhi[k], r[TR_HI + k]);
      }
    }
    box.insert(box.end(), {blo[0], blo[1], blo[2], bhi[0], bhi[1], bhi[2]});
    link.insert(link.end(), {rec0 + lo, hi - lo});
    return;
  }
  double clo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, chi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
  for (int i = lo; i < hi; ++i)
    for (int k = 0; k < 3; ++k) {
      clo[k] = std::min(clo[k], cen(order[i], k));
      chi[k] = std::max(chi[k], cen(order[i], k));
    }
  int ax = 0;
  for (int k = 1; k < 3; ++k)
    if (chi[k] - clo[k] > chi[ax] - clo[ax]) ax = k;
  const int mid = (lo + hi) / 2;
  std::nth_element(order.begin() + lo, order.begin() + mid, order.begin() + hi,
                   [&](int a, int b) { return cen(a, ax) < cen(b, ax) || (cen(a, ax) == cen(b, ax) && a < b); });
  mesh_build_clusters(rec, order, lo, mid, leaf, rec0, box, link);
  mesh_build_clusters(rec, order, mid, hi, leaf, rec0, box, link);
}

struct BlobBuilder {
  std::vector<char> bytes;
  template <class T>
  size_t add(const T* data, size_t count) {
    size_t off = (bytes.size() + 15) & ~size_t(15);
    bytes.resize(off + sizeof(T) * std::max<size_t>(count, 1), 0);
    if (count) std::memcpy(bytes.data() + off, data, sizeof(T) * count);
    return off;
  }
};

bool finite_all(const double* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

int obj_geom_type(const mpg_world_desc* d, int id) {
  return d->geom_type[id < d->n_moving ? d->moving_geom[id] : d->static_geom[id - d->n_moving]];
}

// a movable object: a moving object whose link is a free frame
bool desc_obj_movable(const mpg_world_desc* d, int id) {
  return id < d->n_moving && d->link_parent[d->moving_link[id]] == MPG_LINK_FREE;
}

// FCL closed-form pair for (o1, o2) in fcl::collide argument order
int closed_form_kind(const mpg_world_desc* d, int a, int b) {
  const int ta = obj_geom_type(d, a), tb = obj_geom_type(d, b);
  if (ta == MPG_GEOM_MESH || tb == MPG_GEOM_MESH) return CF_MESH;
  if (ta == MPG_GEOM_OCTREE || tb == MPG_GEOM_OCTREE) return CF_OCTREE;
  if (ta == MPG_GEOM_BOX && tb == MPG_GEOM_BOX) return CF_BOX_BOX;
  if (ta == MPG_GEOM_SPHERE && tb == MPG_GEOM_SPHERE) return CF_SPHERE_SPHERE;
  if (ta == MPG_GEOM_SPHERE && tb == MPG_GEOM_BOX) return CF_SPHERE_BOX;
  if (ta == MPG_GEOM_BOX && tb == MPG_GEOM_SPHERE) return CF_BOX_SPHERE;
  if (ta == MPG_GEOM_SPHERE && tb == MPG_GEOM_CAPSULE) return CF_SPHERE_CAPSULE;
  if (ta == MPG_GEOM_CAPSULE && tb == MPG_GEOM_SPHERE) return CF_CAPSULE_SPHERE;
  if (ta == MPG_GEOM_SPHERE && tb == MPG_GEOM_CYLINDER) return CF_SPHERE_CYLINDER;
  if (ta == MPG_GEOM_CYLINDER && tb == MPG_GEOM_SPHERE) return CF_CYLINDER_SPHERE;
  return CF_NONE;
}

int validate(const mpg_world_desc* d) {
  if (!d) return set_error(MPG_E_INVALID, "desc is NULL");
  if (d->gjk_solver != MPG_GJK_LIBCCD && d->gjk_solver != MPG_GJK_INDEP)
    return set_error(MPG_E_INVALID, "gjk_solver must be MPG_GJK_LIBCCD or MPG_GJK_INDEP");
  if (d->n_joints < 0 || d->n_joints > kMaxJoints) return set_error(MPG_E_INVALID, "n_joints out of range [0, 32]");
  if (d->dof < 0) return set_error(MPG_E_INVALID, "dof < 0");
  if (d->n_links < 0 || d->n_geoms < 0 || d->n_moving < 0 || d->n_static < 0 || d->n_pairs < 0)
    return set_error(MPG_E_INVALID, "negative count");
  for (int j = 0; j < d->n_joints; ++j) {
    if (d->joint_type[j] < 0 || d->joint_type[j] > MPG_JOINT_RUB_UNALIGNED)
      return set_error(MPG_E_INVALID, "bad joint type");
    if (d->joint_parent[j] < 0 || d->joint_parent[j] > j)
      return set_error(MPG_E_INVALID, "joint_parent must reference an earlier joint (0 = universe)");
    if (d->joint_q_source[j] >= d->dof) return set_error(MPG_E_INVALID, "joint_q_source >= dof");
  }
  for (int l = 0; l < d->n_links; ++l) {
    if (d->link_parent[l] < MPG_LINK_FREE || d->link_parent[l] > d->n_joints)
      return set_error(MPG_E_INVALID, "bad link_parent");
    if (l > 0 && d->link_parent[l] != MPG_LINK_FREE && d->link_parent[l - 1] == MPG_LINK_FREE)
      return set_error(MPG_E_INVALID, "free frames (link_parent MPG_LINK_FREE) must be the trailing links");
  }
  for (int g = 0; g < d->n_geoms; ++g) {
    const int t = d->geom_type[g];
    if (t < MPG_GEOM_CONVEX || t > MPG_GEOM_TRIANGLE) return set_error(MPG_E_UNSUPPORTED, "unsupported geometry type");
    if (t == MPG_GEOM_TRIANGLE && (d->geom_vertex_count[g] != 3 || d->geom_vertex_start[g] < 0 ||
                                   (int64_t)d->geom_vertex_start[g] + 3 > d->n_vertices))
      return set_error(MPG_E_INVALID, "a TriangleP needs 3 vertices inside the vertex array");
    if (t == MPG_GEOM_ELLIPSOID || t == MPG_GEOM_CONE) {
      const double* p = d->geom_param + 4 * g;
      const int np = t == MPG_GEOM_ELLIPSOID ? 3 : 2;
      for (int k = 0; k < np; ++k)
        if (!(p[k] > 0.0 && std::isfinite(p[k])))
          return set_error(MPG_E_INVALID, "ellipsoid radii / cone radius and lz must be positive and finite");
    }
    if (t == MPG_GEOM_CONVEX || t == MPG_GEOM_MESH) {
      if (d->geom_vertex_count[g] <= 0 || d->geom_vertex_start[g] < 0 ||
          (int64_t)d->geom_vertex_start[g] + d->geom_vertex_count[g] > d->n_vertices)
        return set_error(MPG_E_INVALID, "convex vertex range out of bounds");
    }
    if (t == MPG_GEOM_CONVEX) {  // faces (FCL layout) inside convex_face, indices inside the hull
      const double f0 = d->geom_param[4 * g], fn = d->geom_param[4 * g + 1];
      if (!(f0 >= 0 && fn >= 0 && f0 == std::floor(f0) && fn == std::floor(fn)))
        return set_error(MPG_E_INVALID, "convex face range out of bounds");
      if (fn > 0) {
        if (!d->convex_face) return set_error(MPG_E_INVALID, "bad convex face array");
        int64_t i = (int64_t)f0;
        for (int64_t f = 0; f < (int64_t)fn; ++f) {
          if (i >= d->n_convex_face_ints) return set_error(MPG_E_INVALID, "convex face range out of bounds");
          const int cnt = d->convex_face[i];
          if (cnt < 1 || i + cnt >= d->n_convex_face_ints) return set_error(MPG_E_INVALID, "convex face range out of bounds");
          for (int k = 1; k <= cnt; ++k)
            if (d->convex_face[i + k] < 0 || d->convex_face[i + k] >= d->geom_vertex_count[g])
              return set_error(MPG_E_INVALID, "convex face vertex index out of range");
          i += cnt + 1;
        }
      }
    }
    if (t == MPG_GEOM_MESH) {
      const double t0 = d->geom_param[4 * g], tn = d->geom_param[4 * g + 1];
      if (!(t0 >= 0 && tn >= 0 && t0 == std::floor(t0) && tn == std::floor(tn) && t0 + tn <= (double)d->n_mesh_triangles))
        return set_error(MPG_E_INVALID, "mesh triangle range out of bounds");
      if (tn > 0 && !d->mesh_triangle) return set_error(MPG_E_INVALID, "bad mesh triangle array");
      for (int64_t i = (int64_t)t0; i < (int64_t)(t0 + tn); ++i)
        for (int k = 0; k < 3; ++k)
          if (d->mesh_triangle[3 * i + k] < 0 || d->mesh_triangle[3 * i + k] >= d->geom_vertex_count[g])
            return set_error(MPG_E_INVALID, "mesh triangle vertex index out of range");
    }
  }
  for (int m = 0; m < d->n_moving; ++m) {
    if (d->moving_link[m] < 0 || d->moving_link[m] >= d->n_links) return set_error(MPG_E_INVALID, "bad moving_link");
    if (d->moving_geom[m] < 0 || d->moving_geom[m] >= d->n_geoms) return set_error(MPG_E_INVALID, "bad moving_geom");
  }
  // one object per free frame, at the frame itself: its world transform is
  // the frame's isometry, bit for bit (compound movable bodies: out of scope)
  for (int l = 0; l < d->n_links; ++l) {
    if (d->link_parent[l] != MPG_LINK_FREE) continue;
    int count = 0;
    for (int m = 0; m < d->n_moving; ++m) {
      if (d->moving_link[m] != l) continue;
      ++count;
      static const double ident[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
      for (int k = 0; k < 12; ++k)
        if (!(d->moving_offset[12 * (size_t)m + k] == ident[k]))
          return set_error(MPG_E_INVALID, "the object of a free frame needs the identity moving_offset");
    }
    if (count != 1) return set_error(MPG_E_INVALID, "a free frame carries exactly one object");
  }
  if (d->n_mesh_triangles < 0 || (d->n_mesh_triangles > 0 && !d->mesh_triangle))
    return set_error(MPG_E_INVALID, "bad mesh triangle array");
  if (d->n_octree_leaves < 0 || (d->n_octree_leaves > 0 && !d->octree_leaf))
    return set_error(MPG_E_INVALID, "bad octree leaf array");
  for (int g = 0; g < d->n_geoms; ++g) {
    if (d->geom_type[g] != MPG_GEOM_OCTREE) continue;
    const double l0 = d->geom_param[4 * g], ln = d->geom_param[4 * g + 1];
    if (!(l0 >= 0 && ln >= 0 && l0 == std::floor(l0) && ln == std::floor(ln) && l0 + ln <= (double)d->n_octree_leaves))
      return set_error(MPG_E_INVALID, "octree leaf range out of bounds");
  }
  if (!finite_all(d->octree_leaf, 6 * (size_t)d->n_octree_leaves))
    return set_error(MPG_E_INVALID, "non-finite octree leaf");
  for (int s = 0; s < d->n_static; ++s)
    if (d->static_geom[s] < 0 || d->static_geom[s] >= d->n_geoms) return set_error(MPG_E_INVALID, "bad static_geom");
  const int nobj = d->n_moving + d->n_static;
  for (int p = 0; p < d->n_pairs; ++p) {
    const int a = d->pair_a[p], b = d->pair_b[p];
    if (a < 0 || a >= nobj || b < 0 || b >= nobj) return set_error(MPG_E_INVALID, "pair object id out of range");
    if (a >= d->n_moving && b >= d->n_moving) return set_error(MPG_E_INVALID, "static-static pair");
    // a movable object (on a free frame) only meets link-borne objects: the
    // cull's far test drops it against the ball that holds those
    const bool fa = desc_obj_movable(d, a), fb = desc_obj_movable(d, b);
    if ((fa && (fb || b >= d->n_moving)) || (fb && a >= d->n_moving))
      return set_error(MPG_E_INVALID, "a movable object pairs with link-borne objects only (not static, not movable)");
    // an OcTree may ride on a link or an attached body (attachObject takes any
    // FCL geometry, planning_world.cpp:174-191), and meet another OcTree
    // (octree_octree_wave; its contacts and distance are refused per call)
    // FCL 0.7.0 GJKSolver_libccd: box-box, sphere-sphere, sphere-box,
    // sphere-capsule and sphere-cylinder have closed forms (all on the
    // device, closed_form_kind); every other shape pair is MPR
    if (!(d->pair_allowed && d->pair_allowed[p])) {
      const int ta = obj_geom_type(d, a), tb = obj_geom_type(d, b);
      const bool tri = ta == MPG_GEOM_TRIANGLE || tb == MPG_GEOM_TRIANGLE;
      if (tri && (ta == MPG_GEOM_MESH || tb == MPG_GEOM_MESH || ta == MPG_GEOM_OCTREE || tb == MPG_GEOM_OCTREE))
        return set_error(MPG_E_UNSUPPORTED, "a TriangleP paired with an OcTree or BVH mesh is not implemented");
    }
    if (d->gjk_solver == MPG_GJK_INDEP && !(d->pair_allowed && d->pair_allowed[p])) {
      const int ta = obj_geom_type(d, a), tb = obj_geom_type(d, b);
      if (ta == MPG_GEOM_MESH || tb == MPG_GEOM_MESH || ta == MPG_GEOM_OCTREE || tb == MPG_GEOM_OCTREE)
        return set_error(MPG_E_UNSUPPORTED,
                         "gjk_solver MPG_GJK_INDEP with an OcTree or BVH mesh in a pair is not implemented");
    }
  }
  if (!finite_all(d->joint_placement, 12 * (size_t)d->n_joints) || !finite_all(d->link_placement, 12 * (size_t)d->n_links) ||
      !finite_all(d->vertices, 3 * (size_t)d->n_vertices))
    return set_error(MPG_E_INVALID, "non-finite value in descriptor");
  if (!(d->gjk_tolerance > 0)) return set_error(MPG_E_INVALID, "gjk_tolerance must be > 0");
  return MPG_OK;
}

void geom_record(const mpg_world_desc* d, int g, double* rec) {
  for (int k = 0; k < G_STRIDE; ++k) rec[k] = 0.0;
  for (int k = 0; k < 4; ++k) rec[G_PARAM + k] = d->geom_param[4 * g + k];
  const int t = d->geom_type[g];
  double lo[3], hi[3];
  if (t == MPG_GEOM_CONVEX || t == MPG_GEOM_MESH) {
    const double* V = d->vertices + 3 * (size_t)d->geom_vertex_start[g];
    const int nv = d->geom_vertex_count[g];
    // FCL 0.7.0 Convex: interior point = (sum of vertices) * (1.0 / n)
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < nv; ++i) {
      s[0] += V[3 * i];
      s[1] += V[3 * i + 1];
      s[2] += V[3 * i + 2];
    }
    const double inv = 1.0 / (double)nv;
    for (int k = 0; k < 3; ++k) rec[G_INTERIOR + k] = s[k] * inv;
    for (int k = 0; k < 3; ++k) lo[k] = hi[k] = V[k];
    for (int i = 1; i < nv; ++i)
      for (int k = 0; k < 3; ++k) {
        lo[k] = std::min(lo[k], V[3 * i + k]);
        hi[k] = std::max(hi[k], V[3 * i + k]);
      }
  } else if (t == MPG_GEOM_BOX) {
    for (int k = 0; k < 3; ++k) {
      hi[k] = d->geom_param[4 * g + k] / 2.0;
      lo[k] = -hi[k];
    }
  } else if (t == MPG_GEOM_SPHERE) {
    for (int k = 0; k < 3; ++k) {
      hi[k] = d->geom_param[4 * g];
      lo[k] = -hi[k];
    }
  } else if (t == MPG_GEOM_TRIANGLE) {  // triCreateGJKObject: centre ((a + b) + c) / 3
    const double* V = d->vertices + 3 * (size_t)d->geom_vertex_start[g];
    for (int k = 0; k < 3; ++k) {
      rec[G_INTERIOR + k] = (V[k] + V[3 + k] + V[6 + k]) / 3;
      lo[k] = std::min(V[k], std::min(V[3 + k], V[6 + k]));
      hi[k] = std::max(V[k], std::max(V[3 + k], V[6 + k]));
    }
  } else if (t == MPG_GEOM_ELLIPSOID) {
    for (int k = 0; k < 3; ++k) {
      hi[k] = d->geom_param[4 * g + k];
      lo[k] = -hi[k];
    }
  } else if (t == MPG_GEOM_OCTREE) {  // union of the occupied leaf boxes (octree frame)
    const int64_t l0 = (int64_t)d->geom_param[4 * g], ln = (int64_t)d->geom_param[4 * g + 1];
    for (int k = 0; k < 3; ++k) {
      lo[k] = ln > 0 ? DBL_MAX : 0.0;
      hi[k] = ln > 0 ? -DBL_MAX : 0.0;
    }
    for (int64_t i = l0; i < l0 + ln; ++i)
      for (int k = 0; k < 3; ++k) {
        lo[k] = std::min(lo[k], d->octree_leaf[6 * i + k]);
        hi[k] = std::max(hi[k], d->octree_leaf[6 * i + 3 + k]);
      }
  } else {  // capsule / cylinder / cone along z
    const double r = d->geom_param[4 * g], hz = d->geom_param[4 * g + 1] / 2.0 + (t == MPG_GEOM_CAPSULE ? r : 0.0);
    lo[0] = lo[1] = -r;
    hi[0] = hi[1] = r;
    lo[2] = -hz;
    hi[2] = hz;
  }
  // local box, widened by a relative epsilon so rounding never shrinks it
  double r2 = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double c = 0.5 * (lo[k] + hi[k]);
    const double e = 0.5 * (hi[k] - lo[k]);
    rec[G_OBB_C + k] = c;
    rec[G_OBB_E + k] = e * (1.0 + 1e-12) + 1e-12;
    rec[G_AABB_E + k] = (hi[k] - lo[k]) * 0.5;
    r2 += rec[G_OBB_E + k] * rec[G_OBB_E + k];
  }
  if (t == MPG_GEOM_CONVEX || t == MPG_GEOM_MESH || t == MPG_GEOM_TRIANGLE) {  // bounding sphere about the box centre: farthest vertex
    const double* V = d->vertices + 3 * (size_t)d->geom_vertex_start[g];
    r2 = 0.0;
    for (int i = 0; i < d->geom_vertex_count[g]; ++i) {
      double s2 = 0.0;
      for (int k = 0; k < 3; ++k) {
        const double dv = V[3 * i + k] - rec[G_OBB_C + k];
        s2 += dv * dv;
      }
      r2 = std::max(r2, s2);
    }
  }
  rec[G_RADIUS] = std::sqrt(r2) * (1.0 + 1e-12) + 1e-12;
  double vmax = 0.0;
  if (t == MPG_GEOM_CONVEX) {
    const double* V = d->vertices + 3 * (size_t)d->geom_vertex_start[g];
    for (int i = 0; i < 3 * d->geom_vertex_count[g]; ++i) vmax = std::max(vmax, std::fabs(V[i]));
  }
  rec[G_VMAX] = vmax;
}

// ---------------------------------------------------------------------------
// FCL 0.7.0 BVHModel<OBBRSS>::endModel -> buildTree for the meshes
// (load_mesh_as_BVH, src/urdf_utils.cpp:136-155) [ext FCL BVH_model-inl.h,
// BV_fitter-inl.h, BV_splitter-inl.h, math/geometry-inl.h; restated, FCL is
// not under /root/reference]: BVFitter<OBBRSS>::fit (covariance of the
// node's triangle vertices, Jacobi eigen_old, axisFromEigen, extent and
// centre of the projections; only the OBB half decides collisions), the
// SPLIT_METHOD_MEAN rule along the first axis (centroid . axis > mean goes
// right, the rest are swapped to the front; an empty side -> n / 2), child
// pairs allocated at num_bvs before recursing.  The oracle builds the same
// tree from its own code (oracle/collide_oracle.c orc_bvh_build).
// ---------------------------------------------------------------------------
struct FclBvh {
  std::vector<double> box;  // [n][FB_STRIDE]
  std::vector<int> link;    // [n][3]
  int max_depth = 0;        // deepest leaf (root = 0), bounds the device gates' descent
};

// eigen_old: Jacobi rotations; vout(r, c) = v[c][r], dout = eigenvalues
void fcl_eigen_old(const double m[9], double dout[3], double vout[9]) {
  double R[3][3] = {{m[0], m[1], m[2]}, {m[3], m[4], m[5]}, {m[6], m[7], m[8]}};
  double b[3], z[3], v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, d[3];
  for (int ip = 0; ip < 3; ++ip) {
    b[ip] = d[ip] = R[ip][ip];
    z[ip] = 0;
  }
  for (int i = 0; i < 50; ++i) {
    double sm = 0;
    for (int ip = 0; ip < 3; ++ip)
      for (int iq = ip + 1; iq < 3; ++iq) sm += std::fabs(R[ip][iq]);
    if (sm == 0.0) {
      for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) vout[3 * r + c] = v[c][r];
      for (int k = 0; k < 3; ++k) dout[k] = d[k];
      return;
    }
    const double tresh = i < 3 ? 0.2 * sm / (3 * 3) : 0.0;
    for (int ip = 0; ip < 3; ++ip)
      for (int iq = ip + 1; iq < 3; ++iq) {
        double g = 100.0 * std::fabs(R[ip][iq]);
        if (i > 3 && std::fabs(d[ip]) + g == std::fabs(d[ip]) && std::fabs(d[iq]) + g == std::fabs(d[iq])) {
          R[ip][iq] = 0.0;
        } else if (std::fabs(R[ip][iq]) > tresh) {
          double h = d[iq] - d[ip], t;
          if (std::fabs(h) + g == std::fabs(h)) {
            t = R[ip][iq] / h;
          } else {
            const double theta = 0.5 * h / R[ip][iq];
            t = 1.0 / (std::fabs(theta) + std::sqrt(1.0 + theta * theta));
            if (theta < 0.0) t = -t;
          }
          const double c = 1.0 / std::sqrt(1 + t * t), s = t * c, tau = s / (1.0 + c);
          h = t * R[ip][iq];
          z[ip] -= h;
          z[iq] += h;
          d[ip] -= h;
          d[iq] += h;
          R[ip][iq] = 0.0;
          auto rot = [&](double& x, double& y) {
            const double gg = x, hh = y;
            x = gg - s * (hh + gg * tau);
            y = hh + s * (gg - hh * tau);
          };
          for (int j = 0; j < ip; ++j) rot(R[j][ip], R[j][iq]);
          for (int j = ip + 1; j < iq; ++j) rot(R[ip][j], R[j][iq]);
          for (int j = iq + 1; j < 3; ++j) rot(R[ip][j], R[iq][j]);
          for (int j = 0; j < 3; ++j) rot(v[j][ip], v[j][iq]);
        }
      }
    for (int ip = 0; ip < 3; ++ip) {
      b[ip] += z[ip];
      d[ip] = b[ip];
      z[ip] = 0.0;
    }
  }
}

// covariance sums -> M -> eigen -> axisFromEigen -> extent / centre of pts
void fcl_fit_obb(const double S1[3], const double S2[6], double n_points, const std::vector<const double*>& pts,
                 double* box) {
  double M[9], E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, ev[3] = {0, 0, 0};
  M[0] = S2[0] - S1[0] * S1[0] / n_points;
  M[4] = S2[1] - S1[1] * S1[1] / n_points;
  M[8] = S2[2] - S1[2] * S1[2] / n_points;
  M[1] = M[3] = S2[3] - S1[0] * S1[1] / n_points;
  M[5] = M[7] = S2[5] - S1[1] * S1[2] / n_points;
  M[2] = M[6] = S2[4] - S1[0] * S1[2] / n_points;
  fcl_eigen_old(M, ev, E);
  int mn, mid, mx;
  if (ev[0] > ev[1]) {
    mx = 0;
    mn = 1;
  } else {
    mn = 0;
    mx = 1;
  }
  if (ev[2] < ev[mn]) {
    mid = mn;
    mn = 2;
  } else if (ev[2] > ev[mx]) {
    mid = mx;
    mx = 2;
  } else {
    mid = 2;
  }
  double* ax = box + FB_AXIS;
  for (int r = 0; r < 3; ++r) {
    ax[3 * r] = E[3 * mx + r];
    ax[3 * r + 1] = E[3 * mid + r];
  }
  ax[2] = ax[3] * ax[7] - ax[6] * ax[4];
  ax[5] = ax[6] * ax[1] - ax[0] * ax[7];
  ax[8] = ax[0] * ax[4] - ax[3] * ax[1];
  double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
  for (const double* p : pts)
    for (int k = 0; k < 3; ++k) {
      const double pr = (ax[k] * p[0] + ax[3 + k] * p[1]) + ax[6 + k] * p[2];
      if (pr > hi[k]) hi[k] = pr;
      if (pr < lo[k]) lo[k] = pr;
    }
  double o[3];
  for (int k = 0; k < 3; ++k) o[k] = (hi[k] + lo[k]) / 2;
  for (int i = 0; i < 3; ++i) box[FB_TO + i] = (ax[3 * i] * o[0] + ax[3 * i + 1] * o[1]) + ax[3 * i + 2] * o[2];
  for (int k = 0; k < 3; ++k) box[FB_EXT + k] = (hi[k] - lo[k]) * 0.5;
}

void fcl_bvh_node(FclBvh& B, const double* V, const int32_t* tri, std::vector<int>& prim, int id, int first, int n,
                  int base, int depth = 0) {
  if (depth > B.max_depth) B.max_depth = depth;
  int* cur = prim.data() + first;
  double S1[3] = {0, 0, 0}, S2[6] = {0, 0, 0, 0, 0, 0};
  std::vector<const double*> pts;
  pts.reserve(3 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    const int32_t* t = tri + 3 * cur[i];
    const double *p1 = V + 3 * t[0], *p2 = V + 3 * t[1], *p3 = V + 3 * t[2];
    for (int k = 0; k < 3; ++k) S1[k] += (p1[k] + p2[k]) + p3[k];
    S2[0] += (p1[0] * p1[0] + p2[0] * p2[0]) + p3[0] * p3[0];
    S2[1] += (p1[1] * p1[1] + p2[1] * p2[1]) + p3[1] * p3[1];
    S2[2] += (p1[2] * p1[2] + p2[2] * p2[2]) + p3[2] * p3[2];
    S2[3] += (p1[0] * p1[1] + p2[0] * p2[1]) + p3[0] * p3[1];
    S2[4] += (p1[0] * p1[2] + p2[0] * p2[2]) + p3[0] * p3[2];
    S2[5] += (p1[1] * p1[2] + p2[1] * p2[2]) + p3[1] * p3[2];
    pts.push_back(p1);
    pts.push_back(p2);
    pts.push_back(p3);
  }
  double* box = B.box.data() + (size_t)FB_STRIDE * (base + id);
  fcl_fit_obb(S1, S2, 3.0 * n, pts, box);
  int* lk = B.link.data() + 3 * (size_t)(base + id);
  lk[1] = first;
  lk[2] = n;
  if (n == 1) {
    lk[0] = -(cur[0] + 1);
    return;
  }
  const double sv[3] = {box[FB_AXIS], box[FB_AXIS + 3], box[FB_AXIS + 6]};
  double c[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const int32_t* t = tri + 3 * cur[i];
    for (int k = 0; k < 3; ++k) c[k] += (V[3 * t[0] + k] + V[3 * t[1] + k]) + V[3 * t[2] + k];
  }
  const double split = ((c[0] * sv[0] + c[1] * sv[1]) + c[2] * sv[2]) / (3 * n);
  const int child = (int)(B.link.size() / 3) - base;  // num_bvs
  lk[0] = base + child;
  B.box.resize(B.box.size() + 2 * FB_STRIDE);
  B.link.resize(B.link.size() + 6);
  int c1 = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t* t = tri + 3 * cur[i];
    double p[3];
    for (int k = 0; k < 3; ++k) p[k] = ((V[3 * t[0] + k] + V[3 * t[1] + k]) + V[3 * t[2] + k]) / 3.0;
    if (!(((sv[0] * p[0] + sv[1] * p[1]) + sv[2] * p[2]) > split)) std::swap(cur[i], cur[c1++]);
  }
  if (c1 == 0 || c1 == n) c1 = n / 2;
  fcl_bvh_node(B, V, tri, prim, child, first, c1, base, depth + 1);
  fcl_bvh_node(B, V, tri, prim, child + 1, first + c1, n - c1, base, depth + 1);
}

// computeBV<OBB>(shape, identity): box I / side/2; sphere I / r; capsule
// I / (r, r, lz/2 + r); cylinder and cone I / (r, r, lz/2); ellipsoid I /
// radii; convex: fitn over the
// vertices (covariance of the points)
void fcl_shape_obb(const mpg_world_desc* d, int g, double* o) {
  std::fill(o, o + FB_STRIDE, 0.0);
  o[FB_AXIS] = o[FB_AXIS + 4] = o[FB_AXIS + 8] = 1.0;
  const double* p = d->geom_param + 4 * g;
  switch (d->geom_type[g]) {
    case MPG_GEOM_BOX:
      for (int k = 0; k < 3; ++k) o[FB_EXT + k] = p[k] * 0.5;
      break;
    case MPG_GEOM_SPHERE:
      o[FB_EXT] = o[FB_EXT + 1] = o[FB_EXT + 2] = p[0];
      break;
    case MPG_GEOM_CAPSULE:
      o[FB_EXT] = o[FB_EXT + 1] = p[0];
      o[FB_EXT + 2] = p[1] / 2 + p[0];
      break;
    case MPG_GEOM_CYLINDER:
    case MPG_GEOM_CONE:
      o[FB_EXT] = o[FB_EXT + 1] = p[0];
      o[FB_EXT + 2] = p[1] / 2;
      break;
    case MPG_GEOM_ELLIPSOID:
      for (int k = 0; k < 3; ++k) o[FB_EXT + k] = p[k];
      break;
    case MPG_GEOM_CONVEX: {
      const double* V = d->vertices + 3 * (size_t)d->geom_vertex_start[g];
      const int nv = d->geom_vertex_count[g];
      double S1[3] = {0, 0, 0}, S2[6] = {0, 0, 0, 0, 0, 0};
      std::vector<const double*> pts;
      for (int i = 0; i < nv; ++i) {
        const double* q = V + 3 * i;
        for (int k = 0; k < 3; ++k) S1[k] += q[k];
        S2[0] += q[0] * q[0];
        S2[1] += q[1] * q[1];
        S2[2] += q[2] * q[2];
        S2[3] += q[0] * q[1];
        S2[4] += q[0] * q[2];
        S2[5] += q[1] * q[2];
        pts.push_back(q);
      }
      if (nv > 0) fcl_fit_obb(S1, S2, (double)nv, pts, o);
      break;
    }
    default:
      break;
  }
}

void static_record(const mpg_world_desc* d, int s, const double* geom_rec_all, double* rec) {
  const double* T = d->static_transform + 12 * s;
  const CQ4 r = gjk_rot_from_matrix(T);  // the ccd_real rotation MPR uses
  const CQ4 ri = quat_invert2(r);
  rec[S_ROT] = r.x; rec[S_ROT + 1] = r.y; rec[S_ROT + 2] = r.z; rec[S_ROT + 3] = r.w;
  rec[S_ROTINV] = ri.x; rec[S_ROTINV + 1] = ri.y; rec[S_ROTINV + 2] = ri.z; rec[S_ROTINV + 3] = ri.w;
  rec[S_POS] = T[9]; rec[S_POS + 1] = T[10]; rec[S_POS + 2] = T[11];
  // broad-phase OBB from the same rotation MPR uses
  double R[9];
  quat_to_mat(r.w, r.x, r.y, r.z, R);
  const double* g = geom_rec_all + G_STRIDE * d->static_geom[s];
  for (int i = 0; i < 3; ++i)
    rec[S_OBBC + i] = ((R[3 * i] * g[G_OBB_C] + R[3 * i + 1] * g[G_OBB_C + 1]) + R[3 * i + 2] * g[G_OBB_C + 2]) + T[9 + i];
  for (int k = 0; k < 9; ++k) rec[S_R + k] = R[k];
}

// cull_lds_per_thread, choose_block (the cull's block size and LDS): mpg_broadphase.h
