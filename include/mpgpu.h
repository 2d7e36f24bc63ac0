/*
 * mpgpu.h -- C ABI of the MI355X batched state-validity checker.
 *
 * This is the drop-in boundary beneath MPlib's PlanningWorld::collide() /
 * collideFull() and the OMPL isStateValid() inner loop.  Plain C, plain
 * pointers and sizes, no C++ or torch types; every call returns an int
 * status (0 = ok) and never throws.  The text of the last error on the
 * calling thread is available from mpg_last_error().
 *
 * Reference interfaces replaced (KolinGuo/MPlib 0.1.1, paths relative to the
 * reference root):
 *   mpg_world_create     <- the mutable FCL/pinocchio state that
 *                           PlanningWorldTpl (src/planning_world.h:52-312),
 *                           ArticulatedModelTpl (src/articulated_model.cpp:15-36),
 *                           FCLModelTpl::init (src/fcl_model.cpp:268-294) and
 *                           AllowedCollisionMatrix (src/collision_matrix.h) hold,
 *                           frozen into an immutable device snapshot.
 *   mpg_collide_batch    <- N x { PlanningWorldTpl::setQposAll(q)
 *                                 (src/planning_world.cpp:250-262);
 *                                 PlanningWorldTpl::collideFull(CollisionRequest())
 *                                 (src/planning_world.cpp:484-490) }
 *                           flags[i]  == collide() (src/planning_world.h:248-250)
 *                           pair_mask == which pairs collideFull() reports,
 *                           after filterCollisions (src/planning_world.cpp:265-274).
 *                           Also the OMPL ValidityCheckerTpl::isValid batch
 *                           (src/ompl_planner.h:59-62): valid = !flags[i].
 *   mpg_fk_batch         <- N x { PinocchioModelTpl::computeForwardKinematics
 *                                 (src/pinocchio_model.cpp:272-274);
 *                                 getLinkPose(i) for every user link
 *                                 (src/pinocchio_model.cpp:277-312) }
 *   mpg_world_destroy    <- shared_ptr release of the above.
 *
 * Memory: buffers are caller-owned.  With MPG_MEM_DEVICE every pointer is a
 * device pointer on the world's device and the work is enqueued on `stream`
 * (a hipStream_t, NULL = default stream) without synchronising.  With
 * MPG_MEM_HOST the call copies through internal device staging buffers and
 * returns after the results are back on the host; batches above the latency
 * path's size (mpg_set_small_batch_max) run as chunks through a pinned ring:
 * the input of one chunk crosses PCIe while earlier chunks compute and are
 * unpacked (internal threads and streams; the call is still synchronous).
 *
 * Threading: a world is immutable after creation, but for the current poses
 * of its free frames (mpg_world_set_free_poses, which is not concurrent with
 * any other call on the world); concurrent calls on one
 * world from several host threads are allowed when each uses its own stream
 * and MPG_MEM_DEVICE.  MPG_MEM_HOST calls on one world are serialised.
 * mpg_distance_batch* and mpg_check_motion_batch use scratch owned by the
 * world: their MPG_MEM_DEVICE calls from several streams are ordered on the
 * device (each waits for the previous call's work), never overlapped.
 */
#ifndef MPGPU_H
#define MPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPG_VERSION_MAJOR 0
#define MPG_VERSION_MINOR 3

/* status codes */
#define MPG_OK 0
#define MPG_E_INVALID 1     /* bad argument / descriptor                    */
#define MPG_E_UNSUPPORTED 2 /* request or geometry pair not implemented     */
#define MPG_E_HIP 3         /* HIP runtime error                            */
#define MPG_E_NOMEM 4
#define MPG_E_FAILED 5      /* the reference itself fails on this input
                               (FCL throws: mpg_distance_batch_req)      */

/* memory kinds for the batch calls */
#define MPG_MEM_HOST 0
#define MPG_MEM_DEVICE 1

/* pinocchio joint models (pinocchio 2.6.21 JointCollectionDefault subset) */
#define MPG_JOINT_RX 0
#define MPG_JOINT_RY 1
#define MPG_JOINT_RZ 2
#define MPG_JOINT_REVOLUTE_UNALIGNED 3
#define MPG_JOINT_PX 4
#define MPG_JOINT_PY 5
#define MPG_JOINT_PZ 6
#define MPG_JOINT_PRISMATIC_UNALIGNED 7
#define MPG_JOINT_RUBX 8  /* continuous joints: user value v -> (cos v, sin v) */
#define MPG_JOINT_RUBY 9
#define MPG_JOINT_RUBZ 10
#define MPG_JOINT_RUB_UNALIGNED 11

/* FCL geometry kinds supported on the device */
#define MPG_GEOM_CONVEX 0   /* fcl::Convex   : vertices, param = first face
                               int, face count (convex_face)             */
#define MPG_GEOM_BOX 1      /* fcl::Box      : param = side x, y, z          */
#define MPG_GEOM_SPHERE 2   /* fcl::Sphere   : param = radius                */
#define MPG_GEOM_CAPSULE 3  /* fcl::Capsule  : param = radius, lz            */
#define MPG_GEOM_CYLINDER 4 /* fcl::Cylinder : param = radius, lz            */
#define MPG_GEOM_OCTREE 5   /* fcl::OcTree   : param = first leaf, leaf count,
                               resolution; static, on a link or attached;
                               a pair of two OcTrees collides (leaf OBBs),
                               its contacts / distance are refused      */
#define MPG_GEOM_MESH 6     /* fcl::BVHModel<OBBRSS> (non-convex mesh):
                               vertices, param = first triangle, triangle
                               count (mesh_triangle)                     */
#define MPG_GEOM_ELLIPSOID 7 /* fcl::Ellipsoid : param = radii a, b, c
                                (python/pybind_fcl.hpp:137-141); libccd
                                supportEllipsoid, MPR with every partner */
#define MPG_GEOM_CONE 8      /* fcl::Cone : param = radius, lz, apex at
                                +lz/2 (python/pybind_fcl.hpp:95-98); libccd
                                supportCone, MPR with every partner       */
#define MPG_GEOM_TRIANGLE 9  /* fcl::TriangleP : vertices a, b, c (vertex
                                count 3, python/pybind_fcl.hpp:168-175);
                                libccd supportTriangle / centerTriangle,
                                MPR with every shape (not paired with an
                                OcTree or BVH mesh)                        */

/*
 * World descriptor.  SE3 values are 12 doubles: a row-major 3x3 rotation
 * followed by the translation.  All arrays are read during
 * mpg_world_create only.
 */
typedef struct mpg_world_desc {
  /* --- kinematics: pinocchio joints 1..n_joints (universe omitted) ------- */
  int32_t n_joints;
  const int32_t *joint_type;     /* MPG_JOINT_*                               */
  const int32_t *joint_parent;   /* parent joint, 0 = universe, else 1-based  */
  const double *joint_axis;      /* [n_joints*3] (unaligned joints only)      */
  const double *joint_placement; /* [n_joints*12] model.jointPlacements       */
  /* joint value source: dof slot d >= 0 reads q[i*dof + d]; -1 uses
   * joint_value_const (fixed, non-move-group joints keep current_qpos_,
   * src/articulated_model.cpp:104-113).                                    */
  const int32_t *joint_q_source; /* [n_joints]                             */
  const double *joint_q_const;   /* [n_joints]                             */
  int32_t dof;                   /* move-group dimension = row length of q */

  /* --- user links (PinocchioModel::setLinkOrder) ---------------------------- */
  int32_t n_links;
  const int32_t *link_parent;     /* frame.parent joint (0 = universe), or
                                     MPG_LINK_FREE: a free frame            */
  const double *link_placement;   /* [n_links*12] frame.placement (of a free
                                     frame: its initial world pose)         */
  /* Free frames.  A user link with link_parent == MPG_LINK_FREE has no joint
   * above it: its pose is an input (mpg_world_set_free_poses,
   * mpg_collide_batch_free, the rows of mpg_collide_link_poses).  Free frames
   * are the trailing entries of the link arrays (n_free, their count, is
   * derived).  Each carries exactly one moving object with the identity
   * moving_offset -- a movable object, whose world transform is the frame's
   * isometry itself (the rotation matrix of the pose's quaternion, Eigen's
   * toRotationMatrix, and the position: the same 12 doubles a static object
   * created at that pose has in static_transform).  A pair with a movable
   * object has a link-borne moving object (robot or attached body) as its
   * other member: movable x static and movable x movable pairs, a second
   * object on a free frame or another offset are MPG_E_INVALID.  Every
   * geometry kind is allowed on a free frame, with the pair refusals above.
   * The initial current pose is link_placement as (p, wxyz), the quaternion by
   * the conversion mpg_fk_batch applies to every link.                     */

  /* --- geometry ------------------------------------------------------------- */
  int32_t n_geoms;
  const int32_t *geom_type;       /* MPG_GEOM_*                             */
  const int32_t *geom_vertex_start;
  const int32_t *geom_vertex_count;
  const double *geom_param;       /* [n_geoms*4]                            */
  int64_t n_vertices;
  const double *vertices;         /* [n_vertices*3] Convex vertices, local  */

  /* --- moving objects: robot collision objects then attached bodies -------- */
  int32_t n_moving;
  const int32_t *moving_link;     /* user link index                        */
  const int32_t *moving_geom;
  const double *moving_offset;    /* [n_moving*12] link -> object pose      */

  /* --- static scene objects -------------------------------------------------- */
  int32_t n_static;
  const int32_t *static_geom;
  const double *static_transform; /* [n_static*12] world pose               */

  /* --- pairs, in output-bit order. Object ids: [0, n_moving) moving,
   *     [n_moving, n_moving + n_static) static.  (pair_a[p], pair_b[p]) keeps
   *     fcl::collide's (o1, o2) argument order.                              */
  int32_t n_pairs;
  const int32_t *pair_a;
  const int32_t *pair_b;
  const uint8_t *pair_allowed;    /* 1: ACM allows it (never reported)      */

  /* --- CollisionRequest -------------------------------------------------------- */
  double gjk_tolerance;           /* CollisionRequest::gjk_tolerance (1e-6) */

  /* --- octrees (MPG_GEOM_OCTREE): the occupied leaves of every octree
   *     geometry as axis-aligned boxes in the octree frame, [min xyz, max xyz]
   *     per leaf, as fcl::OcTree's getRootBV / computeChildBV recursion
   *     yields them (PlanningWorldTpl::addPointCloud, planning_world.cpp:102-110) */
  int64_t n_octree_leaves;
  const double *octree_leaf;      /* [n_octree_leaves*6]                    */

  /* --- BVH meshes (MPG_GEOM_MESH, load_mesh_as_BVH, src/urdf_utils.cpp:
   *     136-155): triangles as three vertex indices relative to the mesh's
   *     geom_vertex_start */
  int64_t n_mesh_triangles;
  const int32_t *mesh_triangle;   /* [n_mesh_triangles*3]                   */

  /* --- convex faces: fcl::Convex(vertices, num_faces, faces) keeps them and
   *     FCL 0.7.0 derives its support from them (Convex::findExtremeVertex
   *     walks the face graph when the hull has more than 32 vertices and the
   *     faces are watertight: src/urdf_utils.cpp:156-183 builds every link hull
   *     that way).  FCL layout: count, count vertex indices (relative to the
   *     geometry's geom_vertex_start), count, ...  For MPG_GEOM_CONVEX,
   *     geom_param[0] = first int of the geometry's faces in convex_face,
   *     geom_param[1] = number of faces (0 = no faces: linear support).     */
  int64_t n_convex_face_ints;
  const int32_t *convex_face;     /* [n_convex_face_ints]                   */

  /* --- joint limits (PinocchioModelTpl::getJointLimit, src/pinocchio_model.cpp:
   *     59-83): [lower, upper] of each joint value, -inf / +inf or NULL =
   *     unbounded.  Only the broad phase reads them: the travel of a prismatic
   *     move-group joint bounds the fp32 cull's coordinates.  A configuration
   *     outside them is still evaluated exactly (every pair of it goes to the
   *     narrow phase), so no input changes a result.                         */
  const double *joint_lower;      /* [n_joints] or NULL                     */
  const double *joint_upper;      /* [n_joints] or NULL                     */

  /* --- CollisionRequest::gjk_solver_type (python/pybind_fcl.hpp:264, 276):
   *     MPG_GJK_LIBCCD (0, the default, libccd MPR in float) or MPG_GJK_INDEP
   *     (FCL's own GJK in double, GJKSolver_indep::shapeIntersect) for every
   *     shape pair without an FCL closed form.  GST_INDEP worlds take shape
   *     geometry only (MPG_GEOM_OCTREE / MPG_GEOM_MESH in a non-allowed pair:
   *     MPG_E_UNSUPPORTED) and the collide entry points only (contacts:
   *     MPG_E_UNSUPPORTED; the distance calls keep libccd, as
   *     DistanceRequest's own default does).                               */
  int32_t gjk_solver;
} mpg_world_desc;

#define MPG_GJK_LIBCCD 0
#define MPG_GJK_INDEP 1
#define MPG_LINK_FREE (-1) /* link_parent of a free frame */

typedef struct mpg_world mpg_world;

typedef struct mpg_world_info {
  int32_t n_pairs;
  int32_t mask_words; /* uint32 words per configuration in pair_mask      */
  int32_t dof;
  int32_t n_links;
  int32_t device;
  int32_t block_size;
  int64_t snapshot_bytes;
} mpg_world_info;

/* Build a device snapshot of the world on `device`: immutable, except the
 * current poses of its free frames. */
int mpg_world_create(const mpg_world_desc *desc, int device, mpg_world **out);
int mpg_world_destroy(mpg_world *world);
int mpg_world_get_info(const mpg_world *world, mpg_world_info *info);

/*
 * q:         [n*dof] row-major move-group joint values (float64).
 * flags:     [n] 1 if the configuration collides (collide() == true).
 * pair_mask: [n*mask_words] bit p of word p/32 set if pair p is reported by
 *            collideFull(); may be NULL when only flags are wanted.
 */
int mpg_collide_batch(mpg_world *world, const double *q, int64_t n, uint8_t *flags,
                      uint32_t *pair_mask, int mem, void *stream);

/*
 * One host batch over several GPUs: worlds[k] (each from mpg_world_create of
 * the same descriptor, on its own device) checks the k-th contiguous shard of
 * q (the first n % n_worlds shards one row longer), all shards concurrently
 * from host threads, results written in place -- isValid is a pure function
 * of the state (src/ompl_planner.h:59-62), so no collective is involved.
 * Host buffers only; the first failing world's status is returned.  The
 * in-process counterpart of mplib_amd.dist (one process per GPU).
 */
int mpg_collide_batch_multi(mpg_world *const *worlds, int32_t n_worlds, const double *q, int64_t n,
                            uint8_t *flags, uint32_t *pair_mask);

/*
 * The shard of a batch of n configurations that part k of n_parts checks:
 * contiguous, the first n % n_parts shards one row longer (the split of
 * mpg_collide_batch_multi and of mplib_amd.dist.shard_range).  Host only.
 */
int mpg_shard_range(int64_t n, int32_t k, int32_t n_parts, int64_t *start, int64_t *count);

/*
 * Device-resident multi-GPU batch: shard k is already on worlds[k]'s device
 * -- q[k] [counts[k] * dof], flags[k] [counts[k]], pair_mask[k]
 * [counts[k] * mask_words] (pair_mask or pair_mask[k] NULL: flags only) --
 * and is enqueued on streams[k] (a hipStream_t of that device; streams or
 * streams[k] NULL: its default stream), one host thread per world; no host
 * round trip, no synchronisation (as MPG_MEM_DEVICE calls).
 * gather_flags / gather_masks (device pointers on worlds[0]'s device, NULL:
 * no gather): every shard's flags / mask rows are also copied there, shard k
 * at row counts[0] + ... + counts[k-1], device to device (peer copies over
 * xGMI on streams[k]); streams[0] then waits for all of them, so work queued
 * on streams[0] after the call sees the whole batch.  The worlds must come
 * from the same descriptor (checked by the snapshot's hash) and be distinct.
 * isValid is a pure function of the state (src/ompl_planner.h:59-62): no
 * collective is involved in the check itself.
 */
int mpg_collide_batch_multi_device(mpg_world *const *worlds, int32_t n_worlds, const double *const *q,
                                   const int64_t *counts, uint8_t *const *flags, uint32_t *const *pair_mask,
                                   void *const *streams, uint8_t *gather_flags, uint32_t *gather_masks);

/*
 * Host-buffer calls (mem == MPG_MEM_HOST) of at most `n` configurations take
 * the latency path: one launch with one wave per (pair, 64-configuration tile)
 * and one synchronisation, instead of the throughput pipeline (6 launches).
 * Identical results; default 1024 (env MPG_SMALL_BATCH_MAX), 0 disables.
 * The planner's validity batches (mplib_amd OMPLPlanner) are this size.
 */
int mpg_set_small_batch_max(mpg_world *world, int64_t n);

/*
 * Drops the device state the world keeps for one caller stream (its phase
 * A/B workspace and the internal side stream of large batches).  Call before
 * destroying a stream that was passed to MPG_MEM_DEVICE calls; without it the
 * state of at most 32 streams is kept, least recently used evicted first.
 * No reference counterpart (the reference has no device state).
 */
int mpg_release_stream(mpg_world *world, void *stream);

/*
 * Same pair evaluation as mpg_collide_batch, but the link poses are given
 * directly instead of being computed from joint values:
 * link_pose [n*n_links*7] = (px, py, pz, qw, qx, qy, qz) per user link.
 * Replaces FCLModelTpl::updateCollisionObjects(vector<Vector7>)
 * (src/fcl_model.cpp:151-167) followed by FCLModelTpl::collideFull
 * (src/fcl_model.cpp:182-193).
 */
int mpg_collide_link_poses(mpg_world *world, const double *link_pose, int64_t n, uint8_t *flags,
                           uint32_t *pair_mask, int mem, void *stream);

/*
 * Movable scene objects (worlds with free frames, see mpg_world_desc).
 *
 * mpg_world_set_free_poses replaces the world's current free poses: pose7
 * [n_free*7] = (px, py, pz, qw, qx, qy, qz) per free frame, host memory.
 * Every entry point evaluates the movable objects there afterwards
 * (mpg_collide_batch, mpg_collide_contacts, mpg_distance_batch*,
 * mpg_check_motion_batch, mpg_collide_count, mpg_fk_batch, which echoes them
 * in the free frames' columns, and the planner on top).  Nothing is rebuilt.
 * NOT concurrent with other calls on the world: it waits for the work already
 * queued on the world's device (a device synchronisation), then overwrites
 * the poses in place; the caller keeps other threads out meanwhile.
 *
 * mpg_collide_batch_free is mpg_collide_batch with the free poses given per
 * call: free_pose [free_rows * n_free * 7], free_rows == n (one pose set per
 * configuration) or 1 (one set shared by the batch); free_pose == NULL: the
 * current poses (then identical to mpg_collide_batch).  `mem` applies to q,
 * free_pose and the outputs alike.  With MPG_MEM_DEVICE the call reads the
 * caller's array from the kernels, keeps no state in the world and does not
 * synchronise: two streams may run it on one world with different pose
 * arrays.  The current poses are not modified.
 *
 * mpg_collide_link_poses and mpg_fk_batch rows are [n_links*7] with the free
 * frames included (the trailing n_free poses): the first reads them, the
 * second writes the current ones.  mpg_collide_link_poses on mpg_fk_batch's
 * kinematic columns plus free poses equals mpg_collide_batch_free.
 *
 * Pose validity.  Host-memory poses (mpg_world_set_free_poses, MPG_MEM_HOST
 * free_pose, the free columns of MPG_MEM_HOST link-pose rows) are checked: a non-finite value, or a quaternion with
 * | |q| - 1 | > 1e-6, is MPG_E_INVALID.  The bound comes from the cull
 * margin: a quaternion of norm 1 + e scales the object's rotation matrix by
 * (1 + e)^2, moving its surface by 2 e r; the margin of a world with free
 * frames is widened by 4e-6 times the largest geometry radius for it.
 * Device-memory poses are the caller's contract; no kernel indexes memory by
 * anything derived from a pose, so a bad pose can only give a wrong bit.
 *
 * Any finite pose gives the exact result: the cull drops a movable object
 * whose bounding sphere lies outside the ball that holds every link-borne
 * object (an exact fp64 test per row and object; mpg_world_get_free_info's
 * far_radius, margins included), so an object parked far away costs nothing
 * in the narrow phase and never widens the fp32 coordinate bound.
 *
 * mpg_distance_batch_free, mpg_check_motion_batch_free and
 * mpg_collide_contacts_free (declared next to the calls they extend) take
 * free_pose / free_rows after their input rows in the same way, with the same
 * rules: NULL = the current poses (then identical to the call without
 * _free, which forwards here), free_rows == 1 or n else MPG_E_INVALID, a
 * non-NULL free_pose on a world without free frames MPG_E_INVALID.
 * MPG_MEM_DEVICE arrays are read by the kernels where the caller keeps them;
 * MPG_MEM_HOST arrays are checked as below and staged in the grow-only
 * scratch of the call's family (no allocation per call once warm).
 *
 * Several objects on one free frame, mpg_collide_batch_multi* with per-call
 * poses (set the poses on each world), a movable base of an articulation and
 * poses that change along an edge are not provided.
 */
int mpg_world_set_free_poses(mpg_world *world, const double *pose7);
int mpg_collide_batch_free(mpg_world *world, const double *q, const double *free_pose, int64_t free_rows,
                           int64_t n, uint8_t *flags, uint32_t *pair_mask, int mem, void *stream);
/* n_free, the far test's radius (0 without free frames) and the current poses
 * [n_free*7] (host); any output pointer may be NULL. */
int mpg_world_get_free_info(const mpg_world *world, int32_t *n_free, double *far_radius, double *pose7);

/*
 * Batched motion validation: for each edge e, OMPL's
 * DiscreteMotionValidator::checkMotion(q_from[e], q_to[e]) over MPlib's state
 * space (src/ompl_planner.cpp:248-293: one RealVectorStateSpace(1) per
 * prismatic/revolute joint, SO2StateSpace for continuous joints, weights 1):
 *   segments[e] = max(1, ceil(distance / longest_valid_segment)),
 *   states q(j/segments), j = 1..segments (the last is q_to itself; q_from is
 *   assumed valid, as OMPL does), each checked with collide().
 *   valid[e] = 1 if every state is collision-free;
 *   first_invalid[e] = smallest colliding j, or -1 (checkMotion's lastValid).
 * so2_mask: bit i set if move-group dof i is an SO2 subspace.  first_invalid
 * and segments may be NULL.  Synchronises `stream` once (the state count
 * sizes the work).
 */
int mpg_check_motion_batch(mpg_world *world, const double *q_from, const double *q_to, int64_t n,
                           uint32_t so2_mask, double longest_valid_segment, uint8_t *valid,
                           int32_t *first_invalid, int32_t *segments, int mem, void *stream);
/* With the free poses given per call (see mpg_collide_batch_free): free_rows
 * == 1, one pose set shared by every edge, or n, one pose set per EDGE --
 * every state along edge e is checked with pose set e (the poses do not
 * change along an edge).  The device keeps one int32 per interpolated state
 * (its edge), never a pose set per state.  At most 2^31 - 1 edges with
 * per-edge poses (MPG_E_UNSUPPORTED beyond). */
int mpg_check_motion_batch_free(mpg_world *world, const double *q_from, const double *q_to,
                                const double *free_pose, int64_t free_rows, int64_t n, uint32_t so2_mask,
                                double longest_valid_segment, uint8_t *valid, int32_t *first_invalid,
                                int32_t *segments, int mem, void *stream);

/*
 * Batched distance: per configuration, PlanningWorldTpl::distanceSelf and
 * distanceOthers (src/planning_world.cpp:493-720) over the pair table, whose
 * first n_self_pairs entries form the self group: ACM-allowed pairs are
 * skipped, each pair's fcl::distance(o1 = pair_a, o2 = pair_b, request) is
 * compared with strict '<' (:513), so the first minimum wins.
 * d_*: minimum distance (DBL_MAX if the group is empty), p_*: its pair
 * index (-1 if none).  What fcl::distance computes [FCL 0.7.0, restated in
 * oracle/collide_oracle.c pair_distance and oracle/fcl_gjk_dist.h]:
 *   shape-shape   DistanceRequest(): GJKSolver_libccd::shapeDistance -- the
 *                 closed forms for sphere-sphere / -box / -capsule /
 *                 -cylinder (either order) and capsule-capsule, else
 *                 GJKDistance: libccd's GJK (__ccdGJK, then _ccdDist) in float
 *                 (ccd_real_t of the reference's libccd build), -1 once GJK
 *                 finds the shapes intersecting.  With enable_signed_distance
 *                 every shape pair runs GJKSignedDistance: GJK, then for
 *                 intersecting shapes FCL's EPA (__ccdEPA to epa_tolerance
 *                 1e-4, penEPAPosClosest): -(penetration depth).  One
 *                 departure: where FCL's EPA would expand a nearest face the
 *                 new support point does not see (its polytope turns
 *                 non-convex and can cycle forever), the EPA stops at that
 *                 face (oracle/fcl_gjk_dist.h, "convexity guard").
 *   OcTree-shape  the minimum over the occupied leaves of shapeDistance(Box
 *                 (leaf), shape) (OcTreeShapeDistanceRecurse).
 *   mesh-shape    the minimum over the triangles of shapeTriangleDistance
 *                 (sphereTriangleDistance for spheres, else GJK on the
 *                 triangle GJK object) (MeshShapeDistanceTraversalNodeOBBRSS).
 *   mesh-mesh     the minimum of triDistance over the triangle pairs (0 when
 *                 one intersects) (MeshDistanceTraversalNodeOBBRSS).
 *   mesh-OcTree   the minimum over (leaf box, triangle) of GJK distance
 *                 (OcTreeMeshDistanceRecurse).
 *   Mesh and OcTree pairs are unsigned whatever the request (their leaves
 *   call the unsigned shapeDistance / triDistance), -1 once a leaf test
 *   penetrates.
 * Device and oracle agree bit for bit on the GJK/EPA floats; between equal
 * minima of a mesh / OcTree pair the first leaf test in the oracle's scan
 * order wins (FCL's RSS-ordered traversal may pick another equal one).
 */
int mpg_distance_batch(mpg_world *world, const double *q, int64_t n, int32_t n_self_pairs, double *d_self,
                       int32_t *p_self, double *d_others, int32_t *p_others, int mem, void *stream);

/*
 * DistanceRequest (python/pybind_fcl.hpp:310-316) as PlanningWorldTpl::
 * distance* passes it to fcl::distance (src/planning_world.cpp:512, 537):
 *   flags: MPG_DISTANCE_SIGNED (enable_signed_distance),
 *          MPG_DISTANCE_NEAREST_POINTS (enable_nearest_points),
 *          MPG_DISTANCE_GJK_INDEP (gjk_solver_type = GST_INDEP);
 *   distance_tolerance: GJKSolver_libccd::distance_tolerance, libccd's
 *          dist_tolerance (default 1e-6).
 * pts_self / pts_others ([n*6], may be NULL): DistanceResult::nearest_points
 * [0] and [1] (world frame) of each group's minimum pair, as FCL leaves them:
 *   shape-shape   always (the shape leaf computes them whatever the flags):
 *                 points on o1 and o2; zeros for an unsigned penetration (-1);
 *   OcTree-shape  always, (leaf box point, shape point) in that order for
 *                 both argument orders (the tree is the traversal's o1);
 *   mesh-shape    always; (mesh point, shape point), swapped to (shape, mesh)
 *                 for a (shape, mesh) pair only with enable_nearest_points;
 *   mesh-mesh     only with enable_nearest_points (zeros otherwise);
 *   mesh-OcTree   always, (leaf box point, triangle point).
 * Where FCL throws (its EPA's FCL_THROW_FAILED_AT_THIS_CONFIGURATION) the
 * configuration's p_self = p_others = MPG_DISTANCE_FCL_THROWS and both
 * distances are NaN; MPG_MEM_HOST calls then return MPG_E_FAILED.  An EPA
 * that outgrows the lane's private polytope (96 vertices) is run again from
 * the start with a 2048-vertex polytope from a per-world pool; only past
 * that is the configuration marked MPG_DISTANCE_EPA_CAPACITY (MPG_MEM_HOST:
 * MPG_E_UNSUPPORTED) -- never a silently different value.
 */
#define MPG_DISTANCE_SIGNED 1
#define MPG_DISTANCE_NEAREST_POINTS 2
#define MPG_DISTANCE_GJK_INDEP 4 /* gjk_solver_type = GST_INDEP: FCL's own GJK
                                    in double (ShapeDistanceIndepImpl, its
                                    gjk_tolerance = distance_tolerance) for
                                    the shape pairs without a closed form;
                                    unsigned only, no OcTree / BVH mesh pair
                                    (MPG_E_UNSUPPORTED)                   */
#define MPG_DISTANCE_FCL_THROWS (-2)
#define MPG_DISTANCE_EPA_CAPACITY (-3)
typedef struct mpg_distance_request {
  int32_t flags;
  double distance_tolerance;
} mpg_distance_request;
int mpg_distance_batch_req(mpg_world *world, const double *q, int64_t n, int32_t n_self_pairs,
                           const mpg_distance_request *request, double *d_self, int32_t *p_self, double *pts_self,
                           double *d_others, int32_t *p_others, double *pts_others, int mem, void *stream);
/* mpg_distance_batch_req with the free poses given per call (see
 * mpg_collide_batch_free): free_rows == n, configuration i measured against
 * the movable objects at pose set i, or 1. */
int mpg_distance_batch_free(mpg_world *world, const double *q, const double *free_pose, int64_t free_rows,
                            int64_t n, int32_t n_self_pairs, const mpg_distance_request *request, double *d_self,
                            int32_t *p_self, double *pts_self, double *d_others, int32_t *p_others,
                            double *pts_others, int mem, void *stream);
/* mpg_distance_batch_req with distance_tolerance = 1e-6 */
int mpg_distance_batch_ex(mpg_world *world, const double *q, int64_t n, int32_t n_self_pairs, int32_t flags,
                          double *d_self, int32_t *p_self, double *pts_self, double *d_others, int32_t *p_others,
                          double *pts_others, int mem, void *stream);

/*
 * Collide with contacts: CollisionRequest(enable_contact=True).  Same flags /
 * pair_mask as mpg_collide_batch (input_kind MPG_INPUT_Q: q rows) or
 * mpg_collide_link_poses (MPG_INPUT_LINK_POSES), plus, for every reported
 * pair p of configuration i, libccd's MPR penetration (FCL GJKCollide ->
 * ccdMPRPenetration, the one contact FCL reports for an MPR pair):
 *   depth[i*P + p], normal[(i*P + p)*3 ..] (from object 1 to object 2),
 *   pos[(i*P + p)*3 ..]; zeros for pairs not reported.  P = n_pairs.
 * FCL closed-form pairs report the contact FCL 0.7's specialisation emits
 * (box-box: boxBox2's clipped face points / edge-edge closest point, with its
 * stored penetration_depth = -(point depth) <= 0; sphere-sphere; sphere-box
 * and box-sphere; sphere-capsule; sphere-cylinder; the shape-sphere orders
 * flip the normal), reduced to the one contact ShapeShapeCollide keeps for
 * num_max_contacts = 1.  A point-cloud (OcTree) pair reports the contact of
 * the first occupied leaf of FCL's traversal that intersects the shape, with
 * the tree as the contact's o1 (normal from the leaf box into the shape).
 * A BVH-mesh pair reports the contact of the first intersecting leaf test
 * in FCL 0.7.0's traversal order of its BVHModel<OBBRSS> tree (the tree is
 * rebuilt as FCL builds it, and only leaf tests FCL's OBB tests let through
 * count): mesh-shape the smallest leaf position (left child first), with the
 * sphere-triangle contact or libccd MPR penetration of (shape, triangle);
 * mesh-mesh the pair whose descent (first tree descended when the second
 * node is a leaf or the first is larger) is lexicographically first, with
 * intersect_Triangle's deepest point of the shallower triangle (o1's frame ->
 * world); mesh-OcTree the first in OcTreeMeshIntersectRecurse's interleaved
 * descent (octree children 0..7, mesh left then right), MPR penetration of
 * (leaf box, triangle).
 */
#define MPG_INPUT_Q 0
#define MPG_INPUT_LINK_POSES 1
int mpg_collide_contacts(mpg_world *world, const double *input, int64_t n, int input_kind, uint8_t *flags,
                         uint32_t *pair_mask, double *depth, double *normal, double *pos, int mem, void *stream);
/* With the free poses given per call (see mpg_collide_batch_free), for
 * MPG_INPUT_Q rows.  MPG_INPUT_LINK_POSES rows already carry the free frames'
 * columns: a non-NULL free_pose with them is MPG_E_INVALID. */
int mpg_collide_contacts_free(mpg_world *world, const double *input, const double *free_pose, int64_t free_rows,
                              int64_t n, int input_kind, uint8_t *flags, uint32_t *pair_mask, double *depth,
                              double *normal, double *pos, int mem, void *stream);

/* link_pose: [n*n_links*7] = getLinkPose(l) -> (px, py, pz, qw, qx, qy, qz);
 * free frames: their current poses. */
int mpg_fk_batch(mpg_world *world, const double *q, int64_t n, double *link_pose, int mem,
                 void *stream);

/*
 * Per-kernel timing with HIP events recorded on the launch stream (off by
 * default; no cost when off).  mpg_profile_read synchronises the recorded
 * events, writes the accumulated milliseconds, launch counts and work units
 * of each stage since the last read (then resets them).  Units: configurations
 * for CULL and BUCKET, narrow-phase (configuration, pair) candidates for
 * NARROW.  Any output pointer may be NULL.
 *   MPG_STAGE_CULL    phase A broad phase           (cull_kernel)
 *   MPG_STAGE_BUCKET  survivor bucketing            (range_sum/range_scan/scatter)
 *   MPG_STAGE_NARROW  phase B exact narrow phase    (narrow_kernel)
 */
#define MPG_STAGE_CULL 0
#define MPG_STAGE_BUCKET 1
#define MPG_STAGE_NARROW 2
#define MPG_NUM_STAGES 3
int mpg_profile_enable(mpg_world *world, int enable);
int mpg_profile_read(mpg_world *world, double *ms, int64_t *launches, int64_t *units, int n_stages);

/*
 * Diagnostics: fcl::collide(geometry geom_a at Ta[i], geometry geom_b at
 * Tb[i]) for i < n (SE3 as 12 doubles each; host buffers), through the same
 * narrow-phase dispatch as mpg_collide_batch (FCL closed form, octree / BVH
 * mesh walk, or libccd MPR) -- the narrow phase without forward kinematics,
 * for parity tests against the CPU restatement.  hit[i] = 1 on contact.
 */
int mpg_debug_collide_pairs(mpg_world *world, int32_t geom_a, int32_t geom_b, int64_t n, const double *Ta,
                            const double *Tb, uint8_t *hit);

/*
 * Diagnostics: the narrow-phase task list of the last bulk collide call
 * (mpg_collide_batch above the latency path's sizes, mpg_collide_contacts,
 * ...) on `stream`'s workspace, read after synchronising the stream: the
 * number of tasks, the task size ts of the first level, the number of
 * task-size levels in use (1 unless the batch holds more candidates than
 * 4 * narrow blocks * 128: then the tasks shrink towards the end of the list)
 * and the number of candidates.  Any output may be NULL.  stream NULL after
 * host-buffer calls: the world's own stream.  The environment variable
 * MPG_NARROW_BLOCKS (read by mpg_world_create, clamped to [1, the resident
 * blocks of the narrow kernel]) shrinks the persistent narrow grid, so that
 * small batches reach several levels.
 */
int mpg_debug_task_plan(mpg_world *world, void *stream, int64_t *tasks, int32_t *task_size, int32_t *levels,
                        int64_t *candidates);

/*
 * Planner.generate_collision_pair (mplib/planner.py:118-163), batched: n
 * configurations of the world's state drawn uniformly in [lower, upper]
 * (dof values each) on the device, evaluated as mpg_collide_batch does, and
 * counts[p] (host, n_pairs) = how many of them report pair p (collide_full()
 * of the sample).  The reference loops set_qpos(random, full=True) +
 * collide_full() 10^6 times on the host; build the world with every joint of
 * the planned articulations as a state value for that semantics.
 * Sampler: value i of the batch (row-major) is lower + (upper - lower) * u,
 * u = (splitmix64(seed + (i + 1) * 0x9E3779B97F4A7C15) >> 11) * 2^-53;
 * mpg_sample_uniform returns the same values (host buffer, rows counted from
 * row_offset).  dof <= 64.
 */
int mpg_collide_count(mpg_world *world, const double *lower, const double *upper, int64_t n, uint64_t seed,
                      int64_t *counts, void *stream);
int mpg_sample_uniform(const double *lower, const double *upper, int32_t dof, int64_t n, uint64_t seed,
                       int64_t row_offset, double *q, int device);

/*
 * Planner.IK's loop (mplib/planner.py:256-350) as one device call: for every
 * goal pose of one user link, rows_per_goal seeds run the closed-loop IK
 * (PinocchioModelTpl::computeIKCLIK, src/pinocchio_model.cpp:376-433,
 * pinocchio's computeIKCLIK with a mask), the answers are wrapped into the
 * joint limits (check_joint_limit, planner.py:170-191), checked by the world's
 * collide() (planner.py:301-303) and compared with the goal by distance_6D
 * (planner.py:165-168, 306-313).  Nothing leaves the device between the steps.
 *
 * Row (goal g, seed r) is stored at g * rows_per_goal + r.
 *  1. CLIK, fp64: err = log6(joint_pose^-1 * oMi[jid]), joint_pose = goal *
 *     link_placement^-1, jid the link's parent joint.  ||err|| < eps ends the
 *     row with MPG_IK_CONVERGED, max_iter iterations end it without.  Else
 *     v = -J^T (J J^T + damp I)^-1 err dt with J the joint-frame (LOCAL)
 *     Jacobian over the supporting joints, and q = integrate(q, v); continuous
 *     joints keep pinocchio's (cos, sin) pair and first-order renormalisation,
 *     their answer is atan2.  Joints that move: the chain's joints with a dof
 *     slot whose mask byte is 0; every other joint is a constant.  A
 *     non-positive Cholesky pivot (the host version throws there) ends the row
 *     with MPG_IK_SINGULAR, without MPG_IK_CONVERGED, at the joint values from
 *     before that step.  iters: steps taken; err: the last log6 error.
 *  2. limits, every dof slot: revolute and continuous joints keep q when
 *     |q - lo| < 1e-3, else q -= 2 pi floor((q - lo) / (2 pi)), and fail when
 *     q > hi + 1e-3; prismatic joints fail when q < lo - 1e-3 or q > hi + 1e-3;
 *     a joint without finite limits never fails and is not wrapped.  q_out
 *     holds the wrapped values; MPG_IK_IN_LIMITS: no slot fails.
 *  3. MPG_IK_COLLISION_FREE: mpg_collide_batch's flag of q_out is 0 (the same
 *     device pipeline on the device-resident rows; movable objects at their
 *     current poses).  MPG_IK_WITHIN_THRESHOLD: |dp| + min(|q1 - q2|,
 *     |q1 + q2|) < threshold between the goal and the link pose mpg_fk_batch
 *     gives at q_out.
 * A row is a usable solution when status & MPG_IK_VALID == MPG_IK_VALID.
 *
 * Seeds: q_init [n_goals * rows_per_goal * dof], or NULL: seed 0 of each goal
 * is q_start, seed r > 0 is row g * rows_per_goal + r of mpg_sample_uniform
 * (seed opt->seed) over the joint limits, [-pi, pi] for continuous joints,
 * masked slots overwritten with q_start.  A move-group joint with neither
 * finite limits nor a continuous type is then MPG_E_INVALID.
 *
 * mem: MPG_MEM_HOST buffers are staged and the call synchronises (poses and
 * joint values checked: finite, quaternion norm within 1e-6);
 * MPG_MEM_DEVICE: goal_pose, q_init, q_start and the outputs are device
 * memory, everything is enqueued on `stream`, nothing synchronises.  opt and
 * its mask are host memory, read during the call.  MPG_E_INVALID: a free-frame
 * link, a link index out of range, q_init and q_start both NULL, max_iter
 * outside [0, 100000]; MPG_E_UNSUPPORTED: dof > 32 or more than 15 joints
 * above the link.  Every loop of the kernel is bounded by max_iter and the row
 * count, so the call ends for any input (a NaN error never converges).
 */
#define MPG_IK_CONVERGED 1
#define MPG_IK_IN_LIMITS 2
#define MPG_IK_COLLISION_FREE 4
#define MPG_IK_WITHIN_THRESHOLD 8
#define MPG_IK_SINGULAR 16
#define MPG_IK_VALID 15

typedef struct mpg_ik_options {
  double eps;           /* 1e-5 */
  int32_t max_iter;     /* 1000; 0 .. 100000, else MPG_E_INVALID */
  double dt;            /* 0.1 */
  double damp;          /* 1e-12 */
  double threshold;     /* 1e-3 */
  const uint8_t *mask;  /* [dof], host memory, 1 = frozen; NULL = none */
  uint64_t seed;
  int32_t max_waves;    /* 0 = as many as are resident; a tuning and test knob */
} mpg_ik_options;

int mpg_ik_batch(mpg_world *world, int32_t link, const double *goal_pose /* [n_goals*7] (p, wxyz) */,
                 int64_t n_goals, int64_t rows_per_goal,
                 const double *q_init /* [n_goals*rows_per_goal*dof] or NULL */,
                 const double *q_start /* [dof] or NULL */, const mpg_ik_options *opt /* NULL = defaults */,
                 double *q_out, uint8_t *status, double *err /* [rows*6] or NULL */,
                 int32_t *iters /* [rows] or NULL */, int mem, void *stream);

/*
 * Planner.plan_screw's loop (mplib/planner.py:526-671) for many goals in one
 * device call: row i moves user link `link` from the state q_start[i] towards
 * the pose goal[i] along the screw between them and returns the joint-space
 * waypoints (the path plan_screw hands to TOPP-RA; the time parametrisation is
 * not part of this call).  fp64, no fused multiply-add.
 *
 * Start.  T = goal * link_pose(q_start)^-1, the link pose with getLinkPose's
 * quaternion round trip.  Exponential coordinates as pose2exp_coordinate
 * (planner.py:575-605), tr the trace of T's rotation:
 *   |tr - 3| <= 1e-8 + 3e-5 (np.isclose): omega = 0, theta = 1 -- a rotation
 *     below about 5.5e-3 rad is dropped, the move is a pure translation;
 *   |tr + 1| <= 1e-8 + 1e-5: the row ends at once with MPG_SCREW_ROT_PI and one
 *     waypoint (plan_screw returns "screw plan failed." there);
 *   else theta = acos((tr - 1) / 2), omega = skew part / (2 sin theta).
 * v = (I / theta - [omega] / 2 + (1 / theta - 1 / (2 tan(theta / 2))) [omega]^2) p
 * and twist = (v, omega) * theta.
 *
 * Step.  J: the WORLD Jacobian of the link's parent joint (getLinkJacobian,
 * local = false) over the joints above the link that have a dof slot; every
 * other slot's column is zero and the slot keeps its start value.
 *   dq = J^T (J J^T)^-1 twist (Cholesky, no damping); dq *= qpos_step / |dq|;
 *   dtw = J dq; if |dtw| > |twist|, both are scaled by |twist| / |dtw| and the
 *   step is the last one; q += dq (a continuous joint adds the angle, it is
 *   not wrapped); twist -= dtw.
 * Row end, the first of (in this order, after the update):
 *   a non-positive (or NaN) Cholesky pivot      MPG_SCREW_SINGULAR, before the update
 *   |dtw| < 1e-4                                MPG_SCREW_STALLED, the state is not stored
 *   a dof slot with finite limits has q < lo - 1e-3 or q > hi + 1e-3 (every
 *     slot of the row, those outside the chain too; no 2 pi wrap: plan_screw's
 *     own test, planner.py:639-647; a joint the snapshot holds as a constant,
 *     such as a gripper finger outside the move group, has no slot and is
 *     not tested)                               MPG_SCREW_LIMIT, the state is not stored
 *   the step was the last one                   stored, MPG_SCREW_REACHED
 *   max_waypoints states are stored             MPG_SCREW_TRUNCATED
 * The reference's loop has no bound; this one stores a waypoint or ends the
 * row in every pass, so it ends for any input (NaNs satisfy no test and end at
 * the cap or at a NaN pivot).
 *
 * Collisions.  The path does not depend on them (plan_screw only aborts on a
 * collision).  After all rows are integrated one mpg_collide_batch pass runs on
 * the same stream over the padded [rows * max_waypoints, dof] path, movable
 * objects at their current poses.  MPG_SCREW_COLLISION_FREE: no waypoint
 * 1 .. n_waypoints - 1 has a non-zero flag; waypoint 0, the start state, is
 * not checked, as in plan_screw.  first_hit: the first such waypoint, or -1.
 * A row is plan_screw's "Success" when status & MPG_SCREW_VALID ==
 * MPG_SCREW_VALID.
 *
 * Deviation: numpy's pinv is an SVD with a 1e-15 cut-off, this call solves
 * the normal equations; the two differ only where J is rank deficient or
 * nearly so.  A link with fewer than six joints with a dof slot above it is
 * therefore MPG_E_UNSUPPORTED, as are dof > 32 and more than 15 joints above
 * the link.  MPG_E_INVALID: a free-frame link, a link index out of range,
 * qpos_step not > 0, max_waypoints outside [2, 4096], rows * max_waypoints >
 * 2^31, a NULL buffer with rows > 0.
 *
 * path [rows * max_waypoints * dof]: the waypoints of row i from i *
 * max_waypoints * dof; the slots past n_waypoints[i] repeat the last stored
 * waypoint.  mem: MPG_MEM_HOST buffers are staged and the call synchronises
 * (poses and joint values checked: finite, quaternion norm within 1e-6);
 * MPG_MEM_DEVICE: goal, q_start and the outputs are device memory, everything
 * is enqueued on `stream`, nothing synchronises.
 */
#define MPG_SCREW_REACHED 1
#define MPG_SCREW_COLLISION_FREE 2
#define MPG_SCREW_VALID 3
#define MPG_SCREW_STALLED 4
#define MPG_SCREW_LIMIT 8
#define MPG_SCREW_TRUNCATED 16
#define MPG_SCREW_SINGULAR 32
#define MPG_SCREW_ROT_PI 64

typedef struct mpg_screw_options {
  double qpos_step;      /* 0.1; > 0, else MPG_E_INVALID */
  int32_t max_waypoints; /* 64; 2 .. 4096 */
} mpg_screw_options;

int mpg_screw_batch(mpg_world *world, int32_t link, const double *goal /* [rows*7] (p, wxyz) */,
                    const double *q_start /* [rows*dof] */, int64_t rows,
                    const mpg_screw_options *opt /* NULL = defaults */, double *path /* [rows*max_waypoints*dof] */,
                    int32_t *n_waypoints /* [rows] */, uint8_t *status /* [rows] */,
                    int32_t *first_hit /* [rows] or NULL */, int mem, void *stream);

/*
 * Planner.plan's RRTConnect (src/ompl_planner.cpp over OMPL 1.6.0
 * RRTConnect::solve) for Q independent (start, goals) rows in one call: the
 * rows advance in lockstep, one growTree call per row and round, and the states
 * all their motion validators look at ride in one mpg_collide_batch pass per
 * round on the same stream (movable objects at their current poses).  fp64, no
 * fused multiply-add, no library call: a row's result is the same bits as the
 * host build of mplib_amd/csrc/mpg_rrt.h with the same validity answers.
 *
 * State space.  Slot d of a state is an SO2 joint where bit d of so2_mask is
 * set (bounds and sampling range [-pi, pi], distance and interpolation the
 * short way round), else a real value within the snapshot's joint limits,
 * which must be finite.  distance = sum over the slots, interpolate, equal,
 * validSegmentCount and satisfiesBounds are OMPL's for a compound space of
 * RealVector(1) / SO2 subspaces with weight 1.  extent = the sum of the
 * slots' widths (pi for SO2), longestValidSegment = 0.01 extent, maxDistance =
 * range, or 0.2 extent when range <= 1e-6.
 *
 * Rounds.  Iteration k (k = 0, 1, ...) draws a sample, grows the start tree
 * (k even) or the goal tree (k odd) towards it from the exact nearest node
 * (first strict minimum, ties to the lowest index), and on ADVANCED / REACHED
 * grows the other tree towards the added state while that answers ADVANCED.
 * growTree validates what OMPL's does: checkMotion(near, new) for the start
 * tree, isValid(new) && checkMotion(new, near) for the goal tree, with the
 * DiscreteMotionValidator's states.  REACHED while connecting ends the row:
 * the path is start root .. connection .. goal root with the duplicate
 * connection state removed.  Every growTree call is one round.
 *
 * Stated deviations from OMPL: (1) the sample of iteration k of a row is row k
 * of mpg_sample_uniform(lo, hi, seed = the row's seed) -- the row's seed is
 * row_seed[r], or splitmix64(seed + (r + 1) * 0x9E3779B97F4A7C15) without the
 * array -- so a row depends on nothing but its own inputs and seed; (2) every
 * goal of the row that is collision-free and within the bounds is a root of
 * the goal tree before the first iteration, in the given order; (3) an invalid
 * start ends the row with MPG_PLAN_START_INVALID, it is not resampled.
 *
 * status: MPG_PLAN_SOLVED; START_INVALID (bounds or collision); GOAL_INVALID
 * (no goal survives); ROUNDS_EXHAUSTED (max_rounds rounds without a solution);
 * NODES_EXHAUSTED (a node did not fit its tree of max_nodes, roots included);
 * TRUNCATED (with SOLVED: the path has more than max_waypoints states;
 * n_waypoints is 0).  path [Q * max_waypoints * dof]: the slots past
 * n_waypoints repeat the last waypoint; a row without a path holds its start
 * state in every slot.  iterations: the iterations a row started; tree_sizes
 * [Q * 2]: nodes of the start and the goal tree.
 *
 * MPG_E_UNSUPPORTED: dof > 32.  MPG_E_INVALID: G outside [1, 16], max_nodes
 * outside [2, 65536], max_waypoints outside [2, 4096], max_rounds < 1,
 * check_every < 1, a non-finite range, an SO2 bit at or above dof, a slot
 * without finite limits that is not SO2, Q * 2 * max_nodes * dof > 2^31 (the
 * trees' doubles), Q * the round's states > 2^31, a NULL buffer with Q > 0,
 * non-finite start / goal values (MPG_MEM_HOST).
 *
 * The host decides when to stop, so the call is not a pure enqueue: with
 * MPG_MEM_DEVICE (start, goal, row_seed and the outputs in device memory) it
 * synchronises `stream` once per check_every rounds, to read the count of
 * unfinished rows, and once at the end; it stops when that count is 0 or
 * after max_rounds rounds.  Results do not depend on check_every.
 * MPG_MEM_HOST buffers are staged.
 */
#define MPG_PLAN_SOLVED 1
#define MPG_PLAN_START_INVALID 2
#define MPG_PLAN_GOAL_INVALID 4
#define MPG_PLAN_ROUNDS_EXHAUSTED 8
#define MPG_PLAN_NODES_EXHAUSTED 16
#define MPG_PLAN_TRUNCATED 32

typedef struct mpg_plan_options {
  double range;          /* 0: 0.2 * extent (OMPL's default) */
  int32_t max_rounds;    /* 20000; >= 1 */
  int32_t max_nodes;     /* 2048 per tree; 2 .. 65536 */
  int32_t max_waypoints; /* 256; 2 .. 4096 */
  int32_t check_every;   /* 8; >= 1 */
  uint64_t seed;         /* row seeds when row_seed is NULL */
  uint32_t so2_mask;     /* bit d: state slot d is an SO2 joint */
} mpg_plan_options;

int mpg_plan_batch(mpg_world *world, const double *start /* [Q*dof] */, const double *goal /* [Q*G*dof] */, int64_t Q,
                   int32_t G, const uint64_t *row_seed /* [Q] or NULL */,
                   const mpg_plan_options *opt /* NULL = defaults */, double *path /* [Q*max_waypoints*dof] */,
                   int32_t *n_waypoints /* [Q] */, uint8_t *status /* [Q] */, int32_t *iterations /* [Q] or NULL */,
                   int32_t *tree_sizes /* [Q*2] or NULL */, int mem, void *stream);

/*
 * Planner.TOPP (mplib/planner.py:358-375) for many joint-space paths in one
 * device call: row r's n = n_waypoints[r] waypoints q_0 .. q_{n-1} (the layout
 * mpg_screw_batch and mpg_plan_batch write) get a cubic spline at s_i = i /
 * (n - 1), the time-optimal parametrisation under the joint velocity and
 * acceleration limits (TOPP-RA, Pham & Pham 2018), and samples every `step`.
 * toppra picks its gridpoints adaptively; this call's algorithm is stated
 * here and in DESIGN.md section 14 instead.  fp64, no fused multiply-add, + - *
 * / sqrt and comparisons only: a row's result is the same bits as the host
 * build of mplib_amd/csrc/mpg_topp.h.
 *
 * Spline.  C2 cubic, not-a-knot ends (scipy CubicSpline's default, toppra's
 * SplineInterpolator).  n = 2: the straight line; n = 3: the parabola.
 * Grid.  N = max(min_grid, grid_per_segment * (n - 1)) intervals, s_k = k / N,
 * delta = 1 / N.
 * Constraints of interval k on x = sdot^2 and u = sddot (first-order
 * interpolation, toppra's default): per joint |q'_k u + q''_k x| <= amax and
 * |(q'_{k+1} + 2 delta q''_{k+1}) u + q''_{k+1} x| <= amax; 0 <= x + 2 delta u
 * <= K_{k+1}; x <= min over the joints with q'_k != 0 of (vmax / q'_k)^2, at
 * most 1e12.
 * Backward.  K_N = 0; K_k = the largest feasible x (u eliminated exactly by
 * Fourier-Motzkin over the (2 dof + 1)^2 pairs of a lower and an upper bound),
 * at least 0.
 * Forward.  x_0 = 0; u_k = the largest u the acceleration rows allow at x_k;
 * x_{k+1} = min(max(x_k + 2 delta u_k, 0), K_{k+1}), the continuation row.
 * Time.  t_{k+1} = t_k + 2 delta / (sqrt x_k + sqrt x_{k+1}); duration = t_N.
 * Samples.  m = int(duration / step) samples at t_i = i duration / (m - 1)
 * (np.linspace(0, duration, m): the spacing is not `step`; m = 1: t = 0).  In
 * the interval with t_k <= t (the largest such k, at most N - 1): tau = t - t_k,
 * sddot = (x_{k+1} - x_k) / (2 delta), sdot = sqrt x_k + sddot tau, s = s_k +
 * sqrt x_k tau + sddot tau^2 / 2 clamped to [s_k, s_{k+1}]; position = q(s),
 * velocity = q'(s) sdot, acceleration = q'(s) sddot + q''(s) sdot^2.
 *
 * status: MPG_TOPP_OK; NO_PATH (n_waypoints < 2, such as a failed plan row);
 * ZERO_LENGTH (all waypoints equal bit for bit); STALLED (an interval with
 * x_k = x_{k+1} = 0, or a duration that is not finite; NaN inputs end here);
 * TRUNCATED (with OK: m > max_samples; duration is valid, n_samples is 0).
 * Rows that are not OK have duration 0 and n_samples 0.  Every loop has a fixed
 * length.  Sample slots past n_samples repeat the last sample; a row without
 * samples holds its first waypoint, zero time, velocity and acceleration.
 * grid_x / grid_t (optional): x_k and t_k with the stride Ncap + 1, Ncap =
 * max(min_grid, grid_per_segment * (max_waypoints - 1)); slots past a row's N
 * repeat the last value, rows without a profile hold zeros.
 *
 * dof is the world's state width; the world's geometry is not used.
 * MPG_E_UNSUPPORTED: dof > 32.  MPG_E_INVALID: options out of range,
 * max_waypoints outside [2, 4096], a limit that is not finite and > 0, rows *
 * max_waypoints * dof, rows * max_samples * dof or rows * (Ncap + 1) above
 * 2^31, a NULL required buffer with rows > 0; with MPG_MEM_HOST also
 * n_waypoints[r] > max_waypoints (the device clamps it) and a non-finite path
 * value inside a row's count.  rows = 0 returns 0.
 *
 * vel_limits, acc_limits and opt are host memory, read during the call.
 * MPG_MEM_DEVICE: every other buffer is device memory, everything is enqueued
 * on `stream`, nothing synchronises (the buffers mpg_screw_batch /
 * mpg_plan_batch just wrote on the same stream can be passed straight in).
 * MPG_MEM_HOST buffers are staged and the call synchronises.
 */
#define MPG_TOPP_OK 1
#define MPG_TOPP_NO_PATH 2
#define MPG_TOPP_ZERO_LENGTH 4
#define MPG_TOPP_STALLED 8
#define MPG_TOPP_TRUNCATED 16

typedef struct mpg_topp_options {
  double step;              /* 0.1; > 0, else MPG_E_INVALID */
  int32_t grid_per_segment; /* 8; 1 .. 64 */
  int32_t min_grid;         /* 100; 2 .. 65536 */
  int32_t max_samples;      /* 256; 1 .. 65536 */
} mpg_topp_options;

int mpg_topp_batch(mpg_world *world, const double *path /* [rows*max_waypoints*dof] */,
                   const int32_t *n_waypoints /* [rows] */, int64_t rows, int32_t max_waypoints,
                   const double *vel_limits /* [dof] */, const double *acc_limits /* [dof] */,
                   const mpg_topp_options *opt /* NULL = defaults */, double *times /* [rows*max_samples] */,
                   double *position, double *velocity, double *acceleration /* each [rows*max_samples*dof] */,
                   int32_t *n_samples /* [rows] */, double *duration /* [rows] */, uint8_t *status /* [rows] */,
                   double *grid_x /* [rows*(Ncap+1)] or NULL */, double *grid_t /* same or NULL */, int mem,
                   void *stream);

/*
 * Diagnostics (host only, no device): the FCL 0.7.0 BVHModel<OBBRSS> tree the
 * snapshot builds for a BVH mesh (BVHModel::endModel -> buildTree:
 * BVFitter<OBBRSS>::fit, SPLIT_METHOD_MEAN; OBB half), whose OBB tests gate
 * mesh pairs as FCL's traversal does.  boxes [(2T - 1) * 15] = per node the
 * row-major axis matrix (columns = box axes), centre, half extents; links
 * [(2T - 1) * 3] = first child node (-(triangle + 1) for a leaf), first leaf
 * position, leaf count; leaf_order [T] = primitive_indices after the build.
 * Returns the node count (2T - 1) or a negative status.
 */
int mpg_fcl_bvh_build(const double *vertices, int32_t n_vertices, const int32_t *triangles, int32_t n_triangles,
                      double *boxes, int32_t *links, int32_t *leaf_order);

/* Diagnostics: the device sin/cos used by the FK (host buffers). */
int mpg_debug_sincos(const double *x, int64_t n, double *s, double *c, int device);

/*
 * Latency server accounting (the resident kernel behind host batches of at
 * most MPG_SMALL_SERVER_MAX states): batches it answered,
 * times it was (re)started, calls that fell back to one launch per batch
 * because it could not be started or did not answer.  state: 0 = not used by
 * this world (MPG_SMALL_SERVER=0, or pairs it does not serve), 1 = in use,
 * 2 = fallen back (it is tried again one second after the failure).  Any
 * output pointer may be NULL.  No reference counterpart (diagnostics).
 */
int mpg_latency_server_stats(mpg_world *world, int64_t *served, int64_t *starts, int64_t *fallbacks,
                             int32_t *state);

/*
 * The lookup grids of the joint-value cull: how many
 * moving objects have one, the cells of all grids together, whether the words
 * have been built yet (the first bulk launch with joint-value input does
 * that; world creation and the latency path do not) and the cell edge in
 * metres.  For the first cap gridded objects: the moving object, its number
 * of static partners, and the grid's box as (lo x y z, hi x y z), the region
 * inside which a centre is looked up.  Any output pointer may be NULL.  No
 * reference counterpart (diagnostics).
 */
int mpg_cull_grid_info(const mpg_world *world, int32_t *objects, int64_t *cells, int32_t *built, double *cell_edge,
                       int32_t cap, int32_t *object, int32_t *partners, double *box);

/* Synchronise the world's device (used after MPG_MEM_DEVICE calls). */
int mpg_synchronize(int device);

int mpg_device_count(int *count);
const char *mpg_last_error(void);
/*
 * The last error text of the calling thread copied into buf (at most size - 1
 * bytes and a terminating NUL; truncated if longer).  Returns the full length
 * of the text (excluding the NUL), as snprintf does, so a caller can size a
 * buffer; buf may be NULL when size is 0.  This is SURVEY.md 8(b)'s
 * mpg_last_error(char*, size_t) form for bindings that cannot hold a pointer
 * into library-owned thread-local storage (cgo / JNI); mpg_last_error() above
 * stays for C and ctypes callers.
 */
int mpg_last_error_copy(char *buf, size_t size);
const char *mpg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MPGPU_H */
