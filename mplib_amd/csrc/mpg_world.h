// mpg_world.h -- struct mpg_world, the host object behind the C ABI's opaque
// handle: snapshot, per-stream workspaces, ring, scratch (included by
// mpg_kernels.hip at global scope, after the device code's anonymous namespace).
//
// Every device / pinned buffer, stream and event below is an owner of
// mpg_devbuf.h, released by ~mpg_world in reverse declaration order.  That
// order matters: the snapshot blob is declared first, so it goes last among
// device memory, and within the world and each nested struct the streams and
// events come before the buffers, so they are destroyed after the buffers are
// freed (which synchronises the device) -- nothing is queued on a stream when
// it goes.  What is ordering beyond that is in the destructor's body.
#pragma once

struct mpg_world {
  ~mpg_world();  // mpg_abi_world.h
  int device = 0;
  DevWorld dw{};
  int n_geoms = 0;
  std::vector<int> geom_type_h;  // host copy of the geometry kinds (diagnostics)
  DevBuf<char> blob;             // the snapshot dw points into
  size_t blob_bytes = 0;
  uint64_t snapshot_hash = 0;  // FNV-1a of the snapshot blob (mpg_collide_batch_multi's same-scene check)
  // host-buffer calls without a stream run on this non-blocking stream (not
  // the legacy default stream, whose synchronisation covers every blocking
  // stream of the device); MPG_OWN_STREAM=0 keeps the caller's NULL stream
  Stream own_stream;
  Event gather_ev;  // mpg_collide_batch_multi_device: this shard's gather copies are queued
  // owners of what dw holds as raw pointers: big_vis, big_busy, stats, free_cur
  DevBuf<unsigned long long> big_vis;
  DevBuf<int> big_busy;
  DevBuf<unsigned long long> stats;
  DevBuf<double> free_dev;
  // the cull's lookup grids (dw.n_grid > 0): the plan world creation left, the
  // words the first bulk launch builds from it (grid_words_for; grid_mu, not
  // host_mu, which some callers of launch_collide hold) and how long that took
  BpGridPlan grid_plan;
  DevBuf<uint32_t> grid_words;
  std::mutex grid_mu;
  std::atomic<bool> grid_ready{false};
  double grid_build_ms = 0.0;
  struct GridInfo {  // what mpg_cull_grid_info reports (kept when the plan is dropped)
    std::vector<int> object, partners;
    std::vector<double> box;  // [objects][6]: the grid's corners, origin and origin + n * h
    long long cells = 0;
    double h = 0.0;
  } grid_info;
  int block = 128;
  size_t lds_bytes = 0;
  // The staging of the MPG_MEM_HOST calls, a struct per family: grow-only
  // device twins of the caller's arrays, filled and read back through a
  // HostStage (mpg_streams_host.h).  One rule for all of them: the call holds
  // host_mu and is synchronous, so a buffer is replaced without a wait.  (The
  // host-buffer calls of distance and motion validation stage in their scratch
  // below, under its own mutex and event.)
  std::mutex host_mu;
  struct FkStage {
    DevBuf<double> q, out;
  } fk_stage;
  struct FreeStage {  // collide_batch of a world with free frames
    DevBuf<double> q, fp, links;
    DevBuf<uint8_t> fl;
    DevBuf<uint32_t> mk;
  } free_stage;
  struct ContactStage {
    DevBuf<double> in, out;
    DevBuf<uint8_t> fl;
    DevBuf<uint32_t> mk;
    DevBuf<double> fp;  // host-memory free poses of the call
  } contact;
  struct IkStage {
    DevBuf<double> goal, q, start, err;
    DevBuf<uint8_t> status;
    DevBuf<int32_t> iters;
  } ik_stage;
  struct ScrewStage {
    DevBuf<double> goal, start, path;
    DevBuf<uint8_t> status;
    DevBuf<int32_t> count, first_hit;
  } screw_stage;
  struct PlanStage {
    DevBuf<double> start, goal, path;
    DevBuf<uint64_t> row_seed;
    DevBuf<uint8_t> status;
    DevBuf<int32_t> count, iters, sizes;
  } plan_stage;
  struct ToppStage {
    DevBuf<double> path, times, samples, dur, grid;  // samples: position, velocity, acceleration; grid: x, t
    DevBuf<int32_t> count, n_samples;
    DevBuf<uint8_t> status;
  } topp_stage;
  // phase A/B workspace, one per stream so concurrent streams never share it
  struct Workspace {
    DevBuf<uint32_t> surv;       // [W * cap] survivor bits, word-major
    DevBuf<uint32_t> cnt;        // [n_tiles][W * 8] byte counts per (tile, pair), a row per tile (mpg_bucket.h)
    DevBuf<uint32_t> part;       // [n_ranges][W * 32] candidates per (range, pair), prefixed inside the group
    DevBuf<uint32_t> grp;        // [n_groups][W * 32] group totals -> each group's base inside its pair
    DevBuf<uint32_t> seg_len;    // [n_pairs]
    DevBuf<uint32_t> seg_start;  // [n_pairs]
    DevBuf<uint32_t> prefix;     // [n_pairs + kPrefixTail] task prefix, task count, task counter, ts, candidates, task plan
    DevBuf<uint32_t> cand;       // [n_pairs * cap] worst case
    DevBuf<float> rq;            // [n_moving * 4 * cap] phase-A rotations (quaternions) for the SAT stage
    DevBuf<double> sc;           // [cap * dof * 2] exact joint (sin, cos) for phase B
    DevBuf<double> links;        // [links_cap * n_links * 7] link-pose rows (worlds with free frames)
    long long links_cap = 0;     // rows
    long long cap = 0;           // configurations: the stride cull_kernel and scatter_kernel read
    uint64_t last = 0;           // LRU tick (get_workspace)
  };
  // large batches: half of the parts on a side stream (per caller stream)
  struct Side {
    Stream side;
    Event fork, join;
    uint64_t last = 0;
  };
  std::mutex ws_mu;
  std::map<hipStream_t, Side> sides;  // guarded by ws_mu
  std::map<hipStream_t, Workspace> ws;
  // mpg_ik_batch: per caller stream the row counter ik_clik_kernel's lanes
  // claim rows from and the collide pass's flags (guarded by ws_mu, released
  // with the stream's workspace); host tables built by mpg_world_create
  struct IkWork {
    DevBuf<unsigned long long> counter;
    DevBuf<uint8_t> flags;  // [rows]
  };
  std::map<hipStream_t, IkWork> ik_ws;
  struct IkTables {
    int cus = 256;
    std::vector<int> chain_start, chain_len, chain_joints, joint_q_source;
    std::vector<double> lo, hi;                  // [dof]
    std::vector<unsigned char> kind, continuous;  // [dof] IKK_*, continuous joint
  } ik;
  // mpg_screw_batch: per caller stream the collide pass's flags of the padded
  // path (guarded by ws_mu, released with the stream's workspace)
  struct ScrewWork {
    DevBuf<uint8_t> flags;  // [rows * max_waypoints]
  };
  std::map<hipStream_t, ScrewWork> screw_ws;
  // mpg_plan_batch: per caller stream the rows' trees, machines and slot
  // blocks (RrtBufs in mpg_kernels.hip; guarded by ws_mu, released with the
  // stream's workspace).  The call ends with a synchronise, so nothing queued
  // reads a buffer when the next call replaces it.
  struct PlanWork {
    DevBuf<double> nodes, newstate, slots;
    DevBuf<int32_t> parent, sizes, phase, added, iter, prop, active;
    DevBuf<uint64_t> seeds;
    DevBuf<uint8_t> flags;
  };
  std::map<hipStream_t, PlanWork> plan_ws;
  // mpg_topp_batch: per caller stream the rows' spline moments, controllable
  // sets, profiles and times (ToppRowBufs per row; guarded by ws_mu, released
  // with the stream's workspace)
  struct ToppWork {
    DevBuf<double> M;        // [rows][max_waypoints][dof]
    DevBuf<double> K, x, t;  // [rows][Ncap + 1]
  };
  std::map<hipStream_t, ToppWork> topp_ws;
  // free frames: the current poses (host copy; free_dev is the device buffer
  // DevWorld::free_cur points to)
  std::vector<double> free_host;
  // optional per-stage timing (mpg_profile_enable)
  struct Mark {
    int stage;
    Event a, b;
  };
  // batched motion validation buffers (grow-only)
  struct Motion {
    Event last;  // the previous call's work (scratch order across streams)
    DevBuf<double> edges;
    DevBuf<int32_t> segs;
    DevBuf<long long> offs;
    DevBuf<char> out;  // staging: first_invalid[n] (int32) then valid[n] bytes
    DevBuf<double> states;
    DevBuf<uint8_t> flags;
    DevBuf<double> fp;       // host-memory free poses of the call: [free_rows * n_free * 7]
    DevBuf<int32_t> row_of;  // per-edge free poses: the edge of each sub-state (motion_rowmap_kernel)
  } motion;
  std::mutex motion_mu;
  bool has_closed_form = false;  // a non-allowed pair uses an FCL closed form
  bool has_octree = false;       // a non-allowed pair involves an octree
  bool octree_first = false;     // a non-allowed pair has its octree as o1 (C ABI only; pymp puts it second)
  bool any_closed_form = false;  // some pair (allowed or not) does, octrees aside
  bool any_octree = false;       // some pair involves an octree
  bool has_mesh = false;         // a non-allowed pair involves a BVH mesh
  bool any_mesh = false;         // some pair involves a BVH mesh
  bool any_gjk = false;          // GST_INDEP world: some pair runs FCL's own GJK (CF_GJK)
  bool has_octree2 = false;      // a non-allowed pair of two OcTrees
  // batched distance buffers (grow-only)
  struct Dist {
    Event last;  // the previous call's work (scratch order across streams)
    DevBuf<double> poses, save64, q;
    DevBuf<char> out;
    DevBuf<double> pts;               // device-buffer calls: points nobody asked for
    DevBuf<double> links;             // worlds with free frames: link-pose rows
    DevBuf<double> fp;                // host-memory free poses of the call: [free_rows * n_free * 7]
    DevBuf<ccdx::BigPolytope> big;    // kBigPool EPA polytopes (distance_redo_kernel)
    DevBuf<unsigned> list;            // overflowed configurations: [count, ids...]
  } dist;
  std::mutex dist_mu;
  std::mutex prof_mu;
  bool prof = false;
  std::vector<Mark> marks;
  std::vector<Event> ev_pool;
  double prof_ms[MPG_NUM_STAGES] = {0, 0, 0};
  int64_t prof_n[MPG_NUM_STAGES] = {0, 0, 0};
  int64_t prof_cfg = 0;                       // configurations launched while profiling
  DevBuf<unsigned long long> prof_units;      // device counter: narrow candidates
  long long max_chunk = 1 << 20;
  int narrow_blocks = 1024;
  // large batches: two halves, the second on an internal stream, so one
  // half's latency-bound bucketing overlaps the other's compute
  long long overlap_min = 1 << 18;  // 0 disables (env MPG_OVERLAP_MIN)
  int overlap_parts = 2;             // env MPG_OVERLAP_PARTS
  // per-stream state (workspaces, side streams) is kept for at most
  // kMaxStreamState caller streams, least recently used evicted first;
  // mpg_release_stream drops one explicitly
  static constexpr size_t kMaxStreamState = 32;
  uint64_t ws_tick = 0;
  // caller streams with a call in progress (StreamPin): never evicted, so no
  // thread frees a workspace or side stream another thread is using
  std::map<hipStream_t, int> busy;  // guarded by ws_mu
  // small-batch latency path (host buffers, n <= small_max): pinned input
  // staging + host-mapped hit bytes written by small_kernel
  long long small_max = 1024;
  struct Small {
    PinnedBuf<double> h_q;      // pinned, [small cap * row]; dev(): the zero-copy input
    PinnedBuf<uint8_t> h_hits;  // pinned coherent host-mapped, [n_pairs * small cap]
    DevBuf<double> d_qs;        // device input of the latency path
    DevBuf<double> d_ssc;       // latency path joint (sin, cos) [small cap * dof * 2]
    PinnedBuf<double> h_ssc;    // pinned host-mapped twin: sin/cos computed on the host (small batches)
  } small;
  int64_t small_host_sc = 64;  // latency batches up to this size: sin/cos on the host (MPG_SMALL_HOST_SC)
  bool small_args = true;      // the fewest states' rows in the kernel arguments (MPG_SMALL_ARGS=0: off)
  std::vector<int> h_rev_src;  // move-group slots of revolute joints (host copy of the snapshot's rule)
  bool small_zero_copy = true; // MPG_SMALL_ZEROCOPY=0: stage through d_qs
  int64_t small_inline_sc = 256;  // latency batches up to this size: sin/cos inline (MPG_SMALL_INLINE_SC)
  // latency server (lat_server_kernel): control block in host-mapped memory,
  // its own stream; started on demand, leaves after srv_idle_us idle
  Stream srv_stream;
  PinnedBuf<SrvCtl> srv;  // one control block
  unsigned long long srv_seq = 0;
  bool srv_running = false;
  bool srv_ok = false;      // the world fits the server (closed-form / MPR pairs only, records, LDS)
  bool srv_broken = false;  // it failed to answer: launches until srv_retry_at
  std::chrono::steady_clock::time_point srv_retry_at{};
  bool srv_quitting = false;  // quit was set after a missed answer; the stream may still run
  int64_t srv_served = 0, srv_starts = 0, srv_fallbacks = 0;  // mpg_latency_server_stats
  int srv_mode = 1;         // MPG_SMALL_SERVER=0: off
  long long srv_idle_us = 1000;
  int srv_g = 8;            // workgroups (MPG_SMALL_SERVER_WG)
  int srv_max_n = kSrvN;    // batches up to this size go to the server (MPG_SMALL_SERVER_MAX)
  size_t srv_lds = 0;
  bool srv_stats = false;
  double srv_stat[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  size_t small_cap = 0;   // configurations (hit bytes per pair)
  size_t small_qcap = 0;  // input doubles (small.h_q, small.d_qs)
  // host-buffer batches above small_max (collide_host_pipelined): chunks
  // through a ring of slots -- the input of one chunk crosses PCIe while the
  // previous one computes and the one before is unpacked on the host.
  // Grow-only, guarded by host_mu.
  static constexpr int kRing = 3;
  struct Ring {
    Stream h2d;   // input copies
    Stream side;  // odd chunks compute here (one chunk's narrow tail overlaps the next's cull)
    Event e_in[kRing], e_done[kRing];
    struct Slot {
      DevBuf<double> d_in;
      DevBuf<uint8_t> d_fl;
      DevBuf<uint32_t> d_mk;
      DevBuf<uint32_t> d_bcnt;    // colliding configurations per kPackCfg block
      PinnedBuf<uint8_t> h_fl;    // pinned, host-mapped: the chunk's flags (mask_pack_kernel)
      PinnedBuf<uint32_t> h_mk;   // pinned, host-mapped: packed mask rows (mask_pack_kernel)
      PinnedBuf<uint32_t> h_bcnt; // pinned, host-mapped copy of d_bcnt (where each block's packed rows start)
    } slot[kRing];
    size_t cap = 0;                // configurations per slot
    size_t in_cap = 0;             // input doubles per slot
  } ring;
  // chunk sizes: profiles/r06a/host_ab*.txt (2^18 / 2^19 chunks, head and
  // tail sizes within +-3 % of each other on cfg3 2^20; this is the best seen)
  long long ring_chunk = 1 << 19;  // largest chunk (env MPG_HOST_CHUNK)
  int ring_streams = 2;            // compute streams of the pipeline (env MPG_HOST_STREAMS: 1 or 2)
  int host_threads = 8;            // threads unpacking a finished chunk (env MPG_HOST_THREADS)
  long long ring_head = 1 << 17, ring_tail = 1 << 16;  // smaller first / last chunk (env MPG_HOST_HEAD / _TAIL)
  std::unique_ptr<mpg_hostpipe::Pool> pool;
  // MPG_STATS: host pipeline phase sums (us): calls, input copy, issue,
  // result wait, unpack, whole call
  double hp_stat[6] = {0, 0, 0, 0, 0, 0};
};
