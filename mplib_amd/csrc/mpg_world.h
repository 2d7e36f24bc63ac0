// mpg_world.h -- struct mpg_world, the host object behind the C ABI's opaque
// handle: snapshot, per-stream workspaces, ring, scratch (included by
// mpg_kernels.hip at global scope, after the device code's anonymous namespace).
#pragma once

struct mpg_world {
  int device = 0;
  DevWorld dw{};
  int n_geoms = 0;
  std::vector<int> geom_type_h;  // host copy of the geometry kinds (diagnostics)
  void* blob = nullptr;
  size_t blob_bytes = 0;
  uint64_t snapshot_hash = 0;  // FNV-1a of the snapshot blob (mpg_collide_batch_multi's same-scene check)
  hipEvent_t gather_ev = nullptr;  // mpg_collide_batch_multi_device: this shard's gather copies are queued
  int block = 128;
  size_t lds_bytes = 0;
  // staging for MPG_MEM_HOST
  std::mutex host_mu;
  double* d_q = nullptr;
  uint8_t* d_flags = nullptr;
  uint32_t* d_masks = nullptr;
  double* d_out = nullptr;
  size_t cap_cfg = 0;
  size_t cap_out = 0;
  // phase A/B workspace, one per stream so concurrent streams never share it
  struct Workspace {
    uint32_t* surv = nullptr;       // [W * cap] survivor bits, word-major
    uint32_t* cnt = nullptr;        // [n_pairs * n_tiles] tile counts -> offsets
    uint32_t* seg_len = nullptr;    // [n_pairs]
    uint32_t* seg_start = nullptr;  // [n_pairs]
    uint32_t* prefix = nullptr;     // [n_pairs + 2] task prefix + task counter
    uint32_t* cand = nullptr;       // [n_pairs * cap] worst case
    float* rq = nullptr;            // [n_moving * 4 * cap] phase-A rotations (quaternions) for the SAT stage
    double* sc = nullptr;           // [cap * dof * 2] exact joint (sin, cos) for phase B
    double* links = nullptr;        // [links_cap * n_links * 7] link-pose rows (worlds with free frames)
    long long links_cap = 0;
    long long cap = 0;
    uint64_t last = 0;              // LRU tick (get_workspace)
  };
  std::mutex ws_mu;
  std::map<hipStream_t, Workspace> ws;
  // free frames: the current poses (host copy, device buffer DevWorld::free_cur
  // points to) and the grow-only staging of host-buffer calls (host_mu)
  std::vector<double> free_host;
  double* free_dev = nullptr;
  struct FreeStage {
    double *q = nullptr, *fp = nullptr, *links = nullptr;
    uint8_t* fl = nullptr;
    uint32_t* mk = nullptr;
    size_t q_cap = 0, fp_cap = 0, links_cap = 0, fl_cap = 0, mk_cap = 0;
  } free_stage;
  // optional per-stage timing (mpg_profile_enable)
  struct Mark {
    int stage;
    hipEvent_t a, b;
  };
  // batched motion validation buffers (grow-only)
  struct Motion {
    double* edges = nullptr;
    size_t edges_cap = 0;
    int32_t* segs = nullptr;
    size_t segs_cap = 0;
    long long* offs = nullptr;
    size_t offs_cap = 0;
    int32_t* out = nullptr;  // staging: first_invalid[n] then valid[n] bytes
    size_t out_cap = 0;
    double* states = nullptr;
    size_t states_cap = 0;
    uint8_t* flags = nullptr;
    size_t flags_cap = 0;
    double* fp = nullptr;  // host-memory free poses of the call: [free_rows * n_free * 7]
    size_t fp_cap = 0;
    int32_t* row_of = nullptr;  // per-edge free poses: the edge of each sub-state (motion_rowmap_kernel)
    size_t row_of_cap = 0;
    hipEvent_t last = nullptr;  // the previous call's work (scratch order across streams)
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
    double* poses = nullptr;
    size_t poses_cap = 0;
    double* save64 = nullptr;
    size_t save_cap = 0;
    double* q = nullptr;
    size_t q_cap = 0;
    char* out = nullptr;
    size_t out_cap = 0;
    double* pts = nullptr;  // device-buffer calls: points nobody asked for
    size_t pts_cap = 0;
    double* links = nullptr;  // worlds with free frames: link-pose rows
    size_t links_cap = 0;
    double* fp = nullptr;  // host-memory free poses of the call: [free_rows * n_free * 7]
    size_t fp_cap = 0;
    hipEvent_t last = nullptr;  // the previous call's work (scratch order across streams)
    ccdx::BigPolytope* big = nullptr;  // kBigPool EPA polytopes (distance_redo_kernel)
    size_t big_cap = 0;
    unsigned* list = nullptr;  // overflowed configurations: [count, ids...]
    size_t list_cap = 0;
  } dist;
  // host-buffer contact calls: grow-only device staging (guarded by host_mu)
  struct ContactStage {
    double *in = nullptr, *out = nullptr;
    uint8_t* fl = nullptr;
    uint32_t* mk = nullptr;
    double* fp = nullptr;  // host-memory free poses of the call
    size_t in_cap = 0, out_cap = 0, fl_cap = 0, mk_cap = 0, fp_cap = 0;
  } contact;
  std::mutex dist_mu;
  std::mutex prof_mu;
  bool prof = false;
  std::vector<Mark> marks;
  std::vector<hipEvent_t> ev_pool;
  double prof_ms[MPG_NUM_STAGES] = {0, 0, 0};
  int64_t prof_n[MPG_NUM_STAGES] = {0, 0, 0};
  int64_t prof_cfg = 0;                       // configurations launched while profiling
  unsigned long long* prof_units = nullptr;   // device counter: narrow candidates
  long long max_chunk = 1 << 20;
  int narrow_blocks = 1024;
  // large batches: two halves, the second on an internal stream, so one
  // half's latency-bound bucketing overlaps the other's compute
  long long overlap_min = 1 << 18;  // 0 disables (env MPG_OVERLAP_MIN)
  int overlap_parts = 2;             // env MPG_OVERLAP_PARTS
  // large batches: half of the parts on a side stream (per caller stream)
  struct Side {
    hipStream_t side;
    hipEvent_t fork, join;
    uint64_t last;
  };
  std::map<hipStream_t, Side> sides;  // guarded by ws_mu
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
  double* h_q = nullptr;       // pinned, [small cap * row]
  uint8_t* h_hits = nullptr;   // pinned coherent host-mapped, [n_pairs * small cap]
  uint8_t* d_hits = nullptr;   // device alias of h_hits
  double* d_qs = nullptr;      // device input of the latency path
  double* d_qmap = nullptr;    // h_q as the device sees it (zero-copy input)
  double* d_ssc = nullptr;     // latency path joint (sin, cos) [small cap * dof * 2]
  double* h_ssc = nullptr;     // pinned host-mapped twin: sin/cos computed on the host (small batches)
  double* d_sscmap = nullptr;  // h_ssc as the device sees it
  int64_t small_host_sc = 64;  // latency batches up to this size: sin/cos on the host (MPG_SMALL_HOST_SC)
  bool small_args = true;      // the fewest states' rows in the kernel arguments (MPG_SMALL_ARGS=0: off)
  std::vector<int> h_rev_src;  // move-group slots of revolute joints (host copy of the snapshot's rule)
  // host-buffer calls without a stream run on this non-blocking stream (not
  // the legacy default stream, whose synchronisation covers every blocking
  // stream of the device); MPG_OWN_STREAM=0 keeps the caller's NULL stream
  hipStream_t own_stream = nullptr;
  bool small_zero_copy = true; // MPG_SMALL_ZEROCOPY=0: stage through d_qs
  int64_t small_inline_sc = 256;  // latency batches up to this size: sin/cos inline (MPG_SMALL_INLINE_SC)
  // latency server (lat_server_kernel): control block in host-mapped memory,
  // its own stream; started on demand, leaves after srv_idle_us idle
  SrvCtl* srv_h = nullptr;
  SrvCtl* srv_d = nullptr;
  hipStream_t srv_stream = nullptr;
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
  size_t small_qcap = 0;  // input doubles (h_q, d_qs)
  // host-buffer batches above small_max (collide_host_pipelined): chunks
  // through a ring of slots -- the input of one chunk crosses PCIe while the
  // previous one computes and the one before is unpacked on the host.
  // Grow-only, guarded by host_mu.
  static constexpr int kRing = 3;
  struct Ring {
    double* d_in[kRing] = {};
    uint8_t* d_fl[kRing] = {};
    uint32_t* d_mk[kRing] = {};
    uint32_t* d_bcnt[kRing] = {};  // colliding configurations per kPackCfg block
    uint8_t* h_fl[kRing] = {};     // pinned, host-mapped: the chunk's flags (mask_pack_kernel)
    uint32_t* h_mk[kRing] = {};    // pinned, host-mapped: packed mask rows (mask_pack_kernel)
    uint32_t* h_mk_d[kRing] = {};  // h_mk as the device sees it
    uint32_t* h_bcnt[kRing] = {};  // pinned, host-mapped copy of d_bcnt (where each block's packed rows start)
    uint8_t* h_fl_d[kRing] = {};   // device aliases of h_fl, h_bcnt
    uint32_t* h_bcnt_d[kRing] = {};
    hipEvent_t e_in[kRing] = {}, e_done[kRing] = {};
    hipStream_t h2d = nullptr;     // input copies
    hipStream_t side = nullptr;    // odd chunks compute here (one chunk's narrow tail overlaps the next's cull)
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
