// Internal host-side structures of libgmmloc_hip.so (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "gmmloc_hip.h"

namespace gl_match {  // gl_match_common.hpp
struct KfSide;
struct MatchSide;
struct MatchPoints;
}  // namespace gl_match

namespace gl {

void set_error(const char* fmt, ...);

#define GL_HIP(expr)                                                                  \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess) {                                                           \
      gl::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return GL_ERR_DEVICE;                                                           \
    }                                                                                 \
  } while (0)

#define GL_REQUIRE(cond, msg)              \
  do {                                     \
    if (!(cond)) {                         \
      gl::set_error("%s: %s", __func__, msg); \
      return GL_ERR_ARG;                   \
    }                                      \
  } while (0)

// the documented size limits of the matcher-side entry points assume gfx950's 160 KB of LDS: on a device with less the REAL limit is
// the LDS the shape needs, reported as such instead of as a raw HIP error of the launch
#define GL_REQUIRE_LDS(c, bytes)                                                                                              \
  do {                                                                                                                        \
    if ((size_t)(bytes) > (size_t)(c)->lds_max) {                                                                             \
      gl::set_error("%s: this shape needs %zu bytes of LDS per workgroup, the device has %d", __func__, (size_t)(bytes), (c)->lds_max); \
      return GL_ERR_ARG;                                                                                                      \
    }                                                                                                                         \
  } while (0)

// Device-resident, immutable GMM (SoA).  Layout (all fp64 unless noted):
//   rec12   K x 12   {mean[3], cov_inv[9]}  -- the association record, 96 B
//   cov     K x 9    row-major covariance
//   det     K
//   scale   K x 3    ascending eigenvalues
//   axis    K x 9    row-major, column c = eigenvector c
//   sqrt_info K x 9  lower Cholesky factor of cov_inv
//   flags   K uint8  bit0 degenerated, bit1 salient
//   plane   K x 8    {normal[3] (= axis col 0), mean[3], pad, pad}
//   nbs_ptr K+1 int32, nbs_idx nnz int32, nbs_dist nnz  (CSR of nbs_)
// Exact cell index of the Mahalanobis argmin (gl_grid.hip): CSR lists of candidate components per
// grid cell + a short list of components every point must evaluate.
struct CellIndex {
  bool enabled = false;
  double lo[3] = {0, 0, 0};
  double h = 0, inv_h = 0, t_resolve = 0;
  int dim[3] = {0, 0, 0};
  int nglob = 0;
  size_t nnz = 0, ncell = 0;
  int32_t* ptr = nullptr;   // ncell + 1
  int32_t* idx = nullptr;   // nnz, ascending within a cell
  int32_t* glob = nullptr;  // nglob, ascending
  // packed cells (round 3): {count, then the list itself when count <= 3, else the offset into idx}: ONE random 16-byte
  // read per point where ptr[c], ptr[c + 1] and idx[...] are two (the kernel is bound by the fabric's random sectors)
  void* cell4 = nullptr;    // ncell x int4, or null (table above the memory budget, or the 8-byte form in use)
  void* cell8 = nullptr;    // ncell x 8 bytes (round 6: option assoc_cell8, K < 2^20), or null
  // the records again, one per 128-byte line (K x 16 doubles, the last four unused): a 96-byte record of rec12 lies across
  // two lines three times out of four, and the cooperative gather is bound by line requests (round 5; null without cell4)
  double* rec16 = nullptr;
};

struct Gmm {
  int device = 0;
  int K = 0;
  std::vector<double> h_mean, h_cov;  // host copies (save_file / get)
  double* rec12 = nullptr;
  double* mean = nullptr;  // K x 3 (kNN kernels)
  double* cov = nullptr;
  double* det = nullptr;
  double* scale = nullptr;
  double* axis = nullptr;
  double* sqrt_info = nullptr;
  double* hgw = nullptr;  // K x 6 sym: sqrt_info * sqrt_info^T (EdgePt2Gaussian J^T J, world frame)
  double* plane4 = nullptr;  // K x 4: axis_.col(0) and its dot product with the mean (EdgePt2GaussianDeg's plane)
  uint8_t* flags = nullptr;
  int32_t* nbs_ptr = nullptr;
  int32_t* nbs_idx = nullptr;
  double* nbs_dist = nullptr;
  int nnz = 0;
  CellIndex grid;
  // fp32 screen records of GL_ASSOC_SCREENED (gl_assoc32.hip), built at gl_gmm_create: K x 12 floats
  // {mean - scr_o (3), cov_inv 00 11 22, cov_inv 01+10, 02+20, 12+21, bound constant, pad, pad}; null when the map has
  // values fp32 cannot hold (the screened mode is then the fp64 sweep)
  float* rec32 = nullptr;
  double scr_o[3] = {0, 0, 0};  // map-wide origin the means and points are shifted by
  double scr_rmax = 0;          // max_k |mean_k - scr_o|_inf, rounded up
  double scr_cmax = 0;          // max_k of the bound constant
  gl_params prm;
};

// Tuning / test knobs of a context.  Read ONCE from the environment (GMMLOC_<NAME>) at gl_ctx_create and
// changed afterwards only through gl_ctx_set_option: no libc environment scan on the call paths.
struct Options {
  double ba_shape = -1;         // gl_track_frames refine: -1 auto, 0 one workgroup per frame, 1 one point per thread
  double ba_step32 = 0;         // 1: point step from an fp32 cache of the pass-A solve (faster, not the default)
  double ba_persist = 1;        // 1: the batch-shaped refine runs as persistent workgroups that draw their frames from a queue (0: one block per frame; A/B)
  double ba_front = 1;          // 1: a batch-shaped gl_track_frames makes each frame's records in the refine's own set-up (0: k_ba1_prep; A/B, tests)
  double ba_slow = 0;           // 1: general kernel k_ba1 also for M <= 2000 (A/B)
  double ba_fixed_pack = 0;     // 1: gl_track_frames_anchored with fixed observers always through the general kernel (k_track_pack -> k_ba_gen; A/B, tests)
  double pose_waves = 0;        // gl_optimize_current_pose: 0 auto, 1 / 4 / 8 waves per frame
  double ba_same_xcd = 0;          //   1: the latency shape may use the same-XCD form of its exchange (outside the HIP memory model: opt-in, gmmloc_hip.h)
  double ba_rendezvous_us = 200;   // time limit of EVERY exchange of the latency shape (the fallback it protects costs ~0.5 ms; 0: a workgroup
                                   // gives up at its first unsuccessful look -> follow-up kernel; tests)
  double ba_test_abort_seq = 0;    // tests: n > 0 makes the last workgroup of every frame give up at its n-th exchange
  double test_scratch_fill = -1;   // tests: 0 .. 255 fills every scratch block and the device staging buffer with that byte when it is set, and
                                   // every block ctx_scratch allocates while it stays >= 0 (-1: off; gmmloc_hip.h)
  double pose_regs = 1;         //   0: the frame-at-a-time shapes read their edges from global memory every trial (A/B)
  double bagen_nb = 0;          // gl_joint_optimization, persistent kernel: 0 auto, n workgroups per problem
  double bagen_mode = 0;        //   0: by WINDOW size (never by B), 1: the persistent kernel k_ba_gen, 2: the pipelined shape, 3: persistent, whole batch in one launch (gmmloc_hip.h)
  double view_slot_lds = 0;     // gl_search2d: accepted-list records kept in LDS (0 = all that fit)
  double view_threads = 0;      //   0 auto, 256 / 1024
  double assoc_index_min = -1;  // pairs below which GL_ASSOC_BRUTE stays on the sweep (-1 = built-in)
  double assoc_grid = -1;       // 0: never use the cell index (every association is the N x K sweep); A/B and bench
  double assoc_coop = 1;        // 1: wave-cooperative record gather in the indexed association (k_assoc_cells_coop), 0: a lane per record
  double pipe_fuse_asm = -1;    // pipelined local BA: the solve kernel assembles the system itself (-1: calls of a few windows, 0 never, 1 always; same bits)
  double pose_compact_cap = 1024;  // the largest stride of a compacted pose problem (tests: 512 / 256 drive frames into the full-stride problem)
  double fuse_records = 1;      // gl_fuse_search: 0 = the walk that reads the features from global memory (A/B)
  double pose_compact = -1;     // gl_optimize_current_pose: problems of more than 1 024 slots compacted to 1 024 where their edges fit (-1, default); 1: every problem of more than 256 slots; 0: never
  double assoc_cell8 = 1;       // the packed cell table in 8 bytes per cell where the component indices fit 20 bits (0: 16 bytes per cell as in rounds 3 - 5)
  double assoc_pack_mb = 512;   // memory budget (MB) of the packed cell table a GMM built with this context may add to its cell index (0: none)
  double assoc_cell = 0;        // > 0: cell size (m) of the index instead of the automatic one (tuning)
  double assoc_globcells = 0;   // > 0: components whose box covers more cells than this are evaluated for every point (tuning)
  double match_desc_lds = -1;   // gl_search_by_projection: descriptors in LDS (-1 auto, 0 / 1)
  double pipe_lanes = -1;       // pipelined local BA in batches: streams a call's windows are split over (-1 auto: 2 from 16 windows; 1 .. 4; A/B)
  double pipe_judge = -1;       //   the verdict on a trial as a kernel of its own (-1 auto: from 32 windows per lane; 0 / 1; A/B)
  double schur_kper = -1;       //   chunks of a block one wave of the Schur pass takes (-1 auto; 1 / 2 / 4 / 8; A/B)
  double assoc_screen32 = 0;    // 1: every all-pairs sweep (launch_assoc_sweep) runs as the fp32 screen + fp64 verify of GL_ASSOC_SCREENED (same bits)
};
// name -> member; nullptr if unknown
double* option_slot(Options& o, const char* name);

// a device block of a context, grown on demand (ctx_scratch)
struct ScratchBlock {
  void* p = nullptr;
  size_t bytes = 0;
};
// the context's blocks: separate because their callers hold one while they use another
enum {
  SCRATCH_MAIN,    // the entry points' own scratch
  SCRATCH_CACHE,   // the matchers' candidate cache (gl_search_local_points keeps the projection loop's outputs in the main block
                   // and hands them to gl_search_by_projection)
  SCRATCH_CHAIN,   // the intermediates of gl_track_frame_chain, whose stages use the two blocks above
  SCRATCH_SCREEN,  // the screened association's per-split candidate lists and its fp64 fallback (launch_assoc_screened), so
                   // that it needs nothing from the block its caller sized for the fp64 sweep
  SCRATCH_LOCALMAP,  // gl_update_local_map's global-path counters / bitmask, and the local-map arrays gl_track_frame_chain_map gathers
                     // for its stages (which use the three blocks above)
  SCRATCH_BAWINDOW,  // gl_update_connections / gl_ba_window_build / _apply: per-window words over the map's rows and the window's lists
  SCRATCH_MAPEDIT,   // gl_map_remove, gl_map_add, gl_map_fuse: each call's marks over the map's rows and its lists, then the rebuild of the
                     // CSR (mapdev::CsrRebuild, gl_map_dev.hpp): the scan words and the copy of the CSR it moves from; gl_cull_map_points:
                     // a first-occurrence word per map point, the copy of the candidate list and its scan words
  SCRATCH_MAPTRI,    // gl_create_map_points_from_map: the pair set-up, the gathered pair tables, the mask and the per-match arrays that its
                     // stages (which use the main block and the cache) hand to one another
  SCRATCH_COUNT
};

struct Ctx {
  int device = 0;
  int ncu = 256;  // compute units of the device (shape decisions: frames vs CUs)
  int lds_max = 160 * 1024;  // LDS a workgroup may have on this device (hipDeviceAttributeMaxSharedMemoryPerBlock: 160 KB on gfx950, 64 KB on gfx942)
  Options opt;
  // per-context (= per device, per host thread) caches of driver queries: the dynamic-LDS limit already set
  // for a kernel (hipFuncSetAttribute is per device) and occupancy answers
  std::map<const void*, size_t> lds_limit;
  std::map<std::tuple<const void*, int, size_t>, int> occupancy;  // (kernel, threads, dynamic LDS) -> blocks per CU
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // the device reports its XCC id per workgroup and places block b on XCD b % 8 (probed once at gl_ctx_create): the
  // latency-shape kernels may then use the same-XCD form of their exchange - after checking the ids again at run time
  bool xcc_ids_trusted = false;
  ScratchBlock scratch[SCRATCH_COUNT];
  // staging of the frame-at-a-time host entry point (gl_track_frame_host): page-locked + device mirror, grown on demand
  void* host_stage = nullptr;
  void* dev_stage = nullptr;
  size_t stage_bytes = 0;
  // device counters (gl_ctx_counter_read): [0] frames of latency-shape launches redone by the follow-up kernel
  int32_t* counters = nullptr;
  long coop_fallbacks = 0;  // host side (GL_COUNTER_BA_COOP_FALLBACK): windows of gl_joint_optimization run with one workgroup after a refused cooperative launch
  int* host_word = nullptr;  // page-locked words (the pipelined local BA's counts of unfinished problems, per lane)
  hipStream_t lane_stream[3] = {nullptr, nullptr, nullptr};  // further lanes of the pipelined local BA in batches (launch_ba_pipe)
  hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
  int pipe_hint = 0;         // cycles the last pipelined local BA needed (the next call enqueues that many + 2 ahead)
  const void* orb_pattern = nullptr;  // the device pattern gl_orb_describe has read back and found inside [-13, 13] (gmmloc_hip.h)
  // optional statistics buffer (gl_ctx_set_stats_buffer)
  int32_t* stats = nullptr;
  int32_t* stats_iters = nullptr;  // (gl_ctx_set_stats_buffers) outer Levenberg iterations per frame
  int stats_n = 0;
  int32_t* stats_edges = nullptr;  // (gl_ctx_set_edge_stats_buffer) n x 2: level-0 reprojection edges x trials / x outer iterations
  int stats_edges_n = 0;
  // timing
  bool timing = false;
  double timer_ms[GL_TIMER_COUNT] = {0};
  int64_t timer_n[GL_TIMER_COUNT] = {0};
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
};

// block `which` (SCRATCH_*) of at least `bytes`; growing it waits for the stream and drops the old contents
int ctx_scratch(Ctx* c, size_t bytes, void** out, int which = SCRATCH_MAIN);
int scratch_fill_now(Ctx* c);  // gl_ctx_set_option(test_scratch_fill >= 0)
// consecutive 256-aligned regions of a scratch block from `off` on
struct Regions {
  size_t off;
  size_t take(size_t bytes) {  // the offset of the next region
    const size_t at = off;
    off += ((bytes + 255) / 256) * 256;
    return at;
  }
};
bool probe_xcc_ids(Ctx* c);  // gl_ba_fast.hip
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per DEVICE and costs a driver call: a context (one device,
// one host thread) remembers the limit it has set for each kernel and raises it only when it grows.  The caller
// has made the context's device current.
inline hipError_t ensure_dynamic_lds(Ctx* c, const void* kernel, size_t bytes) {
  size_t& have = c->lds_limit[kernel];
  if (bytes <= have) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) have = bytes;
  return e;
}
// blocks of `kernel` a CU holds at once with `threads` threads and `lds` bytes of dynamic LDS (0 when the query fails): a driver
// call, remembered by the context
inline hipError_t ctx_occupancy(Ctx* c, const void* kernel, int threads, size_t lds, int* occ) {
  const auto key = std::make_tuple(kernel, threads, lds);
  auto hit = c->occupancy.find(key);
  if (hit == c->occupancy.end()) {
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, kernel, threads, lds);
    if (e != hipSuccess) {
      *occ = 0;
      return e;
    }
    hit = c->occupancy.emplace(key, *occ).first;
  }
  *occ = hit->second;
  return hipSuccess;
}
// bracket a launch region with events when timing is enabled
struct TimerScope {
  Ctx* c;
  int id;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  TimerScope(Ctx* ctx, int timer);
  ~TimerScope();
};

inline gl::Gmm* G(const gl_gmm_t* g) { return (gl::Gmm*)g; }
inline gl::Ctx* C(gl_ctx_t* c) { return (gl::Ctx*)c; }

// .gmm stream (gl_io.cpp)
int read_gmm_file(const char* path, std::vector<double>& mean, std::vector<double>& cov);
int write_gmm_file(const char* path, const double* mean, const double* cov, const uint8_t* flags, int K);

// vocabulary file and tree rules (gl_io.cpp); the device object (gl_bow.hip)
struct VocFile {
  int n_nodes = 0, k = 0, L = 0;  // n_nodes: root included; the arrays hold the records of the nodes 1 .. n_nodes - 1
  std::vector<int32_t> parent;
  std::vector<uint8_t> desc, is_leaf;
  std::vector<float> weight;
};
struct VocLayout {
  std::vector<int32_t> nchild, first;  // by node id (root = 0): child count, layout position of the first child
  std::vector<int32_t> pos, word;      // by record (node id - 1): layout position, word id (-1: not a leaf)
  int n_words = 0, max_children = 0, min_leaf_level = 0;
};
int voc_check(int n_nodes, const int32_t* parent, const uint8_t* is_leaf, int err, VocLayout* out);
int read_voc_file(const char* path, VocFile* out);
// Device-resident, immutable vocabulary.  The records in layout order (VocLayout::pos): the children of a node are contiguous and in
// child order, the root's children come first.
//   desc  n_rec x 32 B   the node's descriptor (two 16-byte halves)
//   meta  n_rec x int4   {node id, child count (0: a leaf), layout position of the first child | word id of a leaf, weight bits}
struct Voc {
  int device = 0;
  int n_nodes = 0, n_words = 0, k = 0, L = 0, max_children = 0, min_leaf_level = 0, root_children = 0;
  size_t bytes = 0;
  void* desc = nullptr;
  void* meta = nullptr;
};

// fixed observer key-frames of gl_track_frames_anchored (the caller's device arrays: gmmloc_hip.h, gl_track_anchor)
struct TrackFixed {
  int F;
  const double* pose;   // B x F x 7
  const double* obs;    // B x M x F x 3
  const int32_t* oct;   // B x M x F
  uint8_t* erase;       // B x M x F out, or null
};
// The launch scratch of the per-frame refine (gl_track_frames*): the shape it runs in and the byte offset of each region.
// ba1_layout (gl_ba_fast.hip) decides the shape first and lays out only what that shape uses.
struct Ba1Layout {
  bool spread;  // the on-chip path's latency shape (SPREAD, then DENSE for the frames it did not complete)
  // general kernel (k_ba1), per point: trial point (3 doubles), chi2, level (1 byte)
  size_t trial, chi, lev;
  // on-chip path, from the start again (a launch runs one of the two kernels): per point the records of k_ba1_prep
  // (prep_view: 36 B); the frame queue of the persistent DENSE workgroups (an int); per frame the prior edge's inverse
  // measurement {R, t} (12 doubles)
  // front: the refine makes those records in its own set-up (the fused front, gl_ba_fast_impl.hpp: ba1_front), k_ba1_prep does not
  // run, and `rec` holds one frame's worth per WORKGROUP of the launch instead of per frame
  bool front;
  size_t rec, frame_ctr, prior_mi;
  // latency shape only: per frame 2 G x 64 exchange words and {abort, done}; the staging area of its results
  // {points B x L x 3 | pose B x 8 | association B x L}, whose inner split the kernel keeps
  size_t parts, ctl, stage;
  // fixed observer key-frames (F > 0, FixedV): per frame and key-frame its pose {R, t}; per point and key-frame the normalised
  // observation, octave | stereo << 4, stale chi2
  size_t frt, fobn, foct, chif;
  size_t end;
};
int ba1_layout(Ctx* c, int B, int L, int F, bool prior, bool fast, Ba1Layout* out, bool front_ok = false, int K = 0);

// launchers implemented across the .hip files
int launch_build_components(Ctx* c, Gmm* g);
int launch_build_neighbours(Ctx* c, Gmm* g);
int build_cell_index(Ctx* c, Gmm* g);
void free_cell_index(Gmm* g);
// gl_search_by_projection_frame with a per-frame gate (gl_match.hip): frames with gate_nm[f] >= gate_min are left untouched
struct PoseCompacted;  // gl_pose_compact.hpp
// (gl_refine_pose.hip) problems whose compacted form exists: see there
int pose_compacted_launch(gl_ctx_t* ctx, const gl_camera* cam, const gl_params* prm, int B, int M, double* pose_dev, const double* Xw_dev,
                          const double* obs_dev, const int32_t* octave_dev, uint8_t* outlier_dev, int32_t* ninlier_dev, int nin_stride,
                          const PoseCompacted& pc);
int optimize_current_pose_plain(gl_ctx_t* ctx, const gl_camera* cam, const gl_params* prm, int B, int M, double* pose_dev, const double* Xw_dev,
                                const double* obs_dev, const int32_t* octave_dev, uint8_t* outlier_dev, int32_t* ninlier_dev, int nin_stride);
// (gl_match_bow.hip) gl_search_by_bow on the two sides (gl_match_common.hpp) with a per-frame switch, checks included
int launch_bow_gated(gl_ctx_t* ctx, float nn_ratio, int check_orientation, int B, const gl_match::KfSide& side1, const gl_match::KfSide& side2,
                     int32_t* match21_dev, int32_t* nmatches_dev, const int32_t* run_flag);
int launch_match_frame_gated(gl_ctx_t* ctx, const gl_camera* cam, float scale_factor, int B, int NF, int NL, const double* pose_cw, const double* pose_lw,
                             const double* feat_uv, const float* feat_ur, const int32_t* feat_oct, const float* feat_angle, const uint8_t* feat_desc,
                             const uint8_t* feat_taken, const double* last_pt, const uint8_t* last_valid, const int32_t* last_oct, const float* last_angle,
                             const uint8_t* last_desc, float th, int mono, int check_orientation, int32_t* feat_match, int32_t* nmatches,
                             const int32_t* gate_nm, int gate_min);
// (gl_localmap.hip) Tracking::updateLocalMap on the device and the gather of the chain's local-map arrays from the whole map.
// LocalMapDerive: feat_mp is first MADE from the chain's associations (gl_track_frame_chain_map, step 2) in the same launch.
struct LocalMapDerive {
  int32_t* match_last;        // B x NF in/out
  int32_t* match_kf;          // B x NF in/out, or null
  const int32_t* last_mp;     // B x NL
  const int32_t* kf_feat_mp;  // B x NK, or null
  const int32_t* counts2;     // B x 4 (mode in [3]), or null: no frame is lost
  int NL, NK;
};
struct LocalMapLists {
  int KFcap, NPcap;
  int32_t *feat_mp, *local_kf, *n_local_kf, *local_mp, *n_local_mp, *ref_kf, *kf_count, *status;
};
struct LocalMapGathered {  // B x NPcap (x 3 / x 32), B x NL, B x NK
  double *mp_pos, *mp_normal;
  float *mp_max_dist, *mp_min_dist;
  uint8_t *mp_cand, *mp_desc;
  int32_t *last_to_local, *kf_to_local;
};
int local_map_check(const gl_map_view* map, int B, int NF, const LocalMapLists& L, bool need_point_arrays);
size_t local_map_scratch_bytes(const Ctx* c, const gl_map_view* map, int B, bool have_kf_count);
int local_map_launch(Ctx* c, const gl_map_view* map, int B, int NF, const LocalMapLists& L, const LocalMapDerive* derive, void* scratch);
size_t local_map_gathered_place(void* base, int B, int NPcap, int NL, int NK, LocalMapGathered* out);  // bytes; base may be null (size only)
int local_map_gather_launch(Ctx* c, const gl_map_view* map, int B, int NL, int NK, const LocalMapLists& L, const int32_t* last_mp,
                            const int32_t* kf_feat_mp, const LocalMapGathered& G);
// (gl_point.hip) k_check_map_association, arguments as gl_check_map_association's and already checked
int launch_check_map_association(Ctx* c, const Gmm* g, const gl_camera* cam, const gl_params* prm, int B, int N, const double* pose_dev,
                                 double* pts_dev, const double* uvr_dev, const int32_t* octave_dev, const int32_t* cand_dev,
                                 const int32_t* ncand_dev, int k, int32_t* out_comp_dev);
// (gl_match_tri.hip) k_search_for_triangulation on the two sides, the values as gl_search_for_triangulation's and already checked
int launch_search_for_triangulation(Ctx* c, float scale_factor, int B, const gl_match::KfSide& side1, const gl_match::KfSide& side2,
                                    const double* fmat_dev, const float* epipole_dev, int only_stereo, int check_orientation, int32_t* match12_dev,
                                    int32_t* nmatches_dev);
// (gl_point.hip) the three kernels of gl_create_map_points over N matches on a scratch region of the caller's
size_t create_map_points_scratch_bytes(int N);
int launch_create_map_points(Ctx* c, const Gmm* g, const gl_camera* cam, const gl_params* prm, float scale_factor, int N, int k,
                             const gl_match::MatchSide& side1, const gl_match::MatchSide& side2, const gl_match::MatchPoints& out, void* scratch);
// association launchers (gl_assoc.hip: all-pairs sweep; gl_grid.hip: cell index + sweep of the rest)
int launch_assoc_brute(Ctx* c, const Gmm* g, const double* pts, int N, int32_t* idx, double* d2);
int launch_assoc_sweep(Ctx* c, const Gmm* g, const double* pts, int N, int32_t* idx, double* d2, const int32_t* list,
                       const int32_t* count_dev, void* scratch);
size_t assoc_scratch_bytes(int K, int N, bool listed = false);
// launch shape of either all-pairs sweep (gl_assoc.hip): the points it is shaped for, and for a given number of points per
// thread its point tiles, K splits and Gaussians per split
inline int sweep_points(int N, bool listed) { return listed ? (N / 16 > 256 ? N / 16 : 256) : N; }
void sweep_split(int K, int N, bool listed, int ppt, int* ptiles, int* nsplit, int* kchunk);
// (gl_assoc32.hip) the fp32-screened sweep: same arguments and results as launch_assoc_sweep, own scratch (SCRATCH_SCREEN)
int build_screen_records(Ctx* c, Gmm* g);
int launch_assoc_screened(Ctx* c, const Gmm* g, const double* pts, int N, int32_t* idx, double* d2, const int32_t* list,
                          const int32_t* count_dev);
int launch_assoc_sweep64(Ctx* c, const Gmm* g, const double* pts, int N, int32_t* idx, double* d2, const int32_t* list,
                         const int32_t* count_dev, void* scratch);
int launch_assoc_index(Ctx* c, const Gmm* g, const double* pts, int N, int32_t* idx, double* d2, bool resolve_all,
                       void* scratch);
size_t assoc_index_scratch_bytes(int K, int N, bool resolve_all);

}  // namespace gl
