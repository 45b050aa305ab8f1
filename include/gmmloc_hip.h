/*
 * gmmloc_hip.h -- C-ABI of libgmmloc_hip.so: the MI355X (gfx950) drop-in for the
 * GMM association + structure-constrained refinement hot path of
 * HyHuang1995/gmmloc.  extern "C", plain pointers and sizes, no C++ types, no
 * exceptions across the boundary.
 *
 * The reference has NO plugin / FFI interface for this path: it is ordinary C++
 * methods on heap objects.  Each entry point below names the
 * reference function it replaces (paths relative to the reference root); the
 * adapter a maintainer would add to the reference host is in INTEGRATION.md and
 * include/gmmloc_hip/gmm_adapter.hpp.
 *
 * Conventions
 *   - every call returns int: 0 = GL_OK, <0 = error (gl_last_error_string()).
 *     "not converged" / "no association" are results, not errors.
 *   - components are identified by int32 index = order in the .gmm file
 *     (GMM::getComponent3d(idx), gaussian_mixture.h:147-149); -1 = none.
 *   - poses are 7 doubles  (qx qy qz qw tx ty tz)  = g2o::SE3Quat T_cw
 *     (world -> camera), Eigen coefficient order.
 *   - pointers suffixed _dev are DEVICE pointers valid on the context's device;
 *     those calls are asynchronous on the context's HIP stream.  Pointers
 *     without the suffix are host pointers and the call is synchronous.
 *   - all arithmetic is IEEE fp64 (the reference's scalar_t = double,
 *     common/eigen_types.h:6); float config scalars stay float (config.h:38-89).
 *   - a gl_gmm_t is immutable after creation and may be shared by contexts /
 *     host threads, and so is a gl_voc_t; a gl_ctx_t (stream + scratch) belongs
 *     to one host thread.
 */
#ifndef GMMLOC_HIP_H_
#define GMMLOC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gl_gmm gl_gmm_t;
typedef struct gl_ctx gl_ctx_t;
typedef struct gl_voc gl_voc_t;

enum gl_status {
  GL_OK = 0,
  GL_ERR_ARG = -1,     /* bad argument (reference: CHECK / CHECK_NOTNULL aborts) */
  GL_ERR_IO = -2,      /* file cannot be opened (gmm_utils.cpp:19-22 -> false)   */
  GL_ERR_FORMAT = -3,  /* malformed .gmm stream (gmm_utils.cpp:27-35,44-51) or
                          vocabulary file (gl_voc_file_read)                     */
  GL_ERR_DEVICE = -4,  /* HIP runtime error                                      */
  GL_ERR_NOMEM = -5
};

/* PinholeCamera (cv/pinhole_camera.h) + camera::bf (config.h:38-52). */
typedef struct gl_camera {
  double fx, fy, cx, cy, bf;
  int32_t width, height;
} gl_camera;

/* Hot-path configuration values (config.h:31-89, cfg/v1.yaml). */
typedef struct gl_params {
  double neighbor_dist_thresh; /* gmmmap::neighbor_dist_thresh (2.5)          */
  float tri_lambda2;           /* loc::tri_lambda2   (400)                    */
  float tri_str_thresh;        /* loc::tri_str_thresh (0.0064)                */
  float ba_lambda2;            /* loc::ba_lambda2    (400)                    */
  int32_t tri_check_str_chi2;  /* loc::tri_check_str_chi2 (true)              */
  int32_t ba_first_as_prior;   /* loc::ba_first_as_prior  (true)              */
  float sigma2_inv[8];         /* frame::sigma2_inv, init_config.hpp:60-79    */
} gl_params;

/* Fills the values of gmmloc_ros/cfg/v1.yaml and the float 1.2^(-2l) table. */
void gl_default_params(gl_params* p);

/* What each entry point reads of gl_camera, of gl_params and of its own scale_factor argument.
 *
 * The intrinsics (fx fy cx cy bf) are expected to be values that float represents exactly: the reference holds them as float
 * (config.h:38) and the matchers / the projection loop cast them to float.  "K" = fx fy cx cy, "size" = width height,
 * "sigma2_inv" = the level table (build it for another pyramid as init_config.hpp:60-79 does for 1.2, in float arithmetic),
 * "-" = the argument is not taken.  Every function is checked on the device under non-default values of what it reads
 * (tests/configs.py, tests/test_gpu_configs.py; gl_tri_pair_setup and gl_create_map_points_from_map under the cameras of
 * tests/create_points_cases.py, one of them with fx != fy for the pair set-up, in tests/test_gpu_create_points.py).
 *
 * entry point                      | gl_camera      | gl_params                                                           | scale_factor
 * ---------------------------------+----------------+---------------------------------------------------------------------+-------------
 * gl_gmm_create                    | -              | neighbor_dist_thresh (captured: the neighbour graph)                | -
 * gl_gmm_load_file                 | -              | neighbor_dist_thresh (captured: the neighbour graph)                | -
 * gl_search2d                      | K size         | -                                                                   | -
 * gl_optimize_point                | K bf           | tri_lambda2 tri_str_thresh tri_check_str_chi2 sigma2_inv            | -
 * gl_check_map_association         | K bf           | as gl_optimize_point (+ the graph the GMM captured)                 | -
 * gl_optimize_triangulation        | K bf           | tri_lambda2 tri_str_thresh tri_check_str_chi2 sigma2_inv            | -
 * gl_create_map_points             | K bf size      | tri_lambda2 tri_str_thresh tri_check_str_chi2 sigma2_inv            | level ratios
 * gl_tri_pair_setup                | K              | -                                                                   | -
 * gl_create_map_points_from_map    | K bf size      | as gl_create_map_points                                             | level ratios, sigma2
 * gl_create_stereo_points          | K bf           | as gl_check_map_association                                         | -
 * gl_create_temporal_points        | K              | -                                                                   | -
 * gl_optimize_current_pose         | K bf           | sigma2_inv                                                          | -
 * gl_joint_optimization            | K bf           | ba_lambda2 tri_str_thresh ba_first_as_prior sigma2_inv              | -
 * gl_joint_optimization_stoppable  | K bf           | ba_lambda2 tri_str_thresh ba_first_as_prior sigma2_inv              | -
 * gl_track_frames                  | K bf           | ba_lambda2 tri_str_thresh sigma2_inv                                | -
 * gl_track_frames_anchored         | K bf           | ba_lambda2 tri_str_thresh ba_first_as_prior sigma2_inv              | -
 * gl_track_frame_host              | K bf           | ba_lambda2 tri_str_thresh sigma2_inv                                | -
 * gl_track_frame_host_anchored     | K bf           | ba_lambda2 tri_str_thresh ba_first_as_prior sigma2_inv              | -
 * gl_search_by_projection          | size           | -                                                                   | level radii
 * gl_search_by_projection_frame    | K bf size      | -                                                                   | level radii
 * gl_search_for_triangulation      | -              | -                                                                   | level sigma2
 * gl_fuse_search                   | size           | -                                                                   | level sigma2
 * gl_project_map_points            | K bf size      | -                                                                   | level steps, band
 * gl_search_local_points           | K bf size      | -                                                                   | both of the above
 * gl_level_steps                   | -              | -                                                                   | level steps
 * gl_update_map_points             | -              | -                                                                   | distance band
 * gl_track_frame_chain             | K bf size      | sigma2_inv                                                          | radii, steps, band
 * gl_track_frame_chain_front       | K bf size      | sigma2_inv                                                          | level radii
 * gl_track_frame_chain_back        | K bf size      | sigma2_inv                                                          | radii, steps, band
 * gl_track_frame_chain_map         | K bf size      | sigma2_inv                                                          | radii, steps, band
 * gl_stereo_matches                | fx bf height   | -                                                                   | level scales, inverses
 * gl_orb_describe                  | -              | -                                                                   | the EXTRACTOR's level scales
 * gl_orb_pyramid(_layout)          | -              | -                                                                   | the EXTRACTOR's inverse scales
 * gl_orb_detect                    | -              | -                                                                   | features per level
 *
 * tri_lambda2 weighs the structure edge of the per-point optimisations (and scales their threshold, tri_str_thresh * tri_lambda2);
 * ba_lambda2 does both for the pose / window optimisations (threshold tri_str_thresh * ba_lambda2).  gl_search_by_bow,
 * gl_bow_transform, gl_associate3d, gl_knn3d, gl_update_local_map, the gl_ba_window_* / gl_map_* calls read none of the three. */

const char* gl_last_error_string(void); /* thread-local */
int gl_device_count(void);

/* ---- context: device + stream + scratch --------------------------------- */
/* hip_stream: the hipStream_t to launch on (e.g. torch's current stream); NULL = the
 * device's default (null) stream. */
int gl_ctx_create(int device, void* hip_stream, gl_ctx_t** out);
int gl_ctx_destroy(gl_ctx_t* ctx);
int gl_ctx_synchronize(gl_ctx_t* ctx);
void* gl_ctx_stream(gl_ctx_t* ctx);
/* Tuning / test options of a context (launch shapes, A/B switches; never the results' meaning).  Each option is
 * initialised ONCE at gl_ctx_create from the environment variable GMMLOC_<NAME IN CAPITALS> and changed only by
 * this call afterwards - no entry point reads the environment.  Names:
 *   ba_shape (-1 auto | 0 one workgroup per frame | 1 one point per thread; same bits either way),
 *   ba_persist (1; 0: the batch-shaped refine of gl_track_frames as one block per frame instead of persistent workgroups drawing frames
 *     from a queue - same bits; A/B),
 *   ba_front (1; 0: a batch-shaped gl_track_frames without d2 output prepares every frame's records in a kernel of its own instead of
 *     in the refine's set-up - same bits; A/B, tests),
 *   ba_step32 (1: fp32-cached point step in gl_track_frames, faster, NOT bit-compatible with the default),
 *   assoc_grid (0: every association is the plain N x K sweep, never the cell index),
 *   assoc_screen32 (0; 1: every all-pairs sweep - GL_ASSOC_EXHAUSTIVE, GL_ASSOC_BRUTE where it sweeps, the points the cell index
 *     leaves unresolved, gl_track_frames* with assoc_grid = 0 - runs as GL_ASSOC_SCREENED: same bits),
 *   assoc_coop (1; 0: the indexed association gathers a record per lane instead of per six lanes - A/B),
 *   ba_rendezvous_us (200): time limit of every exchange between the workgroups of a frame on the latency shape of
 *     gl_track_frames (one point per thread, up to 8 workgroups per frame, launched plainly).  A frame whose workgroups do
 *     not find each other in time - another launch holds the CUs - or lose each other later gives up; its results only
 *     ever reach the caller's buffers through the one-workgroup kernel that always follows, which copies the staged result
 *     of a complete frame and recomputes the others from the untouched inputs: same bits, <= ~0.5 ms more.
 *     GL_COUNTER_BA_REDONE counts those frames,
 *   ba_same_xcd (0): 1 lets the exchange of that shape use its same-XCD form - workgroup-scope atomic stores that stay in
 *     the XCD's L2, polled by the siblings with agent-scope (L1-bypassing) loads: 0.34 instead of 0.37 ms per frame of 2 000
 *     points.  OPT-IN, because it rests on a HARDWARE ASSUMPTION outside the HIP memory model: a workgroup-scope store becomes
 *     visible to an agent-scope load of ANOTHER workgroup on the same XCD because the vector L1 of gfx942 / gfx950 is
 *     write-through and the XCD's workgroups share one L2.  Even when enabled it is used only if (a) a probe at gl_ctx_create
 *     found block b on XCC id b % 8 and (b) the frame's workgroups reported one and the same id in the launch's first
 *     (device-scope) exchange; a word that did not become visible would time the exchange out (ba_rendezvous_us) and send the
 *     frame to the follow-up kernel.  The default (0) uses device-scope stores only: the model-conforming path; same bits,
 *   bagen_mode (0): launch shape of gl_joint_optimization.  A window's RESULT BITS and the call's BLOCKING BEHAVIOUR are a
 *     function of the window shape (P, F, L, NOBS) and this option alone - never of B:
 *       0  by window: the pipelined shape (a kernel per phase, cycles enqueued ahead; 1.4 - 2 x less per Levenberg trial) for
 *          windows of >= 3 000 observations (NOBS), the persistent cooperative kernel below that;
 *       1  the persistent kernel for every window: ASYNCHRONOUS on the context's stream (stream-capturable; the caller
 *          synchronises).  Its workgroup count per window follows NOBS; a batch too large to keep B x that many workgroups
 *          co-resident is launched in sub-batches, in stream order;
 *       2  the pipelined shape for every window that fits it (P <= 22, P + F <= 32): BLOCKING - the call returns with the work
 *          complete (it reads the count of unfinished windows back between chunks of cycles; not stream-capturable);
 *       3  the persistent kernel with the whole batch in ONE launch and as many workgroups per window as stay co-resident:
 *          the fastest form of large batches (round 3's default); asynchronous; the ONE mode in which a window's bits depend
 *          on the batch size (the workgroup count decides the order of its partial sums).
 *     Same arithmetic everywhere, every mode held to the oracle; the shapes add their partial sums in different orders, so a
 *     window may take a different number of trials in each,
 *   assoc_pack_mb (512; memory budget in MB of the packed cell table of a GMM created with this context, 0 = none),
 *   assoc_cell8 (1; that table in 8 bytes per cell where K < 2^20, 0 = 16 bytes per cell; same results),
 *   pose_compact (-1; gl_optimize_current_pose moves the edges of a problem of more than 1 024 slots - one slot per feature, 1 200 in the
 *     reference - to the front of a problem of 1 024 where they fit: one frame of 420 edges 0.31 -> 0.21 ms; 1: every problem of more than
 *     256 slots; 0: never.  Same decisions, poses within 1e-9 of the uncompacted problem's),
 *   assoc_cell, assoc_globcells (> 0: cell size in metres / cell-count threshold of the index instead of the automatic ones),
 *   ba_fixed_pack (1: fixed observers of gl_track_frames_anchored always through the general kernel),
 *   pipe_lanes, pipe_judge, schur_kper (-1 automatic; A/B switches of the pipelined local BA in batches: streams a call is split over,
 *     the verdict on a trial as a kernel of its own, chunks per wave of the Schur pass - none changes a bit),
 *   test_scratch_fill (-1 off; TEST-ONLY): setting it to v in 0 .. 255 fills every scratch block the context holds, and the device
 *     staging buffer of gl_track_frame_host, over its whole length with byte v (a memset on the context's stream); while it stays
 *     >= 0 every scratch block the context allocates is filled the same way right after its allocation.  Nothing else reads it - no
 *     fill between the stages of a call - and setting it back to -1 only stores the value.  No entry point's result may depend on v,
 *   ba_slow, ba_test_abort_seq, pose_waves, pose_regs, bagen_nb, view_slot_lds, view_threads, assoc_index_min, match_desc_lds, fuse_records, pose_compact_cap. */
int gl_ctx_set_option(gl_ctx_t* ctx, const char* name, double value);
int gl_ctx_get_option(gl_ctx_t* ctx, const char* name, double* value);
/* Kernel timing with HIP events on the context's stream: while enabled, every
 * launch of the named hot kernel class is bracketed by events.  Returns the
 * accumulated milliseconds / launch count since the last reset. */
enum gl_timer {
  GL_TIMER_ASSOC = 0,       /* association kernels                                             */
  GL_TIMER_REFINE_POSE = 1, /* k_optimize_current_pose                                         */
  GL_TIMER_BA = 2,          /* the refine kernel proper (k_ba1_fast / k_ba1 / k_ba_gen)        */
  GL_TIMER_BA_PREP = 3,     /* k_ba1_prep: set-up launch of gl_track_frames' refine            */
  GL_TIMER_COUNT = 8
};
int gl_ctx_timing_enable(gl_ctx_t* ctx, int on);
int gl_ctx_timing_read(gl_ctx_t* ctx, int timer, double* total_ms, int64_t* launches, int reset);
/* Event counters of a context (device-side, read with one small synchronous copy on the context's stream). */
enum gl_counter {
  GL_COUNTER_BA_REDONE = 0, /* frames of latency-shape launches of gl_track_frames that gave up and were recomputed by the follow-up kernel */
  GL_COUNTER_MATCH_ROUNDS = 1, /* rounds of the owner fixed point, summed over the frames / pairs of gl_search_by_projection{,_frame},
                                  gl_search_for_triangulation, gl_search_by_bow (what the reference's order-dependent loop costs here) */
  GL_COUNTER_MATCH_UNITS = 2,  /* ... and the number of those frames / pairs */
  GL_COUNTER_BA_COOP_FALLBACK = 3, /* windows of gl_joint_optimization (persistent kernel) that ran with ONE workgroup because even a single
                                      window's cooperative launch was refused (another context holds the CUs): same arithmetic, but the
                                      window's partial sums are added in another order - the one exception to "a window's bits depend on
                                      its shape and bagen_mode only" (a refused sub-batch is first halved at the same workgroup count) */
  GL_COUNTER_ASSOC_SCREEN_VERIFIED = 4, /* (point, Gaussian) pairs that the screened sweep (GL_ASSOC_SCREENED, option assoc_screen32)
                                           re-evaluated in fp64 after its fp32 screen */
  GL_COUNTER_ASSOC_SCREEN_FALLBACK = 5, /* points the screened sweep sent through the full fp64 sweep instead (candidate lists too long,
                                           coordinates fp32 cannot hold, or a map whose records fp32 cannot hold) */
  GL_COUNTER_COUNT = 6
};
int gl_ctx_counter_read(gl_ctx_t* ctx, int counter, int64_t* value, int reset);
/* Optional statistics: while a device buffer of n int32 is registered, gl_track_frames (and gl_track_frames_anchored,
 * gl_joint_optimization) write the number of Levenberg trials (linearise + solve + evaluate) each frame / problem
 * b < n spent, so that the algorithmic work of a launch can be reported.  NULL / 0 unregisters. */
int gl_ctx_set_stats_buffer(gl_ctx_t* ctx, int32_t* trials_dev, int n);
/* ... and, for the per-frame refine (gl_track_frames / gl_track_frames_anchored), the number of OUTER Levenberg iterations
 * (g2o's optimize() iterations: one linearisation each; a trial beyond the first of an iteration re-solves the same
 * linearisation with a larger lambda) into iters_dev (n int32, may be NULL): the two counts bracket the algorithmic work. */
int gl_ctx_set_stats_buffers(gl_ctx_t* ctx, int32_t* trials_dev, int32_t* iters_dev, int n);
/* ... and the ACTIVE part of that work (gl_track_frames / gl_track_frames_anchored on the on-chip refine, M <= 2000): per frame
 * b < n two int32 {sum over its Levenberg trials, sum over its outer iterations} of the number of level-0 reprojection edges the
 * trial / iteration ran on.  The reference puts gated-out edges at level 1 (localization_opt.cpp:799-825): they are in no
 * linearisation after that, so a flop model prices these sums, not points x trials.  edges_dev: n x 2 int32; NULL / 0 unregisters. */
int gl_ctx_set_edge_stats_buffer(gl_ctx_t* ctx, int32_t* edges_dev, int n);

/* ---- GMM map: replaces GMMUtility::loadGMMModel (gmm_utils.cpp:9-67),
 *      GaussianComponent ctor + decompose (gaussian.h:30-39, gaussian.cpp:36-63)
 *      and the GMM::GMM neighbour graph (gaussian_mixture.cpp:43-91) ---------- */
/* mean: K x 3, cov: K x 9 row-major, host pointers. Builds the device-resident
 * SoA (inverse, det, eigen axes/scales, chol(cov^-1), flags) and the
 * Bhattacharyya neighbour graph (CSR) on the GPU. */
int gl_gmm_create(gl_ctx_t* ctx, const double* mean, const double* cov, int K, const gl_params* prm,
                  gl_gmm_t** out);
/* .gmm stream reader: varint32 count, then count x {varint32 size, ComponentProto}
 * (protobuf_utils.cpp:12-29,42-80; GMM.proto:5-14). */
int gl_gmm_load_file(gl_ctx_t* ctx, const char* path, const gl_params* prm, gl_gmm_t** out);
/* GMMUtility::saveGMMModel (gmm_utils.cpp:69-119): same stream, byte-compatible. */
int gl_gmm_save_file(const gl_gmm_t* gmm, const char* path);
int gl_gmm_destroy(gl_gmm_t* gmm);
int gl_gmm_count(const gl_gmm_t* gmm);
/* Host-only halves of the two calls above (no device needed): parse a .gmm stream into
 * caller arrays (mean cap x 3, cov cap x 9 row-major; either may be NULL to query *K_out),
 * and write one (flags: bit0 is_degenerated, bit1 is_salient per component). */
int gl_gmm_file_read(const char* path, double* mean, double* cov, int cap, int* K_out);
int gl_gmm_file_write(const char* path, const double* mean, const double* cov, const uint8_t* flags, int K);

/* Map::summarize (map.cpp:162-188), host only: writes `timestamp tx ty tz qx qy qz qw` (T_wc, TUM format,
 * fixed notation, 6 / 9 digits) for N frames; pose_wc N x 7 in the library's (qx qy qz qw tx ty tz) order. */
int gl_write_tum_trajectory(const char* path, const double* stamps, const double* pose_wc, int N);

enum gl_gmm_field {
  GL_F_MEAN = 0,      /* K x 3 double */
  GL_F_COV = 1,       /* K x 9 double */
  GL_F_COV_INV = 2,   /* K x 9 double   cov_inv_                         */
  GL_F_DET = 3,       /* K double       det_                             */
  GL_F_SCALE = 4,     /* K x 3 double   scale_ (ascending eigenvalues)   */
  GL_F_AXIS = 5,      /* K x 9 double   axis_ row-major, column = vector */
  GL_F_SQRT_INFO = 6, /* K x 9 double   sqrt_info_ = chol_L(cov_inv_)    */
  GL_F_FLAGS = 7,     /* K uint8        bit0 is_degenerated, bit1 is_salient */
  GL_F_NBS_PTR = 8,   /* (K+1) int32    CSR row pointer of nbs_          */
  GL_F_NBS_IDX = 9,   /* nnz int32      neighbour component index        */
  GL_F_NBS_DIST = 10, /* nnz double     NeighbourInfo::dist              */
  GL_F_HGW = 11,      /* K x 6 double   sqrt_info_ sqrt_info_^T, upper triangle 00 01 02 11 12 22 (EdgePt2Gaussian's J^T J) */
  GL_F_PLANE4 = 12    /* K x 4 double   axis_.col(0), axis_.col(0) . mean (EdgePt2GaussianDeg's plane) */
};
/* Copies a derived array to host memory (bytes = capacity of host_out). */
int gl_gmm_get(const gl_gmm_t* gmm, int field, void* host_out, size_t bytes);
int gl_gmm_nbs_count(const gl_gmm_t* gmm);

/* ---- association --------------------------------------------------------- */
enum gl_assoc_mode {
  GL_ASSOC_BRUTE = 0,       /* argmin_k GaussianComponent::chi2 (gaussian.cpp:65-70) over ALL K:
                               the north-star `associate`; first index wins ties.  Served by an
                               exact cell index built at gl_gmm_create (candidates whose chi2 <= 9
                               ellipsoid can reach the point's cell) + an all-pairs sweep of the
                               points it cannot resolve: identical output to GL_ASSOC_EXHAUSTIVE */
  GL_ASSOC_KNN5_EUCLID = 1, /* GMM::queryPoint (gaussian_mixture.cpp:545-576): nearest mean
                               of the exact 5-NN; d2 = its chi2                          */
  GL_ASSOC_EXHAUSTIVE = 2,  /* the same argmin by the plain N x K sweep (no index)       */
  GL_ASSOC_SCREENED = 3     /* the same output as GL_ASSOC_EXHAUSTIVE, bit for bit: an N x K sweep in packed fp32
                               with a rigorous per-pair error bound, then an fp64 re-evaluation (chi2 as above) of
                               every component the bound cannot rule out; points it cannot screen go through the
                               fp64 sweep (GL_COUNTER_ASSOC_SCREEN_VERIFIED / _FALLBACK count both) */
};
/* pts_dev: N x 3; idx_dev: N int32; d2_dev: N double (may be NULL). */
int gl_associate3d(gl_ctx_t* ctx, const gl_gmm_t* gmm, const double* pts_dev, int N, int mode, int32_t* idx_dev,
                   double* d2_dev);
/* Diagnostics of the cell index behind GL_ASSOC_BRUTE (gl_grid.hip).
 * info[8] = {enabled, cell size [m], dim x, dim y, dim z, entries (sum of list lengths),
 *            always-evaluated components, resolve threshold (chi2)}. */
int gl_gmm_index_info(const gl_gmm_t* gmm, double info[8]);
/* Device memory of that index: bytes[3] = {cell pointers, candidate lists, packed cell table}.  The packed table (16 bytes per
 * cell: one random read per point instead of two; 176 MB on the 4 096-Gaussian bench map) is built only within the memory
 * budget of the creating context's option assoc_pack_mb (default 512, 0 = never). */
int gl_gmm_index_bytes(const gl_gmm_t* gmm, double bytes[3]);
/* Number of (point, component) chi2 evaluations the index performs for these N points (its
 * algorithmic work, excluding the exhaustive sweep of unresolved points): *pairs_dev (device
 * int64) is overwritten. */
int gl_assoc_index_work(gl_ctx_t* ctx, const gl_gmm_t* gmm, const double* pts_dev, int N, int64_t* pairs_dev);

/* exact k-NN (k <= 8) on the 3-D means, ascending squared L2 (queryPoint's knnSearch).
 * idx_dev: N x k; dist_dev: N x k (may be NULL).  With fewer than k means (or a NaN query, or NaN means, which are
 * never returned) the remaining entries are padded with idx = -1, dist = +inf.
 * Equal distances are returned lowest index first.  The reference's nanoflann returns them in the order its kd-tree
 * visits the leaves, which is not the index order: on an exact tie the index ORDER differs, and where the tie straddles
 * the k-th place so does the index SET; the distances are the same. */
int gl_knn3d(gl_ctx_t* ctx, const gl_gmm_t* gmm, const double* pts_dev, int N, int k, int32_t* idx_dev,
             double* dist_dev);

/* GMM::renderView (gaussian_mixture.cpp:271-371) + GMM::searchCorrespondence
 * (gaussian_mixture.cpp:484-534) for B key-frames at once
 * (= GMMLoc::associateMapElements, gmmloc_opt.cpp:115-135).
 *  pose_dev: B x 7; uv_dev: B x N x 2; nfeat_dev: B int32 (<= N) or NULL (= N);
 *  cand_dev: B x N x k int32 parent indices in kNN order, gated by 2-D MDist2 < 9, -1 padded;
 *  ncand_dev: B x N int32;
 *  view_ids_dev (optional): B x view_cap int32 rendered parent ids sorted by depth
 *  descending (components2d_ order), -1 padded; nview_dev (optional): B int32.
 *  Components of bit-equal depth keep the order of the merged list (the slot a component took, not its
 *  index): the reference's std::sort leaves them unspecified, the sort here is stable.  nview counts every
 *  rendered component; view_ids holds the first view_cap of them when there are more (the candidate tables
 *  are searched over all of them either way). */
int gl_search2d(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, int B, const double* pose_dev, int N,
                const double* uv_dev, const int32_t* nfeat_dev, int k, int32_t* cand_dev, int32_t* ncand_dev,
                int view_cap, int32_t* view_ids_dev, int32_t* nview_dev);

/* ---- feature matching (the producer of optimizeCurrentPose's correspondences) ---- */
/* ORBmatcher::searchByProjection(Frame&, mappts, stats, th) (orb_matcher.cpp:27-110) with
 * Frame::assignFeaturesToGrid / getFeaturesInArea (frame.cpp:54-79, 121-177),
 * ORBmatcher::DescriptorDistance (orb_matcher.cpp:580-596) and computeRadiusByViewingCos (:112-117),
 * for B frames of NF <= 3072 feature slots and NP <= 4096 projected map points.
 *  cam: width / height size the 64 x 48 feature grid (init_config.hpp:50-54); scale_factor: ORB pyramid
 *  factor (frame::scale_factor, 1.2).
 *  feat_uv B x NF x 2 double; feat_ur B x NF float (u_right, <= 0: none); feat_oct B x NF int32
 *  (< 0: empty slot); feat_desc B x NF x 32 bytes; feat_taken B x NF uint8 (1 = F.mappoints_[i] is set and
 *  has observations on entry);
 *  mp_uvr B x NP x 3 double (ProjStat::uvr); mp_level B x NP int32 (scale_pred, 0..7); mp_viewcos B x NP
 *  double; mp_valid B x NP uint8 (is_in_view_ && !not_valid_); mp_desc B x NP x 32 bytes;
 *  th (3 / 5 in searchLocalPoints, tracking.cpp:258-266), nn_ratio (0.8).
 *  out: feat_match B x NF int32 = index of the map point this call assigned to the feature
 *  (F.mappoints_[bestIdx] = mappt), -1 none; nmatches B int32 (the return value).
 *  The map points are processed in index order exactly like the reference loop: a feature assigned to a
 *  map point is not offered to the later ones. */
int gl_search_by_projection(gl_ctx_t* ctx, const gl_camera* cam, float scale_factor, int B, int NF, int NP,
                            const double* feat_uv_dev, const float* feat_ur_dev, const int32_t* feat_oct_dev,
                            const uint8_t* feat_desc_dev, const uint8_t* feat_taken_dev, const double* mp_uvr_dev,
                            const int32_t* mp_level_dev, const double* mp_viewcos_dev, const uint8_t* mp_valid_dev,
                            const uint8_t* mp_desc_dev, float th, float nn_ratio, int32_t* feat_match_dev,
                            int32_t* nmatches_dev);

/* ORBmatcher::searchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)
 * (orb_matcher.cpp:410-542) + computeThreeMaxima (:544-578): the matcher of
 * Tracking::trackWithMotionModel (tracking.cpp:334-350).  Per frame pair: pose_cw / pose_lw = getTcw() of the
 * current / last frame (B x 7); the current frame's features as above plus feat_angle B x NF float
 * (cv::KeyPoint::angle); the last frame's NL features: last_pt B x NL x 3 (position of its map point),
 * last_valid B x NL uint8 (mappoints_[i] && !is_outlier_[i]), last_oct B x NL int32, last_angle B x NL float,
 * last_desc B x NL x 32 (the map point's descriptor).  th = 7 or 14; mono = bMono; check_orientation =
 * ORBmatcher::check_orientation_.  cam supplies fx fy cx cy bf (as the float config scalars) and width /
 * height.  out: feat_match B x NF int32 = index i of the last-frame feature whose map point the feature
 * received, -1 none (after the rotation-consistency filter); nmatches B int32. */
int gl_search_by_projection_frame(gl_ctx_t* ctx, const gl_camera* cam, float scale_factor, int B, int NF, int NL,
                                  const double* pose_cw_dev, const double* pose_lw_dev, const double* feat_uv_dev,
                                  const float* feat_ur_dev, const int32_t* feat_oct_dev, const float* feat_angle_dev,
                                  const uint8_t* feat_desc_dev, const uint8_t* feat_taken_dev, const double* last_pt_dev,
                                  const uint8_t* last_valid_dev, const int32_t* last_oct_dev,
                                  const float* last_angle_dev, const uint8_t* last_desc_dev, float th, int mono,
                                  int check_orientation, int32_t* feat_match_dev, int32_t* nmatches_dev);
/* ORBmatcher::searchForTriangulation (orb_matcher.cpp:141-293) with checkEpipolarDist (:119-139) and the rotation histogram
 * (computeThreeMaxima, :544-578) for B key-frame pairs: the matches Localization::createMapPoints triangulates
 * (localization_opt.cpp:266).  Per pair and key-frame k = 1, 2 (strides N1 / N2 features, NN1 / NN2 vocabulary nodes):
 *   uv{k}_dev B x N x 2 double, ur{k}_dev B x N float (u_right, < 0: mono), oct{k}_dev B x N int32 (< 0: padding slot),
 *   angle{k}_dev B x N float (key-point angle, degrees), desc{k}_dev B x N x 32 uint8, has_mp{k}_dev B x N uint8 (the feature
 *   already has a map point: getMapPoint(idx) != nullptr);
 *   the DBoW2::FeatureVector of the key-frame as CSR: nnode{k}_dev B int32 (nodes in use), node_id{k}_dev B x NN int32
 *   ASCENDING (std::map order), node_ptr{k}_dev B x (NN + 1) int32, node_idx{k}_dev B x N int32 (feature indices, list order);
 *   fmat_dev B x 9 double: MathUtils::computeFundamentalMatrix(Tcw1, K1, Tcw2, K2), row-major; epipole_dev B x 2 float:
 *   (ex, ey) of :155-160 - both built by the host (Eigen there), see INTEGRATION.md;
 *   scale_factor: frame::scale_factor (the level tables of init_config.hpp:63-79 are rebuilt from it);
 *   only_stereo: bOnlyStereo; check_orientation: ORBmatcher::check_orientation_.
 * out: match12_dev B x N1 int32 = matches12 (feature of key-frame 2 or -1; `matched_pairs` = its non-negative entries in
 * index order), nmatches_dev B int32 (the return value).  Order-exact: the same pairs as the sequential loop. */
int gl_search_for_triangulation(gl_ctx_t* ctx, float scale_factor, int B, int N1, int N2, int NN1, int NN2,
                                const double* uv1_dev, const float* ur1_dev, const int32_t* oct1_dev, const float* angle1_dev,
                                const uint8_t* desc1_dev, const uint8_t* has_mp1_dev, const int32_t* nnode1_dev,
                                const int32_t* node_id1_dev, const int32_t* node_ptr1_dev, const int32_t* node_idx1_dev,
                                const double* uv2_dev, const float* ur2_dev, const int32_t* oct2_dev, const float* angle2_dev,
                                const uint8_t* desc2_dev, const uint8_t* has_mp2_dev, const int32_t* nnode2_dev,
                                const int32_t* node_id2_dev, const int32_t* node_ptr2_dev, const int32_t* node_idx2_dev,
                                const double* fmat_dev, const float* epipole_dev, int only_stereo, int check_orientation,
                                int32_t* match12_dev, int32_t* nmatches_dev);
/* The projection / visibility loop in front of gl_search_by_projection and gl_fuse_search - Tracking::searchLocalPoints
 * (tracking.cpp:233-256), Localization::fuseObservations (localization.cpp:242-254): per map point Frame::project3 (frame.cpp:98-119,
 * pinhole_camera.cpp:46-66, 128-150) and MapPoint::checkScaleAndVisible (mappoint.cpp:257-303).  B frames x NP map points: pose_cw
 * B x 7 (getTcw), t_wc B x 3 (T_w_c_->translation()), pos / normal B x NP x 3 (getPosition, normal_), max_dist / min_dist B x NP float
 * (max_dist_, min_dist_), cand B x NP uint8 (the host's tests in front: non-null, valid, not seen / observed already).  Out: uvr
 * B x NP x 3, level B x NP int32 (ProjStat::scale_pred), viewcos / dist B x NP double (ProjStat), inview B x NP uint8 (is_in_view_ =
 * project3 && checkScaleAndVisible): exactly the mp_* inputs of the two matchers.  cam: fx fy cx cy bf as the float config scalars,
 * width / height. */
/* Host only (no device work): the seven steps of the predicted level of MapPoint::checkScaleAndVisible (mappoint.cpp:289-293) as
 * the HOST's libm gives them - step7[L] = the largest float ratio with ceil(logf(ratio) / logf(scale_factor)) <= L - which
 * gl_project_map_points compares against on the device.  scale_factor in (1, 1.7]. */
int gl_level_steps(float scale_factor, float* step7);
int gl_project_map_points(gl_ctx_t* ctx, const gl_camera* cam, float scale_factor, int B, int NP, const double* pose_cw_dev,
                          const double* t_wc_dev, const double* pos_dev, const double* normal_dev, const float* max_dist_dev,
                          const float* min_dist_dev, const uint8_t* cand_dev, double* uvr_dev, int32_t* level_dev,
                          double* viewcos_dev, double* dist_dev, uint8_t* inview_dev);
/* Tracking::searchLocalPoints (tracking.cpp:213-270), the device part in one call: gl_project_map_points followed by
 * gl_search_by_projection (ORBmatcher(0.8), th 3 - or 5 for the first two frames) on its outputs, which stay in the context's
 * scratch.  Arguments as in the two calls; inview_dev (B x NP uint8, may be null): is_in_view_ per map point, for num_visible_++
 * (tracking.cpp:251) - the host's, or gl_map_stats_track's on the device. */
int gl_search_local_points(gl_ctx_t* ctx, const gl_camera* cam, float scale_factor, int B, int NF, int NP, const double* feat_uv_dev,
                           const float* feat_ur_dev, const int32_t* feat_oct_dev, const uint8_t* feat_desc_dev,
                           const uint8_t* feat_taken_dev, const double* pose_cw_dev, const double* t_wc_dev, const double* mp_pos_dev,
                           const double* mp_normal_dev, const float* mp_max_dist_dev, const float* mp_min_dist_dev,
                           const uint8_t* mp_cand_dev, const uint8_t* mp_desc_dev, float th, float nn_ratio, int32_t* feat_match_dev,
                           int32_t* nmatches_dev, uint8_t* inview_dev);
/* MapPoint::computeDistinctiveDescriptors (mappoint.cpp:126-190) and MapPoint::updateNormalAndDepth (:211-255) for NP points: the
 * refresh of the matchers' per-point inputs after a point's observations change.  what: 1 = descriptor, 2 = normal + depth, 3 = both;
 * an output `what` does not select is not written.  The key-frame table has the layout of gl_fuse_search's feat_oct / feat_desc:
 * kf_twc NKF x 3 (getTwc().translation()), kf_valid NKF uint8 (!not_valid_; NULL: all valid), kf_oct NKF x NFK (features_[i].octave),
 * kf_desc NKF x NFK x 32 (features_[i].desc).  Points: pos NP x 3, pt_valid NP uint8 (!not_valid_; NULL: all valid), ref_kf NP (the
 * row of ref_kf_ in the key-frame table), observations_ as CSR: obs_ptr NP + 1, obs_kf / obs_feat NOBS (key-frame row, feature index).
 * In / out, in the layouts of mp_desc / mp_normal / mp_max_dist / mp_min_dist: desc NP x 32, normal NP x 3, max_dist / min_dist NP.
 * Descriptor arrays 16-byte aligned.  Asynchronous on the context's stream; no allocation.  Needed: obs_ptr (NP > 0), obs_kf / obs_feat (NOBS > 0); what & 1: kf_desc,
 * desc; what & 2: kf_twc, kf_oct, pos, ref_kf, normal, max_dist, min_dist and a finite scale_factor > 0.  The rules (bit for bit):
 *   ORDER       a point's CSR row lists observations_ in the host's iteration order of the unordered_map (as INTEGRATION section 6
 *               does for the local BA); that order is the reference's order and decides the ties.
 *   DESCRIPTOR  only observations whose key-frame is valid count; N = their number.  D[i][j] = 256-bit Hamming distance over those N
 *               descriptors; the median of row i is element (N-1)/2 of the sorted row, D[i][i] = 0 included; the winner is the first
 *               row whose median is strictly the smallest - so N <= 2 takes the first valid observation.  N = 0, a point without
 *               observations or an invalid point: desc untouched.  Exact for any N (rows of more than 32 take a slower path).
 *   NORMAL      normal = (sum over ALL observations, key-frame validity not checked, in list order, of normalized(pos - Ow_i)) / n;
 *               norm = sqrt(x*x + y*y + z*z) (oracle/og_math.hpp), normalized divides by it, a zero vector stays zero (Eigen 3.3+:
 *               assumed).  dist = (float)|pos - Ow_ref|.  level = the octave of the ref key-frame's own observation of the point (its
 *               first in the row); when the ref key-frame does not observe the point, feature 0's octave (observations[pRefKF] inserts
 *               it on the local copy, :245).  max_dist = dist * sf[level], min_dist = max_dist / sf[7], in float; sf = the float
 *               recurrence of init_config.hpp:67-76, 8 levels.  normal, max_dist and min_dist untouched when the point is invalid,
 *               has no observations, its level is outside 0..7, or ref_kf is outside [0, NKF).
 *   MALFORMED   a point whose [obs_ptr[p], obs_ptr[p+1]) is not a sub-range of [0, NOBS], or with an observation whose key-frame is
 *               outside [0, NKF) or feature outside [0, NFK), is left entirely untouched. */
int gl_update_map_points(gl_ctx_t* ctx, float scale_factor, int what, int NP, int NKF, int NFK, int NOBS, const double* kf_twc_dev,
                         const uint8_t* kf_valid_dev, const int32_t* kf_oct_dev, const uint8_t* kf_desc_dev, const double* pos_dev,
                         const uint8_t* pt_valid_dev, const int32_t* ref_kf_dev, const int32_t* obs_ptr_dev, const int32_t* obs_kf_dev,
                         const int32_t* obs_feat_dev, uint8_t* desc_dev, double* normal_dev, float* max_dist_dev, float* min_dist_dev);

/* One tracked frame, device resident (round 5; round 6: the fallback, temporal points, the two halves): what Tracking::track
 * (tracking.cpp:34-118) runs per frame - trackWithMotionModel (:333-376), trackKeyFrame when that fails (:297-331),
 * searchLocalPoints (:210-270), trackLocalMap (:272-299) - for B frames as ONE enqueued sequence on the context's stream, every
 * intermediate array in the context's scratch:
 *   1  gl_search_by_projection_frame(th_mm, check_orientation = 1): ORBmatcher(0.9, true).searchByProjection(curr, last, 7); a frame
 *      with fewer than 20 matches is searched again with 2 x th_mm (:340-346; the second launch skips the other frames)
 *   2  a frame with 20 matches or more: gl_optimize_current_pose on the matched features (Xw = the last frame's map point), then the
 *      outliers lose their map point and their is_outlier_ flag (:356-373; drop_src remembers the map point: it has been seen,
 *      :368).  counts2[0] = what trackWithMotionModel returns: the kept matches whose map point has observations (last_observed).
 *      A frame with FEWER than 20 matches returns before the optimisation as the reference does (:352): counts2[0] = 0, its pose
 *      (pose_mm = pose_cw as passed in, bit for bit), its stage-1 matches and its flags are left alone, counts[1] = 0, drop_src = -1
 *      throughout - no map point of it has been seen.
 *   2b (only with the key-frame buffers, kf_desc != NULL) a frame with counts2[0] < 10 (:50-58) goes through trackKeyFrame instead:
 *      gl_search_by_bow(0.7, check_orientation = 1) against the reference key-frame, pose = the LAST frame's, gl_optimize_current_pose,
 *      outliers dropped (drop_kf); its associations are then the key-frame's alone (match_last = -1, match_kf).  The other frames'
 *      workgroups return at once.  counts2[3] = 1 (tracked through the key-frame) or 2 (fewer than 10 kept matches: the reference
 *      reports a tracking failure, :66-71, and the later outputs of the frame mean nothing).
 *   3  gl_search_local_points from the refined pose (t_wc = -R^T t computed on the device): candidates = mp_cand minus the local map
 *      points the frame holds or dropped (last_visible_idx_ == idx, :243); a feature is taken if its map point has observations -
 *      a TEMPORAL point (createTemporalPoints, :44-46: no observation; last_observed = 0) stays matchable and is REPLACED by the
 *      local map point found for its feature (orb_matcher.cpp:74-76, 104: match_last of that feature ends as -1)
 *   4  gl_optimize_current_pose on all features with a map point (trackLocalMap, :276); its outliers are reported, not cleared.
 * THE LOCAL MAP: the reference rebuilds local_mappoints_ between 2 and 3 (Tracking::updateLocalMap, :119-207: the key-frames that
 * observe the frame's CURRENT map points and their neighbours) - host code on host containers.  gl_track_frame_chain takes ONE
 * local map, fixed before stage 1: it reproduces Tracking::track only if that list is the one updateLocalMap would produce
 * (e.g. the previous frame's local map when the covisibility set did not change); stage 3's matches are order-exact for the
 * list it is given, not for a list it never saw.  A host that wants the reference's sequence in one call hands the whole map to
 * gl_track_frame_chain_map (below: updateLocalMap on the device, canonical order); one that must keep its own containers' order
 * calls the two halves -
 *      gl_track_frame_chain_front (1, 2, 2b)  ->  its own updateLocalMap  ->  gl_track_frame_chain_back (3, 4)
 * - one round trip instead of three; front needs drop_src (and drop_kf with the fallback) as OUTPUT buffers, back reads match_last /
 * match_kf / drop_src / drop_kf and the to_local maps against the NEW local map.
 * What the host keeps doing: countObservations bookkeeping (num_visible_ / num_found_: gl_map_stats_track on these outputs, or the
 * host's own), the decision on counts2[0] / counts2[3]
 * (without the fallback buffers: on counts[0] < 20 as before).  All pointers are DEVICE pointers; layouts as in the single calls. */
typedef struct gl_track_chain_io {
  /* current frame: B x NF (x 2 / x 32) */
  const double* feat_uv;
  const float* feat_ur;
  const int32_t* feat_oct;
  const float* feat_angle;
  const uint8_t* feat_desc;
  const uint8_t* feat_taken; /* features that may not be matched at all (normally zeros) */
  /* last frame: B x NL; last_to_local: index of the feature's map point in the local map below, or -1 */
  const double* pose_lw;
  const double* last_pt;
  const uint8_t* last_valid;
  const int32_t* last_oct;
  const float* last_angle;
  const uint8_t* last_desc;
  const int32_t* last_to_local;
  /* local map: B x NP */
  const double* mp_pos;
  const double* mp_normal;
  const float* mp_max_dist;
  const float* mp_min_dist;
  const uint8_t* mp_cand;
  const uint8_t* mp_desc;
  /* in / out */
  double* pose_cw;      /* B x 7: in the motion-model prediction, out the pose after trackLocalMap (front: after stage 2 / 2b)       */
  double* pose_mm;      /* B x 7 out (may be NULL): the pose after stage 2 / 2b                                                     */
  int32_t* match_last;  /* B x NF out: last-frame feature whose map point the feature holds, or -1                                  */
  int32_t* match_local; /* B x NF out: local map point found in stage 3, or -1                                                      */
  uint8_t* outlier;     /* B x NF out: is_outlier_ after stage 4                                                                    */
  int32_t* counts;      /* B x 4 out: matches of stage 1 (after the retry), inliers of stage 2 (2b), matches of stage 3, inliers of stage 4 */
  uint8_t* inview;      /* B x NP out (may be NULL): is_in_view_ of stage 3                                                         */
  /* ---- round 6; every pointer below may be NULL (a zero-initialised struct behaves as in round 5) ---- */
  const uint8_t* last_observed; /* B x NL: countObservations() > 0 of the last-frame feature's map point (NULL: all of them)        */
  int32_t* drop_src;    /* B x NF out: the last-frame feature whose map point stage 2 dropped as an outlier, or -1                  */
  int32_t* counts2;     /* B x 4 out: {return value of trackWithMotionModel, searchByBoW matches, return value of trackKeyFrame,
                           mode 0 motion model / 1 key-frame / 2 lost}; required with the fallback                                  */
  /* the fallback (trackKeyFrame): the reference key-frame, side 1 of gl_search_by_bow, B x NK; kf_desc == NULL: no fallback        */
  int32_t NK, NNK, NNF; /* key-frame features; node capacities of the key-frame's and the frame's feature vectors                   */
  int32_t reserved_;
  const float* kf_angle;
  const uint8_t* kf_desc;
  const uint8_t* kf_has_mp;
  const int32_t* kf_nnode;
  const int32_t* kf_node_id;
  const int32_t* kf_node_ptr;
  const int32_t* kf_node_idx;
  const double* kf_pt;          /* B x NK x 3: position of the key-frame feature's map point                                         */
  const int32_t* kf_to_local;   /* B x NK: index of that map point in the local map, or -1                                           */
  const int32_t* feat_nnode;    /* the frame's DBoW2::FeatureVector as CSR (ORBVocabulary::transform, :298): B, B x NNF, B x (NNF+1), B x NF */
  const int32_t* feat_node_id;
  const int32_t* feat_node_ptr;
  const int32_t* feat_node_idx;
  int32_t* match_kf;    /* B x NF out: key-frame feature whose map point the feature holds (mode 1), or -1                          */
  int32_t* drop_kf;     /* B x NF out: the key-frame feature whose map point stage 2b dropped, or -1                                */
} gl_track_chain_io;
int gl_track_frame_chain(gl_ctx_t* ctx, const gl_camera* cam, const gl_params* prm, float scale_factor, int B, int NF, int NL, int NP,
                         const gl_track_chain_io* io, float th_mm, float th_local, float nn_ratio, int mono);
int gl_track_frame_chain_front(gl_ctx_t* ctx, const gl_camera* cam, const gl_params* prm, float scale_factor, int B, int NF, int NL, int NP,
                               const gl_track_chain_io* io, float th_mm, int mono);
int gl_track_frame_chain_back(gl_ctx_t* ctx, const gl_camera* cam, const gl_params* prm, float scale_factor, int B, int NF, int NL, int NP,
                              const gl_track_chain_io* io, float th_local, float nn_ratio);

/* Tracking::updateLocalMap (tracking.cpp:119-207) on the device, for B frames at once, over the WHOLE map as caller-owned device arrays -
 * the arrays gl_update_map_points reads and writes, plus one key-frame table:
 *   NMP, NKF, NFK, NOBS   map points, key-frames, feature slots per key-frame, observations
 *   mp_valid   NMP uint8, NULL = all        !not_valid_ of a map point
 *   obs_ptr    NMP+1 int32, obs_kf NOBS     observations_ as the CSR of gl_update_map_points (obs_feat is not needed)
 *   kf_valid   NKF uint8, NULL = all        !not_valid_ of a key-frame
 *   kf_mp      NKF x NFK int32              mappoints_[i] of the key-frame as a map-point row, -1 = null
 *   mp_pos NMP x 3 f64, mp_normal NMP x 3 f64, mp_max_dist / mp_min_dist NMP float, mp_desc NMP x 32 uint8: the per-point matcher
 *              inputs of the whole map (read by gl_track_frame_chain_map only; gl_update_local_map ignores them, NULL allowed)
 * What the reference does, per frame (quirks reproduced, not fixed):
 *   1 (:129-145) for every FEATURE i with a map point (feat_mp[i] >= 0): an invalid point -> feat_mp[i] = -1 (mappoints_[i] = nullptr);
 *     else kf_count[kf] += 1 for every observation of the point.  Per feature: a point held by two features counts twice; a temporal
 *     point (no observations) adds nothing.
 *   2 (:147-148) no counter entry at all -> return: local_kf, n_local_kf, local_mp, n_local_mp, ref_kf keep the values passed in
 *     (status bit 1).
 *   3 (:150-166, :183-188) local key-frames = the counted key-frames that are valid; ref_kf = the valid one with the largest count.
 *     An invalid key-frame is counted (kf_count shows it) but is neither local nor ref_kf; when every counted key-frame is invalid the
 *     lists become EMPTY and ref_kf is unchanged.
 *   4 (:167-181) the neighbour loop adds a covisible key-frame only `if (set_local_kfs.count(neigh_kf))`, i.e. only if the set already
 *     holds it: it never adds anything, and its `> 80` break has nothing to limit.  The device version therefore takes no
 *     covisibility input at all.
 *   5 (:191-206) local map points = the union over the local key-frames of their mappoints_ that are non-null and valid, each once.
 * DECLARED DEVIATION: the reference's tie among key-frames of the same maximal count and the ORDER of local_keyframes_ /
 * local_mappoints_ follow unordered_map / unordered_set<pointer> iteration, i.e. the allocator; no second implementation can
 * reproduce them.  Here: ties -> the LOWEST key-frame row; local_kf and local_mp in ASCENDING row order.  (The order of
 * local_mappoints_ decides stage 3's matches where two points compete for a feature.)  A host that must keep its own container
 * order keeps using gl_track_frame_chain_front / _back.
 * In/out: feat_mp B x NF int32.  In/out (step 2 leaves them untouched): local_kf B x KFcap int32 + n_local_kf B, local_mp B x NPcap
 * int32 + n_local_mp B, ref_kf B.  Out: kf_count B x NKF int32 (NULL allowed) - the counter itself, which is also the histogram
 * KeyFrame::updateConnections builds (keyframe.cpp:243-263) when feat_mp is a key-frame's own mappoints_; status B int32 bit flags:
 * GL_LOCAL_MAP_KEPT counter empty (lists kept), GL_LOCAL_MAP_MP_TRUNCATED / _KF_TRUNCATED: more rows than NPcap / KFcap - the LOWEST
 * rows are kept and n_local_* still hold the TRUE counts (local_mp is always made from ALL local key-frames).
 * MALFORMED input is skipped, never read out of bounds: a feat_mp / kf_mp entry outside [-1, NMP) (left as it is, counts nothing), a
 * point whose [obs_ptr[p], obs_ptr[p+1]) is not a sub-range of [0, NOBS] (counts nothing), an observation whose key-frame is outside
 * [0, NKF) (that observation alone).
 * One workgroup per frame; integer LDS / global atomics only, so the result does not depend on scheduling.  The key-frame counters
 * (NKF <= 4 096) and the bitmask over map-point rows (NMP <= 1 048 576) live in LDS sized to the map passed; beyond either bound that
 * array lives in the context's scratch (slower, same result).  Stateless, asynchronous on the context's stream. */
#define GL_LOCAL_MAP_KEPT 1
#define GL_LOCAL_MAP_MP_TRUNCATED 2
#define GL_LOCAL_MAP_KF_TRUNCATED 4
typedef struct gl_map_view {
  int32_t NMP, NKF, NFK, NOBS;
  const uint8_t* mp_valid;
  const int32_t* obs_ptr;
  const int32_t* obs_kf;
  const uint8_t* kf_valid;
  const int32_t* kf_mp;
  const double* mp_pos;
  const double* mp_normal;
  const float* mp_max_dist;
  const float* mp_min_dist;
  const uint8_t* mp_desc;
} gl_map_view;
int gl_update_local_map(gl_ctx_t* ctx, const gl_map_view* map, int B, int NF, int KFcap, int NPcap, int32_t* feat_mp_dev,
                        int32_t* local_kf_dev, int32_t* n_local_kf_dev, int32_t* local_mp_dev, int32_t* n_local_mp_dev, int32_t* ref_kf_dev,
                        int32_t* kf_count_dev, int32_t* status_dev);

/* The tracked frame as ONE call that follows Tracking::track's own sequence: stages 1, 2, 2b, then updateLocalMap on the map points the
 * frame holds after the first optimisation, then stages 3, 4 on THAT local map - no host round trip, nothing uploaded mid-frame.
 * `io` is the gl_track_chain_io of gl_track_frame_chain with mp_pos / mp_normal / mp_max_dist / mp_min_dist / mp_cand / mp_desc /
 * last_to_local / kf_to_local IGNORED (may be NULL): the chain makes them itself, in the context's scratch.  Enqueued in order:
 *   1  stages 1, 2, 2b as gl_track_frame_chain_front
 *   2  feat_mp[i] = match_last[i] >= 0 ? last_mp[match_last[i]] : match_kf[i] >= 0 ? kf_feat_mp[match_kf[i]] : -1; a frame whose
 *      mode is 2 (lost: the reference returns before updateLocalMap) gets -1 throughout, so its lists are kept.  A held point that
 *      is invalid in mp_valid is cleared in full: feat_mp[i] = -1 AND match_last[i] / match_kf[i] = -1 - in the reference
 *      mappoints_[i] = nullptr (:138-139, again :218-219) also takes the feature out of trackLocalMap's pose problem and lets
 *      stage 3 match it again.  mp_valid is ONE snapshot for the whole call (the reference reads a flag another thread may flip
 *      mid-frame; that race is not reproduced).
 *   3  gl_update_local_map on it (in the same launch as 2)
 *   4  the chain's local-map arrays (B x NPcap) gathered from the map's arrays through local_mp: slot s < min(n_local_mp, NPcap) is
 *      map-point row local_mp[s] with mp_cand = 1, the slots above are zeros with mp_cand = 0; last_to_local / kf_to_local by binary
 *      search of last_mp / kf_feat_mp in the ascending list
 *   5  stages 3, 4 as gl_track_frame_chain_back.  match_local indexes local_mp; inview is B x NPcap against it.
 * The padding slots change nothing: every output equals, bit for bit, the two halves run with NP = n_local_mp on the unpadded list.
 * NF and NPcap are bounded by stage 3 as in every chain call (gl_search_local_points: 3 072 features, 4 096 map points on chip); a
 * frame whose local map is larger runs on its lowest NPcap rows and says so (GL_LOCAL_MAP_MP_TRUNCATED).
 * lm: last_mp B x NL int32, kf_feat_mp B x NK int32 (NULL without the fallback): the map-point row behind each last-frame /
 * reference-key-frame feature, -1 for none and for temporal points; feat_mp B x NF out; the lists, ref_kf, kf_count (NULL allowed)
 * and status of gl_update_local_map (the lists in/out: the previous frame's values). */
typedef struct gl_local_map_io {
  const int32_t* last_mp;
  const int32_t* kf_feat_mp;
  int32_t* feat_mp;
  int32_t KFcap;
  int32_t reserved_;
  int32_t* local_kf;
  int32_t* n_local_kf;
  int32_t* local_mp;
  int32_t* n_local_mp;
  int32_t* ref_kf;
  int32_t* kf_count;
  int32_t* status;
} gl_local_map_io;
int gl_track_frame_chain_map(gl_ctx_t* ctx, const gl_camera* cam, const gl_params* prm, float scale_factor, int B, int NF, int NL, int NPcap,
                             const gl_track_chain_io* io, const gl_map_view* map, const gl_local_map_io* lm, float th_mm, float th_local,
                             float nn_ratio, int mono);

/* ---- the mapping thread on the resident map: covisibility, the local-BA window, the write-back ----
 * KeyFrame::updateConnections (keyframe.cpp:243-316) for B key-frames kf_row (B int32 rows of the map's key-frame tables), over the
 * gl_map_view of gl_update_local_map:
 *   1 (:253-272) kf_count[k] += 1 for every observation, by key-frame k != kf_row, of every non-null valid map point in kf_row's kf_mp
 *   2 (:275-276) empty counter -> return: n_conn = 0, status GL_CONN_KEPT (the reference keeps its previous lists; conn_* untouched)
 *   3 (:278-300) the observers with a count >= 15; if none reaches 15, the single observer with the largest count
 *   4 (:302-315) ordered by weight, descending: conn_kf / conn_w B x Ccap int32 = ordered_keyframes_ / ordered_weights_, n_conn B the
 *     TRUE length (more than Ccap: the first Ccap are written, status GL_CONN_TRUNCATED); kf_count B x NKF int32 (NULL allowed) =
 *     map_frame_weights_ as a dense row.
 * An invalid key-frame is counted and listed like any other, as in the reference (its callers filter on not_valid_).  The list is
 * getVectorCovisibleKeyFrames(); getBestCovisibilityKeyFrames(n) is its first n entries (createMapPoints, searchInNeighbors).
 * DECLARED DEVIATION: the reference breaks ties of weight - and the tie for the single largest - by POINTER value (sort on
 * pair<int, KeyFrame*>; unordered_map order for nmax).  Here ties go to the LOWEST key-frame row first.
 * This call only RECOUNTS the key-frame's own list.  addConnection on the OTHER key-frames (:293, :299), removeConnection and best_cov_kf_
 * are gl_covis_update / gl_covis_remove on the resident graph (gl_map_covis, below); a host without it keeps that bookkeeping itself.
 * Malformed input is skipped as in gl_update_local_map; a kf_row outside [0, NKF) gives n_conn = 0 and GL_CONN_BAD_ROW.
 * One workgroup per key-frame, integer atomics only; counters in LDS up to 4 096 key-frames, in the context's scratch above. */
#define GL_CONN_KEPT 1
#define GL_CONN_TRUNCATED 2
#define GL_CONN_BAD_ROW 4
int gl_update_connections(gl_ctx_t* ctx, const gl_map_view* map, int B, const int32_t* kf_row_dev, int Ccap, int32_t* conn_kf_dev,
                          int32_t* conn_w_dev, int32_t* n_conn_dev, int32_t* kf_count_dev, int32_t* status_dev);

/* The rest of the resident map, what the local BA needs and the tracker does not: caller-owned device arrays, row-indexed like
 * gl_map_view.
 *   kf_pose   NKF x 7 f64          getTcw() as (qx qy qz qw tx ty tz); read by build, written by apply
 *   kf_twc    NKF x 3 f64          the camera centres gl_update_map_points reads; written by apply; NULL allowed
 *   kf_uvr    NKF x NFK x 3 f64    features_[i].uv.x, uv.y, u_right (u_right < 0: a monocular observation)
 *   kf_oct    NKF x NFK int32      features_[i].octave (the table of gl_update_map_points)
 *   obs_feat  NOBS int32           feature index of each CSR entry (the array of gl_update_map_points)
 *   mp_assoc  NMP int32            index of asscociations_[0], or -1; read by build, written by apply
 *   kf_first  row of the key-frame with idx_ == 0, or -1 (sets prior[j]) */
typedef struct gl_map_ba_view {
  double* kf_pose;
  double* kf_twc;
  const double* kf_uvr;
  const int32_t* kf_oct;
  const int32_t* obs_feat;
  int32_t* mp_assoc;
  int32_t kf_first;
  int32_t reserved_;
} gl_map_ba_view;
/* B local-BA windows, one slab each (row b of every array), in the layout gl_joint_optimization takes for B = 1; each slab is compact
 * inside its capacity and the entries behind its contents are never written.
 *   poses B x (Pcap + Fcap) x 7: free poses [0, P), fixed poses [P, P + F) - contiguous, the fixed ones start at P, not at Pcap
 *   prior B x Pcap uint8; points B x Lcap x 3; assoc B x Lcap int32; obs_ptr B x (Lcap + 1) int32;
 *   obs_pose B x Ocap int32; obs_uvr B x Ocap x 3; obs_oct B x Ocap int32
 *   the back-maps: win_kf B x (Pcap + Fcap) int32 (key-frame row of pose j), win_mp B x Lcap int32 (map-point row of point l),
 *   win_obs B x Ocap int32 (the position in the map's CSR of observation g)
 *   sizes B x 4 int32 = {P, F, L, nobs}, the TRUE counts; status B int32 (bits below; the points dropped are counted from bit 8 up) */
typedef struct gl_ba_window {
  int32_t Pcap, Fcap, Lcap, Ocap;
  double* poses;
  uint8_t* prior;
  double* points;
  int32_t* assoc;
  int32_t* obs_ptr;
  int32_t* obs_pose;
  double* obs_uvr;
  int32_t* obs_oct;
  int32_t* win_kf;
  int32_t* win_mp;
  int32_t* win_obs;
  int32_t* sizes;
  int32_t* status;
} gl_ba_window;
#define GL_BA_WINDOW_NO_CONN 1      /* empty covisibility counter: the key-frame is the only free pose */
#define GL_BA_WINDOW_P_TRUNCATED 2  /* P > Pcap */
#define GL_BA_WINDOW_F_TRUNCATED 4  /* F > Fcap */
#define GL_BA_WINDOW_L_TRUNCATED 8  /* L > Lcap */
#define GL_BA_WINDOW_O_TRUNCATED 16 /* nobs > Ocap */
#define GL_BA_WINDOW_BAD_ROW 32     /* kf_row outside [0, NKF): sizes = 0 */
#define GL_BA_WINDOW_TRUNCATED 30     /* any of the four */
#define GL_BA_WINDOW_DROPPED_SHIFT 8
/* The window selection of Localization::jointOptimization (localization_opt.cpp:460-516) and the flattening of :639-763, for B
 * key-frames kf_row on the resident map - what INTEGRATION section 6 has the host do by walking its pointer graph.  Quirks reproduced:
 *   free poses   kf_row (whatever its own validity, :462), then the list of gl_update_connections in its order, each MARKED local;
 *                an invalid one is marked but not added (:466-471), so it is neither free nor fixed
 *   points       the free key-frames in that order, their kf_mp slots ascending: every non-null valid point at its FIRST occurrence
 *                (:473-489)
 *   observations each point's CSR entries in CSR order (the host's unordered_map order as uploaded, not re-sorted), those whose
 *                key-frame is valid (:698): obs_pose = the window index of the key-frame, obs_uvr / obs_oct gathered through obs_feat
 *                from kf_uvr / kf_oct
 *   fixed poses  the valid key-frames not marked local, in the order of their FIRST observation in that walk (:491-516).
 *                fixcam_obs / best_obs are dead code (flag_fixsingle is false at :585) and have no counterpart here
 *   prior        prior[j] = (win_kf[j] == kf_first)
 *   no edge      a point that ends with no observation by a valid key-frame and has mp_assoc < 0 has no edge in the reference's graph:
 *                g2o leaves the vertex out of the active set and setPosition (:920) writes back what it read.  Such a point is
 *                DROPPED from the window (the map keeps its position, which is what the reference leaves) and counted in
 *                status >> GL_BA_WINDOW_DROPPED_SHIFT.
 * The order is fully determined by the inputs (the tie rule of gl_update_connections apart): first occurrences by atomicMin on a key,
 * ordered compaction by prefix sum, nothing depends on scheduling.
 * CAPACITIES: a window larger than a capacity sets the truncation bit(s); sizes still hold the TRUE counts; nothing is written outside
 * the slab, and what the slab then holds is not to be optimised - the host grows its buffers and calls again.
 * MALFORMED input is skipped, never read out of bounds: kf_mp / obs_kf rows outside the tables, CSR ranges outside [0, NOBS] (the
 * point then has no observation), an observation whose feature index is outside [0, NFK) (that observation alone).
 * The sizes reach the host by a 16-byte copy of `sizes` and one synchronise; then gl_joint_optimization(B = 1, P, F, L, nobs, the
 * slab's pointers).  Requires NKF x NFK < 2^31.  One workgroup per window; per-key-frame words in LDS up to 4 096 key-frames, else in
 * the context's scratch, which always holds the per-map-point word and the window's lists (B x (3 NMP + NKF) words and a bit per
 * key-frame slot). */
int gl_ba_window_build(gl_ctx_t* ctx, const gl_map_view* map, const gl_map_ba_view* ba, int B, const int32_t* kf_row_dev,
                       const gl_ba_window* win);
/* The write-back of Localization::jointOptimization (:837-853 associations, :898-922 poses and points) onto the resident rows, from
 * the slabs after gl_joint_optimization[_stoppable] (assoc_dropped B x Lcap, obs_erase B x Ocap, iters B: its outputs).  Per window:
 *   kf_pose[win_kf[j]] = poses[j] for j < P;
 *   kf_twc[row] = -(R^T t) when kf_twc is given: with n = sqrt(qx qx + qy qy + qz qz + qw qw), (x, y, z, w) = q / n and R as in
 *     quat_to_R - R00 = 1 - 2 (y y + z z), R01 = 2 (x y - z w), R02 = 2 (x z + y w), R10 = 2 (x y + z w), R11 = 1 - 2 (x x + z z),
 *     R12 = 2 (y z - x w), R20 = 2 (x z - y w), R21 = 2 (y z + x w), R22 = 1 - 2 (x x + y y) - component c is
 *     -((R0c tx + R1c ty) + R2c tz), every operation rounded once (the library is built with -ffp-contract=off);
 *   mp_pos[win_mp[l]] = points[l];  mp_assoc[win_mp[l]] = -1 where assoc_dropped[l] is set;
 *   erase_obs B x Ocap int32 out: the CSR positions win_obs[g] of the observations with obs_erase[g] set, ASCENDING, n_erase B their
 *   number.  Removing them edits the CSR and kf_mp: gl_map_remove(erase_obs, n_erase) on the resident rows, before the next build.
 * A window whose iters is 0 (the stop word was set on entry, nothing ran) or whose sizes exceed a capacity applies nothing
 * (n_erase = 0).  mp_pos_dev is map->mp_pos, non-const; the map's other point arrays are not touched (gl_update_map_points(what = 2)
 * refreshes normals and distances from the new positions and kf_twc). */
int gl_ba_window_apply(gl_ctx_t* ctx, const gl_map_view* map, double* mp_pos_dev, const gl_map_ba_view* ba, int B, const gl_ba_window* win,
                       const uint8_t* assoc_dropped_dev, const uint8_t* obs_erase_dev, const int32_t* iters_dev, int32_t* erase_obs_dev,
                       int32_t* n_erase_dev);

/* ---- editing the resident map: key-frame culling and removals -------------
 * Localization::removeKeyFrames (localization.cpp:334-399) for B candidate lists on ONE unedited map: the verdicts of the sequential
 * loop in list order, each list on its own copy of the state.  The map is NOT modified (gl_map_remove applies a list).
 *   kf_depth  NKF x NFK float   features_[i].depth (-1: none);  th_depth = frame::th_depth
 *   cand_kf   B x Ccap int32, n_cand B int32, on the device: conn_kf / n_conn of gl_update_connections as they are (n_cand above Ccap:
 *             the first Ccap; below 0: none)
 * Per list, per candidate in list order:
 *   - a row outside [0, NKF): GL_CULL_BAD_ROW; else a row that appeared earlier in the list: GL_CULL_DUPLICATE; else kf_first:
 *     GL_CULL_FIRST (:344); else an invalid key-frame: GL_CULL_INVALID.  Nothing is decided for these: cull = 0, counts 0.
 *   - per slot i whose kf_mp holds a valid point that is not DEAD (below): skipped when depth > th_depth || depth < 0 (float compares);
 *     else num_mps++; when the point's weighted count is > 3: its observations by OTHER key-frames outside C with
 *     kf_oct[obs_kf][obs_feat] <= kf_oct[kf][i] + 1 are counted, three make the slot redundant (:366-389; the early break changes nothing)
 *   - cull = (double)num_redundant > 0.9 * (double)num_mps (:394); a culled candidate joins the set C.
 * The state the loop carries is C alone (Map::removeKeyFrame map.cpp:60-110, MapPoint::removeObservation mappoint.cpp:94-118,
 * Map::removeMapPoint map.cpp:40-58): an observation by a key-frame in C does not exist; a point is DEAD when some key-frame in C
 * observes it and its weighted count over the observers outside C is <= 2.
 * The WEIGHTED COUNT of a point is DEFINED from the CSR and kf_uvr: 2 for an observation whose u_right (kf_uvr[obs_kf][obs_feat][2])
 * is >= 0, 1 for a monocular one (mappoint.cpp:78-81).  The reference keeps a counter, num_obs_, that equals it on a consistent map.
 * Out (B x Ccap; entries at and behind n_cand are not written): cull uint8, num_mps / num_redundant int32 (what the loop computed),
 * cand_status int32, cull_rows int32 + n_cull B: the culled rows in list order - the rm_kf of gl_map_remove.
 * MALFORMED input is skipped as in gl_ba_window_build: kf_mp / obs_kf rows outside the tables (that slot / that observation), CSR
 * ranges outside [0, NOBS] (no observation); an obs_feat outside [0, NFK): that observation alone has no octave and no weight (it
 * still makes its key-frame an observer).
 * BOUND: one workgroup per list; C and the rows seen are two bit sets in LDS, 2 x NKF bits: NKF <= GL_CULL_MAX_KF (128 KB of the
 * 160 KB a workgroup has on gfx950).  A larger map is refused: GL_ERR_ARG, nothing launched. */
#define GL_CULL_JUDGED 0
#define GL_CULL_FIRST 1
#define GL_CULL_BAD_ROW 2
#define GL_CULL_INVALID 3
#define GL_CULL_DUPLICATE 4
#define GL_CULL_MAX_KF 524288
int gl_cull_keyframes(gl_ctx_t* ctx, const gl_map_view* map, const gl_map_ba_view* ba, const float* kf_depth_dev, float th_depth, int B, int Ccap,
                      const int32_t* cand_kf_dev, const int32_t* n_cand_dev, uint8_t* cull_dev, int32_t* num_mps_dev, int32_t* num_redundant_dev,
                      int32_t* cand_status_dev, int32_t* cull_rows_dev, int32_t* n_cull_dev);

/* Removals applied IN PLACE to the resident map's mutable arrays (all required but mp_ref_kf; row-indexed as in gl_map_view /
 * gl_map_ba_view; mp_ref_kf NMP int32 = the ref_kf array of gl_update_map_points). */
typedef struct gl_map_edit {
  uint8_t* mp_valid;
  uint8_t* kf_valid;
  int32_t* kf_mp;
  int32_t* obs_ptr;
  int32_t* obs_kf;
  int32_t* obs_feat;
  int32_t* mp_ref_kf; /* NULL allowed */
} gl_map_edit;
/* Three lists of rows on the device, any of them NULL / empty.  The length of a list is *n_x when n_x is given (a device int32,
 * clamped to [0, x_cap]) and x_cap otherwise.
 *   rm_mp      map-point rows (rm_mp / n_rm of gl_cull_map_points - Localization::removeMapPoints :127-152 - or a host's own culling)
 *   erase_obs  CSR positions: erase_obs / n_erase of gl_ba_window_apply (row b of a batch)
 *   rm_kf      key-frame rows IN REMOVAL ORDER: cull_rows / n_cull of gl_cull_keyframes */
typedef struct gl_map_remove_lists {
  const int32_t* rm_mp;
  const int32_t* n_rm_mp;
  const int32_t* erase_obs;
  const int32_t* n_erase;
  const int32_t* rm_kf;
  const int32_t* n_rm_kf;
  int32_t rm_mp_cap, erase_cap, rm_kf_cap;
  int32_t reserved_;
} gl_map_remove_lists;
/* result  3 int32 on the device: {the new NOBS, n_dead, status bits}
 * dead_mp dead_cap int32: the rows of the points that died in this call, ASCENDING (more than dead_cap: the first dead_cap,
 *         GL_MAP_REMOVE_DEAD_TRUNCATED; n_dead stays true); NULL allowed with dead_cap 0
 * obs_new_pos  old NOBS int32, NULL allowed: the new CSR position of every old entry, -1 for one that is gone */
typedef struct gl_map_remove_out {
  int32_t* result;
  int32_t* dead_mp;
  int32_t* obs_new_pos;
  int32_t dead_cap;
  int32_t reserved_;
} gl_map_remove_out;
#define GL_MAP_REMOVE_FIRST_REFUSED 1  /* rm_kf held kf_first: not removed (map.cpp:63) */
#define GL_MAP_REMOVE_DEAD_TRUNCATED 2
/* "The points of rm_mp (Map::removeMapPoint), then the observations of erase_obs (the erase loop of the local BA,
 * localization_opt.cpp:884-894), then the key-frames of rm_kf in list order (Map::removeKeyFrame)", with the reference's cascade - a
 * point whose num_obs_ falls to <= 2 by a removal dies (mappoint.cpp:112, map.cpp:72-73) - as ONE parallel edit.  With w(p) the
 * weighted count (gl_cull_keyframes) of the observations point p keeps:
 *   - an observation is LOST when erase_obs lists it or its key-frame is in rm_kf; a point of rm_mp loses all of them;
 *   - a point of rm_mp, or one that lost something and keeps w <= 2, DIES: mp_valid = 0, no CSR entries, the kf_mp slot of every
 *     remaining observer set to -1; any other point keeps exactly the entries it did not lose, in their order;
 *   - an erased observation clears its observer's slot (keyframe.cpp:200-205);
 *   - the rows of the REMOVED key-frames follow the order of the list (removeKeyFrame never nulls the removed key-frame's own
 *     mappoints_, removeMapPoint nulls the slot of every key-frame that STILL observes the dying point): with rm_kf = r_0, r_1, ... and
 *     t(p) the step at which p dies (-1: before the key-frames; walk p's removed observers in list order, subtract their weights, stop
 *     at the first w <= 2), the slot of r_i that holds p is cleared iff p dies with t(p) < i - kept when r_i's own removal kills p,
 *     and kept for a point that survives;
 *   - kf_valid[rm_kf] = 0.  kf_first is refused (map.cpp:63, GL_MAP_REMOVE_FIRST_REFUSED).  An already invalid key-frame or point, a
 *     duplicate in a list (the FIRST occurrence gives the rank), a row or position outside its table change nothing;
 *   - the CSR is COMPACTED, stable: obs_ptr is rewritten, result[0] = the new NOBS; obs_kf / obs_feat behind it are not written;
 *   - mp_ref_kf[p], when given: a point that SURVIVES and lost the observation by its ref_kf gets the key-frame of its first
 *     surviving CSR entry.  DECLARED DEVIATION: the reference takes observations_.begin() of an unordered_map<pointer>
 *     (mappoint.cpp:108-110).  The entry of a point that dies is left as it is.
 * The map is taken as consistent (kf_mp[obs_kf[o]][obs_feat[o]] is the point of entry o).  Where it is not, the CSR decides what is
 * lost and a slot is cleared only if it holds that point; an entry whose key-frame or feature is outside the tables has no weight and
 * no slot; a point whose CSR range is not inside [0, NOBS] has no entries afterwards; nothing is read or written out of bounds.
 * What stays with the host, from dead_mp / obs_new_pos and the lists it passed: mappoints_.erase, keyframes_.erase, removeConnection,
 * best_cov_kf_, the re-parenting of frame_info_, asscociations_.
 * The cost follows the map, not the edit: flags over NOBS / NMP and a rank per key-frame in the context's scratch (set and reset by
 * the call), a point per thread, a device-wide scan of the surviving counts, and the move THROUGH A COPY of obs_kf / obs_feat in the
 * scratch (an in-place parallel compaction would read what another workgroup has overwritten).  Integer stores and atomicMin only:
 * the result does not depend on scheduling.  Asynchronous on the context's stream, stateless, no host synchronise. */
int gl_map_remove(gl_ctx_t* ctx, int NMP, int NKF, int NFK, int NOBS, const gl_map_edit* ed, const double* kf_uvr_dev, int kf_first,
                  const gl_map_remove_lists* lists, const gl_map_remove_out* out);

/* ---- growing the resident map: new rows, new observations, fuse matches applied in order -------------
 * The counterparts of gl_map_remove on the same caller-owned arrays (gl_map_edit; mp_pos of gl_map_view, mp_assoc of gl_map_ba_view).
 * The arrays keep their allocation and the counts grow, so both calls take CAPACITIES: NMPcap = the rows of the per-point arrays
 * (obs_ptr has NMPcap + 1 entries), OBScap = the entries of obs_kf / obs_feat.  A call first computes the sizes it would produce; if
 * one exceeds its capacity it writes NOTHING to the map, sets GL_MAP_GROW_MP_TRUNCATED / GL_MAP_GROW_OBS_TRUNCATED in its status and
 * `result` holds the sizes that are NEEDED (as gl_ba_window_build does): the host grows its buffers and calls again.
 * The key-frame rows are the caller's: it has written a new key-frame's kf_uvr / kf_oct / kf_desc / kf_pose / kf_mp rows (the one
 * upload that stays) and passes the new NKF.
 * DECLARED CSR ORDER: an entry a point gains is appended BEHIND the entries it holds, in the order of the list (gl_map_add) or of the
 * steps (gl_map_fuse); the reference's observations_ is an unordered_map<pointer> and has no order to follow.
 *
 * gl_map_add - insert and attach, one parallel edit.  Four device lists, any of them NULL / empty, lengths as in gl_map_remove_lists
 * (*n_x when given, clamped to [0, x_cap], else x_cap):
 *   new points  new_pos n x 3 f64, new_assoc n int32, new_ref_kf n int32 (required when mp_ref_kf is given): rows [NMP, NMP + n) get
 *               them, mp_valid = 1 and an empty CSR range at the end.  Descriptor, normal and distances are gl_update_map_points'.
 *   new_kf      key-frame rows whose kf_valid becomes 1; a row outside [0, NKF) changes nothing
 *   attach      triples (att_mp, att_kf, att_feat) IN LIST ORDER, each `mappt->addObservation(kf, feat); kf->addObservation(mappt,
 *               feat)` (mappoint.cpp:72-82, keyframe.cpp:190-193) statement for statement: the point side does nothing when the point
 *               already has an observation by that key-frame - in the CSR or from an earlier triple - and the key-frame side sets
 *               kf_mp[kf][feat] = mp unconditionally, so the LAST triple that names a slot owns it.  Triples may name the new rows.
 *               SKIPPED, each counted in n_skipped: a triple whose point row or feature is outside its table, whose point is invalid,
 *               whose key-frame row is outside the table or invalid (new_kf counts as valid).
 *   walk_kf     per listed row the loop of processNewKeyFrame (localization.cpp:424-437), after the triples, in list order: its
 *               kf_mp slots ascending; a non-null valid point WITHOUT an observation by the key-frame gains the entry (kf, i); one
 *               that has one - in the CSR, from a triple, from a lower slot - is written to already_mp (candidate_mappts_), in slot
 *               order.  A row outside the table, an invalid key-frame and a row listed before change nothing.
 * result 6 int32 = {new NMP, new NOBS, n_attached (entries gained), n_skipped, n_already, status}; already_mp already_cap int32 (more:
 * the first already_cap, GL_MAP_ADD_ALREADY_TRUNCATED, n_already stays true); obs_new_pos old NOBS int32, NULL allowed: the new
 * position of every old entry (nothing is lost; a host mirror follows it as with gl_map_remove).  After a capacity truncation
 * n_attached / n_skipped / n_already are still the true counts and already_mp is written; the map is untouched and obs_new_pos holds
 * -1 in every entry (it is reset before the sizes are known): the host's mirror does not follow it then.
 * "Already" and "last" are decided by LIST INDEX, never by arrival: atomicMax of the triple's index on a word per slot, atomicMin
 * of the request's index in a table keyed by (point, key-frame); a point's gained entries are ordered by index.  The cost follows the
 * map, not the edit, like gl_map_remove: a word per kf_mp slot and per point in the context's scratch (set and reset by the call), a
 * device-wide scan, the CSR moved through a copy in the scratch.  The map is taken as consistent; a point whose CSR range is not inside
 * [0, NOBS] has only its gained entries afterwards; nothing is read or written out of bounds.
 *
 * gl_map_fuse - what Localization::fuseObservations does with its matches (localization.cpp:299-321) and Map::replaceMapPoint
 * (map.cpp:112-150), for ONE key-frame row kf, in list order.  cand_mp n_cand int32: the map-point rows the host passed to the
 * search, in its order; best_idx n_cand int32: gl_fuse_search's output for that list (< 0 or >= NFK: no match).  Per candidate with a
 * match the call re-tests :237-241 ITSELF on the state the steps before left: skipped when its row is outside the table, when it is
 * invalid, when it has an observation by kf - so a duplicate later in the list finds its own earlier attach, or that it has been
 * replaced, as in the reference.  Then with q = kf_mp[kf][best_idx]:
 *   q < 0       the candidate gains (kf, best_idx), the slot becomes the candidate (:315-316)
 *   q invalid   (or a row outside the table) nothing changes (:303);  q == candidate: nothing (map.cpp:113)
 *   q valid     by the WEIGHTED COUNT (gl_cull_keyframes) of the entries each point holds NOW, gained ones included: w(q) > w(cand)
 *               -> replace(src = cand, tgt = q), else replace(src = q, tgt = cand) - a tie goes to the candidate (:305-313)
 * and each of the three counts in n_fused (:320).  replace(src, tgt): src becomes invalid and loses all entries; its entries are
 * walked in ITS CSR ORDER, the ones it gained behind its old ones (the declared order; the reference walks an unordered_map): where
 * tgt has no observation by that key-frame the slot becomes tgt and tgt gains the entry behind what it holds, otherwise the slot
 * becomes -1 and the entry is gone (:138).  mp_ref_kf and mp_assoc of either point are not touched.
 * result 5 int32 = {new NOBS, n_fused, n_attached, n_replaced, status}; repl_src / repl_tgt repl_cap int32 in step order (more: the
 * first repl_cap, GL_MAP_FUSE_REPL_TRUNCATED; n_replaced stays true and the MAP edit is complete either way); obs_new_pos old NOBS
 * int32, NULL allowed: -1 for an entry that is gone, the new position of one that stayed or moved to tgt.
 * NOBS grows only by the attaches, so the capacity is checked BEFORE anything runs: OBScap >= NOBS + n_cand, else result[0] =
 * NOBS + n_cand with GL_MAP_GROW_OBS_TRUNCATED and nothing else is written.  That figure is an UPPER BOUND, not the size the edit
 * produces: a list of which few candidates attach, or whose replaces drop entries, is refused all the same below it.
 * What stays with the host, from repl_src / repl_tgt: mappoints_.erase (num_visible_ / num_found_, :142-143, are gl_map_stats_merge's on
 * the same two lists, ptr_replaced_, :126, is gl_map_note_replaced's), and
 * computeDistinctiveDescriptors of tgt (:144) - gl_update_map_points on the resident arrays before the next key-frame's search.
 * The steps depend on one another through slots, counts and gained entries, so ONE workgroup walks the list; inside a step it works in
 * parallel over src's and tgt's entries.  The walk never edits the CSR: its state (a word per point, a chain of gained entries per
 * point in a log of NOBS + n_cand nodes, a flag per old entry, a stamp per key-frame) lives in the context's scratch, set and reset by
 * the call; one parallel rebuild (count, device-wide scan, stable move through a copy) writes obs_ptr / obs_kf / obs_feat.  The cost
 * follows the map plus the steps.  The map is taken as consistent; where CSR ranges overlap nothing is written at or behind OBScap, and
 * a point whose CSR range is not inside [0, NOBS] has only its gained entries afterwards.
 * Both: integer stores and integer atomics only - the bytes do not depend on scheduling; asynchronous on the context's stream,
 * stateless, no host synchronise.  obs_kf / obs_feat behind the new NOBS are not written.  Map fields read / written:
 *   call        | reads                                                    | writes
 *   gl_map_add  | mp_valid kf_valid kf_mp obs_ptr obs_kf obs_feat          | the same, mp_pos mp_assoc mp_ref_kf (new rows only)
 *   gl_map_fuse | mp_valid kf_mp obs_ptr obs_kf obs_feat kf_uvr (u_right)  | mp_valid kf_mp obs_ptr obs_kf obs_feat */
#define GL_MAP_GROW_OBS_TRUNCATED 1
#define GL_MAP_GROW_MP_TRUNCATED 2
#define GL_MAP_FUSE_REPL_TRUNCATED 4
#define GL_MAP_ADD_ALREADY_TRUNCATED 8
typedef struct gl_map_add_lists {
  const double* new_pos;
  const int32_t* new_assoc;
  const int32_t* new_ref_kf;
  const int32_t* n_new_mp;
  const int32_t* new_kf;
  const int32_t* n_new_kf;
  const int32_t* att_mp;
  const int32_t* att_kf;
  const int32_t* att_feat;
  const int32_t* n_attach;
  const int32_t* walk_kf;
  const int32_t* n_walk;
  int32_t new_mp_cap, new_kf_cap, attach_cap, walk_cap;
} gl_map_add_lists;
typedef struct gl_map_add_out {
  int32_t* result;
  int32_t* already_mp;
  int32_t* obs_new_pos;
  int32_t already_cap;
  int32_t reserved_;
} gl_map_add_out;
int gl_map_add(gl_ctx_t* ctx, int NMP, int NKF, int NFK, int NOBS, int NMPcap, int OBScap, const gl_map_edit* ed, double* mp_pos_dev,
               int32_t* mp_assoc_dev, const gl_map_add_lists* lists, const gl_map_add_out* out);
typedef struct gl_map_fuse_out {
  int32_t* result;
  int32_t* repl_src;
  int32_t* repl_tgt;
  int32_t* obs_new_pos;
  int32_t repl_cap;
  int32_t reserved_;
} gl_map_fuse_out;
int gl_map_fuse(gl_ctx_t* ctx, int NMP, int NKF, int NFK, int NOBS, int OBScap, const gl_map_edit* ed, const double* kf_uvr_dev, int kf,
                int n_cand, const int32_t* cand_mp_dev, const int32_t* best_idx_dev, const gl_map_fuse_out* out);

/* ---- the resident map's found / visible counters and Localization::removeMapPoints -------------
 * Per map point the reference keeps num_visible_ and num_found_ (std::atomic_int, both 1 from the key-frame constructor,
 * mappoint.cpp:18-19) and the const ref_idx_ (the idx_ of the key-frame that made the point, mappoint.cpp:18; -1 by default,
 * mappoint.h:86); the mapping thread keeps the std::list candidate_mappts_.  gl_map_stats holds them on the device beside the arrays
 * of gl_map_edit: caller-owned, row-indexed like it, with capacities like gl_map_add.  The five calls below keep them current from
 * the tracker's and the mapper's own outputs and run removeMapPoints on them; nothing is copied to the host.
 * Every writer of the reference, and the call that is it here:
 *   tracking.cpp:213-225     every FEATURE of the frame that holds a valid map point: num_visible_ += 1 (a point   gl_map_stats_track
 *                            held by two features: +2; an invalid point is un-held instead)
 *   tracking.cpp:249-254     every local map point the frame does not hold that passes project3 and                gl_map_stats_track
 *                            checkScaleAndVisible (is_in_view_): num_visible_ += 1
 *   tracking.cpp:279-292     after trackLocalMap's optimisation every feature that holds a map point and is no     gl_map_stats_track
 *                            outlier: num_found_ += 1
 *   tracking.cpp:62-72       a lost frame returns before the three rows above                                      gl_map_stats_track
 *   mappoint.cpp:18-19       a new point: both counters 1, ref_idx_ = the key-frame's idx_                         gl_map_stats_new_points
 *   map.cpp:124-125,142-143  replaceMapPoint(src, tgt): tgt's counters += src's; nothing when src == tgt (:113)    gl_map_stats_merge
 *   localization.cpp:433, localization_opt.cpp:442, localization_gmm.cpp:445  candidate_mappts_.push_back          gl_map_cand_append
 *   localization.cpp:127-152 removeMapPoints                                                                       gl_cull_map_points
 * Counter arithmetic is 32-bit two's-complement wrap-around (fetch_add on atomic_int), so the order of the adds never matters.
 * All five: asynchronous on the context's stream, stateless, no host synchronise; integer stores and integer atomics only - the bytes
 * do not depend on scheduling; MALFORMED input is skipped as in gl_update_local_map (a row outside its table counts nothing and
 * changes nothing), nothing is read or written out of bounds.  A temporal point has no row and no counter. */
typedef struct gl_map_stats {
  int32_t* mp_visible;   /* NMPcap: num_visible_ */
  int32_t* mp_found;     /* NMPcap: num_found_ */
  int32_t* mp_ref_idx;   /* NMPcap: ref_idx_ */
  const int32_t* kf_idx; /* NKF: idx_ of the key-frame row; NULL = the row itself */
  int32_t* cand;         /* cand_cap: candidate_mappts_ as map-point rows, in list order */
  int32_t* n_cand;       /* 1 device int32, in/out (read clamped to [0, cand_cap]) */
  int32_t cand_cap, reserved_;
} gl_map_stats;
#define GL_MAP_STATS_MP_TRUNCATED 1   /* gl_map_stats_new_points: rows at or above NMPcap were not written */
#define GL_MAP_STATS_CAND_TRUNCATED 2 /* gl_map_cand_append: the list would exceed cand_cap, nothing appended */
#define GL_MAP_STATS_BAD_ROW 4        /* gl_cull_map_points: the list held a row outside [0, NMP) (verdict 5) */
/* The three tracker rows of the table for B frames, on what gl_track_frame_chain_map left on the device (or gl_track_frame_chain_front
 * -> host -> _back with the host's own local_mp): feat_mp B x NF int32, match_local B x NF int32 (an index into local_mp's row),
 * outlier B x NF uint8, inview B x NPcap uint8, local_mp B x NPcap int32, n_local_mp B int32, counts2 B x 4 int32 or NULL (every frame
 * tracked).  A frame with counts2[3] == 2 (lost) adds nothing.  For a tracked frame b:
 *   visible[feat_mp[i]] += 1              per feature with feat_mp[i] >= 0 (the chain has un-held the invalid ones)
 *   visible[local_mp[s]] += 1             per slot s < min(n_local_mp, NPcap) with inview[s]
 *   found[r] += 1                         per feature with !outlier[i], r = local_mp[match_local[i]] when match_local[i] >= 0 (a
 *                                         match_local at or above NPcap: none), else feat_mp[i], and r >= 0
 * The increments of the B frames sum; a row outside [0, NMP) counts nothing.  Only mp_visible / mp_found of `st` are read. */
int gl_map_stats_track(gl_ctx_t* ctx, int NMP, const gl_map_stats* st, int B, int NF, int NPcap, const int32_t* feat_mp_dev,
                       const int32_t* match_local_dev, const uint8_t* outlier_dev, const uint8_t* inview_dev, const int32_t* local_mp_dev,
                       const int32_t* n_local_mp_dev, const int32_t* counts2_dev);
/* The rows [first, first + n) - n the host's, or *n_dev (clamped to [0, n]) when given: n_new_mp of gl_map_add_lists - get visible =
 * found = 1 and ref_idx = kf_idx[new_ref_kf[j]] (the row new_ref_kf[j] itself when kf_idx is NULL; -1, the reference's default, when it
 * is outside [0, NKF)).  new_ref_kf n int32: the list gl_map_add took.  Rows at or above NMPcap (or below 0) are not written:
 * *status_dev (1 int32, always written) = GL_MAP_STATS_MP_TRUNCATED then, else 0. */
int gl_map_stats_new_points(gl_ctx_t* ctx, int NMPcap, int NKF, const gl_map_stats* st, int first, int n, const int32_t* n_dev,
                            const int32_t* new_ref_kf_dev, int32_t* status_dev);
/* candidate_mappts_.push_back in order: the device list rows_dev (already_mp / n_already of gl_map_add), or with rows_dev NULL the
 * row range [first, first + n) (the new rows of createMapPoints), n as above, appended to cand at *n_cand.  If the result would exceed
 * cand_cap NOTHING is appended, *n_cand stays and the status is GL_MAP_STATS_CAND_TRUNCATED; result_dev 2 int32 = {the size of the list
 * afterwards - after a truncation the size NEEDED -, status}.  One workgroup. */
int gl_map_cand_append(gl_ctx_t* ctx, const gl_map_stats* st, const int32_t* rows_dev, int first, int n, const int32_t* n_dev,
                       int32_t* result_dev);
/* repl_src / repl_tgt of gl_map_fuse, n steps (or *n_dev clamped to [0, n]: result[3] of gl_map_fuse against repl_cap), IN STEP ORDER:
 * visible[tgt] += visible[src], found[tgt] += found[src] (map.cpp:142-143).  A step with src == tgt or with a row outside [0, NMP)
 * changes nothing.  The target of one step may be the source of a later one (a -> b, then b -> c): the result is that of the walk in
 * list order.  One workgroup: per 1 024 steps it gathers the at most 2 048 rows into LDS (one slot per distinct row), one lane walks
 * the steps there, the slots are scattered back. */
int gl_map_stats_merge(gl_ctx_t* ctx, int NMP, const gl_map_stats* st, const int32_t* repl_src_dev, const int32_t* repl_tgt_dev, int n,
                       const int32_t* n_dev);
/* Localization::removeMapPoints (localization.cpp:127-152) on the UNEDITED map (gl_map_edit is only read; kf_uvr for the weight) for
 * the key-frame row kf_row: curr_idx = kf_idx[kf_row] (kf_row when kf_idx is NULL).  Per entry of cand, in list order, the first true
 * branch wins:
 *   1  not_valid_ (mp_valid == 0)                                                      -> erased from the list
 *   2  (float)num_found_ / (float)num_visible_ < 0.25f (int -> float and the division   -> removeMapPoint, erased
 *      rounded to nearest; 0/0 = NaN and n/0 = inf are not below 0.25f: they fall through)
 *   3  curr_idx - ref_idx_ >= 2 (in 64 bits on the int32 values) and the point's        -> removeMapPoint, erased
 *      WEIGHTED COUNT (gl_cull_keyframes; 0 for a CSR range outside [0, NOBS]) <= 3
 *   4  curr_idx - ref_idx_ >= 3                                                         -> erased
 *   0  otherwise                                                                        -> kept
 *   5  DECLARED (the reference's list holds no such entry): a row outside [0, NMP)      -> erased, not removed
 * Map::removeMapPoint (map.cpp:40-58) touches only the removed point and the slots that hold it, so a verdict depends on no verdict
 * before it - but for a row listed twice: its later occurrence finds not_valid_ (verdict 1) when the first one removed it and is
 * judged like the first otherwise.  The walk is therefore one parallel pass over a snapshot, a candidate per thread, with a
 * first-occurrence rule decided by LIST INDEX (atomicMin on a word per point in the context's scratch, set by the call), never by
 * arrival.  Out: verdict cand_cap int32 (the old n entries are written); cand compacted IN PLACE, stable, through a copy in the
 * scratch, *n_cand = kept; rm_mp cand_cap int32 + *n_rm_dev: the removed rows in list order, each once, at its first occurrence -
 * rm_mp / n_rm_mp of gl_map_remove_lists as they stand; result 4 int32 = {kept, removed, erased without removal, status}.  The map and
 * the counters are not written. */
int gl_cull_map_points(gl_ctx_t* ctx, int NMP, int NKF, int NFK, int NOBS, const gl_map_edit* ed, const double* kf_uvr_dev,
                       const gl_map_stats* st, int kf_row, int32_t* rm_mp_dev, int32_t* n_rm_dev, int32_t* verdict_dev, int32_t* result_dev);

/* ---- the covisibility graph as part of the resident map ----
 * What a key-frame's connection containers hold is STORED STATE, not a function of the observations: the lists its last
 * updateConnections left, patched by every later addConnection from another key-frame (keyframe.cpp:293, :299, :116-128) and every
 * removeConnection of a culled one (map.cpp:67-68, keyframe.cpp:318-330).  searchInNeighbors reads those lists of OTHER key-frames
 * (localization.cpp:170), so the graph is kept on the device, row-indexed like gl_map_view, NKFcap rows:
 *   cov_kf, cov_w   NKFcap x Wcap int32   map_frame_weights_ of the row in the DECLARED ORDER: weight descending, ties to the lowest
 *                                         key-frame row first (the tie rule of gl_update_connections)
 *   cov_n           NKFcap int32          the number of entries
 *   cov_nord        NKFcap int32          the length of ordered_keyframes_ / ordered_weights_, ALWAYS A PREFIX of the row:
 *                                           after the row's own updateConnections the entries with w >= 15, or the single largest if
 *                                           none reaches 15 (:291-300) - in a descending row both are prefixes, and with the tie rule
 *                                           the single largest is entry 0;
 *                                           after an addConnection that inserted or changed a weight, or a removeConnection that erased
 *                                           something, updateBestCovisibles rebuilds the list from the WHOLE weight map, entries below
 *                                           15 included (:130-150): cov_nord = cov_n.  REPRODUCED, not repaired.
 *   best_cov        NKFcap int32          best_cov_kf_, -1 = none
 * A new row starts with cov_n = cov_nord = 0, best_cov = -1.  A reader cuts cov_n to [0, Wcap] and cov_nord to [0, cov_n].
 * The calls below: caller-owned device arrays, asynchronous on the context's stream, stateless (what a call reads of the context's
 * scratch it has written itself), integer stores and integer atomics whose final value the inputs determine - no byte depends on
 * scheduling -, no scratch memory in any kernel.  A row outside its table (an entry of a list, an entry of cov_kf) is skipped and
 * counted (GL_COVIS_BAD_ROW); nothing is read or written out of bounds.  Every call writes result, 4 int32, [1] = the status bits.
 * CAPACITY, as in gl_map_add: gl_covis_update first finds the widest row it would produce; above Wcap it writes nothing to the graph,
 * sets GL_COVIS_W_TRUNCATED and returns the width it needs in result[0] - the host re-strides the tables and calls again.
 * DECLARED DEVIATIONS, together:
 *   tie order        the reference sorts pair<int, KeyFrame*> and breaks ties of weight by POINTER; here the lowest row comes first
 *   target order     the reference iterates an unordered_set<KeyFrame*> (localization.cpp:183, :193); tgt_kf is in INSERTION order.  The
 *                    order decides results because the fuses are sequential
 *   empty list       Map::removeKeyFrame indexes ordered_keyframes_[0] of a key-frame whose list is empty (map.cpp:82, undefined);
 *                    here best_cov stays as it is and GL_COVIS_EMPTY_LIST is set */
typedef struct gl_map_covis {
  int32_t NKFcap;
  int32_t Wcap;
  int32_t* cov_kf;
  int32_t* cov_w;
  int32_t* cov_n;
  int32_t* cov_nord;
  int32_t* best_cov;
} gl_map_covis;
#define GL_COVIS_W_TRUNCATED 8     /* (beside GL_CONN_KEPT / _TRUNCATED / _BAD_ROW in the same word) */
#define GL_COVIS_EMPTY_LIST 16
#define GL_COVIS_BAD_ROW 32
#define GL_COVIS_LIST_TRUNCATED 64 /* tgt_kf / cand_mp: the true count is above the capacity, the first entries are written */
/* KeyFrame::updateConnections WITH its side effects (keyframe.cpp:243-316) for ONE key-frame row kf_row of `map`:
 *   1  the counter of gl_update_connections (its kernel's counting: an invalid observer is counted like any other)
 *   2  (:275-276) empty counter: nothing changes, status GL_CONN_KEPT, n_conn = 0
 *   3  (:312) the own row becomes the WHOLE counter in the declared order; cov_nord = the entries >= 15, or 1
 *   4  (:293, :299) for every observer with a count >= 15 - the single largest if there is none - addConnection(kf_row, w) on THAT row,
 *      whatever its state (an invalid key-frame's row gains the entry too): absent -> inserted in order; present with another weight
 *      -> changed and moved; in both cases that row's cov_nord = cov_n.  Present with the same weight -> nothing, cov_nord stays.
 *   5  conn_kf / conn_w (Ccap int32) / n_conn (1 int32) exactly as gl_update_connections writes them for the row: a drop-in for it at
 *      processNewKeyFrame (localization.cpp:440) and at the end of searchInNeighbors (:223).
 * result = {the widest row of the call, status (GL_CONN_* | GL_COVIS_W_TRUNCATED), other rows changed, 0}.  Wcap x 8 bytes of LDS. */
int gl_covis_update(gl_ctx_t* ctx, const gl_map_view* map, const gl_map_covis* cov, int kf_row, int Ccap, int32_t* conn_kf_dev, int32_t* conn_w_dev,
                    int32_t* n_conn_dev, int32_t* result_dev);
/* The graph part of Map::removeKeyFrame (map.cpp:60-87) for the rows cull_rows[0 .. n) IN REMOVAL ORDER, n = *n_cull_dev cut to
 * [0, cull_cap] (cull_cap when NULL): cull_rows / n_cull of gl_cull_keyframes.  Per listed row r, one after the other:
 *   (:63)     r == kf_first: skipped
 *   (:67-68)  every row NAMED IN r's weights loses its entry for r if it has one (removeConnection), and then has cov_nord = cov_n.  A
 *             row that names r but is not named BY r keeps its dangling entry, as in the reference: readers filter on kf_valid
 *   (:82-84)  best_cov[r] = entry 0 of r's ordered list (empty: DECLARED above); cov_n[r] = cov_nord[r] = 0.  A row listed twice meets
 *             the empty list at its second occurrence.
 * It stands beside gl_map_remove(rm_kf) and touches no observation, so the order of the two does not matter.  The host re-parents
 * frame_info_ (:89-104) from best_cov.  result = {rows removed, status, entries erased, rows skipped as malformed}. */
int gl_covis_remove(gl_ctx_t* ctx, int NKF, const gl_map_covis* cov, int kf_first, const int32_t* cull_rows_dev, const int32_t* n_cull_dev,
                    int cull_cap, int32_t* result_dev);
/* getBestCovisibilityKeyFrames(N) (keyframe.cpp:163-170; N <= 0: getVectorCovisibleKeyFrames, :152-155) for B rows kf_row: conn_kf /
 * conn_w B x Ccap int32 = the first min(N, cov_nord) entries, n_conn B int32 their TRUE number (above Ccap: the first Ccap, status
 * GL_CONN_TRUNCATED) - the lists gl_create_map_points_from_map, gl_cull_keyframes and gl_tri_pair_setup take.  A row outside [0, NKF):
 * n_conn = 0.  result = {0, status, 0, rows outside the table}. */
int gl_covis_best(gl_ctx_t* ctx, int NKF, const gl_map_covis* cov, int B, const int32_t* kf_row_dev, int N, int Ccap, int32_t* conn_kf_dev,
                  int32_t* conn_w_dev, int32_t* n_conn_dev, int32_t* result_dev);
/* The target key-frames of Localization::searchInNeighbors (localization.cpp:155-179; nn = 10, nn2 = 5 there): for each of the first nn
 * entries kf1 of kf_row's ordered list - invalid or already a target: skipped, and with it its second neighbours (:162-164) - kf1 is
 * inserted, then each of the first nn2 entries kf2 of kf1's ordered list that is valid, not yet a target and not kf_row (:172-174).
 * kf_valid NKF uint8 (NULL: all valid).  tgt_kf Tcap int32 in INSERTION order (declared above), *n_tgt the true count (at most
 * nn + nn x nn2 <= 4 096; above Tcap: the first Tcap, GL_COVIS_LIST_TRUNCATED).  result = {count, status, 0, entries skipped as malformed}. */
int gl_fuse_targets(gl_ctx_t* ctx, int NKF, const gl_map_covis* cov, const uint8_t* kf_valid_dev, int kf_row, int nn, int nn2, int Tcap,
                    int32_t* tgt_kf_dev, int32_t* n_tgt_dev, int32_t* result_dev);
/* The candidates of the reverse fuse (localization.cpp:188-206): the targets tgt_kf[0 .. n) in list order (n = *n_tgt cut to
 * [0, Tcap]), each target's kf_mp slots ascending; a non-null valid point is appended at its FIRST occurrence (the fuse_tgt_kf_ stamp).
 * Validity is the map's when the call runs - after the forward fuses.  kf_idx = curr_kf_->idx_: fuse_tgt_kf_ starts at 0
 * (mappoint.h:95), so for kf_idx == 0 every point looks stamped and the list is empty - REPRODUCED.  First occurrence is decided by
 * atomicMin of (target position x NFK + slot) on a word per point in the context's scratch (set by the call), then flags, the
 * device-wide scan of the CSR rebuilds and a compaction.  cand_mp cand_cap int32, *n_cand the true count (above cand_cap: the first
 * cand_cap, GL_COVIS_LIST_TRUNCATED).  result = {count, status, 0, targets outside the table}. */
int gl_fuse_candidates(gl_ctx_t* ctx, const gl_map_view* map, const int32_t* tgt_kf_dev, const int32_t* n_tgt_dev, int Tcap, int kf_idx,
                       int cand_cap, int32_t* cand_mp_dev, int32_t* n_cand_dev, int32_t* result_dev);

/* Localization::fuseObservations (localization.cpp:226-318), the matching half, for B key-frames: per candidate map point the most
 * similar feature inside Frame::getFeaturesInArea(u, v, th * scale_factors[level]) (frame.cpp:121-177) with octave level - 1 or
 * level and Feature::error(uvr) * sigma2_inv[octave] within 5.99 (mono) / 7.8 (stereo).  Features as in gl_search_by_projection
 * (feat_uv B x NF x 2, feat_ur B x NF float (< 0: mono), feat_oct B x NF (< 0: padding slot), feat_desc B x NF x 32); map points:
 * mp_uvr B x NP x 3 = Frame::project3's (u, v, u_right), mp_level B x NP int32 = ProjStat::scale_pred, mp_valid B x NP uint8 = the
 * host's tests of :238-254 (non-null, valid, not observed by the key-frame, project3 and checkScaleAndVisible passed), mp_desc
 * B x NP x 32.  Out: best_idx B x NP int32 (the feature, if its distance is <= TH_LOW = 50, else -1) and best_dist B x NP int32 (256:
 * no candidate).  The map points do not interact in this loop; what the reference does with a match (:296-312: addObservation, or
 * replaceMapPoint by observation count), in list order, is gl_map_fuse on the resident map - or the host's, on its own containers.
 * cam supplies width / height (the 64 x 48 grid). */
int gl_fuse_search(gl_ctx_t* ctx, const gl_camera* cam, float scale_factor, int B, int NF, int NP, const double* feat_uv_dev,
                   const float* feat_ur_dev, const int32_t* feat_oct_dev, const uint8_t* feat_desc_dev, const double* mp_uvr_dev,
                   const int32_t* mp_level_dev, const uint8_t* mp_valid_dev, const uint8_t* mp_desc_dev, float th,
                   int32_t* best_idx_dev, int32_t* best_dist_dev);
/* ORBmatcher::searchByBoW (orb_matcher.cpp:295-408; computeThreeMaxima :544-578) for B key-frame / frame pairs: the matcher of
 * Tracking::trackReferenceKeyFrame (tracking.cpp:303), the last function of the reference's ORBmatcher.  Side 1 = the reference
 * key-frame: angle B x N1 float, desc B x N1 x 32, has_mp B x N1 uint8 (the feature holds a map point that is valid: `pMP &&
 * !pMP->not_valid_`), its DBoW2::FeatureVector as CSR like gl_search_for_triangulation's (nnode B; node_id B x NN1 ascending;
 * node_ptr B x (NN1 + 1); node_idx B x N1 in list order); side 2 = the current frame: angle, desc, feature vector.  nn_ratio /
 * check_orientation: the matcher's constructor arguments (tracking.cpp:300: 0.7, true).  Out: match21 B x N2 int32 - the
 * KEY-FRAME FEATURE whose map point the reference stores in matches[realIdxF], or -1 - and nmatches B.  Equal to the sequential
 * loop bit for bit (the first of equal best distances wins, a later equal one becomes second best). */
int gl_search_by_bow(gl_ctx_t* ctx, float nn_ratio, int check_orientation, int B, int N1, int N2, int NN1, int NN2,
                     const float* angle1_dev, const uint8_t* desc1_dev, const uint8_t* has_mp1_dev, const int32_t* nnode1_dev,
                     const int32_t* node_id1_dev, const int32_t* node_ptr1_dev, const int32_t* node_idx1_dev,
                     const float* angle2_dev, const uint8_t* desc2_dev, const int32_t* nnode2_dev, const int32_t* node_id2_dev,
                     const int32_t* node_ptr2_dev, const int32_t* node_idx2_dev, int32_t* match21_dev, int32_t* nmatches_dev);

/* ---- the DBoW2 vocabulary and ORBVocabulary::transform (orb_vocabulary.cpp:20-40): the PRODUCER of the feature vectors above -------
 * The reference converts a frame's descriptors and calls TemplatedVocabulary::transform(features, bow_vec, feat_vec, 4)
 * (orb_dbow2/include/orb_dbow2/dbow2/TemplatedVocabulary.h:1150-1218) for every key-frame (gmmloc_opt.cpp:25) and for a frame that
 * falls back to trackKeyFrame (tracking.cpp:298).  Only the FeatureVector is built here: bow_vec_ has no reader in gmmloc/.
 *
 * The tree.  Node 0 is the root; the other nodes have the ids 1, 2, ... of their records, a parent in [0, own id), a 32-byte
 * descriptor, a float weight and a leaf flag.  A node's children are ordered by id (loadFromBinaryFile pushes them in file order,
 * :1497-1517); word ids count the leaf-flagged records in id order (:1508-1513).
 *
 * Per feature (TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup), :1241-1283): start at the root; at each node
 * take the child with the smallest FORB::distance (256-bit Hamming), `d < best_d`, so the FIRST of equal children in child order
 * wins; stop at a node without children.  word_id / weight are that leaf's; nid is the node reached at level L - levelsup (level 1 =
 * the root's children), 0 when L - levelsup <= 0.  A feature enters the feature vector iff `weight > 0` (:1181, :1209): 0.0f,
 * -0.0f and NaN are stopped words.  FeatureVector is a std::map<NodeId, vector<unsigned>>: nodes ascending by id, the features of a
 * node ascending by index.
 *
 * DECLARED:
 *   - phantom node: `while (!f.eof())` (:1497) reads one record more than the file holds and appends a copy of the last node to that
 *     node's parent.  Its descriptor equals an earlier sibling's, so under the strict compare it never wins: the reader here takes
 *     exactly nb_nodes - 1 records and makes none.
 *   - rejected input (the reference indexes out of range or never terminates): size_node != 41, nb_nodes < 2, a parent outside
 *     [0, own id), a record flagged leaf that has a child, a record not flagged leaf without one, a file shorter or longer than its
 *     header says: GL_ERR_FORMAT from the file readers, GL_ERR_ARG from gl_voc_create (its arrays are arguments).
 *   - shallow leaf: a feature that reaches a leaf above level L - levelsup leaves *nid unwritten in the reference (:1275 never
 *     fires); here nid is that leaf's id.
 *   - levelsup < 0 is GL_ERR_ARG.
 *
 * File (loadFromBinaryFile, :1477-1522): uint32 nb_nodes (root included), uint32 size_node, int32 k, int32 L, int32 scoring, int32
 * weighting, then nb_nodes - 1 records of 41 bytes {int32 parent, 32 descriptor bytes, float weight, uint8 is_leaf}.
 *
 * gl_voc_file_read - host only, like gl_gmm_file_read: *n_nodes_out = nb_nodes, k_L_out[2] = {k, L} (NULL allowed); the records of
 *   the nodes 1 .. nb_nodes - 1 into parent (cap) int32, desc (cap x 32) uint8, weight (cap) float, is_leaf (cap) uint8, cap >=
 *   nb_nodes - 1; all four NULL: the counts alone.
 * gl_voc_create - the same arrays (n_nodes - 1 records, host pointers) and the same consistency checks; synchronous.  The nodes are
 *   laid out on the device so that the children of a node are contiguous and in child order.  k is informative; L sets the level
 *   of nid.  A gl_voc_t is immutable and may be used by every context of its device.
 * gl_voc_info - info[7] = {nodes (root included), words, k, L, largest child count, shallowest leaf level, device bytes}.
 *
 * gl_bow_transform - the transform for B frames of NF feature slots: feat_desc B x NF x 32 uint8; feat_oct B x NF int32, < 0 marks a
 *   padding slot (the matchers' convention), NULL: every slot is a feature.  Asynchronous on the context's stream, stateless, no host
 *   synchronise; the context's scratch is written before it is read.  B <= 65 535 (B = 0: nothing is done), 1 <= NF <= 4 096, 1 <= NNcap
 *   <= 4 096, 0 <= levelsup (the reference passes 4); feat_desc aligned to 16 bytes, as the matchers read it.  out:
 *     word_id, node B x NF int32, weight B x NF float - per feature, stopped words included; a padding slot gets -1 / -1 / 0; each
 *       may be NULL;
 *     nnode B, node_id B x NNcap ascending, node_ptr B x (NNcap + 1), node_idx B x NF - exactly the arrays of gl_search_by_bow,
 *       gl_search_for_triangulation, gl_track_chain_io.feat_node_* and a row of gl_map_kf_tables;
 *     status B int32: 0, or GL_BOW_NODES_TRUNCATED for a frame with more distinct nodes than NNcap: its true count goes into nnode,
 *       its node_id / node_ptr / node_idx stay untouched, its per-feature outputs are complete.
 *   Not written: node_id from nnode on, node_ptr from nnode + 1 on, node_idx from node_ptr[nnode] on.
 *   After an argument error nothing has been written. */
typedef struct gl_bow_out {
  int32_t* word_id;
  int32_t* node;
  float* weight;
  int32_t* nnode;
  int32_t* node_id;
  int32_t* node_ptr;
  int32_t* node_idx;
  int32_t* status;
} gl_bow_out;
#define GL_BOW_NODES_TRUNCATED 1
#define GL_BOW_MAX_FEATURES 4096
int gl_voc_file_read(const char* path, int32_t* parent, uint8_t* desc, float* weight, uint8_t* is_leaf, int cap, int* n_nodes_out,
                     int* k_L_out);
int gl_voc_create(gl_ctx_t* ctx, int n_nodes, const int32_t* parent, const uint8_t* desc, const float* weight, const uint8_t* is_leaf, int k,
                  int L, gl_voc_t** out);
int gl_voc_load_file(gl_ctx_t* ctx, const char* path, gl_voc_t** out);
int gl_voc_destroy(gl_voc_t* voc);
int gl_voc_info(const gl_voc_t* voc, double info[7]);
int gl_bow_transform(gl_ctx_t* ctx, const gl_voc_t* voc, int levelsup, int B, int NF, int NNcap, const uint8_t* feat_desc_dev,
                     const int32_t* feat_oct_dev, const gl_bow_out* out);
/* The matches of gl_search_for_triangulation as the per-match arrays of gl_create_map_points, without leaving the device:
 * what Localization::createMapPoints reads per matched pair (localization_opt.cpp:286-420) - the two key-frames' poses,
 * key-points, depths, octaves and candidate components (kf->comps_[idx]).  Inputs per pair and key-frame: pose B x 7, uv B x N x 2,
 * ur / depth B x N float, oct B x N, cand B x N x k int32 (+ ncand B x N).  Output: the matches of all pairs, pair after pair, inside
 * a pair in ascending feature index of key-frame 1 (= matched_pairs), compacted: pair_off_dev B + 1 int32 (exclusive scan of the
 * counts; [B] = total), m_* arrays of `cap` entries (entries beyond cap are dropped: size cap >= sum of nmatches, e.g. B x
 * min(N1, N2)), m_pair / m_idx1 / m_idx2: the pair and the two feature indices of every match. */
int gl_gather_triangulation_matches(gl_ctx_t* ctx, int B, int N1, int N2, int k, int cap, const int32_t* match12_dev,
                                    const int32_t* nmatches_dev, const double* pose1_dev, const double* uv1_dev, const float* ur1_dev,
                                    const float* depth1_dev, const int32_t* oct1_dev, const int32_t* cand1_dev, const int32_t* ncand1_dev,
                                    const double* pose2_dev, const double* uv2_dev, const float* ur2_dev, const float* depth2_dev,
                                    const int32_t* oct2_dev, const int32_t* cand2_dev, const int32_t* ncand2_dev, int32_t* pair_off_dev,
                                    double* m_pose1_dev, double* m_uvr1_dev, float* m_depth1_dev, int32_t* m_oct1_dev, int32_t* m_cand1_dev,
                                    int32_t* m_n1_dev, double* m_pose2_dev, double* m_uvr2_dev, float* m_depth2_dev, int32_t* m_oct2_dev,
                                    int32_t* m_cand2_dev, int32_t* m_n2_dev, int32_t* m_pair_dev, int32_t* m_idx1_dev, int32_t* m_idx2_dev);

/* ---- point refinement ----------------------------------------------------- */
/* GMMLoc::optimizePoint (gmmloc_opt.cpp:260-342), N independent problems.
 * pts N x 3, uvr N x 3 (u, v, u_right), octave N, pose N x 7, comp N, proj_z2 N.
 * out: res N uint8, chi2_proj N, chi2_str N, pt_est N x 3.  A problem without a component (comp < 0 or
 * >= K) or with an octave outside 0..7 is not solved: res = 0, chi2 = 0, pt_est = pts. */
int gl_optimize_point(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, const gl_params* prm, int N,
                      const double* pts_dev, const double* uvr_dev, const int32_t* octave_dev,
                      const double* pose_dev, const int32_t* comp_dev, const double* proj_z2_dev,
                      uint8_t* res_dev, double* chi2_proj_dev, double* chi2_str_dev, double* pt_est_dev);

/* GMMLoc::checkMapAssociation (gmmloc_opt.cpp:156-258) for the N features of B
 * key-frames: pose_dev B x 7; pts_dev B x N x 3 in/out (written where the reference
 * writes pt3d); uvr B x N x 3; octave B x N (<0 = skip feature); cand B x N x k,
 * ncand B x N (from gl_search2d); out_comp B x N (component or -1). */
int gl_check_map_association(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, const gl_params* prm,
                             int B, int N, const double* pose_dev, double* pts_dev, const double* uvr_dev,
                             const int32_t* octave_dev, const int32_t* cand_dev, const int32_t* ncand_dev, int k,
                             int32_t* out_comp_dev);

/* Localization::optimizeTriangulationVec (localization_opt.cpp:27-204), N problems.
 * x3d N x 3 in/out; pose1/pose2 N x 7; uvr1/uvr2 N x 3 (u_right < 0 => mono edge);
 * oct1/oct2 N; cand1/cand2 N x k with n1/n2 N; out_comp N (an octave outside 0..7: -1, x3d untouched). */
int gl_optimize_triangulation(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, const gl_params* prm,
                              int N, double* x3d_dev, const double* pose1_dev, const double* uvr1_dev,
                              const int32_t* oct1_dev, const double* pose2_dev, const double* uvr2_dev,
                              const int32_t* oct2_dev, const int32_t* cand1_dev, const int32_t* n1_dev,
                              const int32_t* cand2_dev, const int32_t* n2_dev, int k, int32_t* out_comp_dev);

/* Localization::createMapPoints, the per-match block (localization_opt.cpp:286-420), for
 * N epipolar matches: parallax test -> linear triangulation (smallest right singular vector of the 4 x 4
 * system, the reference's JacobiSVD) or stereo unprojection (frame.cpp:27-35) -> optimizeTriangulationVec
 * (= gl_optimize_triangulation, with u_right taken as -1 unless depth > 0, :116-137) -> project3 into both
 * key-frames, reprojection checks (both with kp1's sigma^2, :370-391) and scale consistency (:393-404).
 *  pose1 / pose2 N x 7 (getTcw of the two key-frames); uvr1 / uvr2 N x 3 (u, v, u_right; < 0 = monocular);
 *  depth1 / depth2 N float (Feature::depth, -1 = none); oct1 / oct2 N; candidate tables as in
 *  gl_optimize_triangulation; scale_factor = frame::scale_factor (1.2).
 *  out: x3d N x 3 (the point after the structure optimisation; zeros when no point was formed),
 *  type N int32: 0 = rejected, 1 FromTriMono, 2 FromTriMonoGMM, 3 FromTriStereo, 4 FromTriStereoGMM
 *  (MapPoint::type_, :407-419), comp N int32 (str_ptr as component index, -1 = none). */
int gl_create_map_points(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, const gl_params* prm, float scale_factor,
                         int N, const double* pose1_dev, const double* uvr1_dev, const float* depth1_dev,
                         const int32_t* oct1_dev, const double* pose2_dev, const double* uvr2_dev,
                         const float* depth2_dev, const int32_t* oct2_dev, const int32_t* cand1_dev,
                         const int32_t* n1_dev, const int32_t* cand2_dev, const int32_t* n2_dev, int k, double* x3d_dev,
                         int32_t* type_dev, int32_t* comp_dev);

/* ---- a key-frame's new map points, triangulated on the resident map ------------------------------------
 * Localization::createMapPoints (localization_opt.cpp:206-454) for ONE key-frame row: the loop over its best covisible neighbours
 * around gl_search_for_triangulation, the match gather and the per-match block of gl_create_map_points.  The loop is sequential:
 * searchForTriangulation skips a feature of key-frame 1 that holds a map point (orb_matcher.cpp:183-186), createMapPoints gives it one
 * (curr_kf_->addObservation(mappt, idx1), :433) before the next neighbour is searched, and the partner it would have taken goes to a
 * later query - so B pairs in one batch of gl_search_for_triangulation are not the reference's result for one key-frame's neighbours.
 *
 * gl_map_kf_tables - the per-key-frame tables the triangulation reads and no other view carries; caller-owned device arrays,
 * row-indexed like gl_map_ba_view (a new key-frame's rows are part of the one upload that stays, but for the feature vector's four
 * arrays, which gl_bow_transform writes in place from kf_desc's row):
 *   kf_angle NKF x NFK f32 (key-point angle, degrees), kf_desc NKF x NFK x 32 u8 (the table of gl_fuse_search / gl_update_map_points),
 *   kf_depth NKF x NFK f32 (Feature::depth, -1 = none); the DBoW2::FeatureVector as CSR like gl_search_for_triangulation's: kf_nnode
 *   NKF, kf_node_id NKF x NNcap ascending, kf_node_ptr NKF x (NNcap + 1), kf_node_idx NKF x NFK; the candidate tables of gl_search2d
 *   (kf->comps_): kf_cand NKF x NFK x k, kf_ncand NKF x NFK.
 *
 * gl_tri_pair_setup - what the loop computes per neighbour before it searches (:246-262, orb_matcher.cpp:146-161), for key-frame row
 * kf_row and the neighbours conn_kf[first_nb .. first_nb + n_nb) of a DEVICE list of conn_cap entries with DEVICE length n_conn (the
 * outputs of gl_update_connections; getBestCovisibilityKeyFrames(nn) is its first nn entries), n_nb <= GL_TRI_NB_MAX:
 *   skip n_nb int32, bits: GL_TRI_SKIP_BEYOND the entry is at or behind min(n_conn, conn_cap); _BAD_ROW its row is outside [0, NKF);
 *     _SELF row == kf_row; _INVALID kf_valid[row] == 0 (DECLARED: skipped - the reference's list holds no bad key-frame); _REPEATED the
 *     row is listed earlier in the range (DECLARED: skipped, gl_map_add's rule for a repeated row); _BASELINE `baseline < kf2->mb`
 *     exactly as :254-262: the double difference of kf_twc, its double norm sqrt((dx dx + dy dy) + dz dz), narrowed to float, float
 *     compare against the float mb (a baseline EQUAL to mb is searched).  BEYOND and BAD_ROW stand alone; the others combine.
 *   fmat n_nb x 9 f64 row-major = MathUtils::computeFundamentalMatrix(Tcw1, K, Tcw2, K) (math_utils.cpp:16-43), in this order - q
 *     = (x y z w) as stored in kf_pose, not renormalised, (fx fy cx cy) the camera's FLOAT scalars widened:
 *       R1 = q1.toRotationMatrix(), R2 likewise   (Eigen's: tx = 2 x ... R00 = 1 - (tyy + tzz), R01 = txy - twz, ...)
 *       R = R1 R2^T:  Rij = (R1i0 R2j0 + R1i1 R2j1) + R1i2 R2j2        rot_c1_w * rot_c2_w.conjugate(), as matrices: the products of two
 *                                                                      rotation matrices agree with a host's Eigen / numpy chain to
 *                                                                      the rounding of the chain, a quaternion product does not
 *       r = R t2:     ri = (Ri0 t2x + Ri1 t2y) + Ri2 t2z;   t12 = -r + t1
 *       E = skew(t12) R without the zero products: E0j = (-tz) R1j + ty R2j, E1j = tz R0j + (-tx) R2j, E2j = (-ty) R0j + tx R1j
 *       ifx = 1 / fx, ify = 1 / fy, mcx = -(cx / fx), mcy = -(cy / fy)          (K^-1 in closed form)
 *       G = E K^-1:  Gi0 = Ei0 ifx, Gi1 = Ei1 ify, Gi2 = (Ei0 mcx + Ei1 mcy) + Ei2
 *       F = K^-T G:  F0j = ifx G0j, F1j = ify G1j, F2j = (mcx G0j + mcy G1j) + G2j
 *   epipole n_nb x 2 f32 (orb_matcher.cpp:156-161): C2 = q2 * t1 + t2 - Tcw1.translation(), not key-frame 1's centre: kept;
 *     invz = 1.0f / (float)C2z; ex = (float)((fx C2x) (double)invz + cx), ey = (float)((fy C2y) (double)invz + cy).
 *   A skipped neighbour (any bit) has fmat = 0 and epipole = 0.  The file is compiled without contraction and uses + - x / only (one
 *   sqrt in the baseline), so the same statements in numpy give the same bits.
 *
 * gl_create_map_points_from_map - the whole loop for one key-frame and the neighbour range [first_nb, first_nb + n_nb), on the map of
 * gl_update_connections (map: kf_valid, kf_mp; ba: kf_pose, kf_twc, kf_uvr, kf_oct) and the tables above.  THE MAP IS NOT WRITTEN:
 * the outputs are gl_map_add's lists.  Asynchronous on the context's stream, stateless, no host synchronise; the context's scratch
 * is written before it is read.  Enqueued, 2 + 6 n_nb launches whatever the device counts are:
 *   1  the pair set-up                                                                  (k_tri_pair_setup)
 *   2  the neighbours' rows gathered into dense pair tables; has_mp2[i] = kf_mp[kf2][i] != -1; a skipped neighbour gets nnode = 0, so
 *      its search has no query and the stages behind it no match; the mask has_mp1[i] = kf_mp[kf_row][i] != -1 - the POINTER test of
 *      getMapPoint(idx1), whatever mp_valid says of the row; feat_new = -1, n_new = n_attach = 0                        (k_tri_rows)
 *   per neighbour, in list order:
 *   3  gl_search_for_triangulation's kernel, B = 1, bOnlyStereo = false, no orientation check (ORBmatcher(0.6, false), :218, :266)
 *   4  the matches in ascending idx1 (= matched_pairs) as the per-match arrays                                    (k_tri_match_rows)
 *   5-7 the per-match block: the three kernels of gl_create_map_points over NFK slots (the slots behind the matches form no point)
 *   8  accept (k_tri_accept): every match with type > 0, in that order, is appended at the running count n_new: new_pos x 3,
 *      new_assoc (= comp; -1 exactly for types 1 and 3), new_ref_kf = kf_row, new_type 1..4, new_nb = its index in the list
 *      (first_nb + j), new_feat1 / new_feat2, and the two triples (mp_base + r, kf_row, idx1), (mp_base + r, kf2, idx2) in that order
 *      (:430-434) at att_*[2 r], [2 r + 1]; has_mp1[idx1] = 1, feat_new[idx1] = mp_base + r.  A rejected match (type 0: `continue`,
 *      :346-404) leaves the mask alone: its feature asks again at the next neighbour.
 * out: the lists (new_* new_cap entries, att_* 2 new_cap) with n_new / n_attach as device counts - gl_map_add's new_* / att_* lists
 * and counts as they stand; feat_new NFK (-1: no new point); nb_stats n_nb x 8 int32 = {row (-1 beyond the list), skip bits, nmatches,
 * created, rejected by type 0, 0, 0, 0}; fmat n_nb x 9 / epipole n_nb x 2 (NULL allowed); status int32: GL_TRI_NONE_SEARCHED when
 * every neighbour of the range was skipped.  Entries of the lists from n_new (2 n_new) on are not written.
 * new_cap < NFK is GL_ERR_ARG: a feature of key-frame 1 gains at most one point, so NFK rows never truncate.  NFK <= 4 096, NNcap
 * and k in 1..8 as in gl_search_for_triangulation / gl_create_map_points, cam width / height set; n_nb > GL_TRI_NB_MAX is GL_ERR_ARG.
 * After an argument error nothing has been written.
 * The reference's `if (i > 0 && checkNewKeyFrames()) return` (:243) is the range: a host that must test between neighbours calls with
 * n_nb = 1, applies gl_map_add (the mask is then read from the map it changed, mp_base is the new NMP) and calls again - the same
 * kernels, the same result.  What stays with the host: computeDistinctiveDescriptors / updateNormalAndDepth of the new rows is
 * gl_update_map_points after gl_map_add; candidate_mappts_ and type_ from new_type. */
#define GL_TRI_NB_MAX 16
#define GL_TRI_SKIP_BEYOND 1
#define GL_TRI_SKIP_BAD_ROW 2
#define GL_TRI_SKIP_SELF 4
#define GL_TRI_SKIP_INVALID 8
#define GL_TRI_SKIP_REPEATED 16
#define GL_TRI_SKIP_BASELINE 32
#define GL_TRI_NONE_SEARCHED 1
typedef struct gl_map_kf_tables {
  const float* kf_angle;
  const uint8_t* kf_desc;
  const float* kf_depth;
  const int32_t* kf_nnode;
  const int32_t* kf_node_id;
  const int32_t* kf_node_ptr;
  const int32_t* kf_node_idx;
  const int32_t* kf_cand;
  const int32_t* kf_ncand;
  int32_t NNcap, k;
} gl_map_kf_tables;
typedef struct gl_tri_points_out {
  double* new_pos;
  int32_t* new_assoc;
  int32_t* new_ref_kf;
  int32_t* new_type;
  int32_t* new_nb;
  int32_t* new_feat1;
  int32_t* new_feat2;
  int32_t* att_mp;
  int32_t* att_kf;
  int32_t* att_feat;
  int32_t* n_new;
  int32_t* n_attach;
  int32_t* feat_new;
  int32_t* nb_stats;
  double* fmat;
  float* epipole;
  int32_t* status;
  int32_t new_cap, reserved_;
} gl_tri_points_out;
int gl_tri_pair_setup(gl_ctx_t* ctx, const gl_camera* cam, int NKF, const uint8_t* kf_valid_dev, const double* kf_pose_dev,
                      const double* kf_twc_dev, int kf_row, const int32_t* conn_kf_dev, const int32_t* n_conn_dev, int conn_cap, int first_nb,
                      int n_nb, float mb, int32_t* skip_dev, double* fmat_dev, float* epipole_dev);
int gl_create_map_points_from_map(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, const gl_params* prm, float scale_factor,
                                  const gl_map_view* map, const gl_map_ba_view* ba, const gl_map_kf_tables* kt, int kf_row,
                                  const int32_t* conn_kf_dev, const int32_t* n_conn_dev, int conn_cap, int first_nb, int n_nb, float mb,
                                  int mp_base, const gl_tri_points_out* out);

/* ---- points from stereo depth: the two depth-ordered walks ------------------ */
/* GMMLoc::createMapPointsFromStereo (gmmloc_opt.cpp:36-113) for B key-frames of NF feature slots (B = 1 live, B > 1 replay), between
 * gl_search2d (whose table stays on the device) and gl_map_add (whose lists and device counts it writes).  Device pointers,
 * asynchronous on the context's stream, no host synchronise; the context's scratch is written before it is read.
 *  in:  pose B x 7 (getTcw); feat_uv B x NF x 2; feat_ur / feat_depth B x NF float; feat_oct B x NF (outside 0..7: a padding slot);
 *       cand B x NF x k, ncand B x NF (gl_search2d; k in 1..8); held B x NF uint8: 0 = mappoints_[i] is null, 1 = a point with
 *       countObservations() >= 1, 2 = a point without observation (a temporal one); kf_row B: the key-frame's row of the map.
 *       mp_base: the map's NMP.  check_depth: !is_first (:30).  th_depth: frame::th_depth, compared as float.
 *  The walk, statement for statement:
 *   entries (:39-44)   the slots with depth > 0 as a float compare (NaN, +-0, negative: out; +inf: in), never a padding slot;
 *   order (:49)        ascending (depth, index), the order of std::sort on the pairs;
 *   create_new (:55-63) held != 1; a held == 2 slot is set to null first;
 *   the point (:72)    Frame::unproject3: z (u - cx) / fx with z the float depth widened, then Twc.map;
 *   the check (:75-80) ncand > 0: checkMapAssociation on that point; a null answer is a `continue` - the entry is neither counted nor
 *                      tested for the break; otherwise a point is created (FromDepthGMM with the component, FromDepth for ncand == 0)
 *                      and counted; a held == 1 entry is counted;
 *   the break (:109)   after a counted entry: check_depth && depth > th_depth && num_points > 100, both strict; the entry that
 *                      breaks has been processed; nothing behind it is touched (a held == 2 slot there keeps its point).
 *  out: pts0 B x NF x 3 or NULL: the unprojected point of every entry (zeros elsewhere);
 *       the new points of key-frame b in WALK order at [b x NF, b x NF + n_new[b]): new_feat, new_pos x 3 (the point as the check left
 *       it), new_assoc (component or -1; FromDepthGMM exactly where >= 0), new_ref_kf = kf_row[b]; the attach triples att_mp = mp_base +
 *       r, att_kf = kf_row[b], att_feat; entries from n_new[b] on are not written;  n_new B;
 *       feat_new B x NF: r for the slot that now holds new point r, -1 untouched, -2 set to null and left so (held 2, walked, rejected);
 *       stats B x 8: {entries, walked, n_new, n_rejected, num_points, broke, 0, 0}.
 *  For B = 1 new_pos / new_assoc / new_ref_kf / n_new and att_* / n_new are gl_map_add's lists and device counts as they stand.
 *  More than GL_STEREO_WALK_MAX slots per key-frame: GL_ERR_ARG, nothing is written. */
#define GL_STEREO_WALK_MAX 4096
typedef struct gl_stereo_points_in {
  const double* pose;
  const double* feat_uv;
  const float* feat_ur;
  const float* feat_depth;
  const int32_t* feat_oct;
  const int32_t* cand;
  const int32_t* ncand;
  const uint8_t* held;
  const int32_t* kf_row;
} gl_stereo_points_in;
typedef struct gl_stereo_points_out {
  double* pts0;
  int32_t* new_feat;
  double* new_pos;
  int32_t* new_assoc;
  int32_t* new_ref_kf;
  int32_t* att_mp;
  int32_t* att_kf;
  int32_t* att_feat;
  int32_t* n_new;
  int32_t* feat_new;
  int32_t* stats;
} gl_stereo_points_out;
int gl_create_stereo_points(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, const gl_params* prm, int B, int NF, int k,
                            const gl_stereo_points_in* in, int mp_base, int check_depth, float th_depth,
                            const gl_stereo_points_out* out);

/* Tracking::createTemporalPoints (tracking.cpp:411-465) for B last frames that are no key-frames (:414 is the caller's): the same
 * walk without a check - every entry is counted, the break is always armed (:462).
 *  in:  pose B x 7 (the last frame's Tcw), feat_uv, feat_depth, feat_oct (padding only), held as above, last_outlier B x NF uint8
 *       (the last frame's is_outlier_), feat_desc B x NF x 32.
 *  out: temp_flag B x NF uint8 (1 = the slot now holds a temporal point), n_temp B, and IN PLACE, for the created points only, the rows
 *       of gl_track_frame_chain's last-frame arrays: last_pt = the unprojected point, last_observed = 0, last_valid = !last_outlier
 *       (clearTemporalPoints leaves a null slot's is_outlier_ alone and orb_matcher.cpp:432 reads it), last_desc = feat_desc.  The rows
 *       of held == 1 slots and of slots that are not walked keep their bytes; a walked held == 2 slot is replaced (:453).
 *       stats B x 8 or NULL: {entries, walked, n_temp, 0, num_pts, broke, 0, 0}.
 *       last_mp B x NF int32 or NULL, IN PLACE: -1 for the created points - the slot's mappoints_[i] is the temporal point now (:453),
 *       which has no row; the other entries keep their bytes.  gl_track_frame_next's held_mp is passed here. */
typedef struct gl_temporal_points_in {
  const double* pose;
  const double* feat_uv;
  const float* feat_depth;
  const int32_t* feat_oct;
  const uint8_t* held;
  const uint8_t* last_outlier;
  const uint8_t* feat_desc;
} gl_temporal_points_in;
typedef struct gl_temporal_points_out {
  uint8_t* temp_flag;
  int32_t* n_temp;
  double* last_pt;
  uint8_t* last_observed;
  uint8_t* last_valid;
  uint8_t* last_desc;
  int32_t* stats;
  int32_t* last_mp;
} gl_temporal_points_out;
int gl_create_temporal_points(gl_ctx_t* ctx, const gl_camera* cam, int B, int NF, const gl_temporal_points_in* in, float th_depth,
                              const gl_temporal_points_out* out);

/* ---- stereo depth: Frame::computeStereoMatches (frame.cpp:179-349) for B frames ------------------- */
/* The two feature columns the calls above read - feat_ur (u_right) and feat_depth - made on the device from the left features, the right
 * key-points and the two image pyramids (GMMLoc::processFrame, gmmloc.cpp:259-261).  One workgroup per frame, asynchronous on the
 * context's stream, device pointers only, no scratch, nothing of the context but its stream.  Every decision is integer arithmetic or a
 * single IEEE binary32 operation (one rounding each, no contraction); the division of the parabola (:313-314) and mbf / disparity (:330)
 * are correctly rounded.  The sequential model is tests/stereo_ref.py, the hand-built cases tests/stereo_cases.py.
 *
 *  cam: fx, bf (mbf = (float)bf, mb = (float)(bf / fx), maxD = mbf / mb in float), height (the rows of the row table).  scale_factor:
 *  the level table of init_config.hpp:63-79 in float, scale_factors_inv[l] = 1.0f / scale_factors[l].
 *  in:  the left features as the chain holds them: feat_uv B x NF x 2 double, feat_oct B x NF, feat_desc B x NF x 32; the right
 *       key-points: r_uv B x NR x 2 FLOAT (kp.pt), r_oct B x NR, r_desc B x NR x 32; n_left / n_right B int32 or NULL (all NF / NR):
 *       slots at or beyond a frame's count are padding - they join nothing and their outputs are -1.
 *  left / right: the pyramids (gl_image_pyramid).  The level image is the ROI as in the reference: column 0 is the ROI's column 0 and
 *       `cols` of :286 is width[l].
 *  out: feat_ur, feat_depth B x NF float: u_right and depth, -1 / -1 for a feature without a match (and after the median rule's reset);
 *       match_r B x NF int32 or NULL: the right index pushed at :332 - also for a feature the median rule resets -, -1 otherwise;
 *       sad B x NF int32 or NULL: the best SAD of such a feature, -1 otherwise;
 *       stat B x 4 int32 or NULL: {features that pass :261, entries of vDistIdx, entries reset by :341-348, the median SAD or -1}.
 *
 *  The rules as the reference states them (the model cites each line): the row band minr = floor(kpY - r) .. maxr = ceil(kpY + r) with
 *  r = 2.0f * scale_factors[octave], in float; the left row is (size_t)(float)uv.y; candidates have levelL - 1 <= octave <= levelL + 1
 *  and minU <= uR <= maxU (minU = uL - maxD, maxU = uL; a feature with maxU < 0 is skipped); the winner is the FIRST strict minimum
 *  below 100 in ascending right index, and goes on iff its distance is below 75; scaleduL / scaledvL = round(double uv x (double)inv) in
 *  double, scaleduR0 = round(uR0 x inv) in FLOAT, round half away from zero; skipped iff scaleduR0 < 0 or scaleduR0 + 11 >= width[l];
 *  eleven 11 x 11 windows (incR = -5 .. 5), each with its own centre value subtracted, L1 distance in integers, first strict minimum,
 *  dropped at incR = -5 / +5; deltaR = (d1 - d3) / (2.0f * (d1 + d3 - 2.0f * d2)), dropped outside [-1, 1]; bestuR = sf[l] *
 *  ((float)scaleduR0 + (float)bestincR + deltaR); kept iff 0 <= uL - bestuR < maxD; a disparity of 0 becomes (float)0.01 with bestuR =
 *  (float)((double)uL - 0.01); depth = mbf / disparity.  The median rule: median = the SAD at position n / 2 of the ascending list,
 *  thDist = (1.5f * 1.4f) * (float)median, every entry with (float)sad >= thDist is reset to -1 / -1 - so a median of 0 resets ALL.
 *
 *  Deviations - each where the reference indexes out of range or throws:
 *   1. the rows of a right key-point outside [0, height) are dropped (the reference writes past vRowIndices);
 *   2. a left feature with (float)uv.y < 0 or (int)(float)uv.y outside [0, height) is skipped;
 *   3. a left feature or right key-point whose octave is outside [0, nlevels) takes no part;
 *   4. a feature any of whose twelve windows would leave its level image is skipped (cv::Mat::rowRange / colRange throw; :286 only tests
 *      scaleduR0 >= 0 although the first right window starts at scaleduR0 - 10);
 *   5. an empty vDistIdx changes nothing (the reference reads element 0 of an empty vector).
 *  ORB key-points keep 16 px of border at their level, so no extractor output meets 1 - 4.
 *
 *  NF or NR above GL_STEREO_MATCH_MAX, nlevels outside 1 .. 8, a level with width / height < 1 or stride < width, B < 1, cam height < 1,
 *  a NULL required pointer: GL_ERR_ARG, nothing is written. */
#define GL_STEREO_MATCH_MAX 4096
typedef struct gl_stereo_in {
  const double* feat_uv;
  const int32_t* feat_oct;
  const uint8_t* feat_desc;
  const float* r_uv;
  const int32_t* r_oct;
  const uint8_t* r_desc;
  const int32_t* n_left;
  const int32_t* n_right;
} gl_stereo_in;
/* B frames' pyramids in one byte buffer: pixel (x, y) of level l of frame b is data[b * frame_stride + offset[l] + y * stride[l] + x].
 * The stride lets a host upload mvImagePyramid's bordered buffers as they stand. */
typedef struct gl_image_pyramid {
  int32_t nlevels; /* 1 .. 8 */
  int32_t reserved_;
  int32_t width[8], height[8];
  int64_t stride[8]; /* bytes per row */
  int64_t offset[8]; /* bytes from a frame's base */
  int64_t frame_stride;
  const uint8_t* data;
} gl_image_pyramid;
typedef struct gl_stereo_out {
  float* feat_ur;
  float* feat_depth;
  int32_t* match_r;
  int32_t* sad;
  int32_t* stat;
} gl_stereo_out;
int gl_stereo_matches(gl_ctx_t* ctx, const gl_camera* cam, double scale_factor, int B, int NF, int NR, const gl_stereo_in* in,
                      const gl_image_pyramid* left, const gl_image_pyramid* right, const gl_stereo_out* out);

/* ---- ORB orientation and descriptors: the second half of ORBextractor (orb_extractor.cpp) for B images ------------------- */
/* IC_Angle (:77-101, :466-473), the 7 x 7 blur of every level (:1029-1030), the steered-BRIEF read (:104-147, :979-986) and the scaling
 * of the key-points (:1039-1046), from the key-points AT THEIR LEVEL and the image pyramid gl_stereo_matches reads.  B is the number of
 * pyramids in `pyr` (a stereo frame's two sides are B = 2 with one buffer, or two calls).  The pyramid, cv::FAST and the octree are
 * gl_orb_pyramid and gl_orb_detect below, whose outputs are this call's inputs.  Two kernels on the context's stream (k_orb_blur: the blurred pyramid into the context's main scratch block, same
 * geometry, tightly packed, every byte written before k_orb_describe reads it), device pointers only except blur_w (4 host ints).
 * The sequential model is tests/orb_ref.py, the hand-built cases tests/orb_cases.py.
 *
 *  in:  kp_xy B x N x 2 int32: the key-point at its level in ROI coordinates, pt + minBorder of :814-815 (cv::FAST gives integers, so
 *       cvRound of :80 / :109 is the identity); kp_oct B x N int32; n_kp B int32 or NULL (all N): slots at or beyond it are padding;
 *       kp_angle B x N float or NULL: when given the orientation is NOT computed, this angle (degrees) steers the descriptor and is
 *       copied to `angle`, and `moments` is 0 0; pattern 512 x 2 int8 (x, y) on the device: the host's own bit_pattern_31_ - the
 *       library ships none; blur_w: the symmetric 7-tap kernel in Q8, centre first (gl_orb_default_blur); scale_factor: the extractor's
 *       own table (:408-418), sf[0] = 1.0f, sf[i] = (float)((double)sf[i - 1] * scale_factor) - NOT the table of init_config.hpp:63-79
 *       (a float times (float)scale_factor), which gl_stereo_matches and the matchers use: for 1.2 the two differ from level 3 on, by one to five units in the last place.
 *  out: desc B x N x 32 uint8; angle B x N float or NULL; moments B x N x 2 int32 {m_10, m_01} or NULL; uv32 B x N x 2 float or NULL:
 *       kp.pt after :1045, (float)x * sf[oct], (float)y * sf[oct] - one float multiply, level 0 untouched; uv64 B x N x 2 double or
 *       NULL: the same values widened, as Feature stores them; stat B x 2 int32 or NULL: {described, skipped} among the first n_kp.
 *       A skipped or padding slot gets a zero descriptor, angle -1, moments 0 0 and uv -1 -1.
 *
 *  rule                   | reference        | stated as
 *  -----------------------+------------------+------------------------------------------------------------------------------------
 *  patch                  | :449-463         | rows v = -15 .. 15, columns |u| <= u_max[|v|], u_max = {15, 15, 15, 15, 14, 14, 14, 13, 13,
 *                         |                  | 12, 11, 10, 9, 8, 6, 3}: 749 pixels
 *  moments                | :78-98           | m_10 = sum u I(x + u, y + v), m_01 = sum v I(x + u, y + v) in int32 on the UNBLURRED level
 *  angle                  | :100             | fastAtan2((float)m_01, (float)m_10), DECLARED here since OpenCV's binary is not at hand: ax = |x|,
 *                         |                  | ay = |y|; c = min / (max + (float)DBL_EPSILON), c2 = c * c,
 *                         |                  | a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c with p_k = (float)c_k * (float)(180 / pi), c_1 =
 *                         |                  | 0.9997878412794807, c_3 = -0.3258083974640975, c_5 = 0.1555786518463281, c_7 = -0.04432655554792128;
 *                         |                  | a = 90 - a when ay > ax, then 180 - a when x < 0, then 360 - a when y < 0; float, one rounding
 *                         |                  | per operation, the division correctly rounded, no contraction; (0, 0) -> 0.  At most 0.0097
 *                         |                  | degrees from atan2 (0.009547 for the polynomial itself, at min = max, plus the float roundings
 *                         |                  | of values up to 360; a sample of 20 000 integer pairs gives 0.00954).  Parity of this polynomial with a host's OpenCV binary is UNPINNED
 *                         |                  |; the patch, `moments`, the argument order and everything from `steering` down are
 *                         |                  | held to the reference's own extractor code (oracle/orb_ref.cpp, tests/test_orb_ref_pin.py).
 *  blur                   | :1029-1030       | on the level's ROI alone (the reference clones the ROI: the bordered buffer's border is never
 *                         |                  | read), BORDER_REFLECT_101 by index (-1 -> 1, n -> n - 2); row pass r = sum_k w[|k|] I(x + k, y),
 *                         |                  | column pass s = sum_k w[|k|] r(x, y + k), both exact integer sums; the result is
 *                         |                  | min((s + 2^15) >> 16, 255) in 32-bit integers.  Which weights an OpenCV build uses is unpinned:
 *                         |                  | hence the argument.
 *  steering               | :103, :106-107   | angle_rad = angle * (float)(CV_PI / 180.f) in float.  The reference's `cos(angle)` / `sin(angle)` on
 *                         |                  | that float are, under its `using namespace std` (:69), the FLOAT overloads of <cmath>: libm's cosf /
 *                         |                  | sinf, whose last bit is that libm's choice (oracle/orb_ref.cpp asserts the overload).  The device's
 *                         |                  | rule is the CORRECTLY ROUNDED float cosine and sine, computed as a = (float)cos((double)angle_rad),
 *                         |                  | b = (float)sin((double)angle_rad): a stated deviation.  Measured against g++ 11.4 / glibc 2.35
 *                         |                  |: that libm's a or b is the neighbouring float at 2.59 % of the angles k x 1e-5
 *                         |                  | degrees (cos 1.30 %, sin 1.29 %), never further; on 27 300 key-points of random scenes no descriptor
 *                         |                  | bit changes with it.  A libm-specific result is no target, and the device's own cosf would be a third choice.
 *  sample (x, y)          | :112-114         | row cvRound(x * b + y * a), column cvRound(x * a - y * b) of the BLURRED level, relative to the
 *                         |                  | key-point: float products and sums, one rounding each, no contraction; cvRound rounds half to even
 *  bit j of byte i        | :116-143         | t0 < t1 for the samples 16 i + 2 j and 16 i + 2 j + 1
 *  scaling                | :1039-1046       | see uv32
 *
 *  Deviations - each where the reference would index out of range:
 *   1. a key-point whose octave is outside [0, nlevels) is skipped;
 *   2. a key-point nearer than 19 px to an edge of its level image (x < 19, x > width - 20, y < 19 or y > height - 20) is skipped: the
 *      patch needs 15 px, the pattern reaches cvRound(13 sqrt 2) = 18 px; the extractor's own key-points keep 19 px;
 *   3. a pattern entry outside [-13, 13]: GL_ERR_ARG.  The pattern lies on the device, so the call reads it back (1 KB, waits for the
 *      stream) when a context first sees the pointer and whenever the pointer changes - otherwise the call is asynchronous.  A host
 *      that rewrites the table in place is not checked again; the kernel clamps every entry to [-13, 13], so no read leaves the image.
 *
 *  blur_w: non-negative, w[0] + 2 (w[1] + w[2] + w[3]) in 1 .. 512, else GL_ERR_ARG.  N above GL_ORB_MAX, nlevels outside 1 .. 8, a
 *  level with width / height < 1, stride < width or a negative offset, B < 1, N < 1, a NULL required pointer: GL_ERR_ARG, nothing is
 *  written.  The host-side time this call saves (sixteen level blurs and 2 x 1 200 descriptors per stereo frame) is NOT measured. */
#define GL_ORB_MAX 4096
typedef struct gl_orb_in {
  const int32_t* kp_xy;
  const int32_t* kp_oct;
  const int32_t* n_kp;
  const float* kp_angle;
  const int8_t* pattern;
  const int32_t* blur_w; /* HOST memory: 4 ints */
  double scale_factor;
} gl_orb_in;
typedef struct gl_orb_out {
  uint8_t* desc;
  float* angle;
  int32_t* moments;
  float* uv32;
  double* uv64;
  int32_t* stat;
} gl_orb_out;
int gl_orb_describe(gl_ctx_t* ctx, int B, int N, const gl_orb_in* in, const gl_image_pyramid* pyr, const gl_orb_out* out);
/* w[0 .. 3] = the Q8 taps of the 7-tap Gaussian of that sigma, centre first - a DECLARED rule: g_i = exp(-i^2 / (2 sigma^2)) in double,
 * normalised over the seven taps, w[i] = nearbyint(256 g_i) for i = 1 .. 3 and the centre takes the remainder, w[0] = 256 - 2 (w[1] +
 * w[2] + w[3]).  sigma = 2 (:1030): the unrounded taps are 55.32 48.82 33.56 17.96, w = {54, 49, 34, 18}.  sigma <= 0 or not finite,
 * or a negative centre: GL_ERR_ARG. */
int gl_orb_default_blur(double sigma, int32_t* w);

/* ---- ORB detection: the first half of ORBextractor (orb_extractor.cpp) for B images ----------------------------------- */
/* ComputePyramid (:1056-1080) and ComputeKeyPointsOctTree without its last loop (:739-819: the cell FAST and DistributeOctTree), so
 * that a frame enters as its raw image: gl_orb_pyramid -> gl_orb_detect -> gl_orb_describe on one stream, the outputs of one the
 * inputs of the next, nothing read back (orb.extract, GMM::orbExtract).  Asynchronous on the context's stream, device pointers only.
 * Integer outputs of a sequential rule: a second run gives the same bytes.  The sequential model is tests/orb_detect_ref.py, the
 * hand-built cases tests/orb_detect_cases.py.  tests/test_orb_detect_ref_pin.py holds both to the reference's OWN ComputePyramid,
 * ComputeKeyPointsOctTree, DistributeOctTree, DivideNode and detect() (oracle/orb_detect_ref.cpp), tests/test_gpu_orb_detect_ref.py the
 * device: every row below from `features per level` to `final pick` and the level sizes are PINNED wherever the reference is determinate
 * (deviation 4).  The rows `resize`, `segment test`, `score`, `suppression` and cvRound's half-to-even stay DECLARED: they are
 * OpenCV's, which is not at hand, and the stand-in answers them with this project's own statement.
 *
 * gl_orb_pyramid_layout (host only) fills the geometry of a pyramid of `nlevels` levels of a width x height image: stride = width[l] +
 * row_pad, `lead` bytes in front of level 0, levels one behind the other, frame_stride their end; `data` is kept.
 * gl_orb_pyramid computes levels 1 .. n - 1 of every frame from level 0, which the caller has written into the same buffer; one
 * launch per level, a thread per pixel.  The 16 + 3 px border of :1072-1077 is NOT built: FAST on the reference's cells reads columns
 * 16 .. cols - 17 of a level, resize reads the ROI alone, and every reader here takes ROI coordinates.  GL_ERR_ARG, nothing written:
 * level sizes that are not the layout rule's for (width[0], height[0], scale_factor), levels or frames that overlap.
 *
 * gl_orb_detect: pyr as above; nfeatures, scale_factor, ini_th (20), min_th (7) the extractor's (:408-410); cand_cap: candidate slots
 * per image and level in the context's main scratch block (1 .. 65 535); N: the output capacity per image.
 *  out: kp_xy B x N x 2 int32: the key-point at its level in ROI coordinates, pt + minBorder of :814-815; kp_oct B x N int32; n_kp B -
 *       exactly gl_orb_describe's inputs; kp_response B x N float or NULL (the corner score); level_count B x 8 or NULL; stat B x 4 or
 *       NULL: {candidates, cells redone at min_th, key-points, overflow level mask}; cand_xy B x 8 x cand_cap x 2 int32, cand_resp
 *       B x 8 x cand_cap float, cand_count B x 8, each or NULL: the candidate lists (vToDistributeKeys, ROI coordinates) for tests,
 *       -1 -1 / 0 behind a level's count.  Slots at or beyond n_kp get xy -1 -1, octave -1, response 0.
 *       Order: level ascending, within a level the order of the reference's vResultKeys (the node list's order).
 *
 *  rule                   | reference        | stated as
 *  -----------------------+------------------+------------------------------------------------------------------------------------
 *  level scales           | :413-424         | sf[0] = 1.0f, sf[i] = (float)((double)sf[i - 1] * scale_factor), inv[l] = 1.0f / sf[l]
 *  level size             | :1058-1060       | cvRound((float)width * inv[l]) x cvRound((float)height * inv[l]), cvRound: half to even
 *  resize                 | :1069            | each level from the level before it; OpenCV's 8-bit INTER_LINEAR in fixed point, DECLARED here
 *                         |                  | since OpenCV's binary is not at hand: scale_x = 1.0 / ((double)dw / (double)sw); per destination
 *                         |                  | column fx = (float)((dx + 0.5) * scale_x - 0.5) (double, one rounding per operation), sx =
 *                         |                  | floor(fx), fx -= sx; sx < 0 gives (0, 0), sx >= sw - 1 gives (sw - 1, 0); a1 = cvRound(fx * 2048),
 *                         |                  | a0 = cvRound((1.f - fx) * 2048) in float, half to even; row pass r = a0 S[sx] + a1 S[min(sx + 1,
 *                         |                  | sw - 1)] in int32; the same in y gives b0, b1; the pixel is (((b0 * (r0 >> 4)) >> 16) + ((b1 *
 *                         |                  | (r1 >> 4)) >> 16) + 2) >> 2.  Parity of this rule with a host's OpenCV build is UNPINNED (DESIGN
 *                         |                  | section 2).
 *  features per level     | :429-441         | gl_orb_features_per_level: factor = (float)(1.0 / scale_factor); n = (float)nfeatures * (1 -
 *                         |                  | factor) / (1 - (float)pow((double)factor, (double)nlevels)) in float; level l < last takes
 *                         |                  | cvRound(n), then n *= factor; the last level max(nfeatures - sum, 0)
 *  cells                  | :743-778         | borders 16 and cols - 16 / rows - 16; width = cols - 32 as float, nCols = (int)(width / 30),
 *                         |                  | wCell = ceil(width / nCols) (<= 59), rows alike; cell (i, j): iniX = 16 + j wCell, maxX = iniX +
 *                         |                  | wCell + 6 clamped to cols - 16, skipped when iniX >= cols - 16 - 6 (rows: >= rows - 16 - 3)
 *  what FAST computes     | :782-783         | rows [3, rows - 3), columns [3, cols - 3) of the cell image: these regions tile the level
 *  segment test           | cv::FAST         | 9 contiguous of the 16 ring pixels of radius 3, all > v + th or all < v - th
 *  score                  | cv::FAST         | the largest t at which the pixel still passes: the maximum over the 16 arcs of the arc's
 *                         |                  | minimum of v - p (and of p - v), minus 1; it is the key-point's response
 *  suppression            | cv::FAST (true)  | kept iff the score is strictly greater than the 8 neighbours'; a neighbour that is no corner at
 *                         |                  | the current threshold, or outside the cell's region, counts 0
 *  fallback               | :785-788         | a cell without a key-point at ini_th is redone at min_th
 *  candidate order        | :763-797         | cells row-major, pixels row-major within a cell
 *  initial nodes          | :535-572         | nIni = round((float)(maxX - minX) / (maxY - minY)), hX = (float)(maxX - minX) / nIni, edges
 *                         |                  | (int)(hX * (float)i), assignment (int)(x / hX): float, one rounding per operation, the division
 *                         |                  | correctly rounded
 *  DivideNode             | :475-527         | halves ceil((float)(UR.x - UL.x) / 2), ceil((float)(BL.y - UL.y) / 2); x < UL.x + halfX, y < UL.y +
 *                         |                  | halfY; keys keep their order: a stable 4-way split; a child with one key is bNoMore
 *  phase-1 sweep          | :594-645         | children pushed to the FRONT, the parent erased: the reversed children, then the bNoMore nodes
 *  stop tests             | :649, :653, :710 | size >= N_l or size == prevSize; phase 2 when size + 3 nToExpand > N_l
 *  phase 2                | :655-712         | one node at a time, largest first, break at size >= N_l, repeated until a stop test holds
 *  final pick             | :720-734         | per node in list order: the key of maximum response, the first of equals
 *
 *  Deviations:
 *   1. a level with nCols < 1 or nRows < 1 (under 62 px) yields no key-points.  The reference's divisions there are FLOAT divisions
 *      (:760-761, width / nCols): they give infinity and trap nothing; converting ceil(inf) to int is undefined, and the value is not
 *      used: with nRows = 0 the row loop does not run, with nCols = 0 the column loop does not.  Run under g++ 11.4 -O2 on x86-64 the
 *      reference makes no FAST call and returns no key-point on 61 x 92, 92 x 61 and 61 x 61 (tests/test_orb_detect_ref_pin.py), which is
 *      what is stated here - a statement of the outcome, not of a defined behaviour;
 *   2. nIni < 1 (a level more than twice as tall as wide) yields no key-points.  The reference's hX = (float)(maxX - minX) / 0 is
 *      infinity and vpIniNodes is empty (:535-542): without a key it returns nothing, as here; its first key indexes element
 *      (int)(x / inf) = 0 of the empty vector (:559), out of range.  That case is never run against it;
 *   3. the initial node index is clamped to nIni - 1;
 *   4. phase 2 sorts (size, node POINTER) pairs (:664): equal sizes come out in address order, the allocator's choice - two runs of
 *      one binary on one input differ.  Declared instead: among equal sizes the node created last is divided first.  Against the
 *      reference's own DistributeOctTree (g++ 11.4, glibc 2.35) the declared order is one of the orders it can take
 *      and no more: on dense 256 x 224 scenes nearly every level has such a tie, and the declared answer was the host's on few of
 *      them.  Where no sort sees equal sizes the reference's answer is determinate and equals this rule's in order (pinned);
 *   5. a level with more than cand_cap candidates sets its bit in stat[3] and that image yields n_kp = 0: the reference's list is
 *      unbounded.
 *  A level's result can exceed N_l: the first sweep leaves up to 4 nIni nodes whatever N_l is; a later sweep runs only when size +
 *  3 nToExpand <= N_l, so it ends at or below N_l; phase 2 starts below N_l and a division adds at most 3.  Hence at most
 *  max(N_l + 2, 4 nIni_l) per level (gl_orb_detect_bound; 0 for a level of deviation 1 or 2).  N below the sum over the levels or
 *  above GL_ORB_MAX: GL_ERR_ARG.  Also GL_ERR_ARG, nothing written: thresholds outside 1 <= min_th <= ini_th <= 254, cand_cap outside
 *  1 .. 65 535, a level above 32 767 px or more than 1 024 times as wide as tall, B < 1, a NULL required pointer.
 *
 *  The octree's working set per (image, level) is 4 bytes per candidate slot (two uint16 permutations) and 72 bytes per node of
 *  max_l(bound_l) + 2: in LDS up to 56 KB, beyond that in the main scratch block.  The host time this saves is NOT measured. */
typedef struct gl_orb_detect_out {
  int32_t* kp_xy;
  int32_t* kp_oct;
  int32_t* n_kp;
  float* kp_response;
  int32_t* level_count;
  int32_t* stat;
  int32_t* cand_xy;
  float* cand_resp;
  int32_t* cand_count;
} gl_orb_detect_out;
int gl_orb_pyramid_layout(int width, int height, int nlevels, double scale_factor, int row_pad, int64_t lead, gl_image_pyramid* pyr);
int gl_orb_pyramid(gl_ctx_t* ctx, int B, const gl_image_pyramid* pyr, double scale_factor);
int gl_orb_features_per_level(int nfeatures, int nlevels, double scale_factor, int32_t* per_level);
int gl_orb_detect_bound(const gl_image_pyramid* pyr, int nfeatures, double scale_factor, int32_t* per_level);
int gl_orb_detect(gl_ctx_t* ctx, int B, int N, const gl_image_pyramid* pyr, int nfeatures, double scale_factor, int ini_th, int min_th, int cand_cap,
                  const gl_orb_detect_out* out);

/* ---- frame end and hand-over: from one tracked frame to the next on the device ------------------ */
/* What the reference does between two calls of gl_track_frame_chain_map - the tail of Tracking::track, GMMLoc::needNewKeyFrame,
 * Map::updateFrameInfo, the pose block of GMMLoc::processFrame, Tracking::updateLastFrame - as three calls on the chain's own outputs
 * and the resident map.  All three: one workgroup per frame (gl_map_note_replaced: one workgroup), asynchronous on the context's
 * stream, stateless, no scratch; the counts are integer reductions, so the bytes do not depend on scheduling; MALFORMED input is
 * skipped as in gl_update_local_map / gl_map_stats_track (a row outside its table holds nothing and counts nothing), nothing is read
 * or written out of bounds; NF is bounded as in the chain (3 072).
 *
 * gl_track_frame_end: tracking.cpp:85-116 and gmmloc.cpp:324-364 for B frames.  Device pointers, the arrays gl_track_frame_chain_map
 * left: feat_mp / match_last / match_local B x NF int32, match_kf B x NF (NULL without the fallback), outlier B x NF uint8, local_mp
 * B x NPcap, n_local_mp B, counts2 B x 4 (NULL: every frame tracked by the motion model), ref_kf B (of gl_local_map_io; read with a
 * rule only), last_observed B x NL uint8 (NULL = all observed), feat_depth B x NF float.  `map` + `ba`: the resident map (obs_ptr,
 * kf_mp, mp_valid; kf_uvr and obs_feat for the weights).
 *   what a feature holds after searchLocalPoints: the row r = local_mp[match_local[i]] when match_local[i] is in [0, min(n_local_mp,
 *       NPcap)), else feat_mp[i] (a point the chain un-held as invalid has left all three).  r outside [0, NMP): no row.  A feature
 *       without a row and with match_last[i] >= 0 whose last-frame slot has last_observed == 0 holds a TEMPORAL point: no row,
 *       countObservations() == 0.  countObservations() of a row is the WEIGHTED COUNT of gl_cull_keyframes; every `> 0` / `< 1` test
 *       below reads it as "the CSR range of the row is not empty" (an observation weighs at least 1).
 *   trackLocalMap (:279-292)       a held point with outlier[i] becomes null, is_outlier_ keeps its value; num_match_inliers = the
 *                                  held non-outlier features whose point has observations.
 *   the statistics (:88-102)       taken after that: num_total = the features with depth > 0 && depth < th_depth as float compares (NaN,
 *                                  +-0: out); num_map = those of them that still hold a point with observations; ratio_map =
 *                                  (float)num_map / (float)max(1, num_total), one IEEE division.
 *   clearTemporalPoints (:379-388) a held point without observations becomes null - a temporal point, and a row whose CSR range is
 *   and :107-111                   empty.  Its `is_outlier_ = false` can only meet a slot that is false already (the outlier ones
 *                                  were nulled by trackLocalMap), and :107-111 finds no held outlier any more: the frame's final
 *                                  is_outlier_ IS the chain's `outlier`, byte for byte.  No array is written for it;
 *                                  gl_create_temporal_points takes `outlier` as last_outlier.
 *   Hence a temporal point leaves no trace in any output: held or not, its slot ends null, uncounted, with the flag the chain gave
 *   it.  match_last, match_kf, last_observed and NL are part of the call for that statement (tests/frame_step_ref.py carries the
 *   temporal points and is_outlier_ through every statement); the kernel has no use for them, and all three pointers may be NULL.
 *   a lost frame (counts2[3] == 2, :65-71)  stat = {0, 10, 0, 0, 0, 0, 0, 0} and NO other output of that frame is written (the
 *                                  reference returns before last_frame_ advances: the rows of frame t - 1 stay the last frame's).
 *   QUIRK, reproduced: after a successful trackKeyFrame (counts2[3] == 1) stat_.res is still false - :55 cleared it, nothing sets it
 *   again.  res = (mode == 0).  A host that goes on after the fallback decides on counts2[3], not on res.
 *   needNewKeyFrame (with `rule` only; without: num_ref_matches = verdict = 0), gmmloc.cpp:327-361 in the reference's types:
 *       num_ref_matches = KeyFrame::countMapPoints(num_kfs <= 2 ? 2 : 3) of key-frame row ref_kf[b] (keyframe.cpp:212-231): the slots
 *                         of kf_mp[ref_kf] that hold a row of [0, NMP) which is valid in mp_valid and whose weighted count reaches
 *                         the threshold; a ref_kf outside [0, NKF): 0
 *       c1a = (float)frame_idx >= (float)kf_frame_idx + fps
 *       c1b = (float)num_match_inliers < (float)num_ref_matches * 0.25f || ratio_map < 0.3f
 *       c2  = ((float)num_match_inliers < (float)num_ref_matches * (num_kfs < 2 ? 0.4f : 0.75f) ||
 *              ratio_map < (num_match_inliers > 300 ? 0.2f : 0.35f)) && num_match_inliers > 15
 *       (c1a || c1b || is_idle) && c2 (:349): idle -> GL_KF_NEED; else GL_KF_INTERRUPT_BA (interruptBA() would have been called), and
 *       GL_KF_NEED with it when n_queue < 3 (:357).
 *  out: held_mp B x NF int32 - the final mappoints_ as map rows, -1 none: the next frame's last_mp, and a new key-frame's kf_mp row
 *       as KeyFrame(*frame) copies it; held B x NF uint8 - 0 / 1, the flags of gl_create_stereo_points (no held point is temporal
 *       any more); stat B x 8 int32 = {res, num_match_inliers, num_map, num_total, num_ref_matches, verdict, 0, 0}; ratio_map B float. */
#define GL_KF_NEED 1
#define GL_KF_INTERRUPT_BA 2
typedef struct gl_frame_end_in {
  const int32_t* feat_mp;
  const int32_t* match_last;
  const int32_t* match_local;
  const int32_t* match_kf;
  const uint8_t* outlier;
  const int32_t* local_mp;
  const int32_t* n_local_mp;
  const int32_t* counts2;
  const int32_t* ref_kf;
  const uint8_t* last_observed;
  const float* feat_depth;
} gl_frame_end_in;
typedef struct gl_kf_rule { /* host scalars, valid for the whole call */
  int32_t num_kfs;      /* map_->countKeyFrames() */
  int32_t frame_idx;    /* curr_frame_->idx_ */
  int32_t kf_frame_idx; /* curr_keyframe_->frame_idx_ */
  float fps;            /* camera::fps */
  int32_t is_idle;      /* localizer_->is_idle_ */
  int32_t n_queue;      /* localizer_->countKFsInQueue() */
} gl_kf_rule;
typedef struct gl_frame_end_out {
  int32_t* held_mp;
  uint8_t* held;
  int32_t* stat;
  float* ratio_map;
} gl_frame_end_out;
int gl_track_frame_end(gl_ctx_t* ctx, const gl_map_view* map, const gl_map_ba_view* ba, int B, int NF, int NL, int NPcap,
                       const gl_frame_end_in* in, float th_depth, const gl_kf_rule* rule, const gl_frame_end_out* out);

/* MapPoint::ptr_replaced_ as a device array: mp_replaced NMPcap int32, caller-owned, -1 = none.  repl_src / repl_tgt of gl_map_fuse,
 * n steps (or *n_dev clamped to [0, n], as in gl_map_stats_merge): mp_replaced[src] = tgt with the result of the sequential loop IN
 * STEP ORDER (map.cpp:126: a later step on the same src wins).  A step with src == tgt (:113) or with a row outside [0, NMPcap)
 * changes nothing.  Enqueued beside gl_map_stats_merge.  One workgroup; per 1 024 steps a step stores unless a later one of the
 * chunk names the same source. */
int gl_map_note_replaced(gl_ctx_t* ctx, int NMPcap, int32_t* mp_replaced_dev, const int32_t* repl_src_dev, const int32_t* repl_tgt_dev, int n,
                         const int32_t* n_dev);

/* gl_track_frame_next: Map::updateFrameInfo (map.cpp:23-38), the pose block of GMMLoc::processFrame (gmmloc.cpp:269-292),
 * Tracking::updateLastFrame (tracking.cpp:397-408) and the last-frame rows of frame t + 1, for B frames.  Called after the key-frame
 * pass, if one ran, and before the next chain call: it reads the map as it is NOW (positions after the BA, validity and observations
 * after the culls).
 *  in:  pose_tracked B x 7 (frame t's Tcw out of the chain); pose_prev B x 7 (the previous frame's pose as THIS call refreshed it one
 *       frame earlier - its pose_lw; NULL: no frame before, the data->idx == 1 branch); ref_kf B (the frame's ref_keyframe_ row NOW:
 *       the new key-frame's row after processKeyFrame, gmmloc_opt.cpp:27); held_mp B x NF in/out; feat_new B x NF + mp_base (of
 *       gl_create_stereo_points; NULL: no key-frame was made); mp_replaced NMPcap int32 (NULL: nothing was replaced), NMPcap >= NMP;
 *       of `map` mp_pos, obs_ptr, and of `ba` kf_pose.
 *  poses (SE3Quat with the normalisation every product does):
 *       t_rc = Tcw(ref_kf) * inverse(pose_tracked), t_cr = inverse(t_rc)               (map.cpp:29, :33)
 *       pose_lw = t_cr * Tcw(ref_kf)                                                   (gmmloc.cpp:275)
 *       pose_cw = pose_lw without pose_prev, else (pose_lw * inverse(pose_prev)) * pose_lw   (:284-290)
 *       A ref_kf outside [0, NKF) leaves the four poses unwritten: status GL_FRAME_NEXT_BAD_REF.
 *  rows, in this order:
 *       held_mp[i] = mp_base + feat_new[i] where feat_new[i] >= 0 (the key-frame's new points, gmmloc_opt.cpp:100; a sum outside
 *       [0, NMP) changes nothing), -1 where it is -2;
 *       then ONE step of mp_replaced (tracking.cpp:402-405: no chain is followed, and the row it names may itself be invalid); an
 *       entry outside [0, NMP) changes nothing.
 *  then per slot, row = held_mp[i] (outside [0, NMP): none, the entry keeps its value):
 *       last_pt = mp_pos[row], zeros without a row; last_valid = a row; last_observed = its CSR range is not empty;
 *       held (of gl_create_temporal_points) = 0 none, 1 observed, 2 a row without observations: a row culled since the frame's end, or
 *       the row one step of mp_replaced led to when that row was itself replaced or culled (A -> B -> C gives B, which is invalid).
 *       createTemporalPoints replaces such a slot (:441, :453): held_mp goes to gl_create_temporal_points as out->last_mp, which sets
 *       the replaced slots to -1, so that the next chain call sees a temporal point there and not a row that holds nothing (a frame
 *       that became a key-frame makes no temporal points and keeps its rows).
 *  last_oct / last_angle of frame t + 1 are frame t's own feature buffers: no copy is made, the caller passes them on.  So is
 *  last_desc for a host that matches against the features' descriptors (out->last_desc NULL: nothing is copied).  The reference
 *  matches a last-frame slot by its MAP POINT's descriptor (gl_search_by_projection_frame): with out->last_desc B x NF x 32 given, the
 *  slots with a row get mp_desc[row] (map->mp_desc required), the others keep their bytes - gl_create_temporal_points writes the
 *  temporal ones.
 *  out: t_rc, t_cr, pose_lw, pose_cw B x 7; held_mp; last_pt B x NF x 3; last_valid, last_observed, held B x NF uint8; status B. */
#define GL_FRAME_NEXT_BAD_REF 1
typedef struct gl_frame_next_in {
  const double* pose_tracked;
  const double* pose_prev;
  const int32_t* ref_kf;
  const int32_t* feat_new;
  const int32_t* mp_replaced;
  int32_t mp_base;
  int32_t NMPcap;
} gl_frame_next_in;
typedef struct gl_frame_next_out {
  double* t_rc;
  double* t_cr;
  double* pose_lw;
  double* pose_cw;
  int32_t* held_mp;
  double* last_pt;
  uint8_t* last_valid;
  uint8_t* last_observed;
  uint8_t* held;
  int32_t* status;
  uint8_t* last_desc; /* NULL allowed */
} gl_frame_next_out;
int gl_track_frame_next(gl_ctx_t* ctx, const gl_map_view* map, const gl_map_ba_view* ba, int B, int NF, const gl_frame_next_in* in,
                        const gl_frame_next_out* out);

/* ---- pose refinement ------------------------------------------------------ */
/* Tracking::optimizeCurrentPose (tracking_opt.cpp:21-217) for B frames.
 *  pose_dev B x 7 in/out; Xw_dev B x M x 3; obs_dev B x M x 3 (u, v, u_right; u_right < 0
 *  => monocular edge); octave_dev B x M int32 (< 0 => feature has no map point);
 *  outlier_dev B x M uint8 (is_outlier_), in/out: rewritten for the features with a map point, left untouched
 *  for the others (the reference resets is_outlier_[i] only where mappoints_[i] exists, :63-69);
 *  ninlier_dev B int32 (return value). */
int gl_optimize_current_pose(gl_ctx_t* ctx, const gl_camera* cam, const gl_params* prm, int B, int M,
                             double* pose_dev, const double* Xw_dev, const double* obs_dev,
                             const int32_t* octave_dev, uint8_t* outlier_dev, int32_t* ninlier_dev);

/* Localization::jointOptimization (localization_opt.cpp:456-925) on B flat problems
 * sharing one shape.  Per problem: P free poses (local key-frames, [0,P)), F fixed
 * poses ([P,P+F)), L points (all marginalised) each with <= 1 GMM association, and
 * observations in CSR order by point.
 *  poses_dev   B x (P+F) x 7   in/out for [0,P)
 *  prior_dev   B x P uint8     1 = key-frame idx_ 0 (prior edge / fixed, :556-581)
 *  points_dev  B x L x 3       in/out
 *  assoc_dev   B x L int32     component or -1
 *  obs_ptr_dev B x (L+1) int32; obs_pose_dev B x NOBS int32; obs_uvr_dev B x NOBS x 3;
 *  obs_oct_dev B x NOBS int32  (NOBS = stride; only obs_ptr[L] entries are used)
 *  out: assoc_dropped_dev B x L uint8 (:837-853), obs_erase_dev B x NOBS uint8 (:855-879),
 *       iters_dev B int32 (actual_iter of the last optimize(40), :827-828). */
int gl_joint_optimization(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, const gl_params* prm, int B,
                          int P, int F, int L, int NOBS, double* poses_dev, const uint8_t* prior_dev,
                          double* points_dev, const int32_t* assoc_dev, const int32_t* obs_ptr_dev,
                          const int32_t* obs_pose_dev, const double* obs_uvr_dev, const int32_t* obs_oct_dev,
                          uint8_t* assoc_dropped_dev, uint8_t* obs_erase_dev, int32_t* iters_dev);

/* The same with the reference's stop word (`pbStopFlag`, Localization::jointOptimization's abort: localization_opt.cpp:541-542
 * setForceStopFlag, :765-767, :792-796).  stop_flag: one int32 in device or host-mapped memory (gl_malloc / gl_malloc_host),
 * read with system scope once per Levenberg trial and acted on where g2o tests terminate() - before an outer iteration:
 *   > 0 on entry      the call returns at once, nothing is written (the reference's `return` at :765-767; iters = 0);
 *   > 0 later         the running outer iteration finishes, no further one starts; the reprojection gating and optimize(40)
 *                     are skipped (bDoMore = false), outputs are those of the last accepted step;
 *   < 0               a BUDGET of -value outer iterations in total (deterministic; what the parity tests use);
 *   0 / NULL          gl_joint_optimization. */
int gl_joint_optimization_stoppable(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, const gl_params* prm, int B,
                                    int P, int F, int L, int NOBS, double* poses_dev, const uint8_t* prior_dev,
                                    double* points_dev, const int32_t* assoc_dev, const int32_t* obs_ptr_dev,
                                    const int32_t* obs_pose_dev, const double* obs_uvr_dev, const int32_t* obs_oct_dev,
                                    uint8_t* assoc_dropped_dev, uint8_t* obs_erase_dev, int32_t* iters_dev,
                                    const int32_t* stop_flag);

/* North-star per-frame path: associate + structure-constrained pose refinement for B
 * frames of M map points each:
 *   1. idx = argmin_k chi2_k(Xw)  (GL_ASSOC_BRUTE), association kept iff chi2 <= 9
 *      (the gate of checkMapAssociation, gmmloc_opt.cpp:230-232);
 *   2. jointOptimization restricted to the frame: 1 free pose, M free marginalised points,
 *      one reprojection edge per point (mono / stereo, Huber) + its GMM edge
 *      (EdgePt2GaussianDeg x ba_lambda2 or EdgePt2Gaussian), schedule 5 / 5 / 40.
 *  pose_dev B x 7 in/out; Xw_dev B x M x 3 in/out; obs_dev B x M x 3; octave_dev B x M
 *  (<0 = no point); assoc_dev B x M int32 out (association after the final gate, -1 = none);
 *  d2_dev B x M double out (chi2 of the argmin at the INPUT point, may be NULL). */
int gl_track_frames(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, const gl_params* prm, int B, int M,
                    double* pose_dev, double* Xw_dev, const double* obs_dev, const int32_t* octave_dev,
                    int32_t* assoc_dev, double* d2_dev);
/* The same with a gauge anchor.  The reference never runs its structure BA without one: the other observers of the
 * local map points enter as FIXED key-frames (localization_opt.cpp:491-516) and key-frame 0 carries an EdgeSE3QuatPrior
 * (factors.cpp:19-53; measurement = its pose on entry, sigma_rot 2 deg, sigma_t 1 cm) or is fixed itself when
 * !ba_first_as_prior (:556-581).  Per frame:
 *   prior_dev       B uint8 or NULL; 1 = the frame's pose is "key-frame 0": prior edge on pose_dev's input value
 *                   (gl_params.ba_first_as_prior != 0) or fixed pose (== 0: only the points move);
 *   F               fixed observer key-frames per frame, 0 .. GL_TRACK_MAX_FIXED;
 *   fixed_pose_dev  B x F x 7; fixed_obs_dev B x M x F x 3 (u, v, u_right; u_right < 0 => mono);
 *   fixed_oct_dev   B x M x F int32: the octave of the observation, 0 .. 7 (the sigma^2 table has eight levels);
 *                   < 0: point not observed by that key-frame, fixed_obs_dev is not read there;
 *   fixed_erase_dev B x M x F uint8 out or NULL (observations the reference would erase, :855-879; 0 where not
 *                   observed and in slots with octave_dev < 0).
 * Three routes, the same verdicts from each:
 *   F == 0                      the on-chip refine of gl_track_frames (the prior costs one 6x6 block per Levenberg trial);
 *   1 <= F <= 4 and M <= 2000   on chip too: the fixed observers' edges are evaluated inside the per-frame refine;
 *   F > 4, or M > 2000, or option ba_fixed_pack = 1: packed into flat problems (P = 1, the frame's own observation
 *                               of a point first, then the fixed key-frames' in index order) and solved by the general
 *                               kernel of gl_joint_optimization.
 * F > GL_TRACK_MAX_FIXED is refused before anything is launched.  Same arithmetic as jointOptimization with P = 1:
 * parity tests against the oracle's joint_optimization(P = 1, prior / F fixed), and a hand-built case on either side
 * of every decision on every route (tests/optim_cases.py, call "anchored"). */
#define GL_TRACK_MAX_FIXED 8
typedef struct gl_track_anchor {
  const uint8_t* prior_dev;
  int32_t F;
  const double* fixed_pose_dev;
  const double* fixed_obs_dev;
  const int32_t* fixed_oct_dev;
  uint8_t* fixed_erase_dev;
} gl_track_anchor;
int gl_track_frames_anchored(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, const gl_params* prm, int B, int M,
                             double* pose_dev, double* Xw_dev, const double* obs_dev, const int32_t* octave_dev,
                             int32_t* assoc_dev, double* d2_dev, const gl_track_anchor* anchor);
/* The same for ONE frame with HOST buffers in and out - what the reference's tracking thread would call once per frame
 * (tracking.cpp:274,312,356).  The context keeps a page-locked staging buffer and its device mirror (grown on demand),
 * enqueues one copy each way around gl_track_frames(B = 1) on its stream and synchronises once; pose_host (7) and
 * Xw_host (M x 3) are updated in place, assoc_host (M) receives the associations.  Blocking. */
int gl_track_frame_host(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, const gl_params* prm, int M,
                        double* pose_host, double* Xw_host, const double* obs_host, const int32_t* octave_host,
                        int32_t* assoc_host);
/* ... anchored by the prior edge on the input pose (gl_track_frames_anchored with prior = 1, F = 0) */
int gl_track_frame_host_anchored(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, const gl_params* prm, int M,
                                 double* pose_host, double* Xw_host, const double* obs_host, const int32_t* octave_host,
                                 int32_t* assoc_host);

/* ---- device memory helpers for hosts without their own HIP allocator ------ */
int gl_malloc(gl_ctx_t* ctx, size_t bytes, void** dev_out);
int gl_free(gl_ctx_t* ctx, void* dev);
int gl_memcpy_h2d(gl_ctx_t* ctx, void* dst_dev, const void* src, size_t bytes); /* synchronous */
int gl_memcpy_d2h(gl_ctx_t* ctx, void* dst, const void* src_dev, size_t bytes); /* synchronous */
/* The frame-at-a-time host path (tracking.cpp:274,312,356 call once per frame): page-locked staging memory and
 * copies that are only ENQUEUED on the context's stream, so a frame costs one gl_ctx_synchronize instead of one per
 * transfer.  The host side of an _async copy must come from gl_malloc_host and stay untouched until the
 * synchronize. */
int gl_malloc_host(gl_ctx_t* ctx, size_t bytes, void** host_out);
int gl_free_host(gl_ctx_t* ctx, void* host);
int gl_memcpy_h2d_async(gl_ctx_t* ctx, void* dst_dev, const void* src_pinned, size_t bytes);
int gl_memcpy_d2h_async(gl_ctx_t* ctx, void* dst_pinned, const void* src_dev, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GMMLOC_HIP_H_ */
