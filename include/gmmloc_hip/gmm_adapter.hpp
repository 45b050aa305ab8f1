// gmm_adapter.hpp -- header-only C++ host mirror of the reference's hot-path interface over
// the C-ABI (include/gmmloc_hip.h).  This is the adapter a maintainer of HyHuang1995/gmmloc
// adds to the host (INTEGRATION.md shows the call-site patch); it depends only on the STL so
// that it also compiles where Eigen / g2o are absent.  Method names follow the reference:
//   gmmloc::GMM::renderView + searchCorrespondence  (gaussian_mixture.cpp:271-371, :484-534)
//   gmmloc::GMM::queryPoint                         (gaussian_mixture.cpp:545-576)
//   GMMUtility::loadGMMModel                        (gmm_utils.cpp:9-67)
//   GMMLoc::optimizePoint / checkMapAssociation     (gmmloc_opt.cpp:156-342)
//   Tracking::optimizeCurrentPose                   (tracking_opt.cpp:21-217)
//   Localization::jointOptimization                 (localization_opt.cpp:456-925), flattened by the host or built on the device
//                                                   from the resident map (jointOptimizationFromMap)
//   Localization::removeKeyFrames                   (localization.cpp:334-399) and the removals of Map::removeKeyFrame /
//                                                   removeMapPoint / the BA's erase loop on the resident map (cullKeyFrames, removeFromMap)
//   Localization::processNewKeyFrame / createMapPoints / fuseObservations + Map::replaceMapPoint, what they ADD to the resident map
//                                                   (localization.cpp:412-444, :299-321, map.cpp:112-150: addToMap, fuseObservationsInMap)
//   GMMLoc::createMapPointsFromStereo               (gmmloc_opt.cpp:36-113: createMapPointsFromStereo; on the resident map, with the
//                                                   association before it and the points' refresh behind it: processKeyFrameInMap)
//   Tracking::createTemporalPoints                  (tracking.cpp:411-465: createTemporalPoints)
//   Frame::computeStereoMatches                     (frame.cpp:179-349: computeStereoMatches, u_right and depth of a frame's features)
//   ORBextractor's orientation and descriptors      (orb_extractor.cpp:77-147, :1029-1046: orbDescribe; the pyramid, FAST and the octree
//                                                   stay with the host)
//   Localization::createMapPoints                   (localization_opt.cpp:206-454, the loop over the neighbours with the triangulation:
//                                                   createMapPointsInMap on the resident map)
//   Localization::removeMapPoints                   (localization.cpp:127-152) with num_visible_ / num_found_ / ref_idx_ and
//                                                   candidate_mappts_ kept on the device (setResidentMapStats, trackStats, growStats,
//                                                   mergeStats, removeMapPointsInMap)
//   the tail of Tracking::track, GMMLoc::needNewKeyFrame, Map::updateFrameInfo, the pose block of GMMLoc::processFrame,
//   Tracking::updateLastFrame                       (tracking.cpp:85-116, gmmloc.cpp:324-364, map.cpp:23-38, gmmloc.cpp:269-292,
//                                                   tracking.cpp:397-408: endFrame, noteReplaced, nextFrame on the resident map)
//   north-star per-frame path: associate + structure-constrained refinement of one frame (trackFrame)
// Host buffers in, host buffers out: each call stages through device memory owned by the
// adapter (gl_malloc / gl_memcpy_*), so the host code never sees a HIP type.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "gmmloc_hip.h"

namespace gmmloc_hip {

// 3: trackFrame is the unanchored refine again, trackFrameAnchored the anchored one (2: trackFrame(..., anchored = true));
//    MapBaRows / flattenMapBa / jointOptimizationFromMap were added without a new version: no existing call changed meaning
// 4: cullKeyFrames / removeFromMap edit the resident map on the device; the erase_obs of jointOptimizationFromMap no longer ask for
//    a re-upload of the CSR (pass them to removeFromMap); setResidentMapCapacity / addToMap / fuseObservationsInMap were added without
//    a new version: no existing call changed meaning
// 5: createMapPointsFromStereo / createTemporalPoints / processKeyFrameInMap: the depth-ordered walks run on the device - a host that
//    walked the answers of checkMapAssociation itself (INTEGRATION section 4 as it was) calls these instead
//    setResidentKeyFrameTables / createMapPointsInMap (the loop of Localization::createMapPoints on the resident map) were added
//    without a new version: no existing call changed meaning
//    setResidentMapStats / trackStats / growStats / mergeStats / removeMapPointsInMap likewise: a host that mirrored the counters keeps
//    working, one that calls these drops its mirror and the copies back of inview, feat_mp, match_local, outlier and repl_src / repl_tgt
//    loadVocabulary / bowTransform / bowTransformIntoTables likewise: a host that runs its own DBoW2 and uploads feat_vec_ keeps working
//    endFrame / noteReplaced / nextFrame likewise: a host that builds mappoints_ and the next frame's rows from the chain's copies back
//    keeps working, one that calls these drops the loop and the copies
//    computeStereoMatches likewise: a host that runs the reference's own OpenCV code and uploads u_right / depth keeps working
//    orbDescribe likewise: a host that runs the reference's ORBextractor to its end keeps working
constexpr int kAdapterVersion = 5;

inline void check(int rc, const char* what) {
  if (rc != GL_OK) throw std::runtime_error(std::string(what) + ": " + gl_last_error_string());
}

// RAII device buffer
class DevBuf {
 public:
  DevBuf(gl_ctx_t* ctx, size_t bytes) : ctx_(ctx), bytes_(bytes) { check(gl_malloc(ctx, bytes, &p_), "gl_malloc"); }
  ~DevBuf() { gl_free(ctx_, p_); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  template <class T>
  T* as() { return static_cast<T*>(p_); }
  void upload(const void* src) { check(gl_memcpy_h2d(ctx_, p_, src, bytes_), "h2d"); }
  void download(void* dst) { check(gl_memcpy_d2h(ctx_, dst, p_, bytes_), "d2h"); }
  void upload(const void* src, size_t n) { check(gl_memcpy_h2d(ctx_, p_, src, n), "h2d"); }
  void download(void* dst, size_t n) { check(gl_memcpy_d2h(ctx_, dst, p_, n), "d2h"); }
  size_t bytes() const { return bytes_; }

 private:
  gl_ctx_t* ctx_;
  void* p_ = nullptr;
  size_t bytes_;
};

struct Pose {  // g2o::SE3Quat T_cw: Eigen quaternion coefficients (x y z w) + translation
  double q[4], t[3];
};

class GMM {
 public:
  // loadGMMModel(path, model): false on failure like the reference (message via last_error())
  static bool loadGMMModel(const std::string& path, GMM& model, int device = 0) {
    model.release();
    if (gl_ctx_create(device, nullptr, &model.ctx_) != GL_OK) return false;
    gl_default_params(&model.prm_);
    if (gl_gmm_load_file(model.ctx_, path.c_str(), &model.prm_, &model.gmm_) != GL_OK) return false;
    return true;
  }
  ~GMM() { release(); }
  size_t countComponents() const { return (size_t)gl_gmm_count(gmm_); }
  void setCamera(const gl_camera& cam) { cam_ = cam; }
  static const char* last_error() { return gl_last_error_string(); }

  // renderView(rot_c_w, t_c_w) followed by searchCorrespondence(kpts, comps, num): one call, because
  // the rendered list only exists to be searched (gmmloc_opt.cpp:121-134).  uv: N x 2.
  // comps[i] = component indices (GaussianComponent2d::parent_ via getComponent3d(idx)).
  void renderViewAndSearch(const Pose& Tcw, const std::vector<double>& uv, std::vector<std::vector<int32_t>>& comps,
                           int num = 5) {
    const int N = (int)(uv.size() / 2);
    DevBuf dpose(ctx_, 56), duv(ctx_, uv.size() * 8 + 8), dcand(ctx_, (size_t)N * num * 4 + 4), dn(ctx_, (size_t)N * 4 + 4);
    dpose.upload(&Tcw);
    if (N) duv.upload(uv.data());
    check(gl_search2d(ctx_, gmm_, &cam_, 1, dpose.as<double>(), N, duv.as<double>(), nullptr, num, dcand.as<int32_t>(),
                      dn.as<int32_t>(), 0, nullptr, nullptr),
          "gl_search2d");
    check(gl_ctx_synchronize(ctx_), "sync");
    std::vector<int32_t> cand((size_t)N * num + 1), n(N + 1);
    dcand.download(cand.data());
    dn.download(n.data());
    comps.assign(N, {});
    for (int i = 0; i < N; ++i) comps[i].assign(cand.begin() + (size_t)i * num, cand.begin() + (size_t)i * num + n[i]);
  }

  // queryPoint(pt, res): res = {nearest component} (the reference pushes ret_index[0])
  void queryPoint(const double pt[3], std::vector<int>& res) {
    DevBuf dp(ctx_, 24), di(ctx_, 8);
    dp.upload(pt);
    check(gl_associate3d(ctx_, gmm_, dp.as<double>(), 1, GL_ASSOC_KNN5_EUCLID, di.as<int32_t>(), nullptr), "queryPoint");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t idx[2];
    di.download(idx);
    res.clear();
    if (idx[0] >= 0) res.push_back(idx[0]);
  }

  // exhaustive Mahalanobis association of N points (north-star `associate`)
  void associate(const std::vector<double>& pts, std::vector<int32_t>& idx, std::vector<double>& d2) {
    const int N = (int)(pts.size() / 3);
    idx.assign(N, -1);
    d2.assign(N, 0.0);
    if (!N) return;
    DevBuf dp(ctx_, pts.size() * 8), di(ctx_, (size_t)N * 4), dd(ctx_, (size_t)N * 8);
    dp.upload(pts.data());
    check(gl_associate3d(ctx_, gmm_, dp.as<double>(), N, GL_ASSOC_BRUTE, di.as<int32_t>(), dd.as<double>()), "associate");
    check(gl_ctx_synchronize(ctx_), "sync");
    di.download(idx.data());
    dd.download(d2.data());
  }

  // Tracking::optimizeCurrentPose for one frame: Xw / obs are M x 3, octave[i] < 0 = no map point.
  // Returns the inlier count; pose and is_outlier are updated like the reference does: the flag of a feature WITH a
  // map point is rewritten, the flags of the others are left as the host had them (tracking_opt.cpp:63-69).
  int optimizeCurrentPose(Pose& Tcw, const std::vector<double>& Xw, const std::vector<double>& obs,
                          const std::vector<int32_t>& octave, std::vector<uint8_t>& is_outlier) {
    const int M = (int)octave.size();
    is_outlier.resize(M, 0);
    // one pooled device buffer, one page-locked staging buffer, one transfer each way, one synchronize:
    //   pose | ninlier | is_outlier || Xw | obs | octave
    const size_t oN = 64, oF = 72, oX = oF + (((size_t)M + 7) / 8) * 8 + 8, oO = oX + (size_t)M * 24, oC = oO + (size_t)M * 24,
                 total = oC + (size_t)M * 4 + 8;
    DevBuf& d = pooled(1, total);
    char* st = stage(total);
    std::memcpy(st, &Tcw, 56);
    std::memset(st + oN, 0, 8);
    if (M) {
      std::memcpy(st + oF, is_outlier.data(), M);
      std::memcpy(st + oX, Xw.data(), (size_t)M * 24);
      std::memcpy(st + oO, obs.data(), (size_t)M * 24);
      std::memcpy(st + oC, octave.data(), (size_t)M * 4);
    }
    char* base = d.as<char>();
    check(gl_memcpy_h2d_async(ctx_, base, st, total), "h2d");
    check(gl_optimize_current_pose(ctx_, &cam_, &prm_, 1, M, reinterpret_cast<double*>(base), reinterpret_cast<const double*>(base + oX),
                                   reinterpret_cast<const double*>(base + oO), reinterpret_cast<const int32_t*>(base + oC),
                                   reinterpret_cast<uint8_t*>(base + oF), reinterpret_cast<int32_t*>(base + oN)),
          "gl_optimize_current_pose");
    check(gl_memcpy_d2h_async(ctx_, st, base, oX), "d2h");
    check(gl_ctx_synchronize(ctx_), "sync");
    std::memcpy(&Tcw, st, 56);
    if (M) std::memcpy(is_outlier.data(), st + oF, M);
    int32_t n;
    std::memcpy(&n, st + oN, 4);
    return n;
  }

  // North-star per-frame path for ONE frame (gl_track_frames, B = 1): exact Mahalanobis association of the
  // frame's M map points (kept iff chi2 <= 9, gmmloc_opt.cpp:230-232) + jointOptimization restricted to the
  // frame (1 free pose, M marginalised points, 5 / 5 / 40 Levenberg schedule).  Tcw and Xw are updated;
  // assoc[i] = component after the final gates or -1; octave[i] < 0 = no map point.
  // trackFrame: the pose is held by the map's Gaussians alone (rounds 1 - 2; the default again since adapter version 3 - version 2
  // silently switched this entry point to the anchored refine).  trackFrameAnchored: with the reference's gauge
  // anchor of key-frame 0 - an EdgeSE3QuatPrior on the pose the call starts from (sigma 2 deg / 1 cm; the pose is FIXED when
  // gl_params.ba_first_as_prior == 0), localization_opt.cpp:556-581: the reference never runs its structure BA without one, so
  // this is the entry point a port of Localization's per-frame refine wants; the two give DIFFERENT poses and points.
  void trackFrame(Pose& Tcw, std::vector<double>& Xw, const std::vector<double>& obs, const std::vector<int32_t>& octave,
                  std::vector<int32_t>& assoc, bool anchored = false) {
    const int M = (int)octave.size();
    assoc.assign(M, -1);
    if (!M) return;
    // the per-frame caller: the library keeps a page-locked staging buffer and its device mirror in the context, one
    // transfer each way on the context's stream and ONE synchronize per frame (gl_track_frame_host[_anchored])
    if (anchored)
      check(gl_track_frame_host_anchored(ctx_, gmm_, &cam_, &prm_, M, reinterpret_cast<double*>(&Tcw), Xw.data(), obs.data(),
                                         octave.data(), assoc.data()),
            "gl_track_frame_host_anchored");
    else
      check(gl_track_frame_host(ctx_, gmm_, &cam_, &prm_, M, reinterpret_cast<double*>(&Tcw), Xw.data(), obs.data(), octave.data(),
                                assoc.data()),
            "gl_track_frame_host");
  }
  void trackFrameAnchored(Pose& Tcw, std::vector<double>& Xw, const std::vector<double>& obs, const std::vector<int32_t>& octave,
                          std::vector<int32_t>& assoc) {
    trackFrame(Tcw, Xw, obs, octave, assoc, true);
  }

  // Localization::jointOptimization on one flattened local window (layout: gmmloc_hip.h, gl_joint_optimization):
  // poses [0,P) free, [P,P+F) fixed; observations in CSR order by point.
  struct LocalWindow {
    int P = 0, F = 0;
    std::vector<Pose> poses;            // P + F, in/out for [0,P)
    std::vector<uint8_t> prior;         // P: key-frame idx_ 0 (prior edge)
    std::vector<double> points;         // L x 3, in/out
    std::vector<int32_t> assoc;         // L: component or -1
    std::vector<int32_t> obs_ptr;       // L + 1
    std::vector<int32_t> obs_pose;      // NOBS
    std::vector<double> obs_uvr;        // NOBS x 3
    std::vector<int32_t> obs_oct;       // NOBS
    std::vector<uint8_t> assoc_dropped; // out, L   (:837-853)
    std::vector<uint8_t> obs_erase;     // out, NOBS (:855-879)
    int iters = 0;                      // out: actual_iter of the last optimize(40)
  };
  // stop_flag: the reference's pbStopFlag (setForceStopFlag, localization_opt.cpp:541-542) as one int32 in memory from
  // gl_malloc_host (another thread raises it to 1) or NULL: the window returns with the state of the last accepted step
  void jointOptimization(LocalWindow& w, const int32_t* stop_flag = nullptr) {
    const int L = (int)w.assoc.size(), NOBS = (int)w.obs_pose.size(), NP = w.P + w.F;
    w.assoc_dropped.assign(L, 0);
    w.obs_erase.assign(NOBS, 0);
    w.iters = 0;
    if (!L || !NOBS || !w.P) return;
    DevBuf dposes(ctx_, (size_t)NP * 56), dprior(ctx_, (size_t)w.P + 8), dpts(ctx_, (size_t)L * 24), dassoc(ctx_, (size_t)L * 4),
        dptr(ctx_, (size_t)(L + 1) * 4), dop(ctx_, (size_t)NOBS * 4), duvr(ctx_, (size_t)NOBS * 24), doct(ctx_, (size_t)NOBS * 4),
        ddrop(ctx_, (size_t)L + 8), derase(ctx_, (size_t)NOBS + 8), dit(ctx_, 8);
    std::vector<uint8_t> pr(w.P + 8, 0);
    std::memcpy(pr.data(), w.prior.data(), w.P);
    dposes.upload(w.poses.data());
    dprior.upload(pr.data());
    dpts.upload(w.points.data());
    dassoc.upload(w.assoc.data());
    dptr.upload(w.obs_ptr.data());
    dop.upload(w.obs_pose.data());
    duvr.upload(w.obs_uvr.data());
    doct.upload(w.obs_oct.data());
    check(gl_joint_optimization_stoppable(ctx_, gmm_, &cam_, &prm_, 1, w.P, w.F, L, NOBS, dposes.as<double>(), dprior.as<uint8_t>(),
                                          dpts.as<double>(), dassoc.as<int32_t>(), dptr.as<int32_t>(), dop.as<int32_t>(),
                                          duvr.as<double>(), doct.as<int32_t>(), ddrop.as<uint8_t>(), derase.as<uint8_t>(),
                                          dit.as<int32_t>(), stop_flag),
          "gl_joint_optimization");
    check(gl_ctx_synchronize(ctx_), "sync");
    dposes.download(w.poses.data());
    dpts.download(w.points.data());
    std::vector<uint8_t> t1(L + 8), t2(NOBS + 8);
    ddrop.download(t1.data());
    derase.download(t2.data());
    std::memcpy(w.assoc_dropped.data(), t1.data(), L);
    std::memcpy(w.obs_erase.data(), t2.data(), NOBS);
    int32_t it[2];
    dit.download(it);
    w.iters = it[0];
  }

  // The same local BA with the window built ON THE DEVICE from the resident map (gl_ba_window_build -> the 16 bytes of `sizes` ->
  // gl_joint_optimization_stoppable(B = 1) on the slab -> gl_ba_window_apply): nothing is flattened, uploaded or written back by the
  // host.  setResidentMap: the device arrays the host keeps (gl_map_view + gl_map_ba_view, e.g. uploaded from flattenMap /
  // flattenMapBa and maintained since); kf_pose, kf_twc, mp_pos and mp_assoc are updated in place on the device.  What comes back is
  // what the host's own bookkeeping needs: the rows of the window's key-frames (free then fixed) and points, the dropped
  // associations (:837-853: clear asscociations_ of win_mp[l] where assoc_dropped[l]), and erase_obs, the positions in the map's
  // CSR of the observations to remove (:855-879: removeFromMap(erase_obs, {}) applies them to the resident rows; the host's own
  // removeObservation / removeMapPoint follow from its dead_mp).  A window larger than the slab grows it and is built once more.
  struct WindowResult {
    int P = 0, F = 0, L = 0, nobs = 0, status = 0, iters = 0;
    std::vector<int32_t> win_kf, win_mp, erase_obs;
    std::vector<uint8_t> assoc_dropped;
  };
  void setResidentMap(const gl_map_view& view, const gl_map_ba_view& ba) {
    map_ = view;
    map_ba_ = ba;
    mp_cap_ = view.NMP;  // (no room to grow until setResidentMapCapacity says otherwise)
    obs_cap_ = view.NOBS;
  }
  WindowResult jointOptimizationFromMap(int32_t kf_row, const int32_t* stop_flag = nullptr) {
    WindowResult r;
    int32_t head[8];  // sizes (4) | status | iters | n_erase
    gl_ba_window w;
    char* base = nullptr;
    for (int attempt = 0;; ++attempt) {
      base = carveWindow(w);
      check(gl_memcpy_h2d(ctx_, base + 32, &kf_row, 4), "h2d");
      check(gl_ba_window_build(ctx_, &map_, &map_ba_, 1, reinterpret_cast<const int32_t*>(base + 32), &w), "gl_ba_window_build");
      check(gl_ctx_synchronize(ctx_), "sync");
      check(gl_memcpy_d2h(ctx_, head, base, 20), "d2h");
      r.P = head[0], r.F = head[1], r.L = head[2], r.nobs = head[3], r.status = head[4];
      if (r.status & GL_BA_WINDOW_BAD_ROW) throw std::runtime_error("jointOptimizationFromMap: kf_row is not a key-frame row");
      if (!(r.status & GL_BA_WINDOW_TRUNCATED)) break;
      if (attempt) throw std::runtime_error("jointOptimizationFromMap: the window still exceeds the capacities it asked for");
      const size_t need[4] = {(size_t)r.P, (size_t)r.F, (size_t)r.L + r.L / 4, (size_t)r.nobs + r.nobs / 4};
      for (int i = 0; i < 4; ++i) caps_[i] = need[i] > caps_[i] ? need[i] : caps_[i];
    }
    uint8_t* dropped = reinterpret_cast<uint8_t*>(base + win_off_[0]);
    uint8_t* erase = reinterpret_cast<uint8_t*>(base + win_off_[1]);
    int32_t* erase_obs = reinterpret_cast<int32_t*>(base + win_off_[2]);
    int32_t* iters = reinterpret_cast<int32_t*>(base + 20);
    const int32_t zero[2] = {0, 0};
    check(gl_memcpy_h2d(ctx_, iters, zero, 8), "h2d");
    zeros_.assign(win_off_[2] - win_off_[0], 0);  // (a BA stopped early may leave its flags unwritten: they start from zeros)
    check(gl_memcpy_h2d(ctx_, dropped, zeros_.data(), zeros_.size()), "h2d");
    if (r.L > 0 && r.nobs > 0)
      check(gl_joint_optimization_stoppable(ctx_, gmm_, &cam_, &prm_, 1, r.P, r.F, r.L, r.nobs, w.poses, w.prior, w.points, w.assoc, w.obs_ptr,
                                            w.obs_pose, w.obs_uvr, w.obs_oct, dropped, erase, iters, stop_flag),
            "gl_joint_optimization");
    check(gl_ba_window_apply(ctx_, &map_, const_cast<double*>(map_.mp_pos), &map_ba_, 1, &w, dropped, erase, iters, erase_obs, iters + 1),
          "gl_ba_window_apply");
    check(gl_ctx_synchronize(ctx_), "sync");
    check(gl_memcpy_d2h(ctx_, head, base, 32), "d2h");
    r.iters = head[5];
    const int ne = head[6];
    r.win_kf.resize((size_t)r.P + r.F);
    r.win_mp.resize(r.L);
    r.assoc_dropped.assign(r.L, 0);
    r.erase_obs.resize(ne);
    if (r.P + r.F) check(gl_memcpy_d2h(ctx_, r.win_kf.data(), w.win_kf, ((size_t)r.P + r.F) * 4), "d2h");
    if (r.L) check(gl_memcpy_d2h(ctx_, r.win_mp.data(), w.win_mp, (size_t)r.L * 4), "d2h");
    if (r.L && r.iters) check(gl_memcpy_d2h(ctx_, r.assoc_dropped.data(), dropped, r.L), "d2h");
    if (ne) check(gl_memcpy_d2h(ctx_, r.erase_obs.data(), erase_obs, (size_t)ne * 4), "d2h");
    return r;
  }

  // Localization::removeKeyFrames for key-frame kf_row on the resident map: gl_update_connections gives its covisible list
  // (getVectorCovisibleKeyFrames, at most Ccap entries), gl_cull_keyframes judges it in list order - no synchronise between the two.
  // kf_depth_dev: NKF x NFK float on the device (features_[i].depth, -1: none).  The map is not modified: pass cull_rows to
  // removeFromMap.  The arrays have one entry per candidate (cull_rows one per culled key-frame, in list order).
  struct CullResult {
    std::vector<int32_t> cand, num_mps, num_redundant, cand_status, cull_rows;
    std::vector<uint8_t> cull;
  };
  CullResult cullKeyFrames(int32_t kf_row, const float* kf_depth_dev, float th_depth, int32_t Ccap = 64) {
    if (Ccap < 1) throw std::runtime_error("cullKeyFrames: Ccap");
    const size_t C = (size_t)Ccap;
    // {kf_row | n_conn | conn_status | n_cull} then conn_kf, conn_w, num_mps, num_redundant, cand_status, cull_rows (C words each), cull (C bytes)
    char* b = pooled(3, 64 + 6 * C * 4 + C).as<char>();
    int32_t* hd = reinterpret_cast<int32_t*>(b);
    int32_t* arr = reinterpret_cast<int32_t*>(b + 64);
    uint8_t* cull = reinterpret_cast<uint8_t*>(b + 64 + 6 * C * 4);
    const int32_t head[4] = {kf_row, 0, 0, 0};
    check(gl_memcpy_h2d(ctx_, hd, head, 16), "h2d");
    check(gl_update_connections(ctx_, &map_, 1, hd, Ccap, arr, arr + C, hd + 1, nullptr, hd + 2), "gl_update_connections");
    check(gl_cull_keyframes(ctx_, &map_, &map_ba_, kf_depth_dev, th_depth, 1, Ccap, arr, hd + 1, cull, arr + 2 * C, arr + 3 * C, arr + 4 * C, arr + 5 * C,
                            hd + 3),
          "gl_cull_keyframes");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t got[4];
    check(gl_memcpy_d2h(ctx_, got, hd, 16), "d2h");
    const size_t n = (size_t)(got[1] < 0 ? 0 : got[1] > Ccap ? Ccap : got[1]), nc = (size_t)got[3];
    CullResult r;
    std::vector<int32_t>* dst[6] = {&r.cand, nullptr, &r.num_mps, &r.num_redundant, &r.cand_status, &r.cull_rows};
    for (int i = 0; i < 6; ++i) {
      if (!dst[i]) continue;
      dst[i]->resize(i == 5 ? nc : n);
      if (!dst[i]->empty()) check(gl_memcpy_d2h(ctx_, dst[i]->data(), arr + i * C, dst[i]->size() * 4), "d2h");
    }
    r.cull.resize(n);
    if (n) check(gl_memcpy_d2h(ctx_, r.cull.data(), cull, n), "d2h");
    return r;
  }
  // gl_map_remove on the resident map: "the points rm_mp, then the observations at the CSR positions erase_obs (WindowResult::erase_obs),
  // then the key-frames rm_kf in list order (CullResult::cull_rows)", the reference's cascade included, in place on the device - mp_valid,
  // kf_valid, kf_mp, the CSR (compacted: the view's NOBS becomes the new one) and mp_ref_kf_dev (NMP int32, may be null).  The lists are
  // the only upload.  dead_mp: the points that died, ascending - the host erases them from its own containers, as it does the key-frames
  // it listed (mappoints_.erase, keyframes_.erase, removeConnection, the re-parenting of frame_info_: map.cpp:56, :67-68, :89-109).
  struct RemoveResult {
    int32_t nobs = 0, status = 0;
    std::vector<int32_t> dead_mp;
  };
  RemoveResult removeFromMap(const std::vector<int32_t>& erase_obs, const std::vector<int32_t>& rm_kf, const std::vector<int32_t>& rm_mp = {},
                             int32_t* mp_ref_kf_dev = nullptr) {
    const size_t ne = erase_obs.size(), nk = rm_kf.size(), np = rm_mp.size(), NMP = (size_t)map_.NMP;
    char* b = pooled(4, 64 + (ne + nk + np + NMP) * 4).as<char>();
    int32_t* res = reinterpret_cast<int32_t*>(b);
    int32_t* l_er = reinterpret_cast<int32_t*>(b + 64);
    int32_t *l_kf = l_er + ne, *l_mp = l_kf + nk, *dead = l_mp + np;
    if (ne) check(gl_memcpy_h2d(ctx_, l_er, erase_obs.data(), ne * 4), "h2d");
    if (nk) check(gl_memcpy_h2d(ctx_, l_kf, rm_kf.data(), nk * 4), "h2d");
    if (np) check(gl_memcpy_h2d(ctx_, l_mp, rm_mp.data(), np * 4), "h2d");
    gl_map_edit ed{};
    ed.mp_valid = const_cast<uint8_t*>(map_.mp_valid);
    ed.kf_valid = const_cast<uint8_t*>(map_.kf_valid);
    ed.kf_mp = const_cast<int32_t*>(map_.kf_mp);
    ed.obs_ptr = const_cast<int32_t*>(map_.obs_ptr);
    ed.obs_kf = const_cast<int32_t*>(map_.obs_kf);
    ed.obs_feat = const_cast<int32_t*>(map_ba_.obs_feat);
    ed.mp_ref_kf = mp_ref_kf_dev;
    gl_map_remove_lists ls{};
    ls.rm_mp = np ? l_mp : nullptr, ls.rm_mp_cap = (int32_t)np;
    ls.erase_obs = ne ? l_er : nullptr, ls.erase_cap = (int32_t)ne;
    ls.rm_kf = nk ? l_kf : nullptr, ls.rm_kf_cap = (int32_t)nk;
    gl_map_remove_out out{};
    out.result = res;
    out.dead_mp = NMP ? dead : nullptr;
    out.dead_cap = (int32_t)NMP;
    check(gl_map_remove(ctx_, map_.NMP, map_.NKF, map_.NFK, map_.NOBS, &ed, map_ba_.kf_uvr, map_ba_.kf_first, &ls, &out), "gl_map_remove");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t got[3];
    check(gl_memcpy_d2h(ctx_, got, res, 12), "d2h");
    RemoveResult r;
    r.nobs = got[0], r.status = got[2];
    r.dead_mp.resize((size_t)got[1]);
    if (got[1]) check(gl_memcpy_d2h(ctx_, r.dead_mp.data(), dead, (size_t)got[1] * 4), "d2h");
    map_.NOBS = r.nobs;
    return r;
  }
  // What ADDS to the resident map (gl_map_add / gl_map_fuse, gmmloc_hip.h), in place on the device arrays of setResidentMap.  The
  // arrays keep their allocation: setResidentMapCapacity says how many rows the per-point arrays (obs_ptr one more) and how many entries
  // obs_kf / obs_feat hold; the view's NMP / NOBS follow every call.  A call that would exceed a capacity changes nothing and says so
  // (status GL_MAP_GROW_*_TRUNCATED, nmp / nobs = the sizes NEEDED): the host allocates larger arrays, copies, calls setResidentMap and
  // calls again.  The new key-frame's own rows (kf_uvr, kf_oct, kf_pose, kf_mp, its descriptors) are the host's upload, made before;
  // the view's NKF already counts it.  setResidentMap RESETS both capacities to the view's sizes (it cannot know the allocation), so
  // every setResidentMap - the one after growing the buffers included - is followed by setResidentMapCapacity.  For
  // fuseObservationsInMap the size NEEDED is the upper bound NOBS + the number of candidates, not the size the edit produces.
  void setResidentMapCapacity(int32_t NMPcap, int32_t OBScap) {
    mp_cap_ = NMPcap;
    obs_cap_ = OBScap;
  }
  // addToMap: the new points (rows NMP, NMP + 1, ...: new_pos x 3, new_assoc, new_ref_kf per point), the key-frames that become valid,
  // the attach triples (att_mp, att_kf, att_feat) in list order - each mappt->addObservation(kf, feat); kf->addObservation(mappt, feat) -
  // and the key-frames walked as processNewKeyFrame walks the new one.  already_mp = candidate_mappts_.
  struct AddLists {
    std::vector<double> new_pos;
    std::vector<int32_t> new_assoc, new_ref_kf, new_kf, att_mp, att_kf, att_feat, walk_kf;
  };
  struct AddResult {
    int32_t nmp = 0, nobs = 0, n_attached = 0, n_skipped = 0, status = 0;
    std::vector<int32_t> already_mp;  // all of them (n_already = its size): the call's already_cap is a slot per walked slot, never short
  };
  AddResult addToMap(const AddLists& l, int32_t* mp_ref_kf_dev = nullptr) {
    const size_t nn = l.new_assoc.size(), nk = l.new_kf.size(), na = l.att_mp.size(), nw = l.walk_kf.size(), NFK = (size_t)map_.NFK;
    if (l.new_pos.size() != nn * 3 || (mp_ref_kf_dev && l.new_ref_kf.size() != nn) || l.att_kf.size() != na || l.att_feat.size() != na)
      throw std::runtime_error("addToMap: lists of different lengths");
    const size_t nr = mp_ref_kf_dev ? nn : 0, words = nn + nr + nk + 3 * na + nw + nw * NFK;
    char* b = pooled(5, 64 + nn * 24 + words * 4).as<char>();
    int32_t* res = reinterpret_cast<int32_t*>(b);
    double* d_pos = reinterpret_cast<double*>(b + 64);
    int32_t* d_assoc = reinterpret_cast<int32_t*>(b + 64 + nn * 24);
    int32_t *d_ref = d_assoc + nn, *d_kf = d_ref + nr, *d_amp = d_kf + nk, *d_akf = d_amp + na, *d_aft = d_akf + na, *d_walk = d_aft + na,
            *d_already = d_walk + nw;
    auto put = [this](void* dst, const void* src, size_t bytes) {
      if (bytes) check(gl_memcpy_h2d(ctx_, dst, src, bytes), "h2d");
    };
    put(d_pos, l.new_pos.data(), nn * 24);
    put(d_assoc, l.new_assoc.data(), nn * 4);
    put(d_ref, l.new_ref_kf.data(), nr * 4);
    put(d_kf, l.new_kf.data(), nk * 4);
    put(d_amp, l.att_mp.data(), na * 4);
    put(d_akf, l.att_kf.data(), na * 4);
    put(d_aft, l.att_feat.data(), na * 4);
    put(d_walk, l.walk_kf.data(), nw * 4);
    const gl_map_edit ed = residentEdit(mp_ref_kf_dev);
    gl_map_add_lists ls{};
    if (nn) ls.new_pos = d_pos, ls.new_assoc = d_assoc, ls.new_ref_kf = nr ? d_ref : nullptr, ls.new_mp_cap = (int32_t)nn;
    if (nk) ls.new_kf = d_kf, ls.new_kf_cap = (int32_t)nk;
    if (na) ls.att_mp = d_amp, ls.att_kf = d_akf, ls.att_feat = d_aft, ls.attach_cap = (int32_t)na;
    if (nw) ls.walk_kf = d_walk, ls.walk_cap = (int32_t)nw;
    gl_map_add_out out{};
    out.result = res;
    out.already_mp = (nw && NFK) ? d_already : nullptr;
    out.already_cap = (int32_t)(nw * NFK);
    check(gl_map_add(ctx_, map_.NMP, map_.NKF, map_.NFK, map_.NOBS, mp_cap_, obs_cap_, &ed, const_cast<double*>(map_.mp_pos), map_ba_.mp_assoc, &ls, &out),
          "gl_map_add");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t got[6];
    check(gl_memcpy_d2h(ctx_, got, res, 24), "d2h");
    AddResult r;
    r.nmp = got[0], r.nobs = got[1], r.n_attached = got[2], r.n_skipped = got[3], r.status = got[5];
    const size_t n_already = std::min((size_t)std::max(got[4], 0), nw * NFK);
    r.already_mp.resize(n_already);
    if (n_already) check(gl_memcpy_d2h(ctx_, r.already_mp.data(), d_already, n_already * 4), "d2h");
    if (!(r.status & (GL_MAP_GROW_MP_TRUNCATED | GL_MAP_GROW_OBS_TRUNCATED))) map_.NMP = r.nmp, map_.NOBS = r.nobs;
    return r;
  }
  // fuseObservationsInMap: what Localization::fuseObservations does with its matches (localization.cpp:299-321, Map::replaceMapPoint)
  // for key-frame kf_row, in list order.  cand_rows: the map-point rows the host gave to the search, in its order; best_idx_dev: the
  // best_idx row gl_fuse_search wrote for that list, still on the device.  repl_src / repl_tgt: the replacements in step order - the
  // host's num_visible_ / num_found_, ptr_replaced_ and mappoints_.erase follow from them; the targets' descriptors are
  // gl_update_map_points' before the next key-frame's search.
  struct FuseResult {
    int32_t nobs = 0, n_fused = 0, n_attached = 0, status = 0;
    std::vector<int32_t> repl_src, repl_tgt;
  };
  FuseResult fuseObservationsInMap(int32_t kf_row, const std::vector<int32_t>& cand_rows, const int32_t* best_idx_dev) {
    const size_t n = cand_rows.size();
    char* b = pooled(5, 64 + 3 * n * 4).as<char>();
    int32_t* res = reinterpret_cast<int32_t*>(b);
    int32_t* d_cand = reinterpret_cast<int32_t*>(b + 64);
    int32_t *d_src = d_cand + n, *d_tgt = d_src + n;
    if (n) check(gl_memcpy_h2d(ctx_, d_cand, cand_rows.data(), n * 4), "h2d");
    const gl_map_edit ed = residentEdit(nullptr);
    gl_map_fuse_out out{};
    out.result = res;
    out.repl_src = n ? d_src : nullptr;
    out.repl_tgt = n ? d_tgt : nullptr;
    out.repl_cap = (int32_t)n;
    check(gl_map_fuse(ctx_, map_.NMP, map_.NKF, map_.NFK, map_.NOBS, obs_cap_, &ed, map_ba_.kf_uvr, kf_row, (int)n, d_cand, best_idx_dev, &out), "gl_map_fuse");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t got[5];
    check(gl_memcpy_d2h(ctx_, got, res, 20), "d2h");
    FuseResult r;
    r.nobs = got[0], r.n_fused = got[1], r.n_attached = got[2], r.status = got[4];
    r.repl_src.resize((size_t)got[3]);
    r.repl_tgt.resize((size_t)got[3]);
    if (got[3]) {
      check(gl_memcpy_d2h(ctx_, r.repl_src.data(), d_src, (size_t)got[3] * 4), "d2h");
      check(gl_memcpy_d2h(ctx_, r.repl_tgt.data(), d_tgt, (size_t)got[3] * 4), "d2h");
    }
    if (!(r.status & GL_MAP_GROW_OBS_TRUNCATED)) map_.NOBS = r.nobs;
    return r;
  }
  // ---- points from stereo depth: the depth-ordered walks of GMMLoc::createMapPointsFromStereo (gmmloc_opt.cpp:36-113) and
  // Tracking::createTemporalPoints (tracking.cpp:411-465) on the device (gl_create_stereo_points / gl_create_temporal_points).
  struct FrameFeatures {          // one frame's features as the host holds them, NF slots
    Pose Tcw;
    std::vector<double> uv;       // NF x 2 (Feature::uv)
    std::vector<float> ur, depth; // u_right, Feature::depth (-1: none)
    std::vector<int32_t> oct;     // outside 0..7: a padding slot
    std::vector<uint8_t> held;    // 0 = mappoints_[i] is null, 1 = countObservations() >= 1, 2 = a point without observation
  };
  // the new points in WALK order: feature, position (as checkMapAssociation left it), component (-1: FromDepth, else FromDepthGMM);
  // feat_new[i]: the new point of slot i, -1 untouched, -2 set to null and left so; cand / ncand: kf->comps_ as a table (NF x num)
  struct StereoPoints {
    int32_t n_new = 0, stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // {entries, walked, n_new, n_rejected, num_points, broke, 0, 0}
    std::vector<int32_t> new_feat, new_assoc, feat_new, cand, ncand;
    std::vector<double> new_pos;
  };
  // associateMapElements + createMapPointsFromStereo for one key-frame: host vectors in, the points to create out.  One synchronise.
  StereoPoints createMapPointsFromStereo(const FrameFeatures& f, int32_t kf_row, int32_t mp_base, bool check_depth, float th_depth, int num = 5) {
    const size_t NF = f.oct.size();
    if (f.uv.size() != NF * 2 || f.ur.size() != NF || f.depth.size() != NF || f.held.size() != NF)
      throw std::runtime_error("createMapPointsFromStereo: arrays of different lengths");
    StereoPoints r;
    r.feat_new.assign(NF, -1);
    r.cand.assign(NF * (size_t)num, -1);
    r.ncand.assign(NF, 0);
    if (!NF) return r;
    size_t off = 64;
    auto take = [&off](size_t bytes) {
      const size_t at = off;
      off += (bytes + 63) / 64 * 64;
      return at;
    };
    const size_t o_pose = take(56), o_uv = take(NF * 16), o_ur = take(NF * 4), o_dep = take(NF * 4), o_oct = take(NF * 4), o_held = take(NF),
                 o_cand = take(NF * num * 4), o_nc = take(NF * 4), o_pos = take(NF * 24), o_int = take(7 * NF * 4);
    char* b = pooled(6, off).as<char>();
    auto put = [this](void* dst, const void* src, size_t bytes) { check(gl_memcpy_h2d(ctx_, dst, src, bytes), "h2d"); };
    put(b + 48, &kf_row, 4);
    put(b + o_pose, &f.Tcw, 56);
    put(b + o_uv, f.uv.data(), NF * 16);
    put(b + o_ur, f.ur.data(), NF * 4);
    put(b + o_dep, f.depth.data(), NF * 4);
    put(b + o_oct, f.oct.data(), NF * 4);
    put(b + o_held, f.held.data(), NF);
    gl_stereo_points_in in{};
    in.pose = reinterpret_cast<double*>(b + o_pose);
    in.feat_uv = reinterpret_cast<double*>(b + o_uv);
    in.feat_ur = reinterpret_cast<float*>(b + o_ur);
    in.feat_depth = reinterpret_cast<float*>(b + o_dep);
    in.feat_oct = reinterpret_cast<int32_t*>(b + o_oct);
    in.cand = reinterpret_cast<int32_t*>(b + o_cand);
    in.ncand = reinterpret_cast<int32_t*>(b + o_nc);
    in.held = reinterpret_cast<uint8_t*>(b + o_held);
    in.kf_row = reinterpret_cast<int32_t*>(b + 48);
    int32_t* ints = reinterpret_cast<int32_t*>(b + o_int);
    gl_stereo_points_out out{};
    out.new_pos = reinterpret_cast<double*>(b + o_pos);
    out.new_feat = ints, out.new_assoc = ints + NF, out.new_ref_kf = ints + 2 * NF, out.att_mp = ints + 3 * NF, out.att_kf = ints + 4 * NF,
    out.att_feat = ints + 5 * NF, out.feat_new = ints + 6 * NF;
    out.n_new = reinterpret_cast<int32_t*>(b);
    out.stats = reinterpret_cast<int32_t*>(b + 16);
    check(gl_search2d(ctx_, gmm_, &cam_, 1, in.pose, (int)NF, in.feat_uv, nullptr, num, const_cast<int32_t*>(in.cand), const_cast<int32_t*>(in.ncand), 0,
                      nullptr, nullptr),
          "gl_search2d");
    check(gl_create_stereo_points(ctx_, gmm_, &cam_, &prm_, 1, (int)NF, num, &in, mp_base, check_depth ? 1 : 0, th_depth, &out), "gl_create_stereo_points");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t head[12];
    check(gl_memcpy_d2h(ctx_, head, b, 48), "d2h");
    r.n_new = head[0];
    std::memcpy(r.stats, head + 4, 32);
    const size_t n = (size_t)r.n_new;
    r.new_feat.resize(n), r.new_assoc.resize(n), r.new_pos.resize(n * 3);
    if (n) {
      check(gl_memcpy_d2h(ctx_, r.new_feat.data(), out.new_feat, n * 4), "d2h");
      check(gl_memcpy_d2h(ctx_, r.new_assoc.data(), out.new_assoc, n * 4), "d2h");
      check(gl_memcpy_d2h(ctx_, r.new_pos.data(), out.new_pos, n * 24), "d2h");
    }
    check(gl_memcpy_d2h(ctx_, r.feat_new.data(), out.feat_new, NF * 4), "d2h");
    check(gl_memcpy_d2h(ctx_, r.cand.data(), in.cand, NF * num * 4), "d2h");
    check(gl_memcpy_d2h(ctx_, r.ncand.data(), in.ncand, NF * 4), "d2h");
    return r;
  }
  // createTemporalPoints for the last frame (not a key-frame: tracking.cpp:414 is the caller's): rows holds the last-frame arrays of
  // gl_track_frame_chain as the host made them for the key-points; the rows of the slots that get a temporal point are rewritten
  // (last_pt, last_observed = 0, last_valid = !last_outlier, last_desc = feat_desc), the others keep their bytes.  -> temp_flag per slot
  struct LastFrameRows {
    std::vector<double> last_pt;                              // NF x 3
    std::vector<uint8_t> last_observed, last_valid, last_desc;  // NF, NF, NF x 32
  };
  std::vector<uint8_t> createTemporalPoints(const FrameFeatures& f, const std::vector<uint8_t>& last_outlier, const std::vector<uint8_t>& feat_desc,
                                            float th_depth, LastFrameRows& rows) {
    const size_t NF = f.oct.size();
    if (f.uv.size() != NF * 2 || f.depth.size() != NF || f.held.size() != NF || last_outlier.size() != NF || feat_desc.size() != NF * 32 ||
        rows.last_pt.size() != NF * 3 || rows.last_observed.size() != NF || rows.last_valid.size() != NF || rows.last_desc.size() != NF * 32)
      throw std::runtime_error("createTemporalPoints: arrays of different lengths");
    std::vector<uint8_t> flag(NF, 0);
    if (!NF) return flag;
    size_t off = 64;
    auto take = [&off](size_t bytes) {
      const size_t at = off;
      off += (bytes + 63) / 64 * 64;
      return at;
    };
    const size_t o_pose = take(56), o_uv = take(NF * 16), o_dep = take(NF * 4), o_oct = take(NF * 4), o_held = take(NF), o_outl = take(NF),
                 o_desc = take(NF * 32), o_flag = take(NF), o_pt = take(NF * 24), o_obs = take(NF), o_val = take(NF), o_ld = take(NF * 32);
    char* b = pooled(7, off).as<char>();
    auto put = [this](void* dst, const void* src, size_t bytes) { check(gl_memcpy_h2d(ctx_, dst, src, bytes), "h2d"); };
    put(b + o_pose, &f.Tcw, 56);
    put(b + o_uv, f.uv.data(), NF * 16);
    put(b + o_dep, f.depth.data(), NF * 4);
    put(b + o_oct, f.oct.data(), NF * 4);
    put(b + o_held, f.held.data(), NF);
    put(b + o_outl, last_outlier.data(), NF);
    put(b + o_desc, feat_desc.data(), NF * 32);
    put(b + o_pt, rows.last_pt.data(), NF * 24);
    put(b + o_obs, rows.last_observed.data(), NF);
    put(b + o_val, rows.last_valid.data(), NF);
    put(b + o_ld, rows.last_desc.data(), NF * 32);
    gl_temporal_points_in in{};
    in.pose = reinterpret_cast<double*>(b + o_pose);
    in.feat_uv = reinterpret_cast<double*>(b + o_uv);
    in.feat_depth = reinterpret_cast<float*>(b + o_dep);
    in.feat_oct = reinterpret_cast<int32_t*>(b + o_oct);
    in.held = reinterpret_cast<uint8_t*>(b + o_held);
    in.last_outlier = reinterpret_cast<uint8_t*>(b + o_outl);
    in.feat_desc = reinterpret_cast<uint8_t*>(b + o_desc);
    gl_temporal_points_out out{};
    out.temp_flag = reinterpret_cast<uint8_t*>(b + o_flag);
    out.n_temp = reinterpret_cast<int32_t*>(b);
    out.last_pt = reinterpret_cast<double*>(b + o_pt);
    out.last_observed = reinterpret_cast<uint8_t*>(b + o_obs);
    out.last_valid = reinterpret_cast<uint8_t*>(b + o_val);
    out.last_desc = reinterpret_cast<uint8_t*>(b + o_ld);
    check(gl_create_temporal_points(ctx_, &cam_, 1, (int)NF, &in, th_depth, &out), "gl_create_temporal_points");
    check(gl_ctx_synchronize(ctx_), "sync");
    check(gl_memcpy_d2h(ctx_, flag.data(), out.temp_flag, NF), "d2h");
    check(gl_memcpy_d2h(ctx_, rows.last_pt.data(), out.last_pt, NF * 24), "d2h");
    check(gl_memcpy_d2h(ctx_, rows.last_observed.data(), out.last_observed, NF), "d2h");
    check(gl_memcpy_d2h(ctx_, rows.last_valid.data(), out.last_valid, NF), "d2h");
    check(gl_memcpy_d2h(ctx_, rows.last_desc.data(), out.last_desc, NF * 32), "d2h");
    return flag;
  }
  // ---- stereo depth: Frame::computeStereoMatches (frame.cpp:179-349) on the device (gl_stereo_matches; the rules and the declared
  // deviations are in gmmloc_hip.h).  Host vectors in and out; a pyramid level is the ROI of mvImagePyramid[l] as it lies in its
  // bordered buffer: the pointer to its first pixel, its size and the buffer's bytes per row.  One upload, one synchronise.
  struct ImageLevel {
    const uint8_t* ptr;
    int32_t width, height;
    int64_t stride;
  };
  struct RightKeyPoints {
    std::vector<float> uv;        // NR x 2 (kp.pt)
    std::vector<int32_t> oct;     // NR
    std::vector<uint8_t> desc;    // NR x 32
  };
  struct StereoMatches {
    std::vector<float> ur, depth;        // NF: Feature::u_right, Feature::depth (-1: none)
    std::vector<int32_t> match_r, sad;   // NF: the right key-point and the best SAD of a feature pushed at :332, -1 otherwise
    int32_t stat[4] = {0, 0, 0, -1};     // {features that pass :261, entries of vDistIdx, entries reset, the median SAD or -1}
  };
  StereoMatches computeStereoMatches(const std::vector<double>& uv, const std::vector<int32_t>& oct, const std::vector<uint8_t>& desc,
                                     const RightKeyPoints& right, const std::vector<ImageLevel>& pyr_left,
                                     const std::vector<ImageLevel>& pyr_right, double scale_factor = 1.2) {
    const size_t NF = oct.size(), NR = right.oct.size(), NL = pyr_left.size();
    if (uv.size() != NF * 2 || desc.size() != NF * 32 || right.uv.size() != NR * 2 || right.desc.size() != NR * 32)
      throw std::runtime_error("computeStereoMatches: arrays of different lengths");
    if (NL < 1 || NL > 8 || pyr_right.size() != NL) throw std::runtime_error("computeStereoMatches: 1 .. 8 levels, the same on both sides");
    StereoMatches r;
    r.ur.assign(NF, -1.0f), r.depth.assign(NF, -1.0f), r.match_r.assign(NF, -1), r.sad.assign(NF, -1);
    if (!NF || !NR) return r;
    size_t off = 64;
    auto take = [&off](size_t bytes) {
      const size_t at = off;
      off += (bytes + 63) / 64 * 64;
      return at;
    };
    const size_t o_uv = take(NF * 16), o_oct = take(NF * 4), o_desc = take(NF * 32), o_ruv = take(NR * 8), o_roct = take(NR * 4),
                 o_rdesc = take(NR * 32), o_ur = take(NF * 4), o_dep = take(NF * 4), o_m = take(NF * 4), o_sad = take(NF * 4);
    gl_image_pyramid pyr[2] = {};
    const std::vector<ImageLevel>* side[2] = {&pyr_left, &pyr_right};
    size_t o_img[2][8], n_img[2][8];
    for (int s = 0; s < 2; ++s) {
      pyr[s].nlevels = (int32_t)NL;
      const size_t base = off;
      for (size_t l = 0; l < NL; ++l) {
        const ImageLevel& im = (*side[s])[l];
        if (!im.ptr || im.width < 1 || im.height < 1 || im.stride < im.width) throw std::runtime_error("computeStereoMatches: bad level image");
        n_img[s][l] = (size_t)(im.height - 1) * (size_t)im.stride + (size_t)im.width;
        o_img[s][l] = take(n_img[s][l]);
        pyr[s].width[l] = im.width, pyr[s].height[l] = im.height, pyr[s].stride[l] = im.stride, pyr[s].offset[l] = (int64_t)(o_img[s][l] - base);
      }
      pyr[s].frame_stride = (int64_t)(off - base);
    }
    char* b = pooled(16, off).as<char>();
    auto put = [this](void* dst, const void* src, size_t bytes) { check(gl_memcpy_h2d(ctx_, dst, src, bytes), "h2d"); };
    put(b + o_uv, uv.data(), NF * 16);
    put(b + o_oct, oct.data(), NF * 4);
    put(b + o_desc, desc.data(), NF * 32);
    put(b + o_ruv, right.uv.data(), NR * 8);
    put(b + o_roct, right.oct.data(), NR * 4);
    put(b + o_rdesc, right.desc.data(), NR * 32);
    for (int s = 0; s < 2; ++s) {
      for (size_t l = 0; l < NL; ++l) put(b + o_img[s][l], (*side[s])[l].ptr, n_img[s][l]);
      pyr[s].data = reinterpret_cast<uint8_t*>(b + o_img[s][0]) - pyr[s].offset[0];  // (the side's base)
    }
    gl_stereo_in in{};
    in.feat_uv = reinterpret_cast<double*>(b + o_uv);
    in.feat_oct = reinterpret_cast<int32_t*>(b + o_oct);
    in.feat_desc = reinterpret_cast<uint8_t*>(b + o_desc);
    in.r_uv = reinterpret_cast<float*>(b + o_ruv);
    in.r_oct = reinterpret_cast<int32_t*>(b + o_roct);
    in.r_desc = reinterpret_cast<uint8_t*>(b + o_rdesc);
    gl_stereo_out out{};
    out.feat_ur = reinterpret_cast<float*>(b + o_ur);
    out.feat_depth = reinterpret_cast<float*>(b + o_dep);
    out.match_r = reinterpret_cast<int32_t*>(b + o_m);
    out.sad = reinterpret_cast<int32_t*>(b + o_sad);
    out.stat = reinterpret_cast<int32_t*>(b);
    check(gl_stereo_matches(ctx_, &cam_, scale_factor, 1, (int)NF, (int)NR, &in, &pyr[0], &pyr[1], &out), "gl_stereo_matches");
    check(gl_ctx_synchronize(ctx_), "sync");
    check(gl_memcpy_d2h(ctx_, r.ur.data(), out.feat_ur, NF * 4), "d2h");
    check(gl_memcpy_d2h(ctx_, r.depth.data(), out.feat_depth, NF * 4), "d2h");
    check(gl_memcpy_d2h(ctx_, r.match_r.data(), out.match_r, NF * 4), "d2h");
    check(gl_memcpy_d2h(ctx_, r.sad.data(), out.sad, NF * 4), "d2h");
    check(gl_memcpy_d2h(ctx_, r.stat, out.stat, 16), "d2h");
    return r;
  }
  // ---- ORB orientation and descriptors: the regular half of ORBextractor (orb_extractor.cpp: IC_Angle, the 7 x 7 blur, the steered
  // BRIEF read, the scaling of the key-points) for ONE image on the device (gl_orb_describe; the rules and the declared deviations are
  // in gmmloc_hip.h).  kp_xy: the key-points AT THEIR LEVEL in ROI coordinates, kp_oct their octaves; pattern: the host's own
  // bit_pattern_31_ as 512 x 2 int8 (checked here: an entry outside [-13, 13] throws); levels as for computeStereoMatches; blur_w: the
  // four Q8 taps (empty: gl_orb_default_blur(2)); kp_angle: empty, or the angles that steer instead of the computed orientation.
  // One upload, one synchronise.
  struct OrbFeatures {
    std::vector<uint8_t> desc;      // N x 32
    std::vector<float> angle;       // N (-1: skipped)
    std::vector<int32_t> moments;   // N x 2 {m_10, m_01}
    std::vector<float> uv32;        // N x 2: kp.pt
    std::vector<double> uv64;       // N x 2: Feature::uv
    int32_t stat[2] = {0, 0};       // {described, skipped}
  };
  OrbFeatures orbDescribe(const std::vector<int32_t>& kp_xy, const std::vector<int32_t>& kp_oct, const std::vector<int8_t>& pattern,
                          const std::vector<ImageLevel>& levels, std::vector<int32_t> blur_w = {}, double scale_factor = 1.2,
                          const std::vector<float>& kp_angle = {}) {
    const size_t N = kp_oct.size(), NL = levels.size();
    if (kp_xy.size() != N * 2 || (!kp_angle.empty() && kp_angle.size() != N)) throw std::runtime_error("orbDescribe: arrays of different lengths");
    if (pattern.size() != 1024) throw std::runtime_error("orbDescribe: the pattern has 512 x 2 entries");
    for (int8_t v : pattern)
      if (v < -13 || v > 13) throw std::runtime_error("orbDescribe: a pattern entry outside [-13, 13]");
    if (NL < 1 || NL > 8) throw std::runtime_error("orbDescribe: 1 .. 8 levels");
    if (blur_w.empty()) {
      blur_w.resize(4);
      check(gl_orb_default_blur(2.0, blur_w.data()), "gl_orb_default_blur");
    }
    if (blur_w.size() != 4) throw std::runtime_error("orbDescribe: blur_w has four taps");
    OrbFeatures r;
    r.desc.assign(N * 32, 0), r.angle.assign(N, -1.0f), r.moments.assign(N * 2, 0), r.uv32.assign(N * 2, -1.0f), r.uv64.assign(N * 2, -1.0);
    if (!N) return r;
    size_t off = 64;
    auto take = [&off](size_t bytes) {
      const size_t at = off;
      off += (bytes + 63) / 64 * 64;
      return at;
    };
    const size_t o_pat = take(1024), o_xy = take(N * 8), o_oct = take(N * 4), o_ang = take(N * 4), o_desc = take(N * 32), o_angle = take(N * 4),
                 o_mom = take(N * 8), o_uv32 = take(N * 8), o_uv64 = take(N * 16);
    gl_image_pyramid pyr = {};
    pyr.nlevels = (int32_t)NL;
    size_t o_img[8], n_img[8];
    const size_t base = off;
    for (size_t l = 0; l < NL; ++l) {
      const ImageLevel& im = levels[l];
      if (!im.ptr || im.width < 1 || im.height < 1 || im.stride < im.width) throw std::runtime_error("orbDescribe: bad level image");
      n_img[l] = (size_t)(im.height - 1) * (size_t)im.stride + (size_t)im.width;
      o_img[l] = take(n_img[l]);
      pyr.width[l] = im.width, pyr.height[l] = im.height, pyr.stride[l] = im.stride, pyr.offset[l] = (int64_t)(o_img[l] - base);
    }
    pyr.frame_stride = (int64_t)(off - base);
    char* b = pooled(17, off).as<char>();
    auto put = [this](void* dst, const void* src, size_t bytes) { check(gl_memcpy_h2d(ctx_, dst, src, bytes), "h2d"); };
    put(b + o_pat, pattern.data(), 1024);
    put(b + o_xy, kp_xy.data(), N * 8);
    put(b + o_oct, kp_oct.data(), N * 4);
    if (!kp_angle.empty()) put(b + o_ang, kp_angle.data(), N * 4);
    for (size_t l = 0; l < NL; ++l) put(b + o_img[l], levels[l].ptr, n_img[l]);
    pyr.data = reinterpret_cast<uint8_t*>(b + base);
    gl_orb_in in{};
    in.kp_xy = reinterpret_cast<int32_t*>(b + o_xy);
    in.kp_oct = reinterpret_cast<int32_t*>(b + o_oct);
    in.kp_angle = kp_angle.empty() ? nullptr : reinterpret_cast<float*>(b + o_ang);
    in.pattern = reinterpret_cast<int8_t*>(b + o_pat);
    in.blur_w = blur_w.data();
    in.scale_factor = scale_factor;
    gl_orb_out out{};
    out.desc = reinterpret_cast<uint8_t*>(b + o_desc);
    out.angle = reinterpret_cast<float*>(b + o_angle);
    out.moments = reinterpret_cast<int32_t*>(b + o_mom);
    out.uv32 = reinterpret_cast<float*>(b + o_uv32);
    out.uv64 = reinterpret_cast<double*>(b + o_uv64);
    out.stat = reinterpret_cast<int32_t*>(b);
    check(gl_orb_describe(ctx_, 1, (int)N, &in, &pyr, &out), "gl_orb_describe");
    check(gl_ctx_synchronize(ctx_), "sync");
    check(gl_memcpy_d2h(ctx_, r.desc.data(), out.desc, N * 32), "d2h");
    check(gl_memcpy_d2h(ctx_, r.angle.data(), out.angle, N * 4), "d2h");
    check(gl_memcpy_d2h(ctx_, r.moments.data(), out.moments, N * 8), "d2h");
    check(gl_memcpy_d2h(ctx_, r.uv32.data(), out.uv32, N * 8), "d2h");
    check(gl_memcpy_d2h(ctx_, r.uv64.data(), out.uv64, N * 16), "d2h");
    check(gl_memcpy_d2h(ctx_, r.stat, out.stat, 8), "d2h");
    return r;
  }
  // ---- ORB detection: the irregular half of ORBextractor (ComputePyramid, the cell FAST, DistributeOctTree) for ONE raw image on the
  // device (gl_orb_pyramid, gl_orb_detect; the rules and the declared deviations are in gmmloc_hip.h).  orbExtract is the composite:
  // the raw image goes up, gl_orb_pyramid -> gl_orb_detect -> gl_orb_describe run on the context's stream with detect's device arrays
  // as describe's inputs, and nothing is read back before the one synchronise at the end.  orbPyramid and orbDetect run the first one or
  // two stages alone.
  struct OrbPyramidHost {
    std::vector<std::vector<uint8_t>> levels;  // tightly packed
    std::vector<int32_t> width, height;
  };
  struct OrbKeyPoints {
    std::vector<int32_t> kp_xy;      // n x 2, AT THEIR LEVEL, ROI coordinates
    std::vector<int32_t> kp_oct;     // n
    std::vector<float> kp_response;  // n
    int32_t level_count[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int32_t stat[4] = {0, 0, 0, 0};  // {candidates, cells redone at min_th, key-points, overflow level mask}
    OrbFeatures features;            // orbExtract: of the n key-points
  };
  struct OrbDetectConfig {
    int nfeatures = 1000, nlevels = 8;
    double scale_factor = 1.2;
    int ini_th = 20, min_th = 7, cand_cap = 8192;
  };
  OrbPyramidHost orbPyramid(const ImageLevel& image, int nlevels = 8, double scale_factor = 1.2) {
    OrbStage s = orb_stage(image, OrbDetectConfig{0, nlevels, scale_factor, 20, 7, 1}, 0);
    check(gl_ctx_synchronize(ctx_), "sync");
    OrbPyramidHost r;
    for (int l = 0; l < nlevels; ++l) {
      r.width.push_back(s.pyr.width[l]), r.height.push_back(s.pyr.height[l]);
      r.levels.emplace_back((size_t)s.pyr.width[l] * (size_t)s.pyr.height[l]);
      check(gl_memcpy_d2h(ctx_, r.levels.back().data(), s.pyr.data + s.pyr.offset[l], r.levels.back().size()), "d2h");
    }
    return r;
  }
  OrbKeyPoints orbDetect(const ImageLevel& image) { return orbDetect(image, OrbDetectConfig()); }
  OrbKeyPoints orbDetect(const ImageLevel& image, const OrbDetectConfig& cfg) { return orb_front(image, cfg, nullptr, {}); }
  OrbKeyPoints orbExtract(const ImageLevel& image, const std::vector<int8_t>& pattern) { return orbExtract(image, pattern, OrbDetectConfig()); }
  OrbKeyPoints orbExtract(const ImageLevel& image, const std::vector<int8_t>& pattern, const OrbDetectConfig& cfg, std::vector<int32_t> blur_w = {}) {
    if (pattern.size() != 1024) throw std::runtime_error("orbExtract: the pattern has 512 x 2 entries");
    for (int8_t v : pattern)
      if (v < -13 || v > 13) throw std::runtime_error("orbExtract: a pattern entry outside [-13, 13]");
    if (blur_w.empty()) {
      blur_w.resize(4);
      check(gl_orb_default_blur(2.0, blur_w.data()), "gl_orb_default_blur");
    }
    if (blur_w.size() != 4) throw std::runtime_error("orbExtract: blur_w has four taps");
    return orb_front(image, cfg, &pattern, blur_w);
  }

 private:
  struct OrbStage {
    gl_image_pyramid pyr;
    gl_orb_detect_out det;
    char* rest;  // behind detect's outputs: describe's
    size_t N;
  };
  // the raw image up, the pyramid built, detect enqueued (stage >= 1); `extra`: bytes kept behind detect's outputs
  OrbStage orb_stage(const ImageLevel& im, const OrbDetectConfig& cfg, int stage, size_t extra = 0) {
    if (!im.ptr || im.width < 1 || im.height < 1 || im.stride < im.width) throw std::runtime_error("orb: bad image");
    OrbStage s{};
    check(gl_orb_pyramid_layout(im.width, im.height, cfg.nlevels, cfg.scale_factor, 0, 0, &s.pyr), "gl_orb_pyramid_layout");
    int32_t bound[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    size_t N = 1;
    if (stage >= 1) {
      check(gl_orb_detect_bound(&s.pyr, cfg.nfeatures, cfg.scale_factor, bound), "gl_orb_detect_bound");
      N = 0;
      for (int l = 0; l < cfg.nlevels; ++l) N += (size_t)bound[l];
      N = N ? N : 1;
    }
    s.N = N;
    size_t off = 0;
    auto take = [&off](size_t bytes) {
      const size_t at = off;
      off += (bytes + 63) / 64 * 64;
      return at;
    };
    const size_t o_img = take((size_t)s.pyr.frame_stride), o_xy = take(N * 8), o_oct = take(N * 4), o_resp = take(N * 4), o_n = take(4), o_lc = take(32),
                 o_stat = take(16), o_rest = take(extra * N + 1024);
    char* b = pooled(18, off).as<char>();
    for (int y = 0; y < im.height && im.stride != im.width; ++y)  // level 0: stride = width
      check(gl_memcpy_h2d(ctx_, b + o_img + (size_t)y * (size_t)im.width, im.ptr + (size_t)y * (size_t)im.stride, (size_t)im.width), "h2d");
    if (im.stride == im.width) check(gl_memcpy_h2d(ctx_, b + o_img, im.ptr, (size_t)im.width * (size_t)im.height), "h2d");
    s.pyr.data = reinterpret_cast<uint8_t*>(b + o_img);
    check(gl_orb_pyramid(ctx_, 1, &s.pyr, cfg.scale_factor), "gl_orb_pyramid");
    s.det.kp_xy = reinterpret_cast<int32_t*>(b + o_xy);
    s.det.kp_oct = reinterpret_cast<int32_t*>(b + o_oct);
    s.det.kp_response = reinterpret_cast<float*>(b + o_resp);
    s.det.n_kp = reinterpret_cast<int32_t*>(b + o_n);
    s.det.level_count = reinterpret_cast<int32_t*>(b + o_lc);
    s.det.stat = reinterpret_cast<int32_t*>(b + o_stat);
    s.rest = b + o_rest;
    if (stage >= 1)
      check(gl_orb_detect(ctx_, 1, (int)N, &s.pyr, cfg.nfeatures, cfg.scale_factor, cfg.ini_th, cfg.min_th, cfg.cand_cap, &s.det), "gl_orb_detect");
    return s;
  }
  OrbKeyPoints orb_front(const ImageLevel& im, const OrbDetectConfig& cfg, const std::vector<int8_t>* pattern, const std::vector<int32_t>& blur_w) {
    OrbStage s = orb_stage(im, cfg, 1, pattern ? 32 + 4 + 8 + 8 + 16 + 64 : 0);
    const size_t N = s.N;
    gl_orb_out out{};
    if (pattern) {  // describe reads detect's arrays where they lie
      char* p = s.rest;
      check(gl_memcpy_h2d(ctx_, p, pattern->data(), 1024), "h2d");
      gl_orb_in in{};
      in.kp_xy = s.det.kp_xy, in.kp_oct = s.det.kp_oct, in.n_kp = s.det.n_kp;
      in.pattern = reinterpret_cast<int8_t*>(p);
      in.blur_w = blur_w.data();
      in.scale_factor = cfg.scale_factor;
      p += 1024;
      out.desc = reinterpret_cast<uint8_t*>(p), p += (N * 32 + 15) / 16 * 16;
      out.uv64 = reinterpret_cast<double*>(p), p += N * 16;
      out.angle = reinterpret_cast<float*>(p), p += (N * 4 + 15) / 16 * 16;
      out.moments = reinterpret_cast<int32_t*>(p), p += N * 8;
      out.uv32 = reinterpret_cast<float*>(p), p += N * 8;
      out.stat = reinterpret_cast<int32_t*>(p);
      check(gl_orb_describe(ctx_, 1, (int)N, &in, &s.pyr, &out), "gl_orb_describe");
    }
    check(gl_ctx_synchronize(ctx_), "sync");
    OrbKeyPoints r;
    int32_t n = 0;
    check(gl_memcpy_d2h(ctx_, &n, s.det.n_kp, 4), "d2h");
    check(gl_memcpy_d2h(ctx_, r.level_count, s.det.level_count, 32), "d2h");
    check(gl_memcpy_d2h(ctx_, r.stat, s.det.stat, 16), "d2h");
    const size_t k = (size_t)n;
    r.kp_xy.resize(k * 2), r.kp_oct.resize(k), r.kp_response.resize(k);
    if (k) {
      check(gl_memcpy_d2h(ctx_, r.kp_xy.data(), s.det.kp_xy, k * 8), "d2h");
      check(gl_memcpy_d2h(ctx_, r.kp_oct.data(), s.det.kp_oct, k * 4), "d2h");
      check(gl_memcpy_d2h(ctx_, r.kp_response.data(), s.det.kp_response, k * 4), "d2h");
    }
    if (pattern) {
      OrbFeatures& f = r.features;
      f.desc.resize(k * 32), f.angle.resize(k), f.moments.resize(k * 2), f.uv32.resize(k * 2), f.uv64.resize(k * 2);
      if (k) {
        check(gl_memcpy_d2h(ctx_, f.desc.data(), out.desc, k * 32), "d2h");
        check(gl_memcpy_d2h(ctx_, f.angle.data(), out.angle, k * 4), "d2h");
        check(gl_memcpy_d2h(ctx_, f.moments.data(), out.moments, k * 8), "d2h");
        check(gl_memcpy_d2h(ctx_, f.uv32.data(), out.uv32, k * 8), "d2h");
        check(gl_memcpy_d2h(ctx_, f.uv64.data(), out.uv64, k * 16), "d2h");
      }
      check(gl_memcpy_d2h(ctx_, f.stat, out.stat, 8), "d2h");
    }
    return r;
  }

 public:
  // GMMLoc::processKeyFrame's GMM half for key-frame kf_row of the resident map, whose own table rows the host has uploaded (the rows
  // of kf_pose / kf_twc / kf_uvr / kf_oct in the views of setResidentMap, and the arrays below): gl_search2d -> gl_create_stereo_points ->
  // gl_map_add (the key-frame becomes valid, the new rows, their attach triples; the counts stay on the device) -> gl_update_map_points
  // on the new rows.  One synchronise.  After a truncation (status) nothing is changed: grow the buffers and call again.
  struct KeyFrameRowsDev {
    const double* uv;        // NFK x 2, kf_uvr's first two columns
    const float* ur;         // NFK, its third as float
    const float* depth;      // NFK
    const uint8_t* held;     // NFK (FrameFeatures::held)
    const uint8_t* kf_desc;  // key-frame rows x NFK x 32: every key-frame's descriptors (gl_update_map_points reads the observers')
  };
  struct KeyFrameResult {
    int32_t nmp = 0, nobs = 0, n_attached = 0, n_skipped = 0, status = 0, n_new = 0, stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<int32_t> feat_new;                             // per slot, as StereoPoints::feat_new: new point r is map row (old NMP) + r
    const int32_t* cand_dev = nullptr;                         // NFK x num / NFK on the device until the next processKeyFrameInMap:
    const int32_t* ncand_dev = nullptr;                        //   kf->comps_ for createMapPoints
  };
  KeyFrameResult processKeyFrameInMap(int32_t kf_row, const KeyFrameRowsDev& d, bool check_depth, float th_depth, int32_t* mp_ref_kf_dev,
                                      float scale_factor = 1.2f, int num = 5) {
    if (kf_row < 0 || kf_row >= map_.NKF || !mp_ref_kf_dev) throw std::runtime_error("processKeyFrameInMap: kf_row / mp_ref_kf_dev");
    const size_t NF = (size_t)map_.NFK;
    const int32_t NMP0 = map_.NMP;
    size_t off = 128;
    auto take = [&off](size_t bytes) {
      const size_t at = off;
      off += (bytes + 63) / 64 * 64;
      return at;
    };
    const size_t o_cand = take(NF * num * 4), o_nc = take(NF * 4), o_pos = take(NF * 24), o_int = take(7 * NF * 4);
    char* b = pooled(8, off).as<char>();  // {n_new | stats at 16 | kf_row at 48 | gl_map_add's result at 64}
    check(gl_memcpy_h2d(ctx_, b + 48, &kf_row, 4), "h2d");
    gl_stereo_points_in in{};
    in.pose = map_ba_.kf_pose + (size_t)kf_row * 7;
    in.feat_uv = d.uv, in.feat_ur = d.ur, in.feat_depth = d.depth, in.held = d.held;
    in.feat_oct = map_ba_.kf_oct + (size_t)kf_row * NF;
    in.cand = reinterpret_cast<int32_t*>(b + o_cand);
    in.ncand = reinterpret_cast<int32_t*>(b + o_nc);
    in.kf_row = reinterpret_cast<int32_t*>(b + 48);
    int32_t* ints = reinterpret_cast<int32_t*>(b + o_int);
    gl_stereo_points_out out{};
    out.new_pos = reinterpret_cast<double*>(b + o_pos);
    out.new_feat = ints, out.new_assoc = ints + NF, out.new_ref_kf = ints + 2 * NF, out.att_mp = ints + 3 * NF, out.att_kf = ints + 4 * NF,
    out.att_feat = ints + 5 * NF, out.feat_new = ints + 6 * NF;
    out.n_new = reinterpret_cast<int32_t*>(b);
    out.stats = reinterpret_cast<int32_t*>(b + 16);
    check(gl_search2d(ctx_, gmm_, &cam_, 1, in.pose, (int)NF, in.feat_uv, nullptr, num, const_cast<int32_t*>(in.cand), const_cast<int32_t*>(in.ncand), 0,
                      nullptr, nullptr),
          "gl_search2d");
    check(gl_create_stereo_points(ctx_, gmm_, &cam_, &prm_, 1, (int)NF, num, &in, NMP0, check_depth ? 1 : 0, th_depth, &out), "gl_create_stereo_points");
    const gl_map_edit ed = residentEdit(mp_ref_kf_dev);
    gl_map_add_lists ls{};
    ls.new_pos = out.new_pos, ls.new_assoc = out.new_assoc, ls.new_ref_kf = out.new_ref_kf, ls.n_new_mp = out.n_new, ls.new_mp_cap = (int32_t)NF;
    ls.new_kf = in.kf_row, ls.new_kf_cap = 1;
    ls.att_mp = out.att_mp, ls.att_kf = out.att_kf, ls.att_feat = out.att_feat, ls.n_attach = out.n_new, ls.attach_cap = (int32_t)NF;
    gl_map_add_out ao{};
    ao.result = reinterpret_cast<int32_t*>(b + 64);
    check(gl_map_add(ctx_, map_.NMP, map_.NKF, map_.NFK, map_.NOBS, mp_cap_, obs_cap_, &ed, const_cast<double*>(map_.mp_pos), map_ba_.mp_assoc, &ls, &ao),
          "gl_map_add");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t head[22];
    check(gl_memcpy_d2h(ctx_, head, b, 88), "d2h");
    KeyFrameResult r;
    std::memcpy(r.stats, head + 4, 32);
    r.nmp = head[16], r.nobs = head[17], r.n_attached = head[18], r.n_skipped = head[19], r.status = head[21];
    r.n_new = r.nmp - NMP0;
    r.cand_dev = in.cand, r.ncand_dev = in.ncand;
    r.feat_new.resize(NF);
    if (NF) check(gl_memcpy_d2h(ctx_, r.feat_new.data(), out.feat_new, NF * 4), "d2h");
    if (r.status & (GL_MAP_GROW_MP_TRUNCATED | GL_MAP_GROW_OBS_TRUNCATED)) return r;
    map_.NMP = r.nmp, map_.NOBS = r.nobs;
    if (r.n_new > 0) {
      const size_t p0 = (size_t)NMP0;
      check(gl_update_map_points(ctx_, scale_factor, 3, r.n_new, map_.NKF, map_.NFK, map_.NOBS, map_ba_.kf_twc, map_.kf_valid, map_ba_.kf_oct, d.kf_desc,
                                 map_.mp_pos + p0 * 3, map_.mp_valid + p0, mp_ref_kf_dev + p0, map_.obs_ptr + p0, map_.obs_kf, map_ba_.obs_feat,
                                 const_cast<uint8_t*>(map_.mp_desc) + p0 * 32, const_cast<double*>(map_.mp_normal) + p0 * 3,
                                 const_cast<float*>(map_.mp_max_dist) + p0, const_cast<float*>(map_.mp_min_dist) + p0),
            "gl_update_map_points");
    }
    return r;
  }
  // Localization::createMapPoints for key-frame kf_row of the resident map (localization_opt.cpp:206-454): gl_update_connections ->
  // gl_create_map_points_from_map over its first nn neighbours -> gl_map_add (the new rows, their attach triples; the counts stay on the
  // device) -> gl_update_map_points on the new rows.  setResidentKeyFrameTables: the per-key-frame tables the triangulation reads
  // (gl_map_kf_tables; a new key-frame's rows belong to its one upload).  mb: Frame::mb (float(bf) / float(fx), frame.cpp:24).  One
  // synchronise.  After a truncation (status) nothing is changed: grow the buffers and call again.  The new points are the map rows
  // [old NMP, old NMP + n_new): candidate_mappts_ gains them, type_ comes from new_type.
  void setResidentKeyFrameTables(const gl_map_kf_tables& t) { kf_tables_ = t; }
  struct CreatePointsResult {
    int32_t nmp = 0, nobs = 0, n_attached = 0, n_skipped = 0, status = 0, n_new = 0, tri_status = 0;
    std::vector<int32_t> new_type, new_nb;  // n_new: MapPoint::type_ (1..4), the neighbour's index in the covisibility list
    std::vector<int32_t> feat_new;          // NFK: the map row of the point a feature gained, -1 for none
    std::vector<int32_t> nb_stats;          // nn x 8: {row, skip bits, nmatches, created, rejected, 0, 0, 0}
  };
  CreatePointsResult createMapPointsInMap(int32_t kf_row, int32_t nn, float mb, int32_t* mp_ref_kf_dev, float scale_factor = 1.2f) {
    if (kf_row < 0 || kf_row >= map_.NKF || !mp_ref_kf_dev || nn < 0 || nn > GL_TRI_NB_MAX || !kf_tables_.kf_desc)
      throw std::runtime_error("createMapPointsInMap: kf_row / nn / mp_ref_kf_dev / setResidentKeyFrameTables");
    const size_t NF = (size_t)map_.NFK, n = (size_t)(nn > 0 ? nn : 1);
    const int32_t NMP0 = map_.NMP;
    size_t off = 128;
    auto take = [&off](size_t bytes) {
      const size_t at = off;
      off += (bytes + 63) / 64 * 64;
      return at;
    };
    const size_t o_conn = take(2 * n * 4), o_pos = take(NF * 24), o_int = take(13 * NF * 4), o_st = take(n * 32);
    // {gl_map_add's result at 0 | kf_row at 32 | n_conn 36 | conn status 40 | n_new 44 | n_attach 48 | status 52}
    char* b = pooled(9, off).as<char>();
    auto at = [b](size_t o) { return reinterpret_cast<int32_t*>(b + o); };
    check(gl_memcpy_h2d(ctx_, b + 32, &kf_row, 4), "h2d");
    int32_t* conn = at(o_conn);
    check(gl_update_connections(ctx_, &map_, 1, at(32), (int)n, conn, conn + n, at(36), nullptr, at(40)), "gl_update_connections");
    int32_t* ints = at(o_int);
    gl_tri_points_out out{};
    out.new_pos = reinterpret_cast<double*>(b + o_pos);
    out.new_assoc = ints, out.new_ref_kf = ints + NF, out.new_type = ints + 2 * NF, out.new_nb = ints + 3 * NF, out.new_feat1 = ints + 4 * NF,
    out.new_feat2 = ints + 5 * NF, out.att_mp = ints + 6 * NF, out.att_kf = ints + 8 * NF, out.att_feat = ints + 10 * NF, out.feat_new = ints + 12 * NF;
    out.n_new = at(44), out.n_attach = at(48), out.status = at(52), out.nb_stats = at(o_st), out.new_cap = (int32_t)NF;
    check(gl_create_map_points_from_map(ctx_, gmm_, &cam_, &prm_, scale_factor, &map_, &map_ba_, &kf_tables_, kf_row, conn, at(36), (int)n, 0, nn, mb, NMP0,
                                        &out),
          "gl_create_map_points_from_map");
    const gl_map_edit ed = residentEdit(mp_ref_kf_dev);
    gl_map_add_lists ls{};
    ls.new_pos = out.new_pos, ls.new_assoc = out.new_assoc, ls.new_ref_kf = out.new_ref_kf, ls.n_new_mp = out.n_new, ls.new_mp_cap = (int32_t)NF;
    ls.att_mp = out.att_mp, ls.att_kf = out.att_kf, ls.att_feat = out.att_feat, ls.n_attach = out.n_attach, ls.attach_cap = (int32_t)(2 * NF);
    gl_map_add_out ao{};
    ao.result = at(0);
    check(gl_map_add(ctx_, map_.NMP, map_.NKF, map_.NFK, map_.NOBS, mp_cap_, obs_cap_, &ed, const_cast<double*>(map_.mp_pos), map_ba_.mp_assoc, &ls, &ao),
          "gl_map_add");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t head[14];
    check(gl_memcpy_d2h(ctx_, head, b, 56), "d2h");
    CreatePointsResult r;
    r.nmp = head[0], r.nobs = head[1], r.n_attached = head[2], r.n_skipped = head[3], r.status = head[5], r.tri_status = head[13];
    r.n_new = r.nmp - NMP0;
    r.feat_new.resize(NF);
    r.nb_stats.resize((size_t)nn * 8);
    r.new_type.resize((size_t)r.n_new);
    r.new_nb.resize((size_t)r.n_new);
    if (NF) check(gl_memcpy_d2h(ctx_, r.feat_new.data(), out.feat_new, NF * 4), "d2h");
    if (nn) check(gl_memcpy_d2h(ctx_, r.nb_stats.data(), out.nb_stats, (size_t)nn * 32), "d2h");
    if (r.n_new > 0) {
      check(gl_memcpy_d2h(ctx_, r.new_type.data(), out.new_type, (size_t)r.n_new * 4), "d2h");
      check(gl_memcpy_d2h(ctx_, r.new_nb.data(), out.new_nb, (size_t)r.n_new * 4), "d2h");
    }
    if (r.status & (GL_MAP_GROW_MP_TRUNCATED | GL_MAP_GROW_OBS_TRUNCATED)) return r;
    map_.NMP = r.nmp, map_.NOBS = r.nobs;
    if (r.n_new > 0) {
      const size_t p0 = (size_t)NMP0;
      check(gl_update_map_points(ctx_, scale_factor, 3, r.n_new, map_.NKF, map_.NFK, map_.NOBS, map_ba_.kf_twc, map_.kf_valid, map_ba_.kf_oct,
                                 kf_tables_.kf_desc, map_.mp_pos + p0 * 3, map_.mp_valid + p0, mp_ref_kf_dev + p0, map_.obs_ptr + p0, map_.obs_kf,
                                 map_ba_.obs_feat, const_cast<uint8_t*>(map_.mp_desc) + p0 * 32, const_cast<double*>(map_.mp_normal) + p0 * 3,
                                 const_cast<float*>(map_.mp_max_dist) + p0, const_cast<float*>(map_.mp_min_dist) + p0),
            "gl_update_map_points");
    }
    return r;
  }
  // ---- num_visible_ / num_found_ / ref_idx_ and candidate_mappts_ on the device (gl_map_stats, gmmloc_hip.h): the host keeps no
  // mirror of the counters and copies nothing back to add 1 to them.  setResidentMapStats: the caller-owned device arrays, mp_visible /
  // mp_found / mp_ref_idx with the rows of setResidentMapCapacity, cand with cand_cap entries.
  void setResidentMapStats(const gl_map_stats& st) { stats_ = st; }
  // trackStats: the three counter rules of the tracker (tracking.cpp:213-225, :249-254, :279-292) for B frames, on the DEVICE outputs of
  // gl_track_frame_chain_map (or of _front / _back with the host's local_mp); counts2_dev may be null (every frame tracked).  Enqueued only.
  void trackStats(int B, int NF, int NPcap, const int32_t* feat_mp_dev, const int32_t* match_local_dev, const uint8_t* outlier_dev,
                  const uint8_t* inview_dev, const int32_t* local_mp_dev, const int32_t* n_local_mp_dev, const int32_t* counts2_dev = nullptr) {
    check(gl_map_stats_track(ctx_, map_.NMP, &stats_, B, NF, NPcap, feat_mp_dev, match_local_dev, outlier_dev, inview_dev, local_mp_dev, n_local_mp_dev,
                             counts2_dev),
          "gl_map_stats_track");
  }
  // growStats, after addToMap / createMapPointsInMap: the rows [first, first + new_ref_kf.size()) get their counters and ref_idx_
  // (mappoint.cpp:18-19), candidate_mappts_ gains already_mp (AddResult::already_mp, localization.cpp:433) and - for the rows of
  // createMapPoints (localization_opt.cpp:442) - the new rows themselves.  status: GL_MAP_STATS_MP_TRUNCATED / _CAND_TRUNCATED (the
  // append that would not fit added nothing; n_cand is then the size NEEDED).
  struct GrowStatsResult {
    int32_t status = 0, n_cand = 0;
  };
  GrowStatsResult growStats(int32_t first, const std::vector<int32_t>& new_ref_kf, const std::vector<int32_t>& already_mp, bool new_rows_are_candidates) {
    const size_t nn = new_ref_kf.size(), na = already_mp.size();
    char* b = pooled(10, 64 + (nn + na) * 4).as<char>();
    int32_t* res = reinterpret_cast<int32_t*>(b);  // {status of the rows | append: size, status | append: size, status}
    int32_t *d_ref = reinterpret_cast<int32_t*>(b + 64), *d_already = d_ref + nn;
    if (nn) check(gl_memcpy_h2d(ctx_, d_ref, new_ref_kf.data(), nn * 4), "h2d");
    if (na) check(gl_memcpy_h2d(ctx_, d_already, already_mp.data(), na * 4), "h2d");
    check(gl_map_stats_new_points(ctx_, mp_cap_, map_.NKF, &stats_, first, (int)nn, nullptr, nn ? d_ref : nullptr, res), "gl_map_stats_new_points");
    check(gl_map_cand_append(ctx_, &stats_, na ? d_already : nullptr, 0, (int)na, nullptr, res + 1), "gl_map_cand_append");
    check(gl_map_cand_append(ctx_, &stats_, nullptr, first, new_rows_are_candidates ? (int)nn : 0, nullptr, res + 3), "gl_map_cand_append");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t got[5];
    check(gl_memcpy_d2h(ctx_, got, res, 20), "d2h");
    GrowStatsResult r;
    r.status = got[0] | got[2] | got[4];
    r.n_cand = got[3];
    return r;
  }
  // mergeStats: FuseResult::repl_src / repl_tgt in step order, tgt's counters += src's (map.cpp:142-143).  Enqueued only (the lists
  // are copied before the call returns).
  void mergeStats(const std::vector<int32_t>& repl_src, const std::vector<int32_t>& repl_tgt) {
    const size_t n = repl_src.size();
    if (repl_tgt.size() != n) throw std::runtime_error("mergeStats: lists of different lengths");
    if (!n) return;
    int32_t* d = pooled(10, 2 * n * 4).as<int32_t>();
    check(gl_memcpy_h2d(ctx_, d, repl_src.data(), n * 4), "h2d");
    check(gl_memcpy_h2d(ctx_, d + n, repl_tgt.data(), n * 4), "h2d");
    check(gl_map_stats_merge(ctx_, map_.NMP, &stats_, d, d + n, (int)n, nullptr), "gl_map_stats_merge");
  }
  // removeMapPointsInMap: Localization::removeMapPoints (localization.cpp:127-152) for key-frame kf_row - gl_cull_map_points on the
  // resident map and the counters, its rm_mp / device count straight into gl_map_remove; one synchronise.  verdict: one per OLD entry
  // of the list (0 kept, 1 invalid, 2 ratio, 3 young and few, 4 aged out, 5 row outside the table); remove.dead_mp: for the host's
  // mappoints_.erase.
  struct RemoveMapPointsResult {
    int32_t kept = 0, removed = 0, erased = 0, status = 0;
    std::vector<int32_t> verdict, rm_mp;
    RemoveResult remove;
  };
  RemoveMapPointsResult removeMapPointsInMap(int32_t kf_row, int32_t* mp_ref_kf_dev = nullptr) {
    const size_t cap = (size_t)stats_.cand_cap, NMP = (size_t)map_.NMP;
    char* b = pooled(10, 64 + (2 * cap + NMP) * 4).as<char>();
    int32_t* res = reinterpret_cast<int32_t*>(b);  // {kept, removed, erased, status | n_rm | gl_map_remove's result (3)}
    int32_t *d_rm = reinterpret_cast<int32_t*>(b + 64), *d_verdict = d_rm + cap, *d_dead = d_verdict + cap;
    const gl_map_edit ed = residentEdit(mp_ref_kf_dev);
    check(gl_cull_map_points(ctx_, map_.NMP, map_.NKF, map_.NFK, map_.NOBS, &ed, map_ba_.kf_uvr, &stats_, kf_row, cap ? d_rm : nullptr, res + 4,
                             cap ? d_verdict : nullptr, res),
          "gl_cull_map_points");
    gl_map_remove_lists ls{};
    ls.rm_mp = cap ? d_rm : nullptr, ls.n_rm_mp = res + 4, ls.rm_mp_cap = (int32_t)cap;
    gl_map_remove_out out{};
    out.result = res + 5;
    out.dead_mp = NMP ? d_dead : nullptr;
    out.dead_cap = (int32_t)NMP;
    check(gl_map_remove(ctx_, map_.NMP, map_.NKF, map_.NFK, map_.NOBS, &ed, map_ba_.kf_uvr, map_ba_.kf_first, &ls, &out), "gl_map_remove");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t got[8];
    check(gl_memcpy_d2h(ctx_, got, res, 32), "d2h");
    RemoveMapPointsResult r;
    r.kept = got[0], r.removed = got[1], r.erased = got[2], r.status = got[3];
    r.verdict.resize((size_t)(got[0] + got[1] + got[2]));
    r.rm_mp.resize((size_t)got[1]);
    if (!r.verdict.empty()) check(gl_memcpy_d2h(ctx_, r.verdict.data(), d_verdict, r.verdict.size() * 4), "d2h");
    if (!r.rm_mp.empty()) check(gl_memcpy_d2h(ctx_, r.rm_mp.data(), d_rm, r.rm_mp.size() * 4), "d2h");
    r.remove.nobs = got[5], r.remove.status = got[7];
    r.remove.dead_mp.resize((size_t)got[6]);
    if (got[6]) check(gl_memcpy_d2h(ctx_, r.remove.dead_mp.data(), d_dead, (size_t)got[6] * 4), "d2h");
    map_.NOBS = r.remove.nobs;
    return r;
  }
  // ---- frame end and hand-over on the device (gl_track_frame_end / gl_map_note_replaced / gl_track_frame_next, gmmloc_hip.h): the loop
  // over the features that followed a tracked frame - mappoints_, the next frame's last-frame rows, the held flags, the refreshed pose
  // and the motion-model prediction, TrackStat and needNewKeyFrame - on the chain's own device outputs and the resident map.  Device
  // pointers in and out, enqueued only: a run of non-key frames reads back stat (8 int32 per frame) and nothing else.
  // endFrame: the tail of Tracking::track (tracking.cpp:85-116) and, with a rule, GMMLoc::needNewKeyFrame (gmmloc.cpp:324-364).
  void endFrame(int B, int NF, int NL, int NPcap, const gl_frame_end_in& in, float th_depth, const gl_kf_rule* rule, const gl_frame_end_out& out) {
    check(gl_track_frame_end(ctx_, &map_, &map_ba_, B, NF, NL, NPcap, &in, th_depth, rule, &out), "gl_track_frame_end");
  }
  // noteReplaced: FuseResult::repl_src / repl_tgt in step order into ptr_replaced_ as the device array mp_replaced (the rows of
  // setResidentMapCapacity, -1 = none; map.cpp:126).  Called beside mergeStats; the lists are copied before the call returns.
  void noteReplaced(int32_t* mp_replaced_dev, const std::vector<int32_t>& repl_src, const std::vector<int32_t>& repl_tgt) {
    const size_t n = repl_src.size();
    if (repl_tgt.size() != n) throw std::runtime_error("noteReplaced: lists of different lengths");
    if (!n) return;
    int32_t* d = pooled(14, 2 * n * 4).as<int32_t>();
    check(gl_memcpy_h2d(ctx_, d, repl_src.data(), n * 4), "h2d");
    check(gl_memcpy_h2d(ctx_, d + n, repl_tgt.data(), n * 4), "h2d");
    check(gl_map_note_replaced(ctx_, mp_cap_, mp_replaced_dev, d, d + n, (int)n, nullptr), "gl_map_note_replaced");
  }
  // nextFrame: Map::updateFrameInfo, the pose block of GMMLoc::processFrame, Tracking::updateLastFrame and the last-frame rows of the
  // next chain call, on the resident map as it is NOW (after the key-frame pass, if one ran).  in.mp_replaced, when given, has the rows
  // of setResidentMapCapacity (in.NMPcap is set here).  For a frame that is no key-frame gl_create_temporal_points follows on the rows
  // written here, with out.held_mp as its out->last_mp: a held == 2 slot it replaces gets -1 there (createTemporalPoints above works on
  // host vectors: its caller sets last_mp = -1 where the returned flag is set).
  void nextFrame(int B, int NF, gl_frame_next_in in, const gl_frame_next_out& out) {
    in.NMPcap = mp_cap_;
    check(gl_track_frame_next(ctx_, &map_, &map_ba_, B, NF, &in, &out), "gl_track_frame_next");
  }
  const gl_map_view& residentMap() const { return map_; }

  // ---- the covisibility graph on the device (gl_map_covis, gmmloc_hip.h): map_frame_weights_, ordered_keyframes_ and best_cov_kf_ of
  // every key-frame as caller-owned device arrays beside the resident map - the host mirrors no connection container, addConnection and
  // removeConnection included.  setResidentCovisibility: the tables (NKFcap rows of Wcap entries; a new row: cov_n = cov_nord = 0,
  // best_cov = -1).
  void setResidentCovisibility(const gl_map_covis& tables, int32_t Wcap) {
    cov_ = tables;
    cov_.Wcap = Wcap;
  }
  // updateConnectionsInMap: KeyFrame::updateConnections WITH its addConnection on the other rows (keyframe.cpp:243-316) for key-frame
  // kf_row, at processNewKeyFrame (localization.cpp:440) and at the end of searchInNeighbors (:223).  conn_kf / conn_w: the ordered list
  // (at most Ccap entries of n_conn).  status & GL_COVIS_W_TRUNCATED: the graph is untouched and `widest` is the Wcap the call needs -
  // re-stride cov_kf / cov_w, setResidentCovisibility, call again.  One synchronise.
  struct ConnectionsResult {
    int32_t n_conn = 0, widest = 0, status = 0, n_changed = 0;
    std::vector<int32_t> conn_kf, conn_w;
  };
  ConnectionsResult updateConnectionsInMap(int32_t kf_row, int32_t Ccap = 256) {
    const size_t C = (size_t)Ccap;
    char* b = pooled(15, 64 + 2 * C * 4).as<char>();
    int32_t* res = reinterpret_cast<int32_t*>(b);  // {result (4) | n_conn}
    int32_t* d_kf = reinterpret_cast<int32_t*>(b + 64);
    check(gl_covis_update(ctx_, &map_, &cov_, kf_row, Ccap, d_kf, d_kf + C, res + 4, res), "gl_covis_update");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t got[5];
    check(gl_memcpy_d2h(ctx_, got, res, 20), "d2h");
    ConnectionsResult r;
    r.widest = got[0], r.status = got[1], r.n_changed = got[2], r.n_conn = got[4];
    const size_t n = (size_t)std::min(got[4], Ccap);
    r.conn_kf.resize(n);
    r.conn_w.resize(n);
    if (n) {
      check(gl_memcpy_d2h(ctx_, r.conn_kf.data(), d_kf, n * 4), "d2h");
      check(gl_memcpy_d2h(ctx_, r.conn_w.data(), d_kf + C, n * 4), "d2h");
    }
    return r;
  }
  // removeFromGraph: the graph part of Map::removeKeyFrame (map.cpp:60-87) for cull_rows IN REMOVAL ORDER (CullResult::cull_rows), beside
  // the gl_map_remove that takes the same list.  best_cov[r] afterwards is where the host re-parents frame_info_ (:89-104).
  struct GraphRemoveResult {
    int32_t removed = 0, status = 0, erased = 0, malformed = 0;
    std::vector<int32_t> best_cov;  // per listed row, after the call
  };
  GraphRemoveResult removeFromGraph(const std::vector<int32_t>& cull_rows) {
    const size_t n = cull_rows.size();
    char* b = pooled(15, 64 + n * 4).as<char>();
    int32_t* res = reinterpret_cast<int32_t*>(b);
    int32_t* d_rows = reinterpret_cast<int32_t*>(b + 64);
    if (n) check(gl_memcpy_h2d(ctx_, d_rows, cull_rows.data(), n * 4), "h2d");
    check(gl_covis_remove(ctx_, map_.NKF, &cov_, map_ba_.kf_first, n ? d_rows : nullptr, nullptr, (int)n, res), "gl_covis_remove");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t got[4];
    check(gl_memcpy_d2h(ctx_, got, res, 16), "d2h");
    GraphRemoveResult r;
    r.removed = got[0], r.status = got[1], r.erased = got[2], r.malformed = got[3];
    r.best_cov.assign(n, -1);
    for (size_t i = 0; i < n; ++i)
      if (cull_rows[i] >= 0 && cull_rows[i] < map_.NKF) check(gl_memcpy_d2h(ctx_, &r.best_cov[i], cov_.best_cov + cull_rows[i], 4), "d2h");
    return r;
  }
  // bestCovisible: getBestCovisibilityKeyFrames(N) (keyframe.cpp:163-170; N <= 0: getVectorCovisibleKeyFrames) of key-frame kf_row.
  std::vector<int32_t> bestCovisible(int32_t kf_row, int32_t N, int32_t Ccap = 256) {
    const size_t C = (size_t)Ccap;
    char* b = pooled(15, 64 + 2 * C * 4).as<char>();
    int32_t* res = reinterpret_cast<int32_t*>(b);  // {result (4) | n_conn | kf_row}
    int32_t* d_kf = reinterpret_cast<int32_t*>(b + 64);
    check(gl_memcpy_h2d(ctx_, res + 5, &kf_row, 4), "h2d");
    check(gl_covis_best(ctx_, map_.NKF, &cov_, 1, res + 5, N, Ccap, d_kf, d_kf + C, res + 4, res), "gl_covis_best");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t n = 0;
    check(gl_memcpy_d2h(ctx_, &n, res + 4, 4), "d2h");
    std::vector<int32_t> out((size_t)std::min(std::max(n, 0), Ccap));
    if (!out.empty()) check(gl_memcpy_d2h(ctx_, out.data(), d_kf, out.size() * 4), "d2h");
    return out;
  }
  // searchInNeighborsInMap: the two lists of Localization::searchInNeighbors on the graph and the resident map - the target key-frames
  // (localization.cpp:155-179) in insertion order, and, called again with `reverse` once the host has run its forward fuses
  // (fuseObservationsInMap per target with the snapshot of kf_row's points), the candidates of the reverse fuse (:188-206) on the map
  // as it is then.  The fuses between the two stay the host's sequence of gl_project_map_points -> gl_fuse_search ->
  // fuseObservationsInMap, as INTEGRATION section 6 step 0.c lists it; updateConnectionsInMap(kf_row) closes the function.
  struct NeighborLists {
    int32_t status = 0;
    std::vector<int32_t> tgt_kf, cand_mp;
  };
  NeighborLists searchInNeighborsInMap(int32_t kf_row, int32_t kf_idx, bool reverse = false, int32_t nn = 10, int32_t nn2 = 5) {
    const size_t T = (size_t)nn + (size_t)nn * nn2, cap = reverse ? T * (size_t)map_.NFK : 0;
    char* b = pooled(15, 64 + (T + cap) * 4).as<char>();
    int32_t* res = reinterpret_cast<int32_t*>(b);  // {targets' result (4) | n_tgt | candidates' result (4) | n_cand}
    int32_t* d_tgt = reinterpret_cast<int32_t*>(b + 64);
    int32_t* d_cand = d_tgt + T;
    check(gl_fuse_targets(ctx_, map_.NKF, &cov_, map_.kf_valid, kf_row, nn, nn2, (int)T, d_tgt, res + 4, res), "gl_fuse_targets");
    if (reverse)
      check(gl_fuse_candidates(ctx_, &map_, d_tgt, res + 4, (int)T, kf_idx, (int)cap, cap ? d_cand : nullptr, res + 9, res + 5), "gl_fuse_candidates");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t got[10] = {0};
    check(gl_memcpy_d2h(ctx_, got, res, reverse ? 40 : 20), "d2h");
    NeighborLists r;
    r.status = got[1] | got[6];
    r.tgt_kf.resize((size_t)std::min<int32_t>(got[4], (int32_t)T));
    if (!r.tgt_kf.empty()) check(gl_memcpy_d2h(ctx_, r.tgt_kf.data(), d_tgt, r.tgt_kf.size() * 4), "d2h");
    r.cand_mp.resize(reverse ? (size_t)std::min<int64_t>(got[9], (int64_t)cap) : 0);
    if (!r.cand_mp.empty()) check(gl_memcpy_d2h(ctx_, r.cand_mp.data(), d_cand, r.cand_mp.size() * 4), "d2h");
    return r;
  }

  // ORBVocabulary::loadFromBinaryFile and ORBVocabulary::transform(descriptors, bow_vec, feat_vec, levelsup) (orb_vocabulary.cpp:20-40;
  // gmmloc_opt.cpp:25 for a key-frame, tracking.cpp:298 for a frame that falls back to trackKeyFrame) on the device: gl_voc_load_file /
  // gl_bow_transform.  Only the FeatureVector is made (bow_vec_ has no reader in gmmloc/).  loadVocabulary: false on failure like
  // loadGMMModel.  bowTransform: descriptors N x 32 bytes in feature order (N <= 4 096) -> the flattened feature vector of INTEGRATION
  // section 6 (node_id ascending; the features of node n are node_idx[node_ptr[n] .. node_ptr[n + 1])); one upload, one synchronise.
  bool loadVocabulary(const std::string& path) {
    if (voc_) gl_voc_destroy(voc_);
    voc_ = nullptr;
    return gl_voc_load_file(ctx_, path.c_str(), &voc_) == GL_OK;
  }
  struct FeatureVector {
    std::vector<int32_t> node_id, node_ptr, node_idx;
  };
  FeatureVector bowTransform(const std::vector<uint8_t>& descriptors, int levelsup = 4) {
    if (!voc_ || descriptors.size() % 32) throw std::runtime_error("bowTransform: loadVocabulary / descriptors of 32 bytes");
    FeatureVector fv;
    const size_t N = descriptors.size() / 32;
    fv.node_ptr.assign(1, 0);
    if (!N) return fv;
    size_t off = 64;  // {nnode at 0 | status at 4}
    auto take = [&off](size_t bytes) {
      const size_t at = off;
      off += (bytes + 63) / 64 * 64;
      return at;
    };
    const size_t o_desc = take(N * 32), o_id = take(N * 4), o_ptr = take((N + 1) * 4), o_idx = take(N * 4);
    char* b = pooled(12, off).as<char>();
    auto at = [b](size_t o) { return reinterpret_cast<int32_t*>(b + o); };
    check(gl_memcpy_h2d(ctx_, b + o_desc, descriptors.data(), N * 32), "h2d");
    gl_bow_out out{};
    out.nnode = at(0), out.status = at(4), out.node_id = at(o_id), out.node_ptr = at(o_ptr), out.node_idx = at(o_idx);
    check(gl_bow_transform(ctx_, voc_, levelsup, 1, (int)N, (int)N, reinterpret_cast<const uint8_t*>(b + o_desc), nullptr, &out), "gl_bow_transform");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t nnode = 0;
    check(gl_memcpy_d2h(ctx_, &nnode, b, 4), "d2h");  // (NNcap = N: never truncated)
    fv.node_id.resize(nnode);
    fv.node_ptr.resize((size_t)nnode + 1);
    if (nnode) check(gl_memcpy_d2h(ctx_, fv.node_id.data(), b + o_id, (size_t)nnode * 4), "d2h");
    check(gl_memcpy_d2h(ctx_, fv.node_ptr.data(), b + o_ptr, ((size_t)nnode + 1) * 4), "d2h");
    fv.node_idx.resize(fv.node_ptr[nnode]);
    if (!fv.node_idx.empty()) check(gl_memcpy_d2h(ctx_, fv.node_idx.data(), b + o_idx, fv.node_idx.size() * 4), "d2h");
    return fv;
  }
  // The feature vector of key-frame row kf_row written in place into the resident tables (setResidentKeyFrameTables: kf_desc[kf_row] is
  // read, kf_nnode / kf_node_id / kf_node_ptr / kf_node_idx [kf_row] are written; the padding slots are those of the resident kf_oct when
  // setResidentMap gave one).  Nothing is uploaded and nothing read back but the status word: GL_BOW_NODES_TRUNCATED when the key-frame
  // has more nodes than the tables' NNcap (its row is then untouched, kf_nnode[kf_row] holds the count needed).
  int32_t bowTransformIntoTables(int32_t kf_row, int levelsup = 4) {
    if (!voc_ || kf_row < 0 || kf_row >= map_.NKF || !kf_tables_.kf_desc)
      throw std::runtime_error("bowTransformIntoTables: loadVocabulary / kf_row / setResidentKeyFrameTables");
    const size_t NF = (size_t)map_.NFK, NN = (size_t)kf_tables_.NNcap, r = (size_t)kf_row;
    int32_t* status = pooled(13, 64).as<int32_t>();
    gl_bow_out out{};
    out.nnode = const_cast<int32_t*>(kf_tables_.kf_nnode) + r;
    out.node_id = const_cast<int32_t*>(kf_tables_.kf_node_id) + r * NN;
    out.node_ptr = const_cast<int32_t*>(kf_tables_.kf_node_ptr) + r * (NN + 1);
    out.node_idx = const_cast<int32_t*>(kf_tables_.kf_node_idx) + r * NF;
    out.status = status;
    check(gl_bow_transform(ctx_, voc_, levelsup, 1, (int)NF, (int)NN, kf_tables_.kf_desc + r * NF * 32, map_ba_.kf_oct ? map_ba_.kf_oct + r * NF : nullptr,
                           &out),
          "gl_bow_transform");
    check(gl_ctx_synchronize(ctx_), "sync");
    int32_t st = 0;
    check(gl_memcpy_d2h(ctx_, &st, status, 4), "d2h");
    return st;
  }
  gl_voc_t* vocabulary() { return voc_; }

  gl_ctx_t* ctx() { return ctx_; }
  gl_gmm_t* handle() { return gmm_; }
  gl_params& params() { return prm_; }
  const gl_camera& camera() const { return cam_; }

 private:
  void release() {
    pool_.clear();
    if (stage_ && ctx_) gl_free_host(ctx_, stage_);
    stage_ = nullptr;
    stage_bytes_ = 0;
    if (voc_) gl_voc_destroy(voc_);
    voc_ = nullptr;
    if (gmm_) gl_gmm_destroy(gmm_);
    if (ctx_) gl_ctx_destroy(ctx_);
    gmm_ = nullptr;
    ctx_ = nullptr;
  }
  DevBuf& pooled(size_t slot, size_t bytes) {
    if (pool_.size() <= slot) pool_.resize(slot + 1);
    if (!pool_[slot] || pool_[slot]->bytes() < bytes) pool_[slot].reset(new DevBuf(ctx_, bytes + bytes / 4 + 64));
    return *pool_[slot];
  }
  char* stage(size_t bytes) {  // page-locked, grown on demand
    if (stage_bytes_ < bytes) {
      if (stage_) gl_free_host(ctx_, stage_);
      stage_ = nullptr;
      stage_bytes_ = 0;
      void* p = nullptr;
      check(gl_malloc_host(ctx_, bytes + bytes / 4 + 64, &p), "gl_malloc_host");
      stage_ = static_cast<char*>(p);
      stage_bytes_ = bytes + bytes / 4 + 64;
    }
    return stage_;
  }
  // the slab of jointOptimizationFromMap in pooled buffer 2: {sizes (16) | status | iters | n_erase | pad | kf_row} in its first 64
  // bytes, then the arrays of gl_ba_window and the BA's outputs, each 64-byte aligned, at the capacities caps_
  char* carveWindow(gl_ba_window& w) {
    const size_t Pc = caps_[0], Fc = caps_[1], Lc = caps_[2], Oc = caps_[3];
    size_t off = 64;
    auto take = [&off](size_t bytes) {
      const size_t at = off;
      off += (bytes + 63) / 64 * 64;
      return at;
    };
    const size_t o_poses = take((Pc + Fc) * 56), o_prior = take(Pc), o_points = take(Lc * 24), o_assoc = take(Lc * 4), o_ptr = take((Lc + 1) * 4),
                 o_op = take(Oc * 4), o_uvr = take(Oc * 24), o_oct = take(Oc * 4), o_wkf = take((Pc + Fc) * 4), o_wmp = take(Lc * 4), o_wobs = take(Oc * 4);
    win_off_[0] = take(Lc);
    win_off_[1] = take(Oc);
    win_off_[2] = take(Oc * 4);
    char* b = pooled(2, off).as<char>();
    w.Pcap = (int32_t)Pc, w.Fcap = (int32_t)Fc, w.Lcap = (int32_t)Lc, w.Ocap = (int32_t)Oc;
    w.poses = reinterpret_cast<double*>(b + o_poses);
    w.prior = reinterpret_cast<uint8_t*>(b + o_prior);
    w.points = reinterpret_cast<double*>(b + o_points);
    w.assoc = reinterpret_cast<int32_t*>(b + o_assoc);
    w.obs_ptr = reinterpret_cast<int32_t*>(b + o_ptr);
    w.obs_pose = reinterpret_cast<int32_t*>(b + o_op);
    w.obs_uvr = reinterpret_cast<double*>(b + o_uvr);
    w.obs_oct = reinterpret_cast<int32_t*>(b + o_oct);
    w.win_kf = reinterpret_cast<int32_t*>(b + o_wkf);
    w.win_mp = reinterpret_cast<int32_t*>(b + o_wmp);
    w.win_obs = reinterpret_cast<int32_t*>(b + o_wobs);
    w.sizes = reinterpret_cast<int32_t*>(b);
    w.status = reinterpret_cast<int32_t*>(b + 16);
    return b;
  }
  gl_map_edit residentEdit(int32_t* mp_ref_kf_dev) const {
    gl_map_edit ed{};
    ed.mp_valid = const_cast<uint8_t*>(map_.mp_valid);
    ed.kf_valid = const_cast<uint8_t*>(map_.kf_valid);
    ed.kf_mp = const_cast<int32_t*>(map_.kf_mp);
    ed.obs_ptr = const_cast<int32_t*>(map_.obs_ptr);
    ed.obs_kf = const_cast<int32_t*>(map_.obs_kf);
    ed.obs_feat = const_cast<int32_t*>(map_ba_.obs_feat);
    ed.mp_ref_kf = mp_ref_kf_dev;
    return ed;
  }
  gl_map_view map_{};
  gl_map_ba_view map_ba_{};
  gl_map_kf_tables kf_tables_{};
  gl_map_stats stats_{};
  gl_map_covis cov_{};
  int32_t mp_cap_ = 0, obs_cap_ = 0;  // the rows of the per-point arrays, the entries of obs_kf / obs_feat
  size_t caps_[4] = {24, 24, 2048, 16384};  // Pcap, Fcap, Lcap, Ocap: grown on demand
  size_t win_off_[3] = {0, 0, 0};           // dropped, erase, erase_obs (consecutive)
  std::vector<uint8_t> zeros_;
  std::vector<std::unique_ptr<DevBuf>> pool_;
  char* stage_ = nullptr;
  size_t stage_bytes_ = 0;
  gl_ctx_t* ctx_ = nullptr;
  gl_gmm_t* gmm_ = nullptr;
  gl_voc_t* voc_ = nullptr;
  gl_params prm_;
  gl_camera cam_{};
};

// ---- the flattening a host needs for gl_update_local_map / gl_track_frame_chain_map (Tracking::updateLocalMap on the device,
// INTEGRATION 5c third form).  The map stays the host's: these helpers only turn its containers into the flat rows of gl_map_view.
// A "row" is the index the host gives a MapPoint* / KeyFrame* in its device arrays (e.g. the slot of gl_update_map_points' outputs).
struct MapRows {
  int32_t NMP = 0, NKF = 0, NFK = 0;
  std::vector<int32_t> kf_mp;            // NKF x NFK: KeyFrame::mappoints_[i] as a map-point row, -1 = null
  std::vector<int32_t> obs_ptr, obs_kf;  // MapPoint::observations_ as CSR over map-point rows (NMP + 1, NOBS)
  std::vector<uint8_t> mp_valid, kf_valid;  // !not_valid_
};
// point_row(k, i): row of key-frame k's i-th map point, or -1 (nullptr / slot i beyond the key-frame's features).  The CSR is made
// from the table itself (observations_[kf] = idx <=> kf->mappoints_[idx] == this, mappoint.cpp:40-60), key-frames ascending per
// point, so the two cannot disagree.  mp_is_valid(p), kf_is_valid(k): !not_valid_.
template <class PointRow, class MpValid, class KfValid>
inline MapRows flattenMap(int32_t NMP, int32_t NKF, int32_t NFK, PointRow point_row, MpValid mp_is_valid, KfValid kf_is_valid) {
  MapRows m;
  m.NMP = NMP;
  m.NKF = NKF;
  m.NFK = NFK;
  m.kf_mp.assign((size_t)NKF * NFK, -1);
  m.obs_ptr.assign((size_t)NMP + 1, 0);
  for (int32_t k = 0; k < NKF; ++k)
    for (int32_t i = 0; i < NFK; ++i) {
      const int32_t p = point_row(k, i);
      if (p < 0 || p >= NMP) continue;
      m.kf_mp[(size_t)k * NFK + i] = p;
      ++m.obs_ptr[(size_t)p + 1];
    }
  for (int32_t p = 0; p < NMP; ++p) m.obs_ptr[(size_t)p + 1] += m.obs_ptr[p];
  m.obs_kf.assign((size_t)m.obs_ptr[NMP], 0);
  std::vector<int32_t> at(m.obs_ptr.begin(), m.obs_ptr.end() - 1);
  for (int32_t k = 0; k < NKF; ++k)
    for (int32_t i = 0; i < NFK; ++i) {
      const int32_t p = m.kf_mp[(size_t)k * NFK + i];
      if (p >= 0) m.obs_kf[(size_t)at[p]++] = k;
    }
  m.mp_valid.resize(NMP);
  m.kf_valid.resize(NKF);
  for (int32_t p = 0; p < NMP; ++p) m.mp_valid[p] = mp_is_valid(p) ? 1 : 0;
  for (int32_t k = 0; k < NKF; ++k) m.kf_valid[k] = kf_is_valid(k) ? 1 : 0;
  return m;
}
// The rest of the resident map, what gl_ba_window_build / gl_ba_window_apply read and write besides MapRows (gl_map_ba_view): built
// ONCE from the host's containers, uploaded, and from then on maintained on the device by jointOptimizationFromMap (and by the host
// where it inserts or culls).  pose_of(k) -> Pose (getTcw()); feature(k, i, uvr, oct) fills features_[i].uv.x, uv.y, u_right
// (u_right < 0: monocular) and .octave of key-frame k, false for a slot beyond its features; assoc_of(p) -> the index of
// asscociations_[0] or -1; is_first(k): idx_ == 0.  obs_feat follows flattenMap's CSR (key-frames ascending per point), kf_twc is
// -(R^T t) by the expression gl_ba_window_apply uses (gmmloc_hip.h), so rows made here and rows written there agree to the bit.
struct MapBaRows {
  std::vector<double> kf_pose, kf_twc, kf_uvr;  // NKF x 7, NKF x 3, NKF x NFK x 3
  std::vector<int32_t> kf_oct, obs_feat, mp_assoc;  // NKF x NFK, NOBS, NMP
  int32_t kf_first = -1;
};
template <class PoseOf, class FeatureOf, class AssocOf, class IsFirst>
inline MapBaRows flattenMapBa(const MapRows& m, PoseOf pose_of, FeatureOf feature, AssocOf assoc_of, IsFirst is_first) {
  MapBaRows b;
  const size_t NKF = (size_t)m.NKF, NFK = (size_t)m.NFK;
  b.kf_pose.assign(NKF * 7, 0.0);
  b.kf_twc.assign(NKF * 3, 0.0);
  b.kf_uvr.assign(NKF * NFK * 3, -1.0);
  b.kf_oct.assign(NKF * NFK, 0);
  b.obs_feat.assign(m.obs_kf.size(), 0);
  b.mp_assoc.resize((size_t)m.NMP);
  std::vector<int32_t> at(m.obs_ptr.begin(), m.obs_ptr.end() - 1);
  for (size_t k = 0; k < NKF; ++k) {
    const Pose T = pose_of((int32_t)k);
    double* q = &b.kf_pose[k * 7];
    std::memcpy(q, &T, 56);
    const double n = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const double x = q[0] / n, y = q[1] / n, z = q[2] / n, w = q[3] / n, tx = q[4], ty = q[5], tz = q[6];
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                            {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                            {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    for (int c = 0; c < 3; ++c) b.kf_twc[k * 3 + c] = -((R[0][c] * tx + R[1][c] * ty) + R[2][c] * tz);
    if (is_first((int32_t)k)) b.kf_first = (int32_t)k;
    for (size_t i = 0; i < NFK; ++i) {
      double uvr[3] = {0.0, 0.0, -1.0};
      int32_t oct = 0;
      if (feature((int32_t)k, (int32_t)i, uvr, oct)) {
        std::memcpy(&b.kf_uvr[(k * NFK + i) * 3], uvr, 24);
        b.kf_oct[k * NFK + i] = oct;
      }
      const int32_t p = m.kf_mp[k * NFK + i];
      if (p >= 0) b.obs_feat[(size_t)at[p]++] = (int32_t)i;
    }
  }
  for (int32_t p = 0; p < m.NMP; ++p) b.mp_assoc[p] = assoc_of(p);
  return b;
}
// last_mp / kf_feat_mp of gl_local_map_io: the map-point row behind each of a frame's (the last frame's, the reference key-frame's)
// n features - row(i) < 0 for a feature without a map point AND for a temporal point (createTemporalPoints, tracking.cpp:44-46: it
// has no observations and no row in the map).
template <class Row>
inline std::vector<int32_t> featureRows(int32_t n, Row row) {
  std::vector<int32_t> r((size_t)n, -1);
  for (int32_t i = 0; i < n; ++i) {
    const int32_t p = row(i);
    r[i] = p < 0 ? -1 : p;
  }
  return r;
}

}  // namespace gmmloc_hip
