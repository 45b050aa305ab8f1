// Driver of tests/test_gpu_key_frame_create_adapter.py: the depth-ordered walks through the C++ host mirror
// (include/gmmloc_hip/gmm_adapter.hpp: createMapPointsFromStereo, createTemporalPoints, processKeyFrameInMap), plain C++17 over the C-ABI.
//   key_frame_create_check model.gmm scene.bin out.bin
// scene.bin: int32 {NMP, NKF, NFK, NOBS, NMPcap, OBScap, kf_first, kf_row, width, height}, double {fx, fy, cx, cy, bf}, float {th_depth}, then the
// resident arrays at their CAPACITIES - mp_valid (NMPcap u8), kf_valid (NKF u8), kf_mp (NKF x NFK i32), obs_ptr (NMPcap + 1 i32), obs_kf,
// obs_feat (OBScap i32), kf_pose (NKF x 7 f64), kf_twc (NKF x 3 f64), kf_uvr (NKF x NFK x 3 f64), kf_oct (NKF x NFK i32), mp_pos, mp_normal
// (NMPcap x 3 f64), mp_max_dist, mp_min_dist (NMPcap f32), mp_desc (NMPcap x 32 u8), mp_assoc, mp_ref_kf (NMPcap i32), kf_desc (NKF x NFK x
// 32 u8) - then the key-frame's depth (NFK f32), held, last_outlier (NFK u8) and the last-frame rows last_pt (NFK x 3 f64), last_observed,
// last_valid (NFK u8), last_desc (NFK x 32 u8).
// The sequence: createMapPointsFromStereo(features of row kf_row, mp_base = NMP) -> createTemporalPoints(the same features) ->
// processKeyFrameInMap(kf_row).
// out.bin: {n_new, stats[8]}, new_feat, new_assoc (n_new i32), new_pos (n_new x 3 f64), feat_new (NFK), cand (NFK x 5), ncand (NFK);
// temp_flag (NFK u8), last_pt, last_observed, last_valid, last_desc; {nmp, nobs, n_attached, n_skipped, status, n_new, stats[8]}, feat_new,
// cand, ncand; then the resident rows at their capacities: mp_valid, kf_valid, kf_mp, obs_ptr, obs_kf, obs_feat, mp_pos, mp_normal,
// mp_max_dist, mp_min_dist, mp_desc, mp_assoc, mp_ref_kf.
#include <cstdio>

#include "driver_io.hpp"

using namespace gmmloc_hip;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  GMM model;
  if (!load_model(argv[1], model)) return 1;
  std::ifstream in(argv[2], std::ios::binary);
  const auto hd = rd<int32_t>(in, 10);
  const auto cm = rd<double>(in, 5);
  const float th = rd<float>(in, 1)[0];
  const int32_t NMP = hd[0], NKF = hd[1], NFK = hd[2], NOBS = hd[3], NMPcap = hd[4], OBScap = hd[5], K = hd[7];
  const size_t nf = (size_t)NFK, cap = (size_t)NMPcap;
  const auto mp_valid = rd<uint8_t>(in, cap), kf_valid = rd<uint8_t>(in, NKF);
  const auto kf_mp = rd<int32_t>(in, (size_t)NKF * nf), obs_ptr = rd<int32_t>(in, cap + 1), obs_kf = rd<int32_t>(in, OBScap), obs_feat = rd<int32_t>(in, OBScap);
  const auto kf_pose = rd<double>(in, (size_t)NKF * 7), kf_twc = rd<double>(in, (size_t)NKF * 3), kf_uvr = rd<double>(in, (size_t)NKF * nf * 3);
  const auto kf_oct = rd<int32_t>(in, (size_t)NKF * nf);
  const auto mp_pos = rd<double>(in, cap * 3), mp_normal = rd<double>(in, cap * 3);
  const auto mp_max = rd<float>(in, cap), mp_min = rd<float>(in, cap);
  const auto mp_desc = rd<uint8_t>(in, cap * 32);
  const auto mp_assoc = rd<int32_t>(in, cap), mp_ref_kf = rd<int32_t>(in, cap);
  const auto kf_desc = rd<uint8_t>(in, (size_t)NKF * nf * 32);
  const auto depth = rd<float>(in, nf);
  const auto held = rd<uint8_t>(in, nf), last_outlier = rd<uint8_t>(in, nf);
  GMM::LastFrameRows rows;
  rows.last_pt = rd<double>(in, nf * 3);
  rows.last_observed = rd<uint8_t>(in, nf);
  rows.last_valid = rd<uint8_t>(in, nf);
  rows.last_desc = rd<uint8_t>(in, nf * 32);
  if (!in) return 3;
  gl_camera cam{};
  cam.fx = cm[0], cam.fy = cm[1], cam.cx = cm[2], cam.cy = cm[3], cam.bf = cm[4], cam.width = hd[8], cam.height = hd[9];
  model.setCamera(cam);
  gl_ctx_t* ctx = model.ctx();

  GMM::FrameFeatures f;
  std::memcpy(&f.Tcw, kf_pose.data() + (size_t)K * 7, 56);
  f.uv.resize(nf * 2), f.ur.resize(nf);
  for (size_t i = 0; i < nf; ++i) {
    const double* u = kf_uvr.data() + ((size_t)K * nf + i) * 3;
    f.uv[i * 2] = u[0], f.uv[i * 2 + 1] = u[1], f.ur[i] = (float)u[2];
  }
  f.depth = depth, f.held = held;
  f.oct.assign(kf_oct.begin() + (size_t)K * nf, kf_oct.begin() + (size_t)(K + 1) * nf);
  std::ofstream out(argv[3], std::ios::binary);
  const GMM::StereoPoints sp = model.createMapPointsFromStereo(f, K, NMP, true, th);
  wr(out, std::vector<int32_t>{sp.n_new});
  wr(out, std::vector<int32_t>(sp.stats, sp.stats + 8));
  wr(out, sp.new_feat), wr(out, sp.new_assoc), wr(out, sp.new_pos), wr(out, sp.feat_new), wr(out, sp.cand), wr(out, sp.ncand);

  const std::vector<uint8_t> desc_row(kf_desc.begin() + (size_t)K * nf * 32, kf_desc.begin() + (size_t)(K + 1) * nf * 32);
  const std::vector<uint8_t> flag = model.createTemporalPoints(f, last_outlier, desc_row, th, rows);
  wr(out, flag), wr(out, rows.last_pt), wr(out, rows.last_observed), wr(out, rows.last_valid), wr(out, rows.last_desc);

  gl_map_view v{};
  v.NMP = NMP, v.NKF = NKF, v.NFK = NFK, v.NOBS = NOBS;
  v.mp_valid = up(ctx, mp_valid);
  v.obs_ptr = up(ctx, obs_ptr);
  v.obs_kf = up(ctx, obs_kf);
  v.kf_valid = up(ctx, kf_valid);
  v.kf_mp = up(ctx, kf_mp);
  v.mp_pos = up(ctx, mp_pos);
  v.mp_normal = up(ctx, mp_normal);
  v.mp_max_dist = up(ctx, mp_max);
  v.mp_min_dist = up(ctx, mp_min);
  v.mp_desc = up(ctx, mp_desc);
  gl_map_ba_view w{};
  w.kf_pose = up(ctx, kf_pose);
  w.kf_twc = up(ctx, kf_twc);
  w.kf_uvr = up(ctx, kf_uvr);
  w.kf_oct = up(ctx, kf_oct);
  w.obs_feat = up(ctx, obs_feat);
  w.mp_assoc = up(ctx, mp_assoc);
  w.kf_first = hd[6];
  int32_t* ref_dev = up(ctx, mp_ref_kf);
  GMM::KeyFrameRowsDev d{};
  d.uv = up(ctx, f.uv), d.ur = up(ctx, f.ur), d.depth = up(ctx, depth), d.held = up(ctx, held), d.kf_desc = up(ctx, kf_desc);
  model.setResidentMap(v, w);
  model.setResidentMapCapacity(NMPcap, OBScap);
  const GMM::KeyFrameResult r = model.processKeyFrameInMap(K, d, true, th, ref_dev);
  wr(out, std::vector<int32_t>{r.nmp, r.nobs, r.n_attached, r.n_skipped, r.status, r.n_new});
  wr(out, std::vector<int32_t>(r.stats, r.stats + 8));
  wr(out, r.feat_new);
  wr(out, down(ctx, r.cand_dev, nf * 5)), wr(out, down(ctx, r.ncand_dev, nf));
  if (model.residentMap().NMP != r.nmp || model.residentMap().NOBS != r.nobs) return 5;
  std::printf("stereo: %d new points of %d entries (%d rejected, broke %d); map: %d -> %d points, %d -> %d entries, %d attached\n", sp.n_new, sp.stats[0],
              sp.stats[3], sp.stats[5], NMP, r.nmp, NOBS, r.nobs, r.n_attached);
  wr(out, down(ctx, v.mp_valid, cap)), wr(out, down(ctx, v.kf_valid, (size_t)NKF)), wr(out, down(ctx, v.kf_mp, (size_t)NKF * nf));
  wr(out, down(ctx, v.obs_ptr, cap + 1)), wr(out, down(ctx, v.obs_kf, (size_t)OBScap)), wr(out, down(ctx, w.obs_feat, (size_t)OBScap));
  wr(out, down(ctx, v.mp_pos, cap * 3)), wr(out, down(ctx, v.mp_normal, cap * 3)), wr(out, down(ctx, v.mp_max_dist, cap)), wr(out, down(ctx, v.mp_min_dist, cap));
  wr(out, down(ctx, v.mp_desc, cap * 32)), wr(out, down(ctx, (const int32_t*)w.mp_assoc, cap)), wr(out, down(ctx, (const int32_t*)ref_dev, cap));
  return out ? 0 : 4;
}
