// Driver of tests/test_gpu_create_points_adapter.py: createMapPoints on the resident map through the C++ host mirror
// (include/gmmloc_hip/gmm_adapter.hpp: setResidentKeyFrameTables, createMapPointsInMap), plain C++17 over the C-ABI.
//   create_points_check model.gmm scene.bin out.bin
// scene.bin: int32 {NMP, NKF, NFK, NOBS, NMPcap, OBScap, kf_first, kf_row, width, height, nn, NNcap, k}, double {fx, fy, cx, cy, bf}, float {mb},
// then the resident arrays at their CAPACITIES - mp_valid (NMPcap u8), kf_valid (NKF u8), kf_mp (NKF x NFK i32), obs_ptr (NMPcap + 1 i32), obs_kf,
// obs_feat (OBScap i32), kf_pose (NKF x 7 f64), kf_twc (NKF x 3 f64), kf_uvr (NKF x NFK x 3 f64), kf_oct (NKF x NFK i32), mp_pos, mp_normal
// (NMPcap x 3 f64), mp_max_dist, mp_min_dist (NMPcap f32), mp_desc (NMPcap x 32 u8), mp_assoc, mp_ref_kf (NMPcap i32) - then the key-frame
// tables of gl_map_kf_tables: kf_angle (NKF x NFK f32), kf_desc (NKF x NFK x 32 u8), kf_depth (NKF x NFK f32), kf_nnode (NKF i32), kf_node_id
// (NKF x NNcap), kf_node_ptr (NKF x (NNcap + 1)), kf_node_idx (NKF x NFK), kf_cand (NKF x NFK x k), kf_ncand (NKF x NFK).
// out.bin: {nmp, nobs, n_attached, n_skipped, status, n_new, tri_status}, new_type, new_nb (n_new i32), feat_new (NFK), nb_stats (nn x 8); then
// the resident rows at their capacities: mp_valid, kf_valid, kf_mp, obs_ptr, obs_kf, obs_feat, mp_pos, mp_normal, mp_max_dist, mp_min_dist,
// mp_desc, mp_assoc, mp_ref_kf.
#include <cstdio>

#include "driver_io.hpp"

using namespace gmmloc_hip;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  GMM model;
  if (!load_model(argv[1], model)) return 1;
  std::ifstream in(argv[2], std::ios::binary);
  const auto hd = rd<int32_t>(in, 13);
  const auto cm = rd<double>(in, 5);
  const float mb = rd<float>(in, 1)[0];
  const int32_t NMP = hd[0], NKF = hd[1], NFK = hd[2], NOBS = hd[3], NMPcap = hd[4], OBScap = hd[5], K = hd[7], nn = hd[10], NNcap = hd[11], kc = hd[12];
  const size_t nf = (size_t)NFK, cap = (size_t)NMPcap, nkf = (size_t)NKF;
  const auto mp_valid = rd<uint8_t>(in, cap), kf_valid = rd<uint8_t>(in, nkf);
  const auto kf_mp = rd<int32_t>(in, nkf * nf), obs_ptr = rd<int32_t>(in, cap + 1), obs_kf = rd<int32_t>(in, OBScap), obs_feat = rd<int32_t>(in, OBScap);
  const auto kf_pose = rd<double>(in, nkf * 7), kf_twc = rd<double>(in, nkf * 3), kf_uvr = rd<double>(in, nkf * nf * 3);
  const auto kf_oct = rd<int32_t>(in, nkf * nf);
  const auto mp_pos = rd<double>(in, cap * 3), mp_normal = rd<double>(in, cap * 3);
  const auto mp_max = rd<float>(in, cap), mp_min = rd<float>(in, cap);
  const auto mp_desc = rd<uint8_t>(in, cap * 32);
  const auto mp_assoc = rd<int32_t>(in, cap), mp_ref_kf = rd<int32_t>(in, cap);
  const auto kf_angle = rd<float>(in, nkf * nf);
  const auto kf_desc = rd<uint8_t>(in, nkf * nf * 32);
  const auto kf_depth = rd<float>(in, nkf * nf);
  const auto kf_nnode = rd<int32_t>(in, nkf), kf_node_id = rd<int32_t>(in, nkf * NNcap), kf_node_ptr = rd<int32_t>(in, nkf * (NNcap + 1));
  const auto kf_node_idx = rd<int32_t>(in, nkf * nf), kf_cand = rd<int32_t>(in, nkf * nf * kc), kf_ncand = rd<int32_t>(in, nkf * nf);
  if (!in) return 3;
  gl_camera cam{};
  cam.fx = cm[0], cam.fy = cm[1], cam.cx = cm[2], cam.cy = cm[3], cam.bf = cm[4], cam.width = hd[8], cam.height = hd[9];
  model.setCamera(cam);
  gl_ctx_t* ctx = model.ctx();

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
  gl_map_kf_tables t{};
  t.kf_angle = up(ctx, kf_angle), t.kf_desc = up(ctx, kf_desc), t.kf_depth = up(ctx, kf_depth), t.kf_nnode = up(ctx, kf_nnode);
  t.kf_node_id = up(ctx, kf_node_id), t.kf_node_ptr = up(ctx, kf_node_ptr), t.kf_node_idx = up(ctx, kf_node_idx);
  t.kf_cand = up(ctx, kf_cand), t.kf_ncand = up(ctx, kf_ncand);
  t.NNcap = NNcap, t.k = kc;
  model.setResidentMap(v, w);
  model.setResidentMapCapacity(NMPcap, OBScap);
  model.setResidentKeyFrameTables(t);
  const GMM::CreatePointsResult r = model.createMapPointsInMap(K, nn, mb, ref_dev);
  std::ofstream out(argv[3], std::ios::binary);
  wr(out, std::vector<int32_t>{r.nmp, r.nobs, r.n_attached, r.n_skipped, r.status, r.n_new, r.tri_status});
  wr(out, r.new_type), wr(out, r.new_nb), wr(out, r.feat_new), wr(out, r.nb_stats);
  if (model.residentMap().NMP != r.nmp || model.residentMap().NOBS != r.nobs) return 5;
  std::printf("createMapPoints: %d new points over %d neighbours; map: %d -> %d points, %d -> %d entries, %d attached\n", r.n_new, nn, NMP, r.nmp, NOBS,
              r.nobs, r.n_attached);
  wr(out, down(ctx, v.mp_valid, cap)), wr(out, down(ctx, v.kf_valid, nkf)), wr(out, down(ctx, v.kf_mp, nkf * nf));
  wr(out, down(ctx, v.obs_ptr, cap + 1)), wr(out, down(ctx, v.obs_kf, (size_t)OBScap)), wr(out, down(ctx, w.obs_feat, (size_t)OBScap));
  wr(out, down(ctx, v.mp_pos, cap * 3)), wr(out, down(ctx, v.mp_normal, cap * 3)), wr(out, down(ctx, v.mp_max_dist, cap)), wr(out, down(ctx, v.mp_min_dist, cap));
  wr(out, down(ctx, v.mp_desc, cap * 32)), wr(out, down(ctx, (const int32_t*)w.mp_assoc, cap)), wr(out, down(ctx, (const int32_t*)ref_dev, cap));
  return out ? 0 : 4;
}
