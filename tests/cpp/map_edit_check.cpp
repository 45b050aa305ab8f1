// Driver of tests/test_gpu_map_edit_adapter.py: the edits of the resident map through the C++ host mirror
// (include/gmmloc_hip/gmm_adapter.hpp: setResidentMap, removeFromMap, cullKeyFrames), plain C++17 over the C-ABI.
//   map_edit_check model.gmm scene.bin out.bin
// scene.bin: int32 {NMP, NKF, NFK, NOBS, kf_row, kf_first, n_erase, n_rm_mp}, float {th_depth}, then mp_valid (NMP u8), kf_valid (NKF u8),
// kf_mp (NKF x NFK i32), obs_ptr (NMP + 1 i32), obs_kf, obs_feat (NOBS i32), kf_uvr (NKF x NFK x 3 f64), kf_oct (NKF x NFK i32), kf_depth
// (NKF x NFK f32), mp_ref_kf (NMP i32), erase_obs (n_erase i32), rm_mp (n_rm_mp i32).
// The sequence: removeFromMap(erase_obs, {}, rm_mp) -> cullKeyFrames(kf_row) -> removeFromMap({}, cull_rows).
// out.bin: {nobs, status, n_dead} + dead_mp of the first removal; {n_cand, n_cull} + cand, cull, num_mps, num_redundant, cand_status,
// cull_rows; {nobs, status, n_dead} + dead_mp of the second; then the resident rows, downloaded: mp_valid, kf_valid, kf_mp, obs_ptr,
// obs_kf, obs_feat (the new NOBS of them), mp_ref_kf.
#include <cstdio>

#include "driver_io.hpp"

using namespace gmmloc_hip;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  GMM model;
  if (!load_model(argv[1], model)) return 1;
  std::ifstream in(argv[2], std::ios::binary);
  const auto hd = rd<int32_t>(in, 8);
  const float th_depth = rd<float>(in, 1)[0];
  const int32_t NMP = hd[0], NKF = hd[1], NFK = hd[2], NOBS = hd[3], kf_row = hd[4], kf_first = hd[5];
  const auto mp_valid = rd<uint8_t>(in, NMP), kf_valid = rd<uint8_t>(in, NKF);
  const auto kf_mp = rd<int32_t>(in, (size_t)NKF * NFK), obs_ptr = rd<int32_t>(in, (size_t)NMP + 1), obs_kf = rd<int32_t>(in, NOBS), obs_feat = rd<int32_t>(in, NOBS);
  const auto kf_uvr = rd<double>(in, (size_t)NKF * NFK * 3);
  const auto kf_oct = rd<int32_t>(in, (size_t)NKF * NFK);
  const auto kf_depth = rd<float>(in, (size_t)NKF * NFK);
  const auto mp_ref_kf = rd<int32_t>(in, NMP), erase_obs = rd<int32_t>(in, hd[6]), rm_mp = rd<int32_t>(in, hd[7]);
  if (!in) return 3;
  gl_ctx_t* ctx = model.ctx();
  gl_map_view v{};
  v.NMP = NMP, v.NKF = NKF, v.NFK = NFK, v.NOBS = NOBS;
  v.mp_valid = up(ctx, mp_valid);
  v.obs_ptr = up(ctx, obs_ptr);
  v.obs_kf = up(ctx, obs_kf);
  v.kf_valid = up(ctx, kf_valid);
  v.kf_mp = up(ctx, kf_mp);
  gl_map_ba_view w{};
  w.kf_uvr = up(ctx, kf_uvr);
  w.kf_oct = up(ctx, kf_oct);
  w.obs_feat = up(ctx, obs_feat);
  w.kf_first = kf_first;
  float* depth_dev = up(ctx, kf_depth);
  int32_t* ref_dev = up(ctx, mp_ref_kf);
  model.setResidentMap(v, w);
  std::ofstream out(argv[3], std::ios::binary);
  const GMM::RemoveResult e = model.removeFromMap(erase_obs, {}, rm_mp, ref_dev);
  wr(out, std::vector<int32_t>{e.nobs, e.status, (int32_t)e.dead_mp.size()});
  wr(out, e.dead_mp);
  const GMM::CullResult c = model.cullKeyFrames(kf_row, depth_dev, th_depth);
  wr(out, std::vector<int32_t>{(int32_t)c.cand.size(), (int32_t)c.cull_rows.size()});
  wr(out, c.cand);
  wr(out, c.cull);
  wr(out, c.num_mps);
  wr(out, c.num_redundant);
  wr(out, c.cand_status);
  wr(out, c.cull_rows);
  const GMM::RemoveResult k = model.removeFromMap({}, c.cull_rows, {}, ref_dev);
  wr(out, std::vector<int32_t>{k.nobs, k.status, (int32_t)k.dead_mp.size()});
  wr(out, k.dead_mp);
  std::printf("erase: nobs %d -> %d, %zu dead; %zu candidates, %zu culled; remove: nobs %d, %zu dead\n", NOBS, e.nobs, e.dead_mp.size(), c.cand.size(),
              c.cull_rows.size(), k.nobs, k.dead_mp.size());
  if (model.residentMap().NOBS != k.nobs) return 5;
  wr(out, down(ctx, v.mp_valid, (size_t)NMP));
  wr(out, down(ctx, v.kf_valid, (size_t)NKF));
  wr(out, down(ctx, v.kf_mp, (size_t)NKF * NFK));
  wr(out, down(ctx, v.obs_ptr, (size_t)NMP + 1));
  wr(out, down(ctx, v.obs_kf, (size_t)k.nobs));
  wr(out, down(ctx, w.obs_feat, (size_t)k.nobs));
  wr(out, down(ctx, ref_dev, (size_t)NMP));
  return out ? 0 : 4;
}
