// Driver of tests/test_gpu_map_stats_adapter.py: the found / visible counters and removeMapPoints through the C++ host mirror
// (include/gmmloc_hip/gmm_adapter.hpp: setResidentMapStats, trackStats, mergeStats, growStats, removeMapPointsInMap), plain C++17 over
// the C-ABI.
//   map_stats_check model.gmm scene.bin out.bin
// scene.bin: int32 {NMP, NKF, NFK, NOBS, kf_row, kf_first, NMPcap, cand_cap, n_cand, B, NF, NPcap, n_merge, n_new, n_already, has_kf_idx},
// then mp_valid (NMP u8), kf_valid (NKF u8), kf_mp (NKF x NFK i32), obs_ptr (NMP + 1 i32), obs_kf, obs_feat (NOBS i32), kf_uvr
// (NKF x NFK x 3 f64), kf_oct (NKF x NFK i32), mp_ref_kf (NMP i32); visible, found, ref_idx (NMPcap i32), kf_idx (NKF i32), cand
// (cand_cap i32); the tracker's arrays feat_mp, match_local (B x NF i32), outlier (B x NF u8), inview (B x NPcap u8), local_mp
// (B x NPcap i32), n_local_mp (B i32), counts2 (B x 4 i32); repl_src, repl_tgt (n_merge i32); new_ref_kf (n_new i32), already_mp
// (n_already i32).
// The sequence: trackStats -> mergeStats -> growStats(first = NMP, the new rows are candidates) -> removeMapPointsInMap(kf_row).
// out.bin: {status, n_cand} of growStats; {kept, removed, erased, status} + verdict + rm_mp; {nobs, status, n_dead} + dead_mp; then,
// downloaded: visible, found, ref_idx (NMPcap), n_cand + cand (cand_cap), mp_valid, kf_mp, obs_ptr, obs_kf, obs_feat (the new NOBS of
// them), mp_ref_kf.
#include <cstdio>

#include "driver_io.hpp"

using namespace gmmloc_hip;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  GMM model;
  if (!load_model(argv[1], model)) return 1;
  std::ifstream in(argv[2], std::ios::binary);
  const auto hd = rd<int32_t>(in, 16);
  const int32_t NMP = hd[0], NKF = hd[1], NFK = hd[2], NOBS = hd[3], kf_row = hd[4], kf_first = hd[5], NMPcap = hd[6], cand_cap = hd[7], n_cand = hd[8];
  const int32_t B = hd[9], NF = hd[10], NPcap = hd[11], n_merge = hd[12], n_new = hd[13], n_already = hd[14];
  const auto mp_valid = rd<uint8_t>(in, NMP), kf_valid = rd<uint8_t>(in, NKF);
  const auto kf_mp = rd<int32_t>(in, (size_t)NKF * NFK), obs_ptr = rd<int32_t>(in, (size_t)NMP + 1), obs_kf = rd<int32_t>(in, NOBS), obs_feat = rd<int32_t>(in, NOBS);
  const auto kf_uvr = rd<double>(in, (size_t)NKF * NFK * 3);
  const auto kf_oct = rd<int32_t>(in, (size_t)NKF * NFK);
  const auto mp_ref_kf = rd<int32_t>(in, NMP);
  const auto visible = rd<int32_t>(in, NMPcap), found = rd<int32_t>(in, NMPcap), ref_idx = rd<int32_t>(in, NMPcap), kf_idx = rd<int32_t>(in, NKF);
  const auto cand = rd<int32_t>(in, cand_cap);
  const auto feat_mp = rd<int32_t>(in, (size_t)B * NF), match_local = rd<int32_t>(in, (size_t)B * NF);
  const auto outlier = rd<uint8_t>(in, (size_t)B * NF), inview = rd<uint8_t>(in, (size_t)B * NPcap);
  const auto local_mp = rd<int32_t>(in, (size_t)B * NPcap), n_local_mp = rd<int32_t>(in, B), counts2 = rd<int32_t>(in, (size_t)B * 4);
  const auto repl_src = rd<int32_t>(in, n_merge), repl_tgt = rd<int32_t>(in, n_merge);
  const auto new_ref_kf = rd<int32_t>(in, n_new), already_mp = rd<int32_t>(in, n_already);
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
  int32_t* ref_dev = up(ctx, mp_ref_kf);
  gl_map_stats st{};
  st.mp_visible = up(ctx, visible);
  st.mp_found = up(ctx, found);
  st.mp_ref_idx = up(ctx, ref_idx);
  st.kf_idx = hd[15] ? up(ctx, kf_idx) : nullptr;
  st.cand = up(ctx, cand);
  st.n_cand = up(ctx, std::vector<int32_t>{n_cand});
  st.cand_cap = cand_cap;
  model.setResidentMap(v, w);
  model.setResidentMapCapacity(NMPcap, NOBS);  // (the counters' rows: nothing is added to the map's own arrays here)
  model.setResidentMapStats(st);
  std::ofstream out(argv[3], std::ios::binary);
  model.trackStats(B, NF, NPcap, up(ctx, feat_mp), up(ctx, match_local), up(ctx, outlier), up(ctx, inview), up(ctx, local_mp), up(ctx, n_local_mp),
                   up(ctx, counts2));
  model.mergeStats(repl_src, repl_tgt);
  const GMM::GrowStatsResult g = model.growStats(NMP, new_ref_kf, already_mp, true);
  wr(out, std::vector<int32_t>{g.status, g.n_cand});
  const GMM::RemoveMapPointsResult r = model.removeMapPointsInMap(kf_row, ref_dev);
  wr(out, std::vector<int32_t>{r.kept, r.removed, r.erased, r.status});
  wr(out, r.verdict);
  wr(out, r.rm_mp);
  wr(out, std::vector<int32_t>{r.remove.nobs, r.remove.status, (int32_t)r.remove.dead_mp.size()});
  wr(out, r.remove.dead_mp);
  std::printf("grow: status %d, %d candidates; cull: %d kept, %d removed, %d erased; nobs %d -> %d\n", g.status, g.n_cand, r.kept, r.removed, r.erased, NOBS,
              r.remove.nobs);
  if (model.residentMap().NOBS != r.remove.nobs) return 5;
  wr(out, down(ctx, st.mp_visible, (size_t)NMPcap));
  wr(out, down(ctx, st.mp_found, (size_t)NMPcap));
  wr(out, down(ctx, st.mp_ref_idx, (size_t)NMPcap));
  wr(out, down(ctx, st.n_cand, 1));
  wr(out, down(ctx, st.cand, (size_t)cand_cap));
  wr(out, down(ctx, v.mp_valid, (size_t)NMP));
  wr(out, down(ctx, v.kf_mp, (size_t)NKF * NFK));
  wr(out, down(ctx, v.obs_ptr, (size_t)NMP + 1));
  wr(out, down(ctx, v.obs_kf, (size_t)r.remove.nobs));
  wr(out, down(ctx, w.obs_feat, (size_t)r.remove.nobs));
  wr(out, down(ctx, ref_dev, (size_t)NMP));
  return out ? 0 : 4;
}
