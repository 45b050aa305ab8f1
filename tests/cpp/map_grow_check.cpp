// Driver of tests/test_gpu_map_grow_adapter.py: what adds to the resident map through the C++ host mirror
// (include/gmmloc_hip/gmm_adapter.hpp: setResidentMap, setResidentMapCapacity, addToMap, fuseObservationsInMap), plain C++17 over the
// C-ABI.
//   map_grow_check model.gmm scene.bin out.bin
// scene.bin: int32 {NMP, NKF, NFK, NOBS, NMPcap, OBScap, kf_first, n_new, n_new_kf, n_attach, n_walk, fuse_kf, n_cand}, then the arrays
// at their CAPACITIES - mp_valid (NMPcap u8), kf_valid (NKF u8), kf_mp (NKF x NFK i32), obs_ptr (NMPcap + 1 i32), obs_kf, obs_feat
// (OBScap i32), kf_uvr (NKF x NFK x 3 f64), mp_pos (NMPcap x 3 f64), mp_assoc, mp_ref_kf (NMPcap i32) - then the lists: new_pos
// (n_new x 3 f64), new_assoc, new_ref_kf (n_new i32), new_kf, att_mp, att_kf, att_feat, walk_kf, cand_mp, best_idx (i32).
// The sequence: addToMap(lists) -> fuseObservationsInMap(fuse_kf, cand_mp, best_idx).
// out.bin: {nmp, nobs, n_attached, n_skipped, n_already, status} + already_mp; {nobs, n_fused, n_attached, n_replaced, status} +
// repl_src + repl_tgt; then the resident rows, downloaded at their capacities: mp_valid, kf_valid, kf_mp, obs_ptr, obs_kf, obs_feat,
// mp_pos, mp_assoc, mp_ref_kf.
#include <cstdio>

#include "driver_io.hpp"

using namespace gmmloc_hip;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  GMM model;
  if (!load_model(argv[1], model)) return 1;
  std::ifstream in(argv[2], std::ios::binary);
  const auto hd = rd<int32_t>(in, 13);
  const int32_t NMP = hd[0], NKF = hd[1], NFK = hd[2], NOBS = hd[3], NMPcap = hd[4], OBScap = hd[5];
  const size_t n_new = (size_t)hd[7], n_att = (size_t)hd[9], n_cand = (size_t)hd[12];
  const auto mp_valid = rd<uint8_t>(in, NMPcap), kf_valid = rd<uint8_t>(in, NKF);
  const auto kf_mp = rd<int32_t>(in, (size_t)NKF * NFK), obs_ptr = rd<int32_t>(in, (size_t)NMPcap + 1), obs_kf = rd<int32_t>(in, OBScap),
             obs_feat = rd<int32_t>(in, OBScap);
  const auto kf_uvr = rd<double>(in, (size_t)NKF * NFK * 3), mp_pos = rd<double>(in, (size_t)NMPcap * 3);
  const auto mp_assoc = rd<int32_t>(in, NMPcap), mp_ref_kf = rd<int32_t>(in, NMPcap);
  GMM::AddLists l;
  l.new_pos = rd<double>(in, n_new * 3);
  l.new_assoc = rd<int32_t>(in, n_new);
  l.new_ref_kf = rd<int32_t>(in, n_new);
  l.new_kf = rd<int32_t>(in, (size_t)hd[8]);
  l.att_mp = rd<int32_t>(in, n_att);
  l.att_kf = rd<int32_t>(in, n_att);
  l.att_feat = rd<int32_t>(in, n_att);
  l.walk_kf = rd<int32_t>(in, (size_t)hd[10]);
  const auto cand_mp = rd<int32_t>(in, n_cand), best_idx = rd<int32_t>(in, n_cand);
  if (!in) return 3;
  gl_ctx_t* ctx = model.ctx();
  gl_map_view v{};
  v.NMP = NMP, v.NKF = NKF, v.NFK = NFK, v.NOBS = NOBS;
  v.mp_valid = up(ctx, mp_valid);
  v.obs_ptr = up(ctx, obs_ptr);
  v.obs_kf = up(ctx, obs_kf);
  v.kf_valid = up(ctx, kf_valid);
  v.kf_mp = up(ctx, kf_mp);
  v.mp_pos = up(ctx, mp_pos);
  gl_map_ba_view w{};
  w.kf_uvr = up(ctx, kf_uvr);
  w.obs_feat = up(ctx, obs_feat);
  w.mp_assoc = up(ctx, mp_assoc);
  w.kf_first = hd[6];
  int32_t* ref_dev = up(ctx, mp_ref_kf);
  int32_t* best_dev = up(ctx, best_idx);
  model.setResidentMap(v, w);
  model.setResidentMapCapacity(NMPcap, OBScap);
  std::ofstream out(argv[3], std::ios::binary);
  const GMM::AddResult a = model.addToMap(l, ref_dev);
  wr(out, std::vector<int32_t>{a.nmp, a.nobs, a.n_attached, a.n_skipped, (int32_t)a.already_mp.size(), a.status});
  wr(out, a.already_mp);
  if (model.residentMap().NMP != a.nmp || model.residentMap().NOBS != a.nobs) return 5;
  const GMM::FuseResult f = model.fuseObservationsInMap(hd[11], cand_mp, best_dev);
  wr(out, std::vector<int32_t>{f.nobs, f.n_fused, f.n_attached, (int32_t)f.repl_src.size(), f.status});
  wr(out, f.repl_src);
  wr(out, f.repl_tgt);
  if (model.residentMap().NOBS != f.nobs) return 5;
  std::printf("add: %d -> %d points, %d -> %d entries, %d attached, %d skipped, %zu already; fuse: %d entries, %d fused, %d attached, %zu replaced\n", NMP,
              a.nmp, NOBS, a.nobs, a.n_attached, a.n_skipped, a.already_mp.size(), f.nobs, f.n_fused, f.n_attached, f.repl_src.size());
  wr(out, down(ctx, v.mp_valid, (size_t)NMPcap));
  wr(out, down(ctx, v.kf_valid, (size_t)NKF));
  wr(out, down(ctx, v.kf_mp, (size_t)NKF * NFK));
  wr(out, down(ctx, v.obs_ptr, (size_t)NMPcap + 1));
  wr(out, down(ctx, v.obs_kf, (size_t)OBScap));
  wr(out, down(ctx, w.obs_feat, (size_t)OBScap));
  wr(out, down(ctx, v.mp_pos, (size_t)NMPcap * 3));
  wr(out, down(ctx, w.mp_assoc, (size_t)NMPcap));
  wr(out, down(ctx, ref_dev, (size_t)NMPcap));
  return out ? 0 : 4;
}
