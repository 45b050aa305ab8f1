// Driver of tests/test_gpu_ba_window_adapter.py: the map-resident local BA through the C++ host mirror
// (include/gmmloc_hip/gmm_adapter.hpp: flattenMap, flattenMapBa, setResidentMap, jointOptimizationFromMap), plain C++17 over the C-ABI.
//   ba_window_check model.gmm scene.bin out.bin
// scene.bin: int32 {NMP, NKF, NFK, kf_row, kf_first, width, height, 0}, double {fx, fy, cx, cy, bf}, then mp_valid (NMP u8), kf_valid
// (NKF u8), kf_mp (NKF x NFK i32), mp_pos (NMP x 3 f64), kf_pose (NKF x 7 f64), kf_uvr (NKF x NFK x 3 f64), kf_oct (NKF x NFK i32),
// mp_assoc (NMP i32).  out.bin: the rows the adapter flattened (obs_ptr, obs_kf, obs_feat, kf_twc), the result of the call
// ({P, F, L, nobs, status, iters, n_erase}, win_kf, win_mp, assoc_dropped, erase_obs) and the resident rows after it (kf_pose, kf_twc,
// mp_pos, mp_assoc), downloaded.
#include <cstdio>

#include "driver_io.hpp"

using namespace gmmloc_hip;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  GMM model;
  if (!load_model(argv[1], model)) return 1;
  std::ifstream in(argv[2], std::ios::binary);
  const auto hd = rd<int32_t>(in, 8);
  const auto cm = rd<double>(in, 5);
  const int32_t NMP = hd[0], NKF = hd[1], NFK = hd[2], kf_row = hd[3], kf_first = hd[4];
  gl_camera cam{cm[0], cm[1], cm[2], cm[3], cm[4], hd[5], hd[6]};
  model.setCamera(cam);
  const auto mp_valid = rd<uint8_t>(in, NMP), kf_valid = rd<uint8_t>(in, NKF);
  const auto kf_mp = rd<int32_t>(in, (size_t)NKF * NFK);
  const auto mp_pos = rd<double>(in, (size_t)NMP * 3), kf_pose = rd<double>(in, (size_t)NKF * 7), kf_uvr = rd<double>(in, (size_t)NKF * NFK * 3);
  const auto kf_oct = rd<int32_t>(in, (size_t)NKF * NFK), mp_assoc = rd<int32_t>(in, NMP);
  if (!in) return 3;
  // the host's containers -> flat rows
  const MapRows m = flattenMap(
      NMP, NKF, NFK, [&](int32_t k, int32_t i) { return kf_mp[(size_t)k * NFK + i]; }, [&](int32_t p) { return mp_valid[p] != 0; },
      [&](int32_t k) { return kf_valid[k] != 0; });
  const MapBaRows b = flattenMapBa(
      m,
      [&](int32_t k) {
        Pose T;
        std::memcpy(&T, &kf_pose[(size_t)k * 7], 56);
        return T;
      },
      [&](int32_t k, int32_t i, double* uvr, int32_t& oct) {
        std::memcpy(uvr, &kf_uvr[((size_t)k * NFK + i) * 3], 24);
        oct = kf_oct[(size_t)k * NFK + i];
        return true;
      },
      [&](int32_t p) { return mp_assoc[p]; }, [&](int32_t k) { return k == kf_first; });
  // ... resident on the device
  gl_ctx_t* ctx = model.ctx();
  gl_map_view v{};
  v.NMP = NMP, v.NKF = NKF, v.NFK = NFK, v.NOBS = (int32_t)m.obs_kf.size();
  v.mp_valid = up(ctx, m.mp_valid);
  v.obs_ptr = up(ctx, m.obs_ptr);
  v.obs_kf = up(ctx, m.obs_kf);
  v.kf_valid = up(ctx, m.kf_valid);
  v.kf_mp = up(ctx, m.kf_mp);
  v.mp_pos = up(ctx, mp_pos);
  gl_map_ba_view w{};
  w.kf_pose = up(ctx, b.kf_pose);
  w.kf_twc = up(ctx, b.kf_twc);
  w.kf_uvr = up(ctx, b.kf_uvr);
  w.kf_oct = up(ctx, b.kf_oct);
  w.obs_feat = up(ctx, b.obs_feat);
  w.mp_assoc = up(ctx, b.mp_assoc);
  w.kf_first = b.kf_first;
  model.setResidentMap(v, w);
  const GMM::WindowResult r = model.jointOptimizationFromMap(kf_row);
  std::printf("window P %d F %d L %d nobs %d status %d iters %d erase %zu\n", r.P, r.F, r.L, r.nobs, r.status, r.iters, r.erase_obs.size());
  std::ofstream out(argv[3], std::ios::binary);
  wr(out, m.obs_ptr);
  wr(out, m.obs_kf);
  wr(out, b.obs_feat);
  wr(out, b.kf_twc);
  wr(out, std::vector<int32_t>{r.P, r.F, r.L, r.nobs, r.status, r.iters, (int32_t)r.erase_obs.size()});
  wr(out, r.win_kf);
  wr(out, r.win_mp);
  wr(out, r.assoc_dropped);
  wr(out, r.erase_obs);
  wr(out, down(ctx, w.kf_pose, (size_t)NKF * 7));
  wr(out, down(ctx, w.kf_twc, (size_t)NKF * 3));
  wr(out, down(ctx, v.mp_pos, (size_t)NMP * 3));
  wr(out, down(ctx, w.mp_assoc, (size_t)NMP));
  return out ? 0 : 4;
}
