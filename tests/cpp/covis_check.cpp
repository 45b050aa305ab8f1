// Driver of tests/test_gpu_covis_adapter.py: the covisibility graph through the C++ host mirror (include/gmmloc_hip/gmm_adapter.hpp:
// setResidentCovisibility, updateConnectionsInMap, removeFromGraph, bestCovisible, searchInNeighborsInMap), plain C++17 over the C-ABI.
//   covis_check model.gmm scene.bin out.bin
// scene.bin: int32 {NMP, NKF, NFK, NOBS, Wcap, Ccap, n_upd, n_rm, n_upd2, kf_first, kf_row, kf_idx, N, 0, 0, 0}, then mp_valid (NMP u8),
// kf_valid (NKF u8), kf_mp (NKF x NFK i32), obs_ptr (NMP + 1 i32), obs_kf (NOBS i32); upd (n_upd i32), rm (n_rm i32), upd2 (n_upd2 i32).
// The sequence: updateConnectionsInMap over upd -> removeFromGraph(rm) -> updateConnectionsInMap over upd2 -> bestCovisible(kf_row, N)
// and (kf_row, 0) -> searchInNeighborsInMap(kf_row, kf_idx) and the same with the reverse list.
// out.bin: per update {n_conn, widest, status, n_changed} + conn_kf + conn_w; {removed, status, erased, malformed} + best_cov (n_rm); the
// two lists of bestCovisible, each behind its length; {status, n_tgt} + tgt_kf; {status, n_tgt, n_cand} + tgt_kf + cand_mp; then,
// downloaded: cov_kf, cov_w (NKF x Wcap), cov_n, cov_nord, best_cov (NKF).
#include <cstdio>

#include "driver_io.hpp"

using namespace gmmloc_hip;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  GMM model;
  if (!load_model(argv[1], model)) return 1;
  std::ifstream in(argv[2], std::ios::binary);
  const auto hd = rd<int32_t>(in, 16);
  const int32_t NMP = hd[0], NKF = hd[1], NFK = hd[2], NOBS = hd[3], Wcap = hd[4], Ccap = hd[5], n_upd = hd[6], n_rm = hd[7], n_upd2 = hd[8];
  const int32_t kf_first = hd[9], kf_row = hd[10], kf_idx = hd[11], N = hd[12];
  const auto mp_valid = rd<uint8_t>(in, NMP), kf_valid = rd<uint8_t>(in, NKF);
  const auto kf_mp = rd<int32_t>(in, (size_t)NKF * NFK), obs_ptr = rd<int32_t>(in, (size_t)NMP + 1), obs_kf = rd<int32_t>(in, NOBS);
  const auto upd = rd<int32_t>(in, n_upd), rm = rd<int32_t>(in, n_rm), upd2 = rd<int32_t>(in, n_upd2);
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
  w.kf_first = kf_first;
  gl_map_covis cov{};
  cov.NKFcap = NKF;
  cov.cov_kf = up(ctx, std::vector<int32_t>((size_t)NKF * Wcap, -77));
  cov.cov_w = up(ctx, std::vector<int32_t>((size_t)NKF * Wcap, -77));
  cov.cov_n = up(ctx, std::vector<int32_t>((size_t)NKF, 0));
  cov.cov_nord = up(ctx, std::vector<int32_t>((size_t)NKF, 0));
  cov.best_cov = up(ctx, std::vector<int32_t>((size_t)NKF, -1));
  model.setResidentMap(v, w);
  model.setResidentCovisibility(cov, Wcap);
  std::ofstream out(argv[3], std::ios::binary);
  auto update = [&](const std::vector<int32_t>& rows) {
    for (int32_t k : rows) {
      const GMM::ConnectionsResult r = model.updateConnectionsInMap(k, Ccap);
      wr(out, std::vector<int32_t>{r.n_conn, r.widest, r.status, r.n_changed});
      wr(out, r.conn_kf);
      wr(out, r.conn_w);
    }
  };
  update(upd);
  const GMM::GraphRemoveResult g = model.removeFromGraph(rm);
  wr(out, std::vector<int32_t>{g.removed, g.status, g.erased, g.malformed});
  wr(out, g.best_cov);
  update(upd2);
  for (int32_t n : {N, 0}) {
    const std::vector<int32_t> b = model.bestCovisible(kf_row, n, Ccap);
    wr(out, std::vector<int32_t>{(int32_t)b.size()});
    wr(out, b);
  }
  const GMM::NeighborLists t = model.searchInNeighborsInMap(kf_row, kf_idx);
  wr(out, std::vector<int32_t>{t.status, (int32_t)t.tgt_kf.size()});
  wr(out, t.tgt_kf);
  const GMM::NeighborLists c = model.searchInNeighborsInMap(kf_row, kf_idx, true);
  wr(out, std::vector<int32_t>{c.status, (int32_t)c.tgt_kf.size(), (int32_t)c.cand_mp.size()});
  wr(out, c.tgt_kf);
  wr(out, c.cand_mp);
  std::printf("graph: %d rows removed, %d entries erased; %zu targets, %zu candidates\n", g.removed, g.erased, c.tgt_kf.size(), c.cand_mp.size());
  wr(out, down(ctx, cov.cov_kf, (size_t)NKF * Wcap));
  wr(out, down(ctx, cov.cov_w, (size_t)NKF * Wcap));
  wr(out, down(ctx, cov.cov_n, (size_t)NKF));
  wr(out, down(ctx, cov.cov_nord, (size_t)NKF));
  wr(out, down(ctx, cov.best_cov, (size_t)NKF));
  return out ? 0 : 4;
}
