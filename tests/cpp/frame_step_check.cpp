// Driver of tests/test_gpu_frame_step_adapter.py: the frame end and the hand-over through the C++ host mirror
// (include/gmmloc_hip/gmm_adapter.hpp: endFrame, noteReplaced, nextFrame), plain C++17 over the C-ABI.
//   frame_step_check model.gmm scene.bin out.bin
// scene.bin: int32 {NMP, NKF, NFK, NOBS, NMPcap, B, NF, NL, NPcap, n_steps, B2, NF2, mp_base, 0, 0, 0}, then the map: mp_valid (NMP u8),
// kf_valid (NKF u8), kf_mp (NKF x NFK i32), obs_ptr (NMP + 1 i32), obs_kf, obs_feat (NOBS i32), kf_uvr (NKF x NFK x 3 f64), kf_oct
// (NKF x NFK i32), kf_pose (NKF x 7 f64), mp_pos (NMP x 3 f64), mp_desc (NMP x 32 u8); the chain's outputs of B frames: feat_mp,
// match_last, match_local (B x NF i32), outlier (B x NF u8), local_mp (B x NPcap i32), n_local_mp (B i32), counts2 (B x 4 i32), ref_kf
// (B i32), last_observed (B x NL u8), feat_depth (B x NF f32), th_depth (f32), the gl_kf_rule (24 bytes); repl_src, repl_tgt (n_steps
// i32); the hand-over of B2 frames: pose_tracked, pose_prev (B2 x 7 f64), ref_kf (B2 i32), held_mp, feat_new (B2 x NF2 i32).
// The sequence: endFrame -> noteReplaced (mp_replaced starts as -1) -> nextFrame with that array.  Every output starts from a poison
// fill (-77 / 77), so that what a call leaves alone shows.
// out.bin, downloaded: held_mp (B x NF i32), held (B x NF u8), stat (B x 8 i32), ratio_map (B f32); mp_replaced (NMPcap i32); t_rc, t_cr,
// pose_lw, pose_cw (B2 x 7 f64), held_mp (B2 x NF2 i32), last_pt (B2 x NF2 x 3 f64), last_valid, last_observed, held (B2 x NF2 u8),
// status (B2 i32), last_desc (B2 x NF2 x 32 u8).
#include <cstdio>

#include "driver_io.hpp"

using namespace gmmloc_hip;

template <class T>
static T* filled(gl_ctx_t* ctx, size_t n, T value) {
  return up(ctx, std::vector<T>(n, value));
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  GMM model;
  if (!load_model(argv[1], model)) return 1;
  std::ifstream in(argv[2], std::ios::binary);
  const auto hd = rd<int32_t>(in, 16);
  const int32_t NMP = hd[0], NKF = hd[1], NFK = hd[2], NOBS = hd[3], NMPcap = hd[4], B = hd[5], NF = hd[6], NL = hd[7], NPcap = hd[8], n_steps = hd[9];
  const int32_t B2 = hd[10], NF2 = hd[11], mp_base = hd[12];
  const auto mp_valid = rd<uint8_t>(in, NMP), kf_valid = rd<uint8_t>(in, NKF);
  const auto kf_mp = rd<int32_t>(in, (size_t)NKF * NFK), obs_ptr = rd<int32_t>(in, (size_t)NMP + 1), obs_kf = rd<int32_t>(in, NOBS), obs_feat = rd<int32_t>(in, NOBS);
  const auto kf_uvr = rd<double>(in, (size_t)NKF * NFK * 3);
  const auto kf_oct = rd<int32_t>(in, (size_t)NKF * NFK);
  const auto kf_pose = rd<double>(in, (size_t)NKF * 7), mp_pos = rd<double>(in, (size_t)NMP * 3);
  const auto mp_desc = rd<uint8_t>(in, (size_t)NMP * 32);
  const auto feat_mp = rd<int32_t>(in, (size_t)B * NF), match_last = rd<int32_t>(in, (size_t)B * NF), match_local = rd<int32_t>(in, (size_t)B * NF);
  const auto outlier = rd<uint8_t>(in, (size_t)B * NF);
  const auto local_mp = rd<int32_t>(in, (size_t)B * NPcap), n_local_mp = rd<int32_t>(in, B), counts2 = rd<int32_t>(in, (size_t)B * 4), ref_kf = rd<int32_t>(in, B);
  const auto last_observed = rd<uint8_t>(in, (size_t)B * NL);
  const auto feat_depth = rd<float>(in, (size_t)B * NF), th_depth = rd<float>(in, 1);
  gl_kf_rule rule;
  static_assert(sizeof(gl_kf_rule) == 24, "gl_kf_rule: six 4-byte scalars");
  in.read(reinterpret_cast<char*>(&rule), sizeof rule);
  const auto repl_src = rd<int32_t>(in, n_steps), repl_tgt = rd<int32_t>(in, n_steps);
  const auto pose_tracked = rd<double>(in, (size_t)B2 * 7), pose_prev = rd<double>(in, (size_t)B2 * 7);
  const auto ref_kf2 = rd<int32_t>(in, B2), held_in = rd<int32_t>(in, (size_t)B2 * NF2), feat_new = rd<int32_t>(in, (size_t)B2 * NF2);
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
  v.mp_desc = up(ctx, mp_desc);
  gl_map_ba_view w{};
  w.kf_pose = up(ctx, kf_pose);
  w.kf_uvr = up(ctx, kf_uvr);
  w.kf_oct = up(ctx, kf_oct);
  w.obs_feat = up(ctx, obs_feat);
  w.kf_first = 0;
  model.setResidentMap(v, w);
  model.setResidentMapCapacity(NMPcap, NOBS);  // (the rows of mp_replaced: nothing is added to the map's own arrays here)
  std::ofstream out(argv[3], std::ios::binary);

  gl_frame_end_in ei{};
  ei.feat_mp = up(ctx, feat_mp), ei.match_last = up(ctx, match_last), ei.match_local = up(ctx, match_local), ei.outlier = up(ctx, outlier);
  ei.local_mp = up(ctx, local_mp), ei.n_local_mp = up(ctx, n_local_mp), ei.counts2 = up(ctx, counts2), ei.ref_kf = up(ctx, ref_kf);
  ei.last_observed = up(ctx, last_observed), ei.feat_depth = up(ctx, feat_depth);
  gl_frame_end_out eo{};
  eo.held_mp = filled<int32_t>(ctx, (size_t)B * NF, -77), eo.held = filled<uint8_t>(ctx, (size_t)B * NF, 77);
  eo.stat = filled<int32_t>(ctx, (size_t)B * 8, -77), eo.ratio_map = filled<float>(ctx, B, -77.0f);
  model.endFrame(B, NF, NL, NPcap, ei, th_depth[0], &rule, eo);

  int32_t* mp_replaced = filled<int32_t>(ctx, NMPcap, -1);
  model.noteReplaced(mp_replaced, repl_src, repl_tgt);

  gl_frame_next_in ni{};
  ni.pose_tracked = up(ctx, pose_tracked), ni.pose_prev = up(ctx, pose_prev), ni.ref_kf = up(ctx, ref_kf2), ni.feat_new = up(ctx, feat_new);
  ni.mp_replaced = mp_replaced, ni.mp_base = mp_base;
  gl_frame_next_out no{};
  const size_t n2 = (size_t)B2 * NF2;
  no.t_rc = filled<double>(ctx, (size_t)B2 * 7, -77.0), no.t_cr = filled<double>(ctx, (size_t)B2 * 7, -77.0);
  no.pose_lw = filled<double>(ctx, (size_t)B2 * 7, -77.0), no.pose_cw = filled<double>(ctx, (size_t)B2 * 7, -77.0);
  no.held_mp = up(ctx, held_in);
  no.last_pt = filled<double>(ctx, n2 * 3, -77.0);
  no.last_valid = filled<uint8_t>(ctx, n2, 77), no.last_observed = filled<uint8_t>(ctx, n2, 77), no.held = filled<uint8_t>(ctx, n2, 77);
  no.status = filled<int32_t>(ctx, B2, -77);
  no.last_desc = filled<uint8_t>(ctx, n2 * 32, 77);
  model.nextFrame(B2, NF2, ni, no);
  check(gl_ctx_synchronize(ctx), "sync");

  wr(out, down(ctx, eo.held_mp, (size_t)B * NF));
  wr(out, down(ctx, eo.held, (size_t)B * NF));
  const auto stat = down(ctx, eo.stat, (size_t)B * 8);
  wr(out, stat);
  wr(out, down(ctx, eo.ratio_map, (size_t)B));
  wr(out, down(ctx, mp_replaced, (size_t)NMPcap));
  wr(out, down(ctx, no.t_rc, (size_t)B2 * 7));
  wr(out, down(ctx, no.t_cr, (size_t)B2 * 7));
  wr(out, down(ctx, no.pose_lw, (size_t)B2 * 7));
  wr(out, down(ctx, no.pose_cw, (size_t)B2 * 7));
  wr(out, down(ctx, no.held_mp, n2));
  wr(out, down(ctx, no.last_pt, n2 * 3));
  wr(out, down(ctx, no.last_valid, n2));
  wr(out, down(ctx, no.last_observed, n2));
  wr(out, down(ctx, no.held, n2));
  wr(out, down(ctx, no.status, (size_t)B2));
  wr(out, down(ctx, no.last_desc, n2 * 32));
  std::printf("end: frame 0 {res %d, inliers %d, map %d / %d, ref %d, verdict %d}; %d steps noted; next: %d frames of %d slots\n", stat[0], stat[1], stat[2],
              stat[3], stat[4], stat[5], n_steps, B2, NF2);
  return out ? 0 : 4;
}
