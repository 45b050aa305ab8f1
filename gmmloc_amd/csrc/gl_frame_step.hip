// Frame end and hand-over (gmmloc_hip.h, gl_track_frame_end / gl_map_note_replaced / gl_track_frame_next): what the reference does
// between two tracked frames, on the chain's outputs and the resident map.  The rule tables with the reference's lines are in the header.
//   end    a workgroup per frame strides over the features: the row each holds at the end of Tracking::track, the three counts packed
//          into one 64-bit word (21 bits each: NF <= 3 072) and summed by mapdev's workgroup scan; with a rule the workgroup then
//          strides over the reference key-frame's slots for countMapPoints, and thread 0 evaluates needNewKeyFrame.
//   note   the sequential one.  One workgroup; per NOTE_STEPS steps the valid sources go to LDS and a step stores unless a later step
//          of the chunk names the same source; the next chunk stores behind a fence and a barrier.
//   next   a workgroup per frame: thread 0 chains the four poses while every thread strides over the slots.
// Integer stores and one integer reduction; the float arithmetic is the one division and the compares of the header, in one thread.
#include "gl_device.hpp"
#include "gl_map_dev.hpp"

namespace {

using namespace gl::mapdev;  // Map, mp_row, kf_row, mp_ok, obs_range, obs_weight, list_len, block_excl_scan

constexpr int T_FS = 256;
constexpr int NOTE_STEPS = 1024;
constexpr int FS_MAX_NF = 3072;  // the chain's bound (gl_search_local_points); the packed counts need NF < 2^21

// countObservations() > 0 of row r (inside the table): its CSR range is not empty
__device__ __forceinline__ bool row_observed(const Map& m, int r) {
  int o0, o1;
  obs_range(m, r, &o0, &o1);
  return o1 > o0;
}

// ---------------------------------------------------------------------------------------------------------------- end
struct EndArgs {
  Map m;
  int NF, NPcap;
  gl_frame_end_in in;
  gl_frame_end_out out;
  float th_depth;
  int has_rule;
  gl_kf_rule rule;
};

// GMMLoc::needNewKeyFrame (gmmloc.cpp:327-361) on the frame's statistics -> the verdict bits
__device__ __forceinline__ int need_new_keyframe(const gl_kf_rule& k, int nmi, float ratio_map, int nref) {
  const float th_ref_ratio = k.num_kfs < 2 ? 0.4f : 0.75f;  // (:327)
  const float th_map_ratio = nmi > 300 ? 0.2f : 0.35f;      // (:328)
  const bool c1a = static_cast<float>(k.frame_idx) >= static_cast<float>(k.kf_frame_idx) + k.fps;  // (:335)
  const bool c1b = static_cast<float>(nmi) < static_cast<float>(nref) * 0.25f || ratio_map < 0.3f;  // (:338-339)
  const bool c2 = (static_cast<float>(nmi) < static_cast<float>(nref) * th_ref_ratio || ratio_map < th_map_ratio) && nmi > 15;  // (:343-345)
  if (!((c1a || c1b || k.is_idle) && c2)) return 0;  // (:349)
  if (k.is_idle) return GL_KF_NEED;                  // (:352)
  return GL_KF_INTERRUPT_BA | (k.n_queue < 3 ? GL_KF_NEED : 0);  // (:355-360)
}

__global__ __launch_bounds__(T_FS) void k_frame_end(EndArgs a) {
  __shared__ u64 s_w[T_FS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const Map& m = a.m;
  int32_t* const stat = a.out.stat + (size_t)b * 8;
  const int mode = a.in.counts2 ? a.in.counts2[(size_t)b * 4 + 3] : 0;
  if (mode == 2) {  // lost (tracking.cpp:65-71): the return before last_frame_ advances
    if (tid < 8) stat[tid] = tid == 1 ? 10 : 0;
    return;
  }
  const int32_t* const fm = a.in.feat_mp + (size_t)b * a.NF;
  const int32_t* const ml = a.in.match_local + (size_t)b * a.NF;
  const uint8_t* const ol = a.in.outlier + (size_t)b * a.NF;
  const float* const dp = a.in.feat_depth + (size_t)b * a.NF;
  const int32_t* const lm = a.in.local_mp + (size_t)b * a.NPcap;
  int32_t* const hm = a.out.held_mp + (size_t)b * a.NF;
  uint8_t* const hd = a.out.held + (size_t)b * a.NF;
  const int nl = min(max(a.in.n_local_mp[b], 0), a.NPcap);
  u64 cnt = 0ull;  // num_match_inliers | num_map << 21 | num_total << 42
  for (int i = tid; i < a.NF; i += T_FS) {
    const int j = ml[i];
    const int r = j >= 0 && j < nl ? lm[j] : fm[i];
    // held after trackLocalMap (:279-292) and clearTemporalPoints (:379-388): a row, no outlier, with observations
    const bool keep = mp_row(m, r) && !ol[i] && row_observed(m, r);
    const float d = dp[i];
    const bool in_depth = d > 0.0f && d < a.th_depth;  // (:91-92)
    hm[i] = keep ? r : -1;
    hd[i] = keep ? 1 : 0;
    cnt += (keep ? 1ull : 0ull) | (keep && in_depth ? 1ull << 21 : 0ull) | (in_depth ? 1ull << 42 : 0ull);
  }
  u64 total;
  block_excl_scan<T_FS, u64>(cnt, s_w, tid, &total);
  u64 ref = 0ull;  // KeyFrame::countMapPoints (keyframe.cpp:212-231) of the reference key-frame
  if (a.has_rule) {
    const int k = a.in.ref_kf[b], need = a.rule.num_kfs <= 2 ? 2 : 3;  // (gmmloc.cpp:331)
    if (kf_row(m, k)) {
      const int32_t* const slots = m.kf_mp + (size_t)k * m.NFK;
      for (int s = tid; s < m.NFK; s += T_FS) {
        const int p = slots[s];
        if (!mp_ok(m, p)) continue;
        int o0, o1, w = 0;
        obs_range(m, p, &o0, &o1);
        for (int o = o0; o < o1 && w < need; ++o) w += obs_weight(m, m.obs_kf[o], m.obs_feat[o]);
        if (w >= need) ref += 1ull;
      }
    }
  }
  u64 nref64;
  block_excl_scan<T_FS, u64>(ref, s_w, tid, &nref64);
  if (tid == 0) {
    const int nmi = (int)(total & 0x1fffffull), num_map = (int)((total >> 21) & 0x1fffffull), num_total = (int)((total >> 42) & 0x1fffffull);
    const int nref = (int)nref64;
    const float ratio_map = static_cast<float>(num_map) / static_cast<float>(max(1, num_total));  // (:102)
    stat[0] = mode == 0 ? 1 : 0;  // (stat_.res: :49, :55 - and nothing after a successful trackKeyFrame)
    stat[1] = nmi;
    stat[2] = num_map;
    stat[3] = num_total;
    stat[4] = nref;
    stat[5] = a.has_rule ? need_new_keyframe(a.rule, nmi, ratio_map, nref) : 0;
    stat[6] = 0;
    stat[7] = 0;
    a.out.ratio_map[b] = ratio_map;
  }
}

// ---------------------------------------------------------------------------------------------------------------- note
__global__ __launch_bounds__(NOTE_STEPS) void k_note_replaced(int NMPcap, int32_t* rep, const int32_t* src, const int32_t* tgt, int n_host,
                                                              const int32_t* n_dev) {
  __shared__ int s_src[NOTE_STEPS];  // the source of the chunk's step, -1: the step changes nothing
  const int tid = threadIdx.x;
  const int n = list_len(n_dev, n_host);
  for (int c0 = 0; c0 < n; c0 += NOTE_STEPS) {
    const int nc = min(n - c0, NOTE_STEPS);
    int s = -1, t = -1;
    if (tid < nc) {
      s = src[c0 + tid];
      t = tgt[c0 + tid];
      if (s < 0 || s >= NMPcap || t < 0 || t >= NMPcap || s == t) s = -1;  // (a row outside the table; map.cpp:113)
    }
    s_src[tid] = s;
    __syncthreads();
    bool wins = s >= 0;
    for (int q = tid + 1; q < nc && wins; ++q) wins = s_src[q] != s;  // (a later step on the same source, :126)
    if (wins) rep[s] = t;
    __threadfence();  // (the next chunk may name the same source: its store comes behind this one)
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------- next
struct NextArgs {
  Map m;
  const uint8_t* mp_desc;  // read with out.last_desc only
  int NF;
  gl_frame_next_in in;
  gl_frame_next_out out;
};

__global__ __launch_bounds__(T_FS) void k_frame_next(NextArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const Map& m = a.m;
  if (tid == 0) {
    const int k = a.in.ref_kf[b];
    int status = 0;
    if (kf_row(m, k)) {
      using namespace gld;
      const SE3 Tkw = se3_load(m.kf_pose + (size_t)k * 7), Tcw = se3_load(a.in.pose_tracked + (size_t)b * 7);
      const SE3 Trc = se3_mul(Tkw, se3_inverse(Tcw));  // (map.cpp:29)
      const SE3 Tcr = se3_inverse(Trc);                // (:33)
      const SE3 lw = se3_mul(Tcr, Tkw);                // (gmmloc.cpp:275)
      SE3 cw = lw;                                     // (:285)
      if (a.in.pose_prev) {
        const SE3 delta = se3_mul(lw, se3_inverse(se3_load(a.in.pose_prev + (size_t)b * 7)));  // (:288)
        cw = se3_mul(delta, lw);                                                                // (:289)
      }
      se3_store(Trc, a.out.t_rc + (size_t)b * 7);
      se3_store(Tcr, a.out.t_cr + (size_t)b * 7);
      se3_store(lw, a.out.pose_lw + (size_t)b * 7);
      se3_store(cw, a.out.pose_cw + (size_t)b * 7);
    } else {
      status = GL_FRAME_NEXT_BAD_REF;
    }
    a.out.status[b] = status;
  }
  int32_t* const hm = a.out.held_mp + (size_t)b * a.NF;
  const int32_t* const fn = a.in.feat_new ? a.in.feat_new + (size_t)b * a.NF : nullptr;
  double* const lp = a.out.last_pt + (size_t)b * a.NF * 3;
  uint8_t* const lv = a.out.last_valid + (size_t)b * a.NF;
  uint8_t* const lo = a.out.last_observed + (size_t)b * a.NF;
  uint8_t* const hd = a.out.held + (size_t)b * a.NF;
  for (int i = tid; i < a.NF; i += T_FS) {
    int h = hm[i];
    if (fn) {  // the key-frame's new points (gmmloc_opt.cpp:100)
      const int f = fn[i];
      const long long r = (long long)a.in.mp_base + f;
      if (f >= 0 && r >= 0 && r < m.NMP) h = (int)r;
      else if (f == -2) h = -1;
    }
    if (a.in.mp_replaced && mp_row(m, h)) {  // ONE step (tracking.cpp:402-405); NMP <= NMPcap
      const int r = a.in.mp_replaced[h];
      if (mp_row(m, r)) h = r;
    }
    hm[i] = h;
    const bool row = mp_row(m, h);
    const bool obs = row && row_observed(m, h);
    lp[3 * i + 0] = row ? m.mp_pos[(size_t)h * 3 + 0] : 0.0;
    lp[3 * i + 1] = row ? m.mp_pos[(size_t)h * 3 + 1] : 0.0;
    lp[3 * i + 2] = row ? m.mp_pos[(size_t)h * 3 + 2] : 0.0;
    lv[i] = row ? 1 : 0;
    lo[i] = obs ? 1 : 0;
    hd[i] = !row ? 0 : obs ? 1 : 2;
    if (row && a.out.last_desc) {  // the map point's descriptor: 32 bytes as eight words (both sides are 32-byte rows of hipMalloc'd arrays)
      const uint32_t* const from = reinterpret_cast<const uint32_t*>(a.mp_desc + (size_t)h * 32);
      uint32_t* const to = reinterpret_cast<uint32_t*>(a.out.last_desc + ((size_t)b * a.NF + i) * 32);
#pragma unroll
      for (int w = 0; w < 8; ++w) to[w] = from[w];
    }
  }
}

}  // namespace

extern "C" int gl_track_frame_end(gl_ctx_t* ctx, const gl_map_view* map, const gl_map_ba_view* ba, int B, int NF, int NL, int NPcap,
                                  const gl_frame_end_in* in, float th_depth, const gl_kf_rule* rule, const gl_frame_end_out* out) {
  GL_REQUIRE(ctx && in && out, "null argument");
  GL_REQUIRE(B >= 0 && B <= 65535 && NF >= 0 && NF <= FS_MAX_NF && NL >= 0 && NPcap >= 0, "bad B / NF / NL / NPcap (NF is bounded by 3 072)");
  EndArgs a = {};
  const int rc = map_from_view(__func__, map, nullptr, &a.m);
  if (rc != GL_OK) return rc;
  if (B == 0) return GL_OK;
  GL_REQUIRE(out->stat && out->ratio_map && (NF == 0 || (out->held_mp && out->held)), "null held_mp / held / stat / ratio_map");
  GL_REQUIRE(NF == 0 || (in->feat_mp && in->match_local && in->outlier && in->feat_depth), "null feat_mp / match_local / outlier / feat_depth");
  GL_REQUIRE(in->n_local_mp && (NPcap == 0 || in->local_mp), "null local_mp / n_local_mp");
  if (rule) {
    GL_REQUIRE(in->ref_kf, "null ref_kf");
    GL_REQUIRE(ba && (a.m.NOBS == 0 || ba->obs_feat) && (a.m.NKF == 0 || a.m.NFK == 0 || ba->kf_uvr), "the rule needs obs_feat / kf_uvr of gl_map_ba_view");
    a.m.obs_feat = (int32_t*)ba->obs_feat;
    a.m.kf_uvr = ba->kf_uvr;
    a.has_rule = 1;
    a.rule = *rule;
  }
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  a.NF = NF, a.NPcap = NPcap, a.in = *in, a.out = *out, a.th_depth = th_depth;
  k_frame_end<<<B, T_FS, 0, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_map_note_replaced(gl_ctx_t* ctx, int NMPcap, int32_t* mp_replaced_dev, const int32_t* repl_src_dev, const int32_t* repl_tgt_dev,
                                    int n, const int32_t* n_dev) {
  GL_REQUIRE(ctx, "null argument");
  GL_REQUIRE(NMPcap >= 0 && n >= 0, "bad NMPcap / n");
  if (n == 0 || NMPcap == 0) return GL_OK;
  GL_REQUIRE(mp_replaced_dev && repl_src_dev && repl_tgt_dev, "null mp_replaced / repl_src / repl_tgt");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  k_note_replaced<<<1, NOTE_STEPS, 0, c->stream>>>(NMPcap, mp_replaced_dev, repl_src_dev, repl_tgt_dev, n, n_dev);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_track_frame_next(gl_ctx_t* ctx, const gl_map_view* map, const gl_map_ba_view* ba, int B, int NF, const gl_frame_next_in* in,
                                   const gl_frame_next_out* out) {
  GL_REQUIRE(ctx && ba && in && out, "null argument");
  GL_REQUIRE(B >= 0 && B <= 65535 && NF >= 0 && NF <= FS_MAX_NF, "bad B / NF (NF is bounded by 3 072)");
  NextArgs a = {};
  const int rc = map_from_view(__func__, map, nullptr, &a.m);
  if (rc != GL_OK) return rc;
  if (B == 0) return GL_OK;
  GL_REQUIRE(a.m.NMP == 0 || a.m.mp_pos, "null mp_pos");
  GL_REQUIRE(a.m.NKF == 0 || ba->kf_pose, "null kf_pose");
  GL_REQUIRE(in->pose_tracked && in->ref_kf, "null pose_tracked / ref_kf");
  GL_REQUIRE(!in->mp_replaced || in->NMPcap >= a.m.NMP, "mp_replaced has fewer rows than the map");
  GL_REQUIRE(out->t_rc && out->t_cr && out->pose_lw && out->pose_cw && out->status, "null t_rc / t_cr / pose_lw / pose_cw / status");
  GL_REQUIRE(NF == 0 || (out->held_mp && out->last_pt && out->last_valid && out->last_observed && out->held),
             "null held_mp / last_pt / last_valid / last_observed / held");
  a.m.kf_pose = ba->kf_pose;
  if (out->last_desc) {
    GL_REQUIRE(a.m.NMP == 0 || map->mp_desc, "last_desc needs mp_desc");
    GL_REQUIRE(((uintptr_t)out->last_desc & 3) == 0 && ((uintptr_t)map->mp_desc & 3) == 0, "last_desc / mp_desc must be 4-byte aligned");
    a.mp_desc = map->mp_desc;
  }
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  a.NF = NF, a.in = *in, a.out = *out;
  k_frame_next<<<B, T_FS, 0, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}
