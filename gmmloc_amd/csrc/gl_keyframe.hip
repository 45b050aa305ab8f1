// The two depth-ordered walks that make points from stereo depth:
//   gl_create_stereo_points    GMMLoc::createMapPointsFromStereo   (gmmloc_opt.cpp:36-113)
//   gl_create_temporal_points  Tracking::createTemporalPoints      (tracking.cpp:411-465)
// Both read as a loop with a counter, a `continue` and an early `break`; both are a sort, independent per-entry work and a prefix
// count.  The order of std::sort on pair<float, index> is the total order on (depth, index), and for positive floats that is the
// order of the 64-bit keys (bits(depth) << 32) | index.  Whether an entry is counted depends on that entry alone (its held state and,
// for createMapPointsFromStereo, the answer of checkMapAssociation), so num_points at an entry is the inclusive prefix count of the
// counted entries in sorted order, and the loop ends behind the FIRST position at which `depth > th_depth && num_points > 100`
// holds on a counted entry (a rejected entry `continue`s past the test).
//   k_stereo_prep   a thread per feature: entry test, unprojection (frame.cpp:27-35), the arguments of k_check_map_association
//   k_check_map_association (gl_point.hip) on the entries with create_new && ncand > 0
//   k_stereo_walk   one workgroup per key-frame: bitonic sort of the keys in LDS, one scan, integer stores
//   k_temporal_walk the same walk without a check; writes the chain's last-frame rows in place
#include "gl_device.hpp"
#include "gl_internal.hpp"
#include "gl_map_dev.hpp"  // block_excl_scan

using namespace gld;

namespace {

constexpr int WALK_T = 1024;                          // threads of a walk workgroup
constexpr int WALK_PER = GL_STEREO_WALK_MAX / WALK_T;  // sorted positions per thread
static_assert(GL_STEREO_WALK_MAX % WALK_T == 0 && (GL_STEREO_WALK_MAX & (GL_STEREO_WALK_MAX - 1)) == 0, "the walk sorts a power of two");
typedef unsigned long long u64;
constexpr u64 NO_ENTRY = ~0ull;  // sorts behind every entry (+inf is 0x7f800000)

struct UnK {
  double fx, fy, cx, cy;
};

// Frame::unproject3 (frame.cpp:27-35): PinholeCamera::unproject3 (pinhole_camera.cpp:30-32) then Twc.map
GL_DEV void unproject(const UnK& k, const SE3& Twc, double u, double v, float depth, double* out) {
  const double z = depth;
  const double ptc[3] = {z * (u - k.cx) / k.fx, z * (v - k.cy) / k.fy, z};
  double r[3];
  qrot(Twc.r, ptc, r);
  for (int i = 0; i < 3; ++i) out[i] = r[i] + Twc.t[i];
}

// `z > 0` (:42) on the bits: sign clear, not zero, not NaN - the float compare whatever the denormal mode of the compare instruction
GL_DEV bool is_entry(float depth, int oct) { return __float_as_uint(depth) - 1u < 0x7f800000u && oct >= 0 && oct <= 7; }

__global__ void k_stereo_prep(UnK k, int B, int NF, const double* __restrict__ pose, const double* __restrict__ feat_uv,
                              const float* __restrict__ feat_ur, const float* __restrict__ feat_depth, const int32_t* __restrict__ feat_oct,
                              const int32_t* __restrict__ ncand, const uint8_t* __restrict__ held, double* __restrict__ pts,
                              double* __restrict__ pts0, double* __restrict__ uvr, int32_t* __restrict__ octm) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)B * NF) return;
  const int b = (int)(gid / NF);
  const float d = feat_depth[gid];
  const int oc = feat_oct[gid];
  const double u = feat_uv[gid * 2], v = feat_uv[gid * 2 + 1];
  double p[3] = {0.0, 0.0, 0.0};
  const bool entry = is_entry(d, oc);
  if (entry) unproject(k, se3_inverse(se3_load(pose + (size_t)b * 7)), u, v, d, p);
  for (int i = 0; i < 3; ++i) {
    pts[gid * 3 + i] = p[i];
    if (pts0) pts0[gid * 3 + i] = p[i];
  }
  uvr[gid * 3] = u;
  uvr[gid * 3 + 1] = v;
  uvr[gid * 3 + 2] = (double)feat_ur[gid];
  // the check runs where the loop calls it: an entry, create_new (:55-63), comps not empty (:75); < 0 = skipped, answer -1
  octm[gid] = (entry && held[gid] != 1 && ncand[gid] > 0) ? oc : -1;
}

// The keys of key-frame / frame b sorted ascending in s_key[0, n2), n2 the power of two >= NF; -> the number of entries (every thread)
GL_DEV int sort_entries(u64* s_key, int* s_cnt, int NF, const float* __restrict__ depth, const int32_t* __restrict__ oct, int tid) {
  int n2 = 2;
  while (n2 < NF) n2 <<= 1;
  if (tid == 0) *s_cnt = 0;
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < n2; i += WALK_T) {
    u64 key = NO_ENTRY;
    if (i < NF) {
      const float d = depth[i];
      if (is_entry(d, oct[i])) {
        key = ((u64)__float_as_uint(d) << 32) | (unsigned)i;
        ++mine;
      }
    }
    s_key[i] = key;
  }
  if (mine) atomicAdd(s_cnt, mine);
  __syncthreads();
  for (int k2 = 2; k2 <= n2; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < n2 / 2; t += WALK_T) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const u64 a = s_key[lo], c = s_key[hi];
        if ((a > c) == ((lo & k2) == 0)) {
          s_key[lo] = c;
          s_key[hi] = a;
        }
      }
      __syncthreads();
    }
  return *s_cnt;
}

struct WalkShared {
  u64 key[GL_STEREO_WALK_MAX];
  u64 scan[WALK_T / 64];
  int cnt, brk;
};

__global__ __launch_bounds__(WALK_T) void k_stereo_walk(int NF, int mp_base, int check_depth, float th_depth,
                                                        const float* __restrict__ feat_depth, const int32_t* __restrict__ feat_oct,
                                                        const int32_t* __restrict__ ncand, const uint8_t* __restrict__ held,
                                                        const int32_t* __restrict__ kf_row, const int32_t* __restrict__ comp,
                                                        const u64* __restrict__ pts, int32_t* __restrict__ new_feat,
                                                        u64* __restrict__ new_pos, int32_t* __restrict__ new_assoc,
                                                        int32_t* __restrict__ new_ref_kf, int32_t* __restrict__ att_mp,
                                                        int32_t* __restrict__ att_kf, int32_t* __restrict__ att_feat,
                                                        int32_t* __restrict__ n_new, int32_t* __restrict__ feat_new,
                                                        int32_t* __restrict__ stats) {
  __shared__ WalkShared s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t f0 = (size_t)b * NF;
  const int ne = sort_entries(s.key, &s.cnt, NF, feat_depth + f0, feat_oct + f0, tid);
  if (tid == 0) s.brk = 0x7fffffff;
  for (int i = tid; i < NF; i += WALK_T) feat_new[f0 + i] = -1;
  // per sorted position: bit 0 counted, bit 1 created, bit 2 rejected with a temporal point in the slot
  int what[WALK_PER], feat[WALK_PER], assoc[WALK_PER];
  float dep[WALK_PER];
  u64 sum = 0;
#pragma unroll
  for (int u = 0; u < WALK_PER; ++u) {
    const int p = tid * WALK_PER + u;
    what[u] = 0;
    feat[u] = 0;
    assoc[u] = -1;
    dep[u] = 0.0f;
    if (p < ne) {
      const u64 key = s.key[p];
      const int i = (int)(unsigned)key;
      const int h = held[f0 + i], cp = comp[f0 + i];
      const bool create_new = h != 1;
      const bool rejected = create_new && ncand[f0 + i] > 0 && cp < 0;  // checkMapAssociation returned nullptr: `continue` (:79-80)
      feat[u] = i;
      assoc[u] = cp;
      dep[u] = __uint_as_float((unsigned)(key >> 32));
      what[u] = (rejected ? 0 : 1) | (create_new && !rejected ? 2 : 0) | (rejected && h == 2 ? 4 : 0);
      sum += (u64)(what[u] & 1) | ((u64)((what[u] >> 1) & 1) << 32);
    }
  }
  u64 total;
  u64 at = gl::mapdev::block_excl_scan<WALK_T, u64>(sum, s.scan, tid, &total);  // (its barriers order s.brk and feat_new too)
  int counted[WALK_PER], row[WALK_PER];
#pragma unroll
  for (int u = 0; u < WALK_PER; ++u) {
    const int p = tid * WALK_PER + u;
    row[u] = (int)(at >> 32);
    at += (u64)(what[u] & 1) | ((u64)((what[u] >> 1) & 1) << 32);
    counted[u] = (int)(unsigned)at;  // num_points after this entry
    if (p < ne && (what[u] & 1) && check_depth && dep[u] > th_depth && counted[u] > 100) atomicMin(&s.brk, p);
  }
  __syncthreads();
  const int brk = s.brk;
  const int walked = brk == 0x7fffffff ? ne : brk + 1;  // the entry that breaks has been processed
  const int kf = kf_row[b];
#pragma unroll
  for (int u = 0; u < WALK_PER; ++u) {
    const int p = tid * WALK_PER + u;
    if (p >= walked) continue;
    const int i = feat[u], r = row[u];
    if (what[u] & 2) {
      const size_t o = f0 + r;
      new_feat[o] = i;
      for (int c = 0; c < 3; ++c) new_pos[o * 3 + c] = pts[(f0 + i) * 3 + c];
      new_assoc[o] = assoc[u];
      new_ref_kf[o] = kf;
      att_mp[o] = mp_base + r;
      att_kf[o] = kf;
      att_feat[o] = i;
      feat_new[f0 + i] = r;
    } else if (what[u] & 4) {
      feat_new[f0 + i] = -2;
    }
    if (p == walked - 1) {
      const int nn = r + ((what[u] >> 1) & 1);
      n_new[b] = nn;
      int32_t* st = stats + (size_t)b * 8;
      st[0] = ne;
      st[1] = walked;
      st[2] = nn;
      st[3] = walked - counted[u];
      st[4] = counted[u];
      st[5] = brk != 0x7fffffff;
      st[6] = 0;
      st[7] = 0;
    }
  }
  if (walked == 0 && tid == 0) {
    n_new[b] = 0;
    for (int c = 0; c < 8; ++c) stats[(size_t)b * 8 + c] = c == 0 ? ne : 0;
  }
}

__global__ __launch_bounds__(WALK_T) void k_temporal_walk(UnK k, int NF, float th_depth, const double* __restrict__ pose,
                                                          const double* __restrict__ feat_uv, const float* __restrict__ feat_depth,
                                                          const int32_t* __restrict__ feat_oct, const uint8_t* __restrict__ held,
                                                          const uint8_t* __restrict__ last_outlier, const uint8_t* __restrict__ feat_desc,
                                                          uint8_t* __restrict__ temp_flag, int32_t* __restrict__ n_temp,
                                                          double* __restrict__ last_pt, uint8_t* __restrict__ last_observed,
                                                          uint8_t* __restrict__ last_valid, uint8_t* __restrict__ last_desc,
                                                          int32_t* __restrict__ stats, int32_t* __restrict__ last_mp) {
  __shared__ WalkShared s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t f0 = (size_t)b * NF;
  const int ne = sort_entries(s.key, &s.cnt, NF, feat_depth + f0, feat_oct + f0, tid);
  for (int i = tid; i < NF; i += WALK_T) temp_flag[f0 + i] = 0;
  // every entry is counted (tracking.cpp:456-459): num_pts at sorted position p is p + 1, and the depths ascend, so the first
  // position with `depth > th_depth && num_pts > 100` (:462) is found by looking at each position alone
  if (tid == 0) s.brk = 0x7fffffff;
  __syncthreads();
  for (int p = tid; p < ne; p += WALK_T)
    if (__uint_as_float((unsigned)(s.key[p] >> 32)) > th_depth && p + 1 > 100) atomicMin(&s.brk, p);
  __syncthreads();
  const int brk = s.brk;
  const int walked = brk == 0x7fffffff ? ne : brk + 1;
  int made = 0;
  const SE3 Twc = se3_inverse(se3_load(pose + (size_t)b * 7));
  for (int p = tid; p < walked; p += WALK_T) {
    const u64 key = s.key[p];
    const size_t g = f0 + (unsigned)key;
    if (held[g] == 1) continue;  // a point with observations stays (:437-443)
    double x[3];
    unproject(k, Twc, feat_uv[g * 2], feat_uv[g * 2 + 1], __uint_as_float((unsigned)(key >> 32)), x);
    for (int c = 0; c < 3; ++c) last_pt[g * 3 + c] = x[c];
    last_observed[g] = 0;
    last_valid[g] = last_outlier[g] ? 0 : 1;  // orb_matcher.cpp:432 reads the slot's is_outlier_, which nothing has cleared
    for (int c = 0; c < 32; ++c) last_desc[g * 32 + c] = feat_desc[g * 32 + c];
    temp_flag[g] = 1;
    if (last_mp) last_mp[g] = -1;  // mappoints_[i] is the temporal point now (:453): no row
    ++made;
  }
  u64 total;
  gl::mapdev::block_excl_scan<WALK_T, u64>((u64)made, s.scan, tid, &total);
  if (tid == 0) {
    n_temp[b] = (int)total;
    if (stats) {
      int32_t* st = stats + (size_t)b * 8;
      st[0] = ne;
      st[1] = walked;
      st[2] = (int)total;
      st[3] = 0;
      st[4] = walked;
      st[5] = brk != 0x7fffffff;
      st[6] = 0;
      st[7] = 0;
    }
  }
}

UnK make_unk(const gl_camera* cam) { return UnK{cam->fx, cam->fy, cam->cx, cam->cy}; }

}  // namespace

extern "C" {

int gl_create_stereo_points(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, const gl_params* prm, int B, int NF, int k,
                            const gl_stereo_points_in* in, int mp_base, int check_depth, float th_depth,
                            const gl_stereo_points_out* out) {
  GL_REQUIRE(ctx && gmm && cam && prm && in && out, "null argument");
  if (B == 0 || NF == 0) return GL_OK;
  GL_REQUIRE(B > 0 && NF > 0 && k >= 1 && k <= 8 && mp_base >= 0, "bad B / NF / k / mp_base");
  GL_REQUIRE(NF <= GL_STEREO_WALK_MAX, "more than GL_STEREO_WALK_MAX features per key-frame");
  GL_REQUIRE((size_t)B * NF * 16 <= 0x7fffffffull, "B x NF too large");
  GL_REQUIRE(in->pose && in->feat_uv && in->feat_ur && in->feat_depth && in->feat_oct && in->cand && in->ncand && in->held && in->kf_row,
             "null input buffer");
  GL_REQUIRE(out->new_feat && out->new_pos && out->new_assoc && out->new_ref_kf && out->att_mp && out->att_kf && out->att_feat &&
                 out->n_new && out->feat_new && out->stats,
             "null output buffer (only pts0 is optional)");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  const size_t n = (size_t)B * NF;
  gl::Regions rg{0};
  const size_t o_pts = rg.take(n * 24), o_uvr = rg.take(n * 24), o_oct = rg.take(n * 4), o_comp = rg.take(n * 4);
  void* scratch = nullptr;
  const int rc = gl::ctx_scratch(c, rg.off, &scratch);
  if (rc != GL_OK) return rc;
  double* pts = (double*)((char*)scratch + o_pts);
  double* uvr = (double*)((char*)scratch + o_uvr);
  int32_t* octm = (int32_t*)((char*)scratch + o_oct);
  int32_t* comp = (int32_t*)((char*)scratch + o_comp);
  k_stereo_prep<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(make_unk(cam), B, NF, in->pose, in->feat_uv, in->feat_ur, in->feat_depth,
                                                                    in->feat_oct, in->ncand, in->held, pts, out->pts0, uvr, octm);
  GL_HIP(hipGetLastError());
  const int rc2 = gl::launch_check_map_association(c, gl::G(gmm), cam, prm, B, NF, in->pose, pts, uvr, octm, in->cand, in->ncand, k, comp);
  if (rc2 != GL_OK) return rc2;
  k_stereo_walk<<<B, WALK_T, 0, c->stream>>>(NF, mp_base, check_depth != 0, th_depth, in->feat_depth, in->feat_oct, in->ncand, in->held,
                                             in->kf_row, comp, (const u64*)pts, out->new_feat, (u64*)out->new_pos, out->new_assoc,
                                             out->new_ref_kf, out->att_mp, out->att_kf, out->att_feat, out->n_new, out->feat_new,
                                             out->stats);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_create_temporal_points(gl_ctx_t* ctx, const gl_camera* cam, int B, int NF, const gl_temporal_points_in* in, float th_depth,
                              const gl_temporal_points_out* out) {
  GL_REQUIRE(ctx && cam && in && out, "null argument");
  if (B == 0 || NF == 0) return GL_OK;
  GL_REQUIRE(B > 0 && NF > 0, "bad B / NF");
  GL_REQUIRE(NF <= GL_STEREO_WALK_MAX, "more than GL_STEREO_WALK_MAX features per frame");
  GL_REQUIRE(in->pose && in->feat_uv && in->feat_depth && in->feat_oct && in->held && in->last_outlier && in->feat_desc, "null input buffer");
  GL_REQUIRE(out->temp_flag && out->n_temp && out->last_pt && out->last_observed && out->last_valid && out->last_desc,
             "null output buffer (only stats is optional)");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  k_temporal_walk<<<B, WALK_T, 0, c->stream>>>(make_unk(cam), NF, th_depth, in->pose, in->feat_uv, in->feat_depth, in->feat_oct, in->held,
                                               in->last_outlier, in->feat_desc, out->temp_flag, out->n_temp, out->last_pt,
                                               out->last_observed, out->last_valid, out->last_desc, out->stats, out->last_mp);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

}  // extern "C"
