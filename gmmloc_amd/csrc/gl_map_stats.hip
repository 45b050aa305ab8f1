// The resident map's found / visible counters and Localization::removeMapPoints (gmmloc_hip.h, gl_map_stats): num_visible_ /
// num_found_ / ref_idx_ per map point and candidate_mappts_ as device arrays beside gl_map_edit's, kept current from the outputs of
// gl_track_frame_chain_map, gl_map_add and gl_map_fuse.  The rule table with the reference's lines is in the header.
//   track       blocks of a frame stride over its features, then over its local-map slots: no-return agent-scope atomicAdd.
//   new points  a row per thread.
//   append      one workgroup: the old length is read once, the rows are copied behind it, thread 0 stores the new length.
//   merge       the sequential one.  One workgroup; per MERGE_STEPS steps: every entry of the 2 x MERGE_STEPS rows finds the first
//               entry that names its row (its SLOT), the slots' counters are gathered into LDS, ONE lane walks the steps there in
//               order, the slots are scattered back.  The next chunk gathers what this one scattered.
//   cull        (a) k_mc_mark: the list index of every row's first occurrence (atomicMin on a word per point); (b) k_mc_judge: a
//               candidate per thread judges its row on the snapshot - a later occurrence of a row judges it again and reads a
//               removal as "invalid" -, the verdict, a copy of the entry, kept | removed << 32 for the scan; (c) mapdev's tile scan
//               and k_mc_top: the totals and the new length; (d) k_mc_move: kept entries and removed rows to their places.
// Everything is integer but the one float division of the ratio test; the atomics are atomicAdd (wrap-around sums, order-free),
// atomicMin and atomicOr on words whose final value the inputs determine.
#include "gl_map_dev.hpp"

namespace {

using namespace gl::mapdev;  // Map, Stats, mp_row, kf_row, obs_range, obs_weight, list_len, tile_scan_top, CsrRebuild, csr_rebuild_scan

constexpr int T_ST = 256;
constexpr int T_ONE = 1024;        // the one-workgroup kernels
constexpr int MERGE_STEPS = 1024;  // steps per chunk of the merge: 2 x MERGE_STEPS slots of 16 bytes and a word per step in LDS (36 KB)
static_assert(MERGE_STEPS == T_ONE, "k_ms_merge: a thread owns the entries tid and tid + T_ONE of a chunk");

__device__ __forceinline__ bool st_row(const Stats& s, int p) { return p >= 0 && p < s.NMP; }
// (the counters wrap like fetch_add on atomic_int: unsigned arithmetic)
__device__ __forceinline__ void st_add1(int32_t* w) { atomicAdd((unsigned*)w, 1u); }

// ---------------------------------------------------------------------------------------------------------------- track
struct TrackArgs {
  Stats s;
  int B, NF, NPcap;
  const int32_t *feat_mp, *match_local, *local_mp, *n_local_mp, *counts2;
  const uint8_t *outlier, *inview;
};

__global__ __launch_bounds__(T_ST) void k_ms_track(TrackArgs a) {
  const int b = blockIdx.y;
  if (a.counts2 && a.counts2[(size_t)b * 4 + 3] == 2) return;  // lost: returns before the three rows (tracking.cpp:62-72)
  const int g = blockIdx.x * T_ST + threadIdx.x, G = gridDim.x * T_ST;
  const Stats& s = a.s;
  const int32_t* const fm = a.feat_mp + (size_t)b * a.NF;
  const int32_t* const ml = a.match_local + (size_t)b * a.NF;
  const uint8_t* const ol = a.outlier + (size_t)b * a.NF;
  const int32_t* const lm = a.local_mp + (size_t)b * a.NPcap;
  const uint8_t* const iv = a.inview + (size_t)b * a.NPcap;
  for (int i = g; i < a.NF; i += G) {
    const int held = fm[i];
    if (st_row(s, held)) st_add1(s.visible + held);  // (:213-225, per feature)
    if (ol[i]) continue;
    const int j = ml[i];
    const int r = j >= 0 ? (j < a.NPcap ? lm[j] : -1) : held;
    if (st_row(s, r)) st_add1(s.found + r);  // (:279-292)
  }
  const int nl = min(max(a.n_local_mp[b], 0), a.NPcap);
  for (int i = g; i < nl; i += G) {
    if (!iv[i]) continue;
    const int r = lm[i];
    if (st_row(s, r)) st_add1(s.visible + r);  // (:249-254)
  }
}

// ---------------------------------------------------------------------------------------------------------------- new points
__global__ __launch_bounds__(T_ST) void k_ms_new(Stats s, int first, int n_host, const int32_t* n_dev, const int32_t* new_ref_kf, int32_t* status) {
  const int j = blockIdx.x * T_ST + threadIdx.x;
  if (j >= list_len(n_dev, n_host)) return;
  const long long row = (long long)first + j;
  if (row < 0 || row >= s.NMPcap) {
    atomicOr(status, GL_MAP_STATS_MP_TRUNCATED);
    return;
  }
  const int k = new_ref_kf[j];
  const bool in = k >= 0 && k < s.NKF;
  s.visible[row] = 1;  // (mappoint.cpp:18-19)
  s.found[row] = 1;
  s.ref_idx[row] = !in ? -1 : s.kf_idx ? s.kf_idx[k] : k;
}

// ---------------------------------------------------------------------------------------------------------------- append
__global__ __launch_bounds__(T_ONE) void k_ms_append(Stats s, const int32_t* rows, int first, int n_host, const int32_t* n_dev, int32_t* result) {
  const int tid = threadIdx.x;
  const int have = min(max(*s.n_cand, 0), s.cand_cap), n = list_len(n_dev, n_host);
  const long long want = (long long)have + n;
  const bool fits = want <= s.cand_cap;
  __syncthreads();  // (every thread has read *n_cand)
  if (fits)
    for (int i = tid; i < n; i += T_ONE) s.cand[have + i] = rows ? rows[i] : (int32_t)((unsigned)first + (unsigned)i);
  if (tid == 0) {
    if (fits) *s.n_cand = (int)want;
    result[0] = (int32_t)min(want, (long long)0x7fffffff);
    result[1] = fits ? 0 : GL_MAP_STATS_CAND_TRUNCATED;
  }
}

// ---------------------------------------------------------------------------------------------------------------- merge
__global__ __launch_bounds__(T_ONE) void k_ms_merge(Stats s, const int32_t* src, const int32_t* tgt, int n_host, const int32_t* n_dev) {
  __shared__ __attribute__((aligned(16))) int s_row[2 * MERGE_STEPS];   // entry 2 i: the source of step i, 2 i + 1: its target (-1: outside the table)
  __shared__ int s_slot[2 * MERGE_STEPS];  // the first entry that names the same row
  __shared__ uint2 s_cnt[2 * MERGE_STEPS]; // per slot {visible, found}
  __shared__ int s_step[MERGE_STEPS];      // source slot << 16 | target slot; -1: the step changes nothing
  const int tid = threadIdx.x;
  const int n = list_len(n_dev, n_host);
  for (int c0 = 0; c0 < n; c0 += MERGE_STEPS) {
    const int nc = min(n - c0, MERGE_STEPS), ne = 2 * nc;
    for (int e = tid; e < ne; e += T_ONE) {
      const int r = (e & 1) ? tgt[c0 + (e >> 1)] : src[c0 + (e >> 1)];
      s_row[e] = st_row(s, r) ? r : -1;
    }
    __syncthreads();
    {  // the slot of the thread's two entries: the lowest entry with the same row.  Every lane reads the same four entries at a time
       // (an LDS broadcast), no early exit: the loads do not wait for the compares
      const int e0 = tid, e1 = tid + T_ONE;
      const int r0 = e0 < ne ? s_row[e0] : -1, r1 = e1 < ne ? s_row[e1] : -1;
      int f0 = e0, f1 = e1;
      for (int q = 0; q < ne; q += 4) {  // (ne is even and at most 2 MERGE_STEPS: q + 3 stays inside s_row; an entry at or behind
        const int4 v = *reinterpret_cast<const int4*>(s_row + q);  // ne is stale and never below f0 / f1)
        const int vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (vv[u] == r0 && q + u < f0) f0 = q + u;
          if (vv[u] == r1 && q + u < f1) f1 = q + u;
        }
      }
      if (e0 < ne) {
        if (r0 < 0) f0 = e0;
        else if (f0 == e0) s_cnt[e0] = make_uint2((unsigned)s.visible[r0], (unsigned)s.found[r0]);
        s_slot[e0] = f0;
      }
      if (e1 < ne) {
        if (r1 < 0) f1 = e1;
        else if (f1 == e1) s_cnt[e1] = make_uint2((unsigned)s.visible[r1], (unsigned)s.found[r1]);
        s_slot[e1] = f1;
      }
    }
    __syncthreads();
    for (int i = tid; i < nc; i += T_ONE) {
      const int x = s_slot[2 * i], y = s_slot[2 * i + 1];
      const bool skip = s_row[2 * i] < 0 || s_row[2 * i + 1] < 0 || x == y;  // (a row outside the table; map.cpp:113)
      s_step[i] = skip ? -1 : (x << 16 | y);
    }
    __syncthreads();
    if (tid == 0) {  // the walk in step order: one word per step, two 8-byte reads and one 8-byte write
      int w = s_step[0];
      for (int i = 0; i < nc; ++i) {
        const int next = i + 1 < nc ? s_step[i + 1] : -1;
        if (w >= 0) {
          const uint2 a = s_cnt[w >> 16];
          uint2 b = s_cnt[w & 0xffff];
          b.x += a.x;  // (:142-143)
          b.y += a.y;
          s_cnt[w & 0xffff] = b;
        }
        w = next;
      }
    }
    __syncthreads();
    for (int e = tid; e < ne; e += T_ONE) {
      const int r = s_row[e];
      if (r >= 0 && s_slot[e] == e) {
        s.visible[r] = (int32_t)s_cnt[e].x;
        s.found[r] = (int32_t)s_cnt[e].y;
      }
    }
    __syncthreads();  // (the next chunk gathers what this one stored: same workgroup, behind the barrier)
  }
}

// ---------------------------------------------------------------------------------------------------------------- cull
struct CullArgs {
  Map m;
  Stats s;
  int kf;
  int32_t *rm_mp, *n_rm, *verdict, *result;
  // scratch
  int32_t* first;  // NMP: the list index of the row's first occurrence (0x7f7f7f7f: not listed - one memset)
  int32_t* copy;   // cand_cap: the list as it was
  int32_t* n_old;  // its length
  u64 *cnt, *tile; // cand_cap, tiles + 1: kept | removed << 32
};

// removeMapPoints' branches for the valid-or-not row p on the snapshot (localization.cpp:133-150) -> 0 .. 4
__device__ __forceinline__ int mc_judge(const Map& m, const Stats& s, int p, int curr) {
  if (!m.mp_valid[p]) return 1;  // (:133)
  const float ratio = static_cast<float>(s.found[p]) / static_cast<float>(s.visible[p]);
  if (ratio < 0.25f) return 2;  // (:135)
  const long long age = (long long)curr - (long long)s.ref_idx[p];
  if (age >= 2) {  // (:139)
    int o0, o1, w = 0;
    obs_range(m, p, &o0, &o1);
    for (int o = o0; o < o1 && w <= 3; ++o) w += obs_weight(m, m.obs_kf[o], m.obs_feat[o]);
    if (w <= 3) return 3;
  }
  return age >= 3 ? 4 : 0;  // (:143)
}

__global__ __launch_bounds__(T_ST) void k_mc_mark(CullArgs a) {
  const int i = blockIdx.x * T_ST + threadIdx.x;
  const int n = min(max(*a.s.n_cand, 0), a.s.cand_cap);
  if (i == 0) *a.n_old = n;
  if (i >= n) return;
  const int p = a.s.cand[i];
  if (mp_row(a.m, p)) atomicMin(a.first + p, i);
}

__global__ __launch_bounds__(T_ST) void k_mc_judge(CullArgs a) {
  const int i = blockIdx.x * T_ST + threadIdx.x;
  if (i >= a.s.cand_cap) return;
  if (i >= *a.n_old) {
    a.cnt[i] = 0ull;
    return;
  }
  const int p = a.s.cand[i];
  a.copy[i] = p;
  int v = 5;
  bool removes = false;
  if (mp_row(a.m, p)) {
    const int curr = a.s.kf_idx ? a.s.kf_idx[a.kf] : a.kf;
    v = mc_judge(a.m, a.s, p, curr);
    if (v == 2 || v == 3) {
      if (a.first[p] == i) removes = true;
      else v = 1;  // its first occurrence removed it: not_valid_ here
    }
  } else {
    atomicOr(a.result + 3, GL_MAP_STATS_BAD_ROW);
  }
  a.verdict[i] = v;
  a.cnt[i] = (v == 0 ? 1ull : 0ull) | (removes ? 1ull << 32 : 0ull);
}

__global__ __launch_bounds__(SCAN_T) void k_mc_top(CullArgs a, int ntile) {
  __shared__ u64 s_w[SCAN_T / 64];
  const int tid = threadIdx.x;
  const u64 carry = tile_scan_top(a.tile, ntile, s_w, tid);
  if (tid == 0) {
    const int kept = (int)(unsigned)(carry & 0xffffffffull), removed = (int)(unsigned)(carry >> 32);
    a.result[0] = kept;
    a.result[1] = removed;
    a.result[2] = *a.n_old - kept - removed;
    *a.s.n_cand = kept;
    *a.n_rm = removed;
  }
}

__global__ __launch_bounds__(T_ST) void k_mc_move(CullArgs a) {
  const int i = blockIdx.x * T_ST + threadIdx.x;
  if (i >= *a.n_old) return;
  // (cnt holds the exclusive sums after the scan: what the entry itself added is read from its verdict again)
  const u64 at = a.cnt[i] + a.tile[i / SCAN_TILE];
  const int v = a.verdict[i], p = a.copy[i];
  if (v == 0) a.s.cand[(int)(unsigned)(at & 0xffffffffull)] = p;
  else if ((v == 2 || v == 3) && a.first[p] == i) a.rm_mp[(int)(unsigned)(at >> 32)] = p;
}

}  // namespace

extern "C" int gl_map_stats_track(gl_ctx_t* ctx, int NMP, const gl_map_stats* st, int B, int NF, int NPcap, const int32_t* feat_mp_dev,
                                  const int32_t* match_local_dev, const uint8_t* outlier_dev, const uint8_t* inview_dev, const int32_t* local_mp_dev,
                                  const int32_t* n_local_mp_dev, const int32_t* counts2_dev) {
  GL_REQUIRE(ctx, "null argument");
  GL_REQUIRE(B >= 0 && B <= 65535 && NF >= 0 && NPcap >= 0, "bad B / NF / NPcap");
  TrackArgs a = {};
  const int rc = stats_from_c(__func__, st, NMP, NMP, 0, STATS_COUNTERS, &a.s);
  if (rc != GL_OK) return rc;
  if (B == 0 || NMP == 0 || (NF == 0 && NPcap == 0)) return GL_OK;
  GL_REQUIRE(NF == 0 || (feat_mp_dev && match_local_dev && outlier_dev), "null feat_mp / match_local / outlier");
  GL_REQUIRE(n_local_mp_dev && (NPcap == 0 || (inview_dev && local_mp_dev)), "null inview / local_mp / n_local_mp");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  a.B = B, a.NF = NF, a.NPcap = NPcap;
  a.feat_mp = feat_mp_dev, a.match_local = match_local_dev, a.outlier = outlier_dev, a.inview = inview_dev;
  a.local_mp = local_mp_dev, a.n_local_mp = n_local_mp_dev, a.counts2 = counts2_dev;
  const int work = std::max(NF, NPcap);
  k_ms_track<<<dim3(std::min((work + T_ST - 1) / T_ST, 64), B), T_ST, 0, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_map_stats_new_points(gl_ctx_t* ctx, int NMPcap, int NKF, const gl_map_stats* st, int first, int n, const int32_t* n_dev,
                                       const int32_t* new_ref_kf_dev, int32_t* status_dev) {
  GL_REQUIRE(ctx && status_dev, "null argument");
  GL_REQUIRE(first >= 0 && n >= 0, "bad first / n");
  Stats s;
  const int rc = stats_from_c(__func__, st, 0, NMPcap, NKF, STATS_COUNTERS | STATS_REF, &s);
  if (rc != GL_OK) return rc;
  GL_REQUIRE(n == 0 || new_ref_kf_dev, "null new_ref_kf");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  GL_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), c->stream));
  if (n > 0) k_ms_new<<<(n + T_ST - 1) / T_ST, T_ST, 0, c->stream>>>(s, first, n, n_dev, new_ref_kf_dev, status_dev);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_map_cand_append(gl_ctx_t* ctx, const gl_map_stats* st, const int32_t* rows_dev, int first, int n, const int32_t* n_dev,
                                  int32_t* result_dev) {
  GL_REQUIRE(ctx && result_dev, "null argument");
  GL_REQUIRE(first >= 0 && n >= 0, "bad first / n");
  Stats s;
  const int rc = stats_from_c(__func__, st, 0, 0, 0, STATS_CAND, &s);
  if (rc != GL_OK) return rc;
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  k_ms_append<<<1, T_ONE, 0, c->stream>>>(s, rows_dev, first, n, n_dev, result_dev);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_map_stats_merge(gl_ctx_t* ctx, int NMP, const gl_map_stats* st, const int32_t* repl_src_dev, const int32_t* repl_tgt_dev, int n,
                                  const int32_t* n_dev) {
  GL_REQUIRE(ctx, "null argument");
  GL_REQUIRE(n >= 0, "bad n");
  Stats s;
  const int rc = stats_from_c(__func__, st, NMP, NMP, 0, STATS_COUNTERS, &s);
  if (rc != GL_OK) return rc;
  if (n == 0 || NMP == 0) return GL_OK;
  GL_REQUIRE(repl_src_dev && repl_tgt_dev, "null repl_src / repl_tgt");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  k_ms_merge<<<1, T_ONE, 0, c->stream>>>(s, repl_src_dev, repl_tgt_dev, n, n_dev);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_cull_map_points(gl_ctx_t* ctx, int NMP, int NKF, int NFK, int NOBS, const gl_map_edit* ed, const double* kf_uvr_dev,
                                  const gl_map_stats* st, int kf_row, int32_t* rm_mp_dev, int32_t* n_rm_dev, int32_t* verdict_dev, int32_t* result_dev) {
  GL_REQUIRE(ctx && ed && n_rm_dev && result_dev, "null argument");
  CullArgs a = {};
  int rc = map_from_edit(__func__, NMP, NKF, NFK, NOBS, ed, kf_uvr_dev, -1, &a.m);
  if (rc != GL_OK) return rc;
  rc = stats_from_c(__func__, st, NMP, NMP, NKF, STATS_COUNTERS | STATS_REF | STATS_CAND, &a.s);
  if (rc != GL_OK) return rc;
  GL_REQUIRE(NKF == 0 || NFK == 0 || kf_uvr_dev, "null kf_uvr");
  GL_REQUIRE(kf_row >= 0 && kf_row < NKF, "kf_row outside [0, NKF)");
  const int cap = a.s.cand_cap;
  GL_REQUIRE(cap == 0 || (rm_mp_dev && verdict_dev), "null rm_mp / verdict");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  a.kf = kf_row;
  a.rm_mp = rm_mp_dev, a.n_rm = n_rm_dev, a.verdict = verdict_dev, a.result = result_dev;
  const int ntile = csr_tiles(cap);
  gl::Regions r = {0};
  const size_t o_first = r.take((size_t)NMP * 4), o_copy = r.take((size_t)cap * 4), o_nold = r.take(4), o_cnt = r.take((size_t)cap * 8),
               o_tile = r.take((size_t)ntile * 8 + 8);
  void* scratch = nullptr;
  const int rs = gl::ctx_scratch(c, r.off, &scratch, gl::SCRATCH_MAPEDIT);
  if (rs != GL_OK) return rs;
  char* s = (char*)scratch;
  a.first = (int32_t*)(s + o_first);
  a.copy = (int32_t*)(s + o_copy);
  a.n_old = (int32_t*)(s + o_nold);
  a.cnt = (u64*)(s + o_cnt);
  a.tile = (u64*)(s + o_tile);
  GL_HIP(hipMemsetAsync(result_dev, 0, 4 * sizeof(int32_t), c->stream));
  if (NMP > 0) GL_HIP(hipMemsetAsync(a.first, 0x7f, (size_t)NMP * 4, c->stream));
  const int nb = std::max((cap + T_ST - 1) / T_ST, 1);
  k_mc_mark<<<nb, T_ST, 0, c->stream>>>(a);
  if (cap > 0) k_mc_judge<<<nb, T_ST, 0, c->stream>>>(a);
  CsrRebuild rb = {};
  rb.cnt = a.cnt, rb.tile = a.tile;
  csr_rebuild_scan(c, rb, ntile, nullptr, cap);
  k_mc_top<<<1, SCAN_T, 0, c->stream>>>(a, ntile);
  if (cap > 0) k_mc_move<<<nb, T_ST, 0, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}
