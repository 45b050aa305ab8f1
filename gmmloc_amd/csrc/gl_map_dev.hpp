// The resident map as the kernels see it (gl_ba_window.hip, gl_map_edit.hip, gl_map_grow.hip, gl_map_stats.hip): ONE description of the
// caller-owned arrays, one copy of each rule that reads them, and the rebuild of the CSR that gl_map_remove, gl_map_add and gl_map_fuse
// share.  The C-ABI hands the same arrays over as gl_map_view + gl_map_ba_view or as sizes + gl_map_edit; map_from_view / map_from_edit
// turn either into a Map and carry the argument checks every entry point has in common; stats_from_c does the same for the counters and
// the candidate list of gl_map_stats (gl_localmap.hip takes those and the workgroup scan; its kernel keeps the view and its own
// spelling of the rules, see there).
#pragma once
#include "gl_internal.hpp"

namespace gl {
namespace mapdev {

typedef unsigned long long u64;

// Row-indexed as in gmmloc_hip.h; a field the entry point's form does not carry is null (kf_first: -1).  The pointers are plain: a
// kernel that only reads takes its arguments const.
struct Map {
  int NMP, NKF, NFK, NOBS;
  uint8_t* mp_valid;  // null = all valid (gl_map_view only; gl_map_edit requires it)
  uint8_t* kf_valid;  // null = all valid (gl_map_view only)
  int32_t* kf_mp;     // NKF x NFK
  int32_t *obs_ptr, *obs_kf, *obs_feat;
  int32_t *mp_ref_kf, *mp_assoc;
  double *kf_pose, *kf_twc;
  const double* kf_uvr;  // NKF x NFK x 3
  const int32_t* kf_oct;
  int kf_first;
  double* mp_pos;  // read by gl_ba_window_build, new rows written by gl_map_add
};

// ---- host: the two forms of the C-ABI -> Map, with the checks they share.  `who` is the entry point the message names.
#define GL_MAP_REQUIRE(cond, msg)            \
  do {                                       \
    if (!(cond)) {                           \
      gl::set_error("%s: %s", who, msg);     \
      return GL_ERR_ARG;                     \
    }                                        \
  } while (0)
inline int map_check_sizes(const char* who, int NMP, int NKF, int NFK, int NOBS, const void* obs_ptr, const void* obs_kf, const void* kf_mp) {
  GL_MAP_REQUIRE(NMP >= 0 && NKF >= 0 && NFK >= 0 && NOBS >= 0, "bad NMP / NKF / NFK / NOBS");
  GL_MAP_REQUIRE((int64_t)NKF * NFK < ((int64_t)1 << 31), "NKF x NFK must be below 2^31");
  GL_MAP_REQUIRE(obs_ptr, "null obs_ptr");
  GL_MAP_REQUIRE(NOBS == 0 || obs_kf, "null obs_kf");
  GL_MAP_REQUIRE(NKF == 0 || NFK == 0 || kf_mp, "null kf_mp");
  return GL_OK;
}
// ba may be null (the tracker's entry points); with it, what every reader of gl_map_ba_view needs of it
inline int map_from_view(const char* who, const gl_map_view* v, const gl_map_ba_view* ba, Map* m) {
  GL_MAP_REQUIRE(v, "null argument");
  const int rc = map_check_sizes(who, v->NMP, v->NKF, v->NFK, v->NOBS, v->obs_ptr, v->obs_kf, v->kf_mp);
  if (rc != GL_OK) return rc;
  *m = Map{};
  m->NMP = v->NMP, m->NKF = v->NKF, m->NFK = v->NFK, m->NOBS = v->NOBS;
  m->mp_valid = (uint8_t*)v->mp_valid;
  m->kf_valid = (uint8_t*)v->kf_valid;
  m->kf_mp = (int32_t*)v->kf_mp;
  m->obs_ptr = (int32_t*)v->obs_ptr;
  m->obs_kf = (int32_t*)v->obs_kf;
  m->mp_pos = (double*)v->mp_pos;
  m->kf_first = -1;
  if (ba) {
    GL_MAP_REQUIRE(v->NOBS == 0 || ba->obs_feat, "null obs_feat");
    GL_MAP_REQUIRE(v->NKF == 0 || v->NFK == 0 || (ba->kf_uvr && ba->kf_oct), "null kf_uvr / kf_oct");
    m->obs_feat = (int32_t*)ba->obs_feat;
    m->mp_assoc = ba->mp_assoc;
    m->kf_pose = ba->kf_pose;
    m->kf_twc = ba->kf_twc;
    m->kf_uvr = ba->kf_uvr;
    m->kf_oct = ba->kf_oct;
    m->kf_first = ba->kf_first;
  }
  return GL_OK;
}
// kf_uvr may be null here (gl_map_add reads no weight): an entry point that needs it says so itself, like kf_valid and the capacities
inline int map_from_edit(const char* who, int NMP, int NKF, int NFK, int NOBS, const gl_map_edit* ed, const double* kf_uvr, int kf_first, Map* m) {
  GL_MAP_REQUIRE(ed, "null argument");
  const int rc = map_check_sizes(who, NMP, NKF, NFK, NOBS, ed->obs_ptr, ed->obs_kf, ed->kf_mp);
  if (rc != GL_OK) return rc;
  GL_MAP_REQUIRE(NMP == 0 || ed->mp_valid, "null mp_valid");
  GL_MAP_REQUIRE(NOBS == 0 || ed->obs_feat, "null obs_feat");
  *m = Map{};
  m->NMP = NMP, m->NKF = NKF, m->NFK = NFK, m->NOBS = NOBS;
  m->mp_valid = ed->mp_valid;
  m->kf_valid = ed->kf_valid;
  m->kf_mp = ed->kf_mp;
  m->obs_ptr = ed->obs_ptr;
  m->obs_kf = ed->obs_kf;
  m->obs_feat = ed->obs_feat;
  m->mp_ref_kf = ed->mp_ref_kf;
  m->kf_uvr = kf_uvr;
  m->kf_first = kf_first;
  return GL_OK;
}
// The counters and the candidate list of gl_map_stats (gl_map_stats.hip) as the kernels see them: NMP = the rows that count, NMPcap =
// the rows the arrays have.  A field the entry point does not need may be null; stats_from_c says which it needs.
struct Stats {
  int NMP, NMPcap, NKF;
  int32_t *visible, *found, *ref_idx;
  const int32_t* kf_idx;  // null = the row itself
  int32_t *cand, *n_cand;
  int cand_cap;
};
enum { STATS_COUNTERS = 1, STATS_REF = 2, STATS_CAND = 4 };
inline int stats_from_c(const char* who, const gl_map_stats* st, int NMP, int NMPcap, int NKF, int need, Stats* s) {
  GL_MAP_REQUIRE(st, "null gl_map_stats");
  GL_MAP_REQUIRE(NMP >= 0 && NMPcap >= NMP && NKF >= 0, "bad NMP / NMPcap / NKF");
  GL_MAP_REQUIRE(!(need & STATS_COUNTERS) || NMPcap == 0 || (st->mp_visible && st->mp_found), "null mp_visible / mp_found");
  GL_MAP_REQUIRE(!(need & STATS_REF) || NMPcap == 0 || st->mp_ref_idx, "null mp_ref_idx");
  GL_MAP_REQUIRE(!(need & STATS_CAND) || (st->cand_cap >= 0 && st->n_cand && (st->cand_cap == 0 || st->cand)), "bad cand_cap / null cand / n_cand");
  *s = Stats{};
  s->NMP = NMP, s->NMPcap = NMPcap, s->NKF = NKF;
  s->visible = st->mp_visible, s->found = st->mp_found, s->ref_idx = st->mp_ref_idx;
  s->kf_idx = st->kf_idx;
  s->cand = st->cand, s->n_cand = st->n_cand, s->cand_cap = st->cand_cap;
  return GL_OK;
}
#undef GL_MAP_REQUIRE

// ---- device: the rules
__device__ __forceinline__ bool mp_row(const Map& m, int p) { return p >= 0 && p < m.NMP; }
__device__ __forceinline__ bool kf_row(const Map& m, int k) { return k >= 0 && k < m.NKF; }
// a (key-frame, feature) pair inside the key-frames' tables
__device__ __forceinline__ bool slot_in(const Map& m, int k, int f) { return kf_row(m, k) && f >= 0 && f < m.NFK; }
__device__ __forceinline__ bool mp_ok(const Map& m, int p) { return mp_row(m, p) && (!m.mp_valid || m.mp_valid[p]); }
__device__ __forceinline__ bool kf_ok(const Map& m, int k) { return !m.kf_valid || m.kf_valid[k]; }  // (k inside the table)
// the CSR range of point p, empty when it is not a sub-range of [0, NOBS]
__device__ __forceinline__ void obs_range(const Map& m, int p, int* o0, int* o1) {
  const int a = m.obs_ptr[p], b = m.obs_ptr[p + 1];
  const bool ok = a >= 0 && b >= a && b <= m.NOBS;
  *o0 = ok ? a : 0;
  *o1 = ok ? b : 0;
}
// what an observation adds to its point's WEIGHTED COUNT (gmmloc_hip.h, gl_cull_keyframes): 2 with a right coordinate, 1 monocular, 0
// outside the tables
__device__ __forceinline__ int obs_weight(const Map& m, int k, int f) {
  if (!slot_in(m, k, f)) return 0;
  return m.kf_uvr[((size_t)k * m.NFK + f) * 3 + 2] >= 0.0 ? 2 : 1;
}
// the length of a device list (gl_map_remove_lists): *n clamped to [0, cap] when n is given, else cap
__device__ __forceinline__ int list_len(const int32_t* n, int cap) { return n ? min(max(*n, 0), cap) : cap; }

// ---- device: workgroup primitives
// exclusive prefix sum of v over the workgroup's T threads; *total = the sum.  s_w: T / 64 words of LDS, free again on return.
template <int T, class V>
__device__ __forceinline__ V block_excl_scan(V v, V* s_w, int tid, V* total) {
  const int lane = tid & 63, w = tid >> 6;
  V inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const V t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  V base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < T / 64; ++i) {
    const V x = s_w[i];
    base += i < w ? x : 0;
    tot += x;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}
// the maximum of v over the workgroup's T threads (every thread).  s_b: T / 64 words of LDS, free again on return.
template <int T>
__device__ __forceinline__ u64 block_max(u64 v, u64* s_b, int tid) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const u64 t = __shfl_xor(v, o);
    v = t > v ? t : v;
  }
  if ((tid & 63) == 0) s_b[tid >> 6] = v;
  __syncthreads();
  u64 r = 0ull;
#pragma unroll
  for (int i = 0; i < T / 64; ++i) r = s_b[i] > r ? s_b[i] : r;
  __syncthreads();
  return r;
}
// words over the rows of a table, in LDS or - a table too large for it - in global memory with agent-scope atomic loads and stores
template <bool LDS>
struct Words {
  int* p;
  __device__ __forceinline__ int get(int i) const {
    if constexpr (LDS) return p[i];
    else return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void set(int i, int v) const {
    if constexpr (LDS) p[i] = v;
    else __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void add(int i) const { atomicAdd(p + i, 1); }
  __device__ __forceinline__ void min_(int i, int v) const { atomicMin(p + i, v); }
};
// the row of a key count << 32 | (0x7fffffff - row): the largest count, then the lowest row
__device__ __forceinline__ int best_row(u64 best) { return 0x7fffffff - (int)(unsigned)(best & 0xffffffffull); }

// ---- KeyFrame::updateConnections' counter and its order (gl_ba_window.hip: gl_update_connections, gl_ba_window_build; gl_covis.hip:
// gl_covis_update).  One workgroup of T_CONN threads per key-frame.
constexpr int T_CONN = 1024;
constexpr int CONN_TH = 15;  // keyframe.cpp:280
// (a) + (b) of the connections: on return the counters hold map_frame_weights_, n15 = the observers that reach the threshold and
// best = count << 32 | (0x7fffffff - row) of the largest count at the lowest row (0: empty counter).  The counters are zero on entry.
template <bool LDS>
__device__ __forceinline__ void conn_count(const Map& m, int kf, Words<LDS> cnt, int tid, int* s_w, u64* s_b, int* n15, u64* best) {
  const int32_t* row = m.kf_mp + (size_t)kf * m.NFK;
  for (int j = tid; j < m.NFK; j += T_CONN) {
    const int p = row[j];
    if (!mp_ok(m, p)) continue;
    int o0, o1;
    obs_range(m, p, &o0, &o1);
    for (int o = o0; o < o1; ++o) {
      const int k = m.obs_kf[o];
      if (!kf_row(m, k) || k == kf) continue;  // (:268-269)
      cnt.add(k);
    }
  }
  if constexpr (!LDS) __threadfence();
  __syncthreads();
  const int ck = (m.NKF + T_CONN - 1) / T_CONN;
  const int k0 = min(tid * ck, m.NKF), k1 = min(k0 + ck, m.NKF);
  int n = 0, tot;
  u64 b = 0ull;
  for (int k = k0; k < k1; ++k) {
    const int c = cnt.get(k);
    if (c <= 0) continue;
    n += c >= CONN_TH;
    const u64 key = ((u64)(unsigned)c << 32) | (unsigned)(0x7fffffff - k);
    b = key > b ? key : b;
  }
  block_excl_scan<T_CONN>(n, s_w, tid, &tot);
  *n15 = tot;
  *best = block_max<T_CONN>(b, s_b, tid);
}
// is key-frame k (count c) in ordered_keyframes_ (:287-300)
__device__ __forceinline__ bool conn_keep(int k, int c, int n15, int best_row) { return n15 > 0 ? c >= CONN_TH : k == best_row; }
// the order of ordered_keyframes_ as a key, smaller first: weight descending, then the lowest row (never 0)
__device__ __forceinline__ u64 conn_key(int k, int c) { return (((u64)(unsigned)(0x7fffffff - c) << 32) | (unsigned)k) + 1ull; }

// The place of every SELECTED key-frame among the selected ones, by key: sel(k) = its key (distinct, non-zero) or 0, out(k, rank).
// A contiguous run of key-frames per thread; the selected ones are compacted into LDS (RANK_LDS of them: a covisible list or a set of
// fixed key-frames is tens of rows) and each counts the keys below its own; a larger selection counts over the whole table instead.
// Returns their number.  Ends with a fence and a barrier.
constexpr int RANK_LDS = 1024;
struct RankLds {
  u64 key[RANK_LDS];
  int row[RANK_LDS];
};
template <class Sel, class Out>
__device__ __forceinline__ int rank_selected(int NKF, int tid, int* s_w, RankLds& s, Sel sel, Out out) {
  const int ck = (NKF + T_CONN - 1) / T_CONN;
  const int k0 = min(tid * ck, NKF), k1 = min(k0 + ck, NKF);
  int n = 0;
  for (int k = k0; k < k1; ++k) n += sel(k) != 0ull;
  int total;
  int at = block_excl_scan<T_CONN>(n, s_w, tid, &total);
  if (total <= RANK_LDS) {
    for (int k = k0; k < k1 && n > 0; ++k) {
      const u64 key = sel(k);
      if (!key) continue;
      s.key[at] = key;
      s.row[at++] = k;
    }
    __syncthreads();
    for (int i = tid; i < total; i += T_CONN) {
      const u64 key = s.key[i];
      int r = 0;
      for (int i2 = 0; i2 < total; ++i2) r += s.key[i2] < key;
      out(s.row[i], r);
    }
  } else {
    for (int k = k0; k < k1 && n > 0; ++k) {
      const u64 key = sel(k);
      if (!key) continue;
      int r = 0;
      for (int k2 = 0; k2 < NKF; ++k2) {
        const u64 key2 = sel(k2);
        r += key2 != 0ull && key2 < key;
      }
      out(k, r);
    }
  }
  __threadfence();
  __syncthreads();
  return total;
}

// ---- the device-wide exclusive scan of the rebuilds of the CSR: SCAN_TILE words per workgroup of SCAN_T threads, then ONE workgroup
// over the tiles' sums.  A word's place is cnt[i] + tile[i / SCAN_TILE] afterwards.
constexpr int SCAN_T = 1024, SCAN_PER = 4, SCAN_TILE = SCAN_T * SCAN_PER;
// workgroup b: the exclusive scan of cnt[0, n) inside tile b, the tile's sum to tile[b].  s_w: SCAN_T / 64 words of LDS.
__device__ __forceinline__ void tile_scan(u64* cnt, u64* tile, size_t n, u64* s_w, int tid, int b) {
  const size_t base = (size_t)b * SCAN_TILE + (size_t)tid * SCAN_PER;
  u64 v[SCAN_PER], sum = 0;
#pragma unroll
  for (int u = 0; u < SCAN_PER; ++u) {
    v[u] = base + u < n ? cnt[base + u] : 0ull;
    sum += v[u];
  }
  u64 total;
  u64 at = block_excl_scan<SCAN_T, u64>(sum, s_w, tid, &total);
#pragma unroll
  for (int u = 0; u < SCAN_PER; ++u) {
    if (base + u < n) cnt[base + u] = at;
    at += v[u];
  }
  if (tid == 0) tile[b] = total;
}
// one workgroup of SCAN_T threads: the exclusive scan of the tiles' sums in place; returns the grand total (every thread)
__device__ __forceinline__ u64 tile_scan_top(u64* tile, int ntile, u64* s_w, int tid) {
  u64 carry = 0;
  for (int i0 = 0; i0 < ntile; i0 += SCAN_T) {
    const int i = i0 + tid;
    const u64 v = i < ntile ? tile[i] : 0ull;
    u64 total;
    const u64 at = block_excl_scan<SCAN_T, u64>(v, s_w, tid, &total);
    if (i < ntile) tile[i] = carry + at;
    carry += total;
  }
  return carry;
}

// ---- the rebuild of the CSR (gl_map_remove, gl_map_add, gl_map_fuse): a word per point (its new entry count in the low half, whatever
// the entry point scans along with it in the high half) -> csr_rebuild_scan -> the entry point's own top kernel (tile_scan_top) -> a
// point per thread moves its entries with csr_move_point, out of the copy of obs_kf / obs_feat that csr_rebuild_begin made, and fills
// nptr, which replaces obs_ptr last.
struct CsrRebuild {
  u64 *cnt, *tile;        // per point, per tile of SCAN_TILE points (and one spare word)
  int32_t *okf, *ofeat;   // NOBS: obs_kf / obs_feat as they were
  int32_t* nptr;          // points + 1
};
inline int csr_tiles(int npoint) { return (npoint + SCAN_TILE - 1) / SCAN_TILE; }
// bytes of a rebuild over npoint points and NOBS old entries; with a base (256-aligned) the pointers into it
inline size_t csr_rebuild_place(void* base, int npoint, int NOBS, CsrRebuild* out) {
  Regions r = {0};
  const size_t o_cnt = r.take((size_t)npoint * 8), o_tile = r.take((size_t)csr_tiles(npoint) * 8 + 8), o_okf = r.take((size_t)NOBS * 4),
               o_ofeat = r.take((size_t)NOBS * 4), o_nptr = r.take(((size_t)npoint + 1) * 4);
  if (base && out) {
    char* s = (char*)base;
    out->cnt = (u64*)(s + o_cnt);
    out->tile = (u64*)(s + o_tile);
    out->okf = (int32_t*)(s + o_okf);
    out->ofeat = (int32_t*)(s + o_ofeat);
    out->nptr = (int32_t*)(s + o_nptr);
  }
  return r.off;
}
// the copy the move reads, and obs_new_pos (null allowed) reset to -1
inline int csr_rebuild_begin(Ctx* c, const CsrRebuild& rb, const Map& m, int32_t* obs_new_pos) {
  if (m.NOBS == 0) return GL_OK;
  GL_HIP(hipMemcpyAsync(rb.okf, m.obs_kf, (size_t)m.NOBS * 4, hipMemcpyDeviceToDevice, c->stream));
  GL_HIP(hipMemcpyAsync(rb.ofeat, m.obs_feat, (size_t)m.NOBS * 4, hipMemcpyDeviceToDevice, c->stream));
  if (obs_new_pos) GL_HIP(hipMemsetAsync(obs_new_pos, 0xff, (size_t)m.NOBS * 4, c->stream));
  return GL_OK;
}
// (gl_map_edit.hip) tile_scan over cnt[0, n) in ntile workgroups: n = *n_dev when n_dev is given (gl_map_add knows it on the device only),
// else n_host
void csr_rebuild_scan(Ctx* c, const CsrRebuild& rb, int ntile, const int32_t* n_dev, int n_host);
// the scanned word of point p: its first new position in the low half
__device__ __forceinline__ u64 csr_place(const CsrRebuild& rb, int p) { return rb.cnt[p] + rb.tile[p / SCAN_TILE]; }
// Point p of the rebuild: nptr[p], then its old entries that keep(o) passes, in order, each recorded in obs_new_pos (null allowed),
// then what gained(put) adds - put(k, f) appends an entry and returns its position.  Nothing is stored at or behind `limit`: put
// returns -1 there and the move ends (the ranges of a malformed CSR may overlap, and then the scanned places run past the arrays).
// A row at or above m.NMP (gl_map_add's new points) and a range outside [0, NOBS] have no old entries.
template <class Keep, class Gained>
__device__ __forceinline__ void csr_move_point(const Map& m, const CsrRebuild& rb, int p, int limit, int32_t* obs_new_pos, Keep keep, Gained gained) {
  int to = (int)(unsigned)(csr_place(rb, p) & 0xffffffffull);
  rb.nptr[p] = to;
  auto put = [&](int k, int f) -> int {
    if (to >= limit) return -1;
    m.obs_kf[to] = k;
    m.obs_feat[to] = f;
    return to++;
  };
  if (p < m.NMP) {
    int o0, o1;
    obs_range(m, p, &o0, &o1);
    for (int o = o0; o < o1; ++o) {
      if (!keep(o)) continue;  // (its obs_new_pos stays -1)
      const int at = put(rb.okf[o], rb.ofeat[o]);
      if (at < 0) return;
      if (obs_new_pos) obs_new_pos[o] = at;
    }
  }
  gained(put);
}

}  // namespace mapdev
}  // namespace gl
