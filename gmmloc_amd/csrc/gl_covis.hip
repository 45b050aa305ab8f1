// The covisibility graph as part of the resident map (gmmloc_hip.h, gl_map_covis): KeyFrame::updateConnections WITH its addConnection
// on the other key-frames (keyframe.cpp:243-316, :116-150), the graph part of Map::removeKeyFrame (map.cpp:60-87, keyframe.cpp:318-330),
// getBestCovisibilityKeyFrames (:163-170), and the two lists of Localization::searchInNeighbors (localization.cpp:155-179, :188-206).
// A row of the graph is map_frame_weights_ in the declared order (weight descending, ties to the lowest row) and ordered_keyframes_ is
// its first cov_nord entries; the rules and the reproduced quirks are in the header.  Integer stores and integer atomics only.
//   update      one workgroup counts as gl_update_connections does (conn_count), ranks the WHOLE counter (rank_selected) into the
//               scratch, finds the widest row the call would produce and - when every row fits - writes the own row; then a
//               workgroup per listed observer: its row through LDS, the place of the new entry by counting the keys below it
//   remove      ONE workgroup walks the list; per listed row a wave per named row: find, shift left; then the row's own end
//   best        a workgroup per row: a copy of the prefix
//   targets     one wave: the double loop as written, membership by ballot over the list in LDS
//   candidates  a thread per (target position, slot): atomicMin of the position on the point's word, flags, the device-wide scan of
//               the CSR rebuilds, compaction (the pattern of gl_cull_map_points)
#include "gl_map_dev.hpp"

#include <algorithm>

namespace {

using namespace gl::mapdev;

constexpr int T_ADD = 256, T_RM = 1024, T_FC = 256;
constexpr int ADD_GRID = 64;
constexpr int TGT_MAX = 4096;  // nn + nn * nn2 at most

// the graph as the kernels see it: NKF rows count, entries of a row are cut to [0, Wcap]
struct Cov {
  int NKF, Wcap;
  int32_t *kf, *w, *n, *nord, *best;
};
__device__ __forceinline__ int cov_len(const Cov& c, int k) { return min(max(c.n[k], 0), c.Wcap); }
__device__ __forceinline__ int cov_ord(const Cov& c, int k) { return min(max(c.nord[k], 0), cov_len(c, k)); }
__device__ __forceinline__ bool cov_row(const Cov& c, int k) { return k >= 0 && k < c.NKF; }

__device__ __forceinline__ void fence_sync() {
  __threadfence();
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------- update
struct UpdArgs {
  Map m;
  Cov c;
  int kf, Ccap;
  int32_t *conn_kf, *conn_w, *n_conn, *result;
  // scratch
  int32_t* kf_words;        // NKF counters, or null: LDS
  int32_t *srt_kf, *srt_w;  // NKF: the counter in the declared order
  int32_t* n_sel;           // the observers the second kernel visits (0 after a refusal or an empty counter)
};

template <bool LDS>
__global__ __launch_bounds__(T_CONN) void k_covis_own(UpdArgs a) {
  extern __shared__ int cv_lds[];
  __shared__ int s_w[T_CONN / 64];
  __shared__ u64 s_b[T_CONN / 64];
  __shared__ RankLds s_rank;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NKF = a.m.NKF, kf = a.kf;
  const Words<LDS> cnt = {LDS ? cv_lds : a.kf_words};
  for (int k = tid; k < NKF; k += T_CONN) cnt.set(k, 0);
  if constexpr (!LDS) __threadfence();
  __syncthreads();
  int n15;
  u64 best;
  conn_count<LDS>(a.m, kf, cnt, tid, s_w, s_b, &n15, &best);
  if (!best) {  // (:275-276) nothing changes
    if (tid == 0) {
      a.n_conn[0] = 0;
      a.result[0] = 0, a.result[1] = GL_CONN_KEPT, a.result[2] = 0, a.result[3] = 0;
      *a.n_sel = 0;
    }
    return;
  }
  // ordered_keyframes_ is a prefix of the whole counter in the declared order: the entries >= 15, or entry 0 = the single largest
  const int nord = n15 > 0 ? n15 : 1;
  const int total = rank_selected(
      NKF, tid, s_w, s_rank,
      [&](int k) -> u64 {
        const int c = cnt.get(k);
        return c > 0 ? conn_key(k, c) : 0ull;
      },
      [&](int k, int r) {
        const int c = cnt.get(k);
        a.srt_kf[r] = k;
        a.srt_w[r] = c;
        if (r < nord && r < a.Ccap) {
          a.conn_kf[r] = k;
          a.conn_w[r] = c;
        }
      });
  // the widest row the call would produce: the own row, and every listed observer's with the entry it may gain
  int need = total;
  for (int i = wave; i < nord; i += T_CONN / 64) {
    const int k = a.srt_kf[i];
    const int m = cov_len(a.c, k);
    bool hit = false;
    for (int j = lane; j < m; j += 64) hit |= a.c.kf[(size_t)k * a.c.Wcap + j] == kf;
    need = max(need, m + (__any(hit) ? 0 : 1));
  }
  const int widest = (int)block_max<T_CONN>((u64)need, s_b, tid);
  const int cstat = nord > a.Ccap ? GL_CONN_TRUNCATED : 0;
  if (widest > a.c.Wcap) {  // the graph is left as it is
    if (tid == 0) {
      a.n_conn[0] = nord;
      a.result[0] = widest, a.result[1] = cstat | GL_COVIS_W_TRUNCATED, a.result[2] = 0, a.result[3] = 0;
      *a.n_sel = 0;
    }
    return;
  }
  for (int r = tid; r < total; r += T_CONN) {  // (:312)
    a.c.kf[(size_t)kf * a.c.Wcap + r] = a.srt_kf[r];
    a.c.w[(size_t)kf * a.c.Wcap + r] = a.srt_w[r];
  }
  if (tid == 0) {
    a.c.n[kf] = total;
    a.c.nord[kf] = nord;
    a.n_conn[0] = nord;
    a.result[0] = widest, a.result[1] = cstat, a.result[2] = 0, a.result[3] = 0;
    *a.n_sel = nord;
  }
}

// addConnection(kf, w) on the rows of the listed observers (keyframe.cpp:116-128 + updateBestCovisibles :130-150)
__global__ __launch_bounds__(T_ADD) void k_covis_add(UpdArgs a) {
  extern __shared__ int cv_lds[];  // 2 x Wcap: the row as it was
  __shared__ int s_pos, s_cnt;
  const int tid = threadIdx.x, W = a.c.Wcap, me = a.kf;
  int* const s_kf = cv_lds;
  int* const s_wt = cv_lds + W;
  const int n_sel = min(max(*a.n_sel, 0), a.m.NKF);
  for (int i = blockIdx.x; i < n_sel; i += gridDim.x) {
    const int k = a.srt_kf[i], w = a.srt_w[i];
    if (!cov_row(a.c, k)) continue;  // (cannot be: the counter's rows)
    const int m = cov_len(a.c, k);
    int32_t* const rk = a.c.kf + (size_t)k * W;
    int32_t* const rw = a.c.w + (size_t)k * W;
    if (tid == 0) s_pos = 0x7fffffff, s_cnt = 0;
    __syncthreads();
    for (int j = tid; j < m; j += T_ADD) {
      const int x = rk[j];
      s_kf[j] = x;
      s_wt[j] = rw[j];
      if (x == me) atomicMin(&s_pos, j);
    }
    __syncthreads();
    const int pos = s_pos == 0x7fffffff ? -1 : s_pos;
    const bool same = pos >= 0 && s_wt[pos] == w;  // (:123-124) nothing, the row's prefix stays
    const bool full = pos < 0 && m >= W;           // (cannot be: the first kernel refused)
    if (!same && !full) {
      const u64 key = conn_key(me, w);
      int below = 0;
      for (int j = tid; j < m; j += T_ADD) below += j != pos && conn_key(s_kf[j], s_wt[j]) < key;
      if (below) atomicAdd(&s_cnt, below);
      __syncthreads();
      const int dst = s_cnt;
      for (int j = tid; j < m; j += T_ADD) {
        if (j == pos) continue;
        const int j1 = j - (pos >= 0 && j > pos ? 1 : 0);
        const int to = j1 + (j1 >= dst ? 1 : 0);
        rk[to] = s_kf[j];
        rw[to] = s_wt[j];
      }
      if (tid == 0) {
        rk[dst] = me;
        rw[dst] = w;
        const int m2 = m + (pos < 0 ? 1 : 0);
        a.c.n[k] = m2;
        a.c.nord[k] = m2;  // updateBestCovisibles lists the WHOLE weight map
        atomicAdd(a.result + 2, 1);
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------- remove
struct RmArgs {
  Cov c;
  int kf_first, cap;
  const int32_t *rows, *n_rows;
  int32_t* result;
};

__global__ __launch_bounds__(T_RM) void k_covis_remove(RmArgs a) {
  __shared__ int s_erased, s_bad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = a.c.Wcap;
  if (tid == 0) s_erased = 0, s_bad = 0;
  __syncthreads();
  const int n = list_len(a.n_rows, a.cap);
  int removed = 0, status = 0;  // (thread 0's count)
  for (int i = 0; i < n; ++i) {
    const int r = a.rows[i];
    if (!cov_row(a.c, r)) {
      if (tid == 0) atomicAdd(&s_bad, 1);
      continue;
    }
    if (r == a.kf_first) continue;  // (map.cpp:63)
    const int m = cov_len(a.c, r);
    const int32_t* const rr = a.c.kf + (size_t)r * W;
    for (int j = wave; j < m; j += T_RM / 64) {  // (:67-68) removeConnection(r) on every row r names
      const int k = rr[j];
      if (!cov_row(a.c, k)) {
        if (lane == 0) atomicAdd(&s_bad, 1);
        continue;
      }
      if (k == r) continue;
      bool dup = false;  // (a malformed row that names k twice: its first entry does the work)
      for (int j0 = lane; j0 < j; j0 += 64) dup |= rr[j0] == k;
      if (__any(dup)) continue;
      const int mk = cov_len(a.c, k);
      int32_t* const rk = a.c.kf + (size_t)k * W;
      int32_t* const rw = a.c.w + (size_t)k * W;
      int pos = -1;
      for (int base = 0; base < mk; base += 64) {
        const int jj = base + lane;
        const u64 mask = __ballot(jj < mk && rk[jj] == r);
        if (mask) {
          pos = base + __ffsll((unsigned long long)mask) - 1;
          break;
        }
      }
      if (pos < 0) continue;  // (keyframe.cpp:322)
      for (int base = pos; base < mk - 1; base += 64) {  // the wave moves 64 entries at a time, each chunk read before it is written
        const int jj = base + lane;
        const bool in = jj < mk - 1;
        const int x = in ? rk[jj + 1] : 0, y = in ? rw[jj + 1] : 0;
        if (in) {
          rk[jj] = x;
          rw[jj] = y;
        }
      }
      if (lane == 0) {
        a.c.n[k] = mk - 1;
        a.c.nord[k] = mk - 1;  // updateBestCovisibles lists the WHOLE weight map
        atomicAdd(&s_erased, 1);
      }
    }
    fence_sync();
    if (tid == 0) {  // (:82-84)
      if (cov_ord(a.c, r) > 0) a.c.best[r] = rr[0];
      else status |= GL_COVIS_EMPTY_LIST;  // the reference indexes an empty vector here: best_cov stays
      a.c.n[r] = 0;
      a.c.nord[r] = 0;
      ++removed;
    }
    fence_sync();
  }
  __syncthreads();
  if (tid == 0) {
    a.result[0] = removed;
    a.result[1] = status | (s_bad ? GL_COVIS_BAD_ROW : 0);
    a.result[2] = s_erased;
    a.result[3] = s_bad;
  }
}

// ---------------------------------------------------------------------------------------------------------------- best
struct BestArgs {
  Cov c;
  int B, N, Ccap;
  const int32_t* kf_row;
  int32_t *conn_kf, *conn_w, *n_conn, *result;
};

__global__ __launch_bounds__(T_ADD) void k_covis_best(BestArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  const int k = a.kf_row[b];
  if (!cov_row(a.c, k)) {
    if (tid == 0) {
      a.n_conn[b] = 0;
      atomicOr(a.result + 1, GL_COVIS_BAD_ROW);
      atomicAdd(a.result + 3, 1);
    }
    return;
  }
  const int nord = cov_ord(a.c, k);
  const int n = a.N <= 0 ? nord : min(a.N, nord);  // (keyframe.cpp:165-169)
  for (int j = tid; j < min(n, a.Ccap); j += T_ADD) {
    a.conn_kf[(size_t)b * a.Ccap + j] = a.c.kf[(size_t)k * a.c.Wcap + j];
    a.conn_w[(size_t)b * a.Ccap + j] = a.c.w[(size_t)k * a.c.Wcap + j];
  }
  if (tid == 0) {
    a.n_conn[b] = n;
    if (n > a.Ccap) atomicOr(a.result + 1, GL_CONN_TRUNCATED);
  }
}

// ---------------------------------------------------------------------------------------------------------------- targets
struct TgtArgs {
  Cov c;
  const uint8_t* kf_valid;
  int kf, nn, nn2, Tcap;
  int32_t *tgt, *n_tgt, *result;
};

__global__ __launch_bounds__(64) void k_fuse_targets(TgtArgs a) {
  __shared__ int s_tgt[TGT_MAX];
  const int lane = threadIdx.x, W = a.c.Wcap, me = a.kf;
  int n = 0, bad = 0;
  auto member = [&](int k) {
    bool hit = false;
    for (int base = 0; base < n; base += 64) hit |= base + lane < n && s_tgt[base + lane] == k;
    return __any(hit) != 0;
  };
  auto push = [&](int k) {
    if (lane == 0) {
      s_tgt[n] = k;
      if (n < a.Tcap) a.tgt[n] = k;
    }
    ++n;
    __syncthreads();
  };
  auto valid = [&](int k) { return !a.kf_valid || a.kf_valid[k]; };
  const int m0 = min(a.nn, cov_ord(a.c, me));
  for (int i = 0; i < m0; ++i) {
    const int k1 = a.c.kf[(size_t)me * W + i];
    if (!cov_row(a.c, k1)) {
      ++bad;
      continue;
    }
    if (!valid(k1) || member(k1)) continue;  // (:162-164) and with it its second neighbours
    push(k1);
    const int m1 = min(a.nn2, cov_ord(a.c, k1));
    for (int j = 0; j < m1; ++j) {
      const int k2 = a.c.kf[(size_t)k1 * W + j];
      if (!cov_row(a.c, k2)) {
        ++bad;
        continue;
      }
      if (!valid(k2) || member(k2) || k2 == me) continue;  // (:172-174)
      push(k2);
    }
  }
  if (lane == 0) {
    *a.n_tgt = n;
    a.result[0] = n;
    a.result[1] = (n > a.Tcap ? GL_COVIS_LIST_TRUNCATED : 0) | (bad ? GL_COVIS_BAD_ROW : 0);
    a.result[2] = 0;
    a.result[3] = bad;
  }
}

// ---------------------------------------------------------------------------------------------------------------- candidates
struct CandArgs {
  Map m;
  const int32_t *tgt, *n_tgt;
  int Tcap, kf_idx, cand_cap, npos;
  int32_t *cand, *n_cand, *result;
  // scratch
  int32_t* first;   // NMP: the first position that holds the point (0x7f7f7f7f: none - one memset)
  u64 *cnt, *tile;  // npos, tiles + 1
};
// the point at position pos = target position * NFK + slot when it is a candidate of the walk (:197), else -1
__device__ __forceinline__ int fc_point(const CandArgs& a, int pos, int n) {
  const int t = pos / a.m.NFK, f = pos - t * a.m.NFK;
  if (t >= n) return -1;
  const int k = a.tgt[t];
  if (!kf_row(a.m, k)) return -1;
  const int p = a.m.kf_mp[(size_t)k * a.m.NFK + f];
  return mp_ok(a.m, p) ? p : -1;
}

__global__ __launch_bounds__(T_FC) void k_fc_mark(CandArgs a) {
  const int pos = blockIdx.x * T_FC + threadIdx.x;
  if (pos >= a.npos) return;
  const int n = list_len(a.n_tgt, a.Tcap);
  const int p = fc_point(a, pos, n);
  if (p >= 0) atomicMin(a.first + p, pos);
  if (pos < n && !kf_row(a.m, a.tgt[pos])) {  // (npos >= Tcap: NFK >= 1)
    atomicOr(a.result + 1, GL_COVIS_BAD_ROW);
    atomicAdd(a.result + 3, 1);
  }
}

__global__ __launch_bounds__(T_FC) void k_fc_flag(CandArgs a) {
  const int pos = blockIdx.x * T_FC + threadIdx.x;
  if (pos >= a.npos) return;
  const int p = fc_point(a, pos, list_len(a.n_tgt, a.Tcap));
  // fuse_tgt_kf_ starts at 0 (mappoint.h:95): for kf_idx == 0 every point looks stamped already (:198)
  a.cnt[pos] = p >= 0 && a.first[p] == pos && a.kf_idx != 0 ? 1ull : 0ull;
}

__global__ __launch_bounds__(SCAN_T) void k_fc_top(CandArgs a, int ntile) {
  __shared__ u64 s_w[SCAN_T / 64];
  const int tid = threadIdx.x;
  const u64 total = tile_scan_top(a.tile, ntile, s_w, tid);
  if (tid == 0) {
    const int n = (int)total;
    *a.n_cand = n;
    a.result[0] = n;
    if (n > a.cand_cap) atomicOr(a.result + 1, GL_COVIS_LIST_TRUNCATED);
  }
}

__global__ __launch_bounds__(T_FC) void k_fc_move(CandArgs a) {
  const int pos = blockIdx.x * T_FC + threadIdx.x;
  if (pos >= a.npos || a.kf_idx == 0) return;
  const int p = fc_point(a, pos, list_len(a.n_tgt, a.Tcap));
  if (p < 0 || a.first[p] != pos) return;
  const u64 at = a.cnt[pos] + a.tile[pos / SCAN_TILE];
  if (at < (u64)a.cand_cap) a.cand[(int)at] = p;
}

int cov_from_c(const char* who, const gl_map_covis* cov, int NKF, Cov* out) {
  if (!cov || NKF < 0 || cov->NKFcap < NKF || cov->Wcap < 1 || !cov->cov_n || !cov->cov_nord || !cov->best_cov ||
      (cov->NKFcap > 0 && (!cov->cov_kf || !cov->cov_w)) || (int64_t)cov->NKFcap * cov->Wcap >= ((int64_t)1 << 31)) {
    gl::set_error("%s: bad gl_map_covis (null array, NKFcap below NKF, Wcap < 1 or NKFcap x Wcap at 2^31)", who);
    return GL_ERR_ARG;
  }
  out->NKF = NKF, out->Wcap = cov->Wcap;
  out->kf = cov->cov_kf, out->w = cov->cov_w, out->n = cov->cov_n, out->nord = cov->cov_nord, out->best = cov->best_cov;
  return GL_OK;
}

}  // namespace

extern "C" int gl_covis_update(gl_ctx_t* ctx, const gl_map_view* map, const gl_map_covis* cov, int kf_row, int Ccap, int32_t* conn_kf_dev,
                               int32_t* conn_w_dev, int32_t* n_conn_dev, int32_t* result_dev) {
  GL_REQUIRE(ctx, "null argument");
  GL_REQUIRE(Ccap >= 1, "bad Ccap");
  UpdArgs a = {};
  int rc = map_from_view(__func__, map, nullptr, &a.m);
  if (rc != GL_OK) return rc;
  rc = cov_from_c(__func__, cov, map->NKF, &a.c);
  if (rc != GL_OK) return rc;
  GL_REQUIRE(kf_row >= 0 && kf_row < map->NKF, "kf_row outside [0, NKF)");
  GL_REQUIRE(conn_kf_dev && conn_w_dev && n_conn_dev && result_dev, "null buffer");
  gl::Ctx* c = gl::C(ctx);
  GL_REQUIRE_LDS(c, (size_t)cov->Wcap * 8 + 64);
  GL_HIP(hipSetDevice(c->device));
  const size_t NKF = (size_t)map->NKF;
  const bool lds = map->NKF <= 4096 && NKF * 4 + 16384 <= (size_t)c->lds_max;
  gl::Regions r = {0};
  const size_t o_words = lds ? 0 : r.take(NKF * 4), o_kf = r.take(NKF * 4), o_w = r.take(NKF * 4), o_sel = r.take(4);
  void* scratch = nullptr;
  rc = gl::ctx_scratch(c, r.off, &scratch, gl::SCRATCH_BAWINDOW);
  if (rc != GL_OK) return rc;
  char* s = (char*)scratch;
  a.kf = kf_row, a.Ccap = Ccap;
  a.conn_kf = conn_kf_dev, a.conn_w = conn_w_dev, a.n_conn = n_conn_dev, a.result = result_dev;
  a.kf_words = lds ? nullptr : (int32_t*)(s + o_words);
  a.srt_kf = (int32_t*)(s + o_kf), a.srt_w = (int32_t*)(s + o_w), a.n_sel = (int32_t*)(s + o_sel);
  if (lds) {
    GL_HIP(gl::ensure_dynamic_lds(c, (const void*)k_covis_own<true>, NKF * 4));
    k_covis_own<true><<<1, T_CONN, NKF * 4, c->stream>>>(a);
  } else {
    k_covis_own<false><<<1, T_CONN, 0, c->stream>>>(a);
  }
  const size_t row_lds = (size_t)cov->Wcap * 8;
  GL_HIP(gl::ensure_dynamic_lds(c, (const void*)k_covis_add, row_lds));
  k_covis_add<<<std::max(std::min(map->NKF, ADD_GRID), 1), T_ADD, row_lds, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_covis_remove(gl_ctx_t* ctx, int NKF, const gl_map_covis* cov, int kf_first, const int32_t* cull_rows_dev, const int32_t* n_cull_dev,
                               int cull_cap, int32_t* result_dev) {
  GL_REQUIRE(ctx && result_dev, "null argument");
  GL_REQUIRE(cull_cap >= 0 && (cull_cap == 0 || cull_rows_dev), "bad cull_cap / null cull_rows");
  RmArgs a = {};
  const int rc = cov_from_c(__func__, cov, NKF, &a.c);
  if (rc != GL_OK) return rc;
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  a.kf_first = kf_first, a.cap = cull_cap, a.rows = cull_rows_dev, a.n_rows = n_cull_dev, a.result = result_dev;
  k_covis_remove<<<1, T_RM, 0, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_covis_best(gl_ctx_t* ctx, int NKF, const gl_map_covis* cov, int B, const int32_t* kf_row_dev, int N, int Ccap, int32_t* conn_kf_dev,
                             int32_t* conn_w_dev, int32_t* n_conn_dev, int32_t* result_dev) {
  GL_REQUIRE(ctx && result_dev, "null argument");
  GL_REQUIRE(B >= 0 && Ccap >= 1, "bad B / Ccap");
  BestArgs a = {};
  const int rc = cov_from_c(__func__, cov, NKF, &a.c);
  if (rc != GL_OK) return rc;
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  GL_HIP(hipMemsetAsync(result_dev, 0, 4 * sizeof(int32_t), c->stream));
  if (B == 0) return GL_OK;
  GL_REQUIRE(kf_row_dev && conn_kf_dev && conn_w_dev && n_conn_dev, "null buffer");
  a.B = B, a.N = N, a.Ccap = Ccap, a.kf_row = kf_row_dev;
  a.conn_kf = conn_kf_dev, a.conn_w = conn_w_dev, a.n_conn = n_conn_dev, a.result = result_dev;
  k_covis_best<<<B, T_ADD, 0, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_fuse_targets(gl_ctx_t* ctx, int NKF, const gl_map_covis* cov, const uint8_t* kf_valid_dev, int kf_row, int nn, int nn2, int Tcap,
                               int32_t* tgt_kf_dev, int32_t* n_tgt_dev, int32_t* result_dev) {
  GL_REQUIRE(ctx && n_tgt_dev && result_dev, "null argument");
  GL_REQUIRE(nn >= 0 && nn2 >= 0 && (int64_t)nn + (int64_t)nn * nn2 <= TGT_MAX, "bad nn / nn2 (nn + nn x nn2 at most 4 096)");
  GL_REQUIRE(Tcap >= 0 && (Tcap == 0 || tgt_kf_dev), "bad Tcap / null tgt_kf");
  TgtArgs a = {};
  const int rc = cov_from_c(__func__, cov, NKF, &a.c);
  if (rc != GL_OK) return rc;
  GL_REQUIRE(kf_row >= 0 && kf_row < NKF, "kf_row outside [0, NKF)");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  a.kf_valid = kf_valid_dev, a.kf = kf_row, a.nn = nn, a.nn2 = nn2, a.Tcap = Tcap;
  a.tgt = tgt_kf_dev, a.n_tgt = n_tgt_dev, a.result = result_dev;
  k_fuse_targets<<<1, 64, 0, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_fuse_candidates(gl_ctx_t* ctx, const gl_map_view* map, const int32_t* tgt_kf_dev, const int32_t* n_tgt_dev, int Tcap, int kf_idx,
                                  int cand_cap, int32_t* cand_mp_dev, int32_t* n_cand_dev, int32_t* result_dev) {
  GL_REQUIRE(ctx && n_cand_dev && result_dev, "null argument");
  CandArgs a = {};
  const int rc = map_from_view(__func__, map, nullptr, &a.m);
  if (rc != GL_OK) return rc;
  GL_REQUIRE(Tcap >= 0 && (Tcap == 0 || tgt_kf_dev), "bad Tcap / null tgt_kf");
  GL_REQUIRE(cand_cap >= 0 && (cand_cap == 0 || cand_mp_dev), "bad cand_cap / null cand_mp");
  GL_REQUIRE((int64_t)Tcap * map->NFK < ((int64_t)1 << 31) - SCAN_TILE, "Tcap x NFK must be below 2^31");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  GL_HIP(hipMemsetAsync(result_dev, 0, 4 * sizeof(int32_t), c->stream));
  GL_HIP(hipMemsetAsync(n_cand_dev, 0, sizeof(int32_t), c->stream));
  const int npos = Tcap * map->NFK;
  if (npos == 0) return GL_OK;
  const int ntile = csr_tiles(npos);
  gl::Regions r = {0};
  const size_t o_first = r.take((size_t)map->NMP * 4), o_cnt = r.take((size_t)npos * 8), o_tile = r.take((size_t)ntile * 8 + 8);
  void* scratch = nullptr;
  const int rs = gl::ctx_scratch(c, r.off, &scratch, gl::SCRATCH_MAPEDIT);
  if (rs != GL_OK) return rs;
  char* s = (char*)scratch;
  a.tgt = tgt_kf_dev, a.n_tgt = n_tgt_dev, a.Tcap = Tcap, a.kf_idx = kf_idx, a.cand_cap = cand_cap, a.npos = npos;
  a.cand = cand_mp_dev, a.n_cand = n_cand_dev, a.result = result_dev;
  a.first = (int32_t*)(s + o_first), a.cnt = (u64*)(s + o_cnt), a.tile = (u64*)(s + o_tile);
  if (map->NMP > 0) GL_HIP(hipMemsetAsync(a.first, 0x7f, (size_t)map->NMP * 4, c->stream));
  const int nb = (npos + T_FC - 1) / T_FC;
  k_fc_mark<<<nb, T_FC, 0, c->stream>>>(a);
  k_fc_flag<<<nb, T_FC, 0, c->stream>>>(a);
  CsrRebuild rb = {};
  rb.cnt = a.cnt, rb.tile = a.tile;
  csr_rebuild_scan(c, rb, ntile, nullptr, npos);
  k_fc_top<<<1, SCAN_T, 0, c->stream>>>(a, ntile);
  k_fc_move<<<nb, T_FC, 0, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}
