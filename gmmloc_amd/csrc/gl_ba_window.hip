// The mapping thread on the resident map (gmmloc_hip.h): KeyFrame::updateConnections (keyframe.cpp:243-316), the window selection and
// flattening of Localization::jointOptimization (localization_opt.cpp:460-516, :639-763) and its write-back (:837-853, :898-922), over
// the caller-owned arrays of gl_map_view + gl_map_ba_view (mapdev::Map).  The rules, the reproduced quirks and the tie rule are in the header.
// One workgroup per key-frame / window; every ORDER comes from a key that the inputs alone determine:
//   connections  (a) a slot of the key-frame per thread: one integer atomic add per observation of the held point into the key-frame
//                counters; (b) a contiguous run of key-frames per thread: how many reach 15, the best (count, lowest row); (c) every
//                kept key-frame finds its place by counting the kept ones that come before it (weight descending, row ascending)
//   window       free poses = the key-frame + the valid kept ones in that order; a POSITION p = (free pose, slot) per thread: the
//                point's word takes the minimum p (atomicMin), a position is a first occurrence where the word equals it; a bit per
//                position (wave ballots), popcount + prefix sum -> the points in walk order; a contiguous run of points per thread:
//                observations counted, prefix sums give every point and observation its index; an unmarked observer's word takes the
//                minimum observation index, the fixed key-frames are ranked by it; a last walk writes the slab.
// The per-key-frame words (counter, then first-observation key; window index) live in dynamic LDS up to BW_KF_LDS key-frames, else in the
// context's scratch (device-scope atomics, atomic loads - same phases, same result).  The per-map-point word, the lists and the
// position bits are always in the scratch: a word per map point does not fit LDS for a real map, and only the touched words are
// initialised, so the cost follows the window, not the map.
#include "gl_map_dev.hpp"

namespace {

using namespace gl::mapdev;  // Map, mp_ok, kf_ok, kf_row, slot_in, obs_range, Words, block_excl_scan, block_max, best_row, conn_count, rank_selected

constexpr int T_BW = 1024;
constexpr int BW_KF_LDS = 4096;  // 2 x 16 KB of words
// window index of a key-frame that has none: valid and not in the window / marked local but invalid (:466-471) / invalid
constexpr int W_NONE = -1, W_MARK = -2, W_INVALID = -3;
constexpr int KEY_INF = 0x7fffffff;

struct BwArgs {
  Map m;
  gl_ba_window w;
  int B;
  const int32_t* kf_row;
  // gl_update_connections
  int Ccap;
  int32_t *conn_kf, *conn_w, *n_conn, *kf_count, *conn_status;
  // scratch (per window: row b)
  int32_t* kf_words;  // B x 2 NKF (connections: B x NKF), or null: LDS
  int32_t* order;     // B x NKF: the window's key-frame rows, free then fixed
  int32_t* mp_word;   // B x NMP: the first position that holds the point
  int32_t* list;      // B x NMP: the points in walk order, before the ones without an edge are dropped
  int32_t* lcnt;      // B x NMP: per point of that list, its edges, then the index of its first observation
  u64* posmask;       // B x maskw: a bit per position
  size_t maskw;
};

__device__ __forceinline__ void bw_sync() {
  __threadfence();
  __syncthreads();
}

// conn_count, conn_keep, conn_key and rank_selected (gl_map_dev.hpp) run with T_BW threads
static_assert(T_BW == T_CONN, "the connection helpers are written for T_CONN threads");

template <bool LDS>
__global__ __launch_bounds__(T_BW) void k_connections(BwArgs a) {
  extern __shared__ int bw_lds[];
  __shared__ int s_w[T_BW / 64];
  __shared__ u64 s_b[T_BW / 64];
  __shared__ RankLds s_rank;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  const int NKF = a.m.NKF;
  const Words<LDS> cnt = {LDS ? bw_lds : a.kf_words + (size_t)b * NKF};
  for (int k = tid; k < NKF; k += T_BW) cnt.set(k, 0);
  if constexpr (!LDS) __threadfence();
  __syncthreads();
  const int kf = a.kf_row[b];
  if (kf < 0 || kf >= NKF) {
    if (LDS && a.kf_count)
      for (int k = tid; k < NKF; k += T_BW) a.kf_count[(size_t)b * NKF + k] = 0;
    if (tid == 0) {
      a.n_conn[b] = 0;
      a.conn_status[b] = GL_CONN_BAD_ROW;
    }
    return;
  }
  int n15;
  u64 best;
  conn_count<LDS>(a.m, kf, cnt, tid, s_w, s_b, &n15, &best);
  if (LDS && a.kf_count)
    for (int k = tid; k < NKF; k += T_BW) a.kf_count[(size_t)b * NKF + k] = cnt.get(k);
  if (!best) {  // (:275-276)
    if (tid == 0) {
      a.n_conn[b] = 0;
      a.conn_status[b] = GL_CONN_KEPT;
    }
    return;
  }
  const int brow = best_row(best);
  const int n = rank_selected(
      NKF, tid, s_w, s_rank,
      [&](int k) -> u64 {
        const int c = cnt.get(k);
        return c > 0 && conn_keep(k, c, n15, brow) ? conn_key(k, c) : 0ull;
      },
      [&](int k, int r) {
        if (r < a.Ccap) {
          a.conn_kf[(size_t)b * a.Ccap + r] = k;
          a.conn_w[(size_t)b * a.Ccap + r] = cnt.get(k);
        }
      });
  if (tid == 0) {
    a.n_conn[b] = n;
    a.conn_status[b] = n > a.Ccap ? GL_CONN_TRUNCATED : 0;
  }
}

// The CSR entries of point mp that make an edge of the window, in CSR order: the key-frame in the table and valid (:698; widx holds
// W_INVALID / W_MARK for the invalid ones), the feature in the key-frame's table.  fn(o, k, f, i) for the i-th of them; returns their
// number.  Four entries at a time, their loads issued together.
template <bool LDS, class Fn>
__device__ __forceinline__ int for_each_edge(const BwArgs& a, const Words<LDS>& widx, int mp, Fn fn) {
  int o0, o1, n = 0;
  obs_range(a.m, mp, &o0, &o1);
  for (int o = o0; o < o1; o += 4) {
    int k[4], f[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool in = o + u < o1;
      k[u] = in ? a.m.obs_kf[o + u] : -1;
      f[u] = in ? a.m.obs_feat[o + u] : -1;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (!slot_in(a.m, k[u], f[u])) continue;
      if (widx.get(k[u]) <= W_MARK) continue;
      fn(o + u, k[u], f[u], n);
      ++n;
    }
  }
  return n;
}

template <bool LDS>
__global__ __launch_bounds__(T_BW) void k_ba_window_build(BwArgs a) {
  extern __shared__ int bw_lds[];
  __shared__ int s_w[T_BW / 64];
  __shared__ u64 s_b[T_BW / 64];
  __shared__ RankLds s_rank;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (b >= a.B) return;
  const int NKF = a.m.NKF, NFK = a.m.NFK, NMP = a.m.NMP;
  int* const words = LDS ? bw_lds : a.kf_words + (size_t)b * 2 * NKF;
  const Words<LDS> cnt = {words}, widx = {words + NKF};  // cnt: the covisibility counter, later the first-observation key
  int32_t* const order = a.order + (size_t)b * NKF;
  int32_t* const mp_word = a.mp_word + (size_t)b * NMP;  // by map-point row: the first position; later by point l: its window index
  int32_t* const list = a.list + (size_t)b * NMP;
  int32_t* const lcnt = a.lcnt + (size_t)b * NMP;  // by point l: edges << 1 | stays; later the index of its first observation
  u64* const posmask = a.posmask + (size_t)b * a.maskw;
  const gl_ba_window& w = a.w;
  const int PFcap = w.Pcap + w.Fcap;

  for (int k = tid; k < NKF; k += T_BW) {
    cnt.set(k, 0);
    widx.set(k, kf_ok(a.m, k) ? W_NONE : W_INVALID);
  }
  bw_sync();
  const int kf = a.kf_row[b];
  if (kf < 0 || kf >= NKF) {
    if (tid < 4) w.sizes[(size_t)b * 4 + tid] = 0;
    if (tid == 0) w.status[b] = GL_BA_WINDOW_BAD_ROW;
    return;
  }
  // ---- the covisible list (gl_update_connections) -> the free poses (:460-471)
  int n15;
  u64 best;
  conn_count<LDS>(a.m, kf, cnt, tid, s_w, s_b, &n15, &best);
  const int brow = best ? best_row(best) : -1;
  const int P = 1 + rank_selected(
                        NKF, tid, s_w, s_rank,
                        [&](int k) -> u64 {  // the listed key-frames that are valid, in list order
                          const int c = cnt.get(k);
                          return c > 0 && conn_keep(k, c, n15, brow) && kf_ok(a.m, k) ? conn_key(k, c) : 0ull;
                        },
                        [&](int k, int r) {
                          widx.set(k, 1 + r);
                          order[1 + r] = k;
                        });
  for (int k = tid; k < NKF; k += T_BW) {
    const int c = cnt.get(k);
    if (c > 0 && conn_keep(k, c, n15, brow) && !kf_ok(a.m, k)) widx.set(k, W_MARK);  // marked local, not added
    cnt.set(k, KEY_INF);
  }
  if (tid == 0) {
    widx.set(kf, kf_ok(a.m, kf) ? 0 : W_MARK);  // (:462: free whatever its validity; its own observations make no edge when it is invalid)
    order[0] = kf;
  }
  bw_sync();

  // ---- the points (:473-489): first occurrences over the positions p = j * NFK + slot.  Four positions per thread at a time, a wave
  // on 64 consecutive ones each time, the loads of the four issued together.
  const int NP = P * NFK, NP64 = (NP + 63) & ~63;
  auto held = [&](int p) -> int {  // the valid map point at position p, or -1
    if (p >= NP) return -1;
    const int j = p / NFK;
    return a.m.kf_mp[(size_t)order[j] * NFK + (p - j * NFK)];
  };
  for (int p = tid; p < NP; p += 4 * T_BW) {
    int mp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) mp[u] = held(p + u * T_BW);
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) ok[u] = mp_ok(a.m, mp[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (ok[u]) __hip_atomic_store(mp_word + mp[u], KEY_INF, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  bw_sync();
  for (int p = tid; p < NP; p += 4 * T_BW) {
    int mp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) mp[u] = held(p + u * T_BW);
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) ok[u] = mp_ok(a.m, mp[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (ok[u]) atomicMin(mp_word + mp[u], p + u * T_BW);
  }
  bw_sync();
  for (int p = tid; p < NP64; p += 4 * T_BW) {  // (NP64 keeps the lanes of a wave together for the ballots)
    int mp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) mp[u] = held(p + u * T_BW);
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) ok[u] = mp_ok(a.m, mp[u]);
    int first[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) first[u] = ok[u] ? __hip_atomic_load(mp_word + mp[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -1;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int pu = p + u * T_BW;
      if (pu >= NP64) break;  // (the same for every lane of the wave)
      const u64 bits = __ballot(ok[u] && first[u] == pu);
      if (lane == 0) posmask[pu >> 6] = bits;
    }
  }
  bw_sync();
  const int nw = NP64 >> 6, cw = (nw + T_BW - 1) / T_BW;
  const int w0 = min(tid * cw, nw), w1 = min(w0 + cw, nw);
  int npt = 0;
  for (int i = w0; i < w1; ++i) npt += __popcll(posmask[i]);
  int Lall;
  int at = block_excl_scan<T_BW>(npt, s_w, tid, &Lall);
  for (int i = w0; i < w1 && npt > 0; ++i) {
    u64 bits = posmask[i];
    while (bits) {
      const int r = __ffsll((long long)bits) - 1;
      bits &= bits - 1;
      list[at++] = held(i * 64 + r);
    }
  }
  bw_sync();

  // ---- the observations (:639-763): a point per thread counts its edges; a contiguous run of points per thread sums them, prefix sums
  // give every point its index and the index of its first observation (a point without an edge is dropped)
  for (int l = tid; l < Lall; l += T_BW) {
    const int mp = list[l];
    const int n = for_each_edge<LDS>(a, widx, mp, [](int, int, int, int) {});
    lcnt[l] = (n << 1) | (n > 0 || a.m.mp_assoc[mp] >= 0 ? 1 : 0);
  }
  bw_sync();
  const int cl = (Lall + T_BW - 1) / T_BW;
  const int l0 = min(tid * cl, Lall), l1 = min(l0 + cl, Lall);
  int np_run = 0, no_run = 0;
  for (int l = l0; l < l1; ++l) {
    const int v = lcnt[l];
    np_run += v & 1;
    no_run += v >> 1;
  }
  int L, nobs;
  int lw = block_excl_scan<T_BW>(np_run, s_w, tid, &L);
  int g = block_excl_scan<T_BW>(no_run, s_w, tid, &nobs);
  for (int l = l0; l < l1; ++l) {
    const int v = lcnt[l];
    mp_word[l] = v & 1 ? lw++ : -1;
    lcnt[l] = g;
    g += v >> 1;
  }
  bw_sync();
  // ---- the slab, a point per thread; obs_pose holds the key-frame ROW until the fixed poses have their places.  An unmarked
  // observer's word takes the index of its first observation (:491-516).
  const size_t sl = (size_t)b * w.Lcap, so = (size_t)b * w.Ocap, sp = (size_t)b * PFcap;
  for (int l = tid; l < Lall; l += T_BW) {
    const int mp = list[l], li = mp_word[l], g0 = lcnt[l];
    for_each_edge<LDS>(a, widx, mp, [&](int o, int k, int f, int i) {
      const int gi = g0 + i;
      if (widx.get(k) == W_NONE) cnt.min_(k, gi);
      if (gi >= w.Ocap) return;
      const size_t ft = (size_t)k * NFK + f;
      w.win_obs[so + gi] = o;
      w.obs_pose[so + gi] = k;
      w.obs_oct[so + gi] = a.m.kf_oct[ft];
#pragma unroll
      for (int c = 0; c < 3; ++c) w.obs_uvr[(so + gi) * 3 + c] = a.m.kf_uvr[ft * 3 + c];
    });
    if (li < 0 || li >= w.Lcap) continue;
    w.win_mp[sl + li] = mp;
    w.assoc[sl + li] = a.m.mp_assoc[mp];
    w.obs_ptr[(size_t)b * (w.Lcap + 1) + li] = g0;
#pragma unroll
    for (int c = 0; c < 3; ++c) w.points[(sl + li) * 3 + c] = a.m.mp_pos[(size_t)mp * 3 + c];
  }
  bw_sync();
  const int F = rank_selected(
      NKF, tid, s_w, s_rank,
      [&](int k) -> u64 {
        const int key = cnt.get(k);
        return key == KEY_INF ? 0ull : (u64)key + 1ull;
      },
      [&](int k, int r) {
        widx.set(k, P + r);
        order[P + r] = k;
      });
  for (int gi = tid; gi < nobs && gi < w.Ocap; gi += T_BW) w.obs_pose[so + gi] = widx.get(w.obs_pose[so + gi]);
  for (int j = tid; j < P + F && j < PFcap; j += T_BW) {
    const int k = order[j];
    w.win_kf[sp + j] = k;
#pragma unroll
    for (int c = 0; c < 7; ++c) w.poses[(sp + j) * 7 + c] = a.m.kf_pose[(size_t)k * 7 + c];
    if (j < P && j < w.Pcap) w.prior[(size_t)b * w.Pcap + j] = k == a.m.kf_first ? 1 : 0;
  }
  if (tid == 0) {
    if (L <= w.Lcap) w.obs_ptr[(size_t)b * (w.Lcap + 1) + L] = nobs;
    int32_t* s = w.sizes + (size_t)b * 4;
    s[0] = P;
    s[1] = F;
    s[2] = L;
    s[3] = nobs;
    const int dropped = min(Lall - L, 0x7fffff);
    w.status[b] = (best ? 0 : GL_BA_WINDOW_NO_CONN) | (P > w.Pcap ? GL_BA_WINDOW_P_TRUNCATED : 0) | (F > w.Fcap ? GL_BA_WINDOW_F_TRUNCATED : 0) |
                  (L > w.Lcap ? GL_BA_WINDOW_L_TRUNCATED : 0) | (nobs > w.Ocap ? GL_BA_WINDOW_O_TRUNCATED : 0) | (dropped << GL_BA_WINDOW_DROPPED_SHIFT);
  }
}

struct ApplyArgs {
  gl_map_view m;
  gl_map_ba_view ba;
  gl_ba_window w;
  int B;
  double* mp_pos;
  const uint8_t* assoc_dropped;
  const uint8_t* obs_erase;
  const int32_t* iters;
  int32_t* erase_obs;
  int32_t* n_erase;
  int32_t* tmp;  // B x Ocap
};

__global__ __launch_bounds__(T_BW) void k_ba_window_apply(ApplyArgs a) {
  __shared__ int s_w[T_BW / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  const gl_ba_window& w = a.w;
  const int32_t* s = w.sizes + (size_t)b * 4;
  const int P = s[0], F = s[1], L = s[2], nobs = s[3];
  if (a.iters[b] == 0 || P < 0 || F < 0 || L < 0 || nobs < 0 || P > w.Pcap || F > w.Fcap || L > w.Lcap || nobs > w.Ocap) {  // (workgroup-uniform)
    if (tid == 0) a.n_erase[b] = 0;
    return;
  }
  const size_t sl = (size_t)b * w.Lcap, so = (size_t)b * w.Ocap, sp = (size_t)b * (w.Pcap + w.Fcap);
  for (int j = tid; j < P; j += T_BW) {  // (:898-910)
    const int row = w.win_kf[sp + j];
    if (row < 0 || row >= a.m.NKF) continue;
    double q[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      q[c] = w.poses[(sp + j) * 7 + c];
      a.ba.kf_pose[(size_t)row * 7 + c] = q[c];
    }
    if (!a.ba.kf_twc) continue;
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const double x = q[0] / n, y = q[1] / n, z = q[2] / n, ww = q[3] / n, tx = q[4], ty = q[5], tz = q[6];
    const double R00 = 1 - 2 * (y * y + z * z), R01 = 2 * (x * y - z * ww), R02 = 2 * (x * z + y * ww);
    const double R10 = 2 * (x * y + z * ww), R11 = 1 - 2 * (x * x + z * z), R12 = 2 * (y * z - x * ww);
    const double R20 = 2 * (x * z - y * ww), R21 = 2 * (y * z + x * ww), R22 = 1 - 2 * (x * x + y * y);
    a.ba.kf_twc[(size_t)row * 3 + 0] = -((R00 * tx + R10 * ty) + R20 * tz);
    a.ba.kf_twc[(size_t)row * 3 + 1] = -((R01 * tx + R11 * ty) + R21 * tz);
    a.ba.kf_twc[(size_t)row * 3 + 2] = -((R02 * tx + R12 * ty) + R22 * tz);
  }
  for (int l = tid; l < L; l += T_BW) {  // (:837-853, :912-922)
    const int mp = w.win_mp[sl + l];
    if (mp < 0 || mp >= a.m.NMP) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.mp_pos[(size_t)mp * 3 + c] = w.points[(sl + l) * 3 + c];
    if (a.assoc_dropped[sl + l]) a.ba.mp_assoc[mp] = -1;
  }
  // the erased observations as CSR positions: compacted in window order, then each finds its place among the others (they are distinct)
  const int cg = (nobs + T_BW - 1) / T_BW;
  const int g0 = min(tid * cg, nobs), g1 = min(g0 + cg, nobs);
  int n = 0;
  for (int g = g0; g < g1; ++g) n += a.obs_erase[so + g] != 0;
  int ne;
  int at = block_excl_scan<T_BW>(n, s_w, tid, &ne);
  int32_t* tmp = a.tmp + so;
  for (int g = g0; g < g1 && n > 0; ++g)
    if (a.obs_erase[so + g]) tmp[at++] = w.win_obs[so + g];
  bw_sync();
  for (int i = tid; i < ne; i += T_BW) {
    const int v = tmp[i];
    int r = 0;
    for (int i2 = 0; i2 < ne; ++i2) r += tmp[i2] < v;
    a.erase_obs[so + r] = v;
  }
  if (tid == 0) a.n_erase[b] = ne;
}

bool kf_in_lds(const gl::Ctx* c, const gl_map_view* m, int arrays) {
  return m->NKF <= BW_KF_LDS && (size_t)m->NKF * 4 * arrays + 2048 <= (size_t)c->lds_max;
}

int check_window(const gl_ba_window* w) {
  GL_REQUIRE(w, "null argument");
  GL_REQUIRE(w->Pcap >= 1 && w->Fcap >= 0 && w->Lcap >= 1 && w->Ocap >= 1, "bad Pcap / Fcap / Lcap / Ocap");
  GL_REQUIRE(w->poses && w->prior && w->points && w->assoc && w->obs_ptr && w->obs_pose && w->obs_uvr && w->obs_oct && w->win_kf && w->win_mp &&
                 w->win_obs && w->sizes && w->status,
             "null buffer");
  return GL_OK;
}

}  // namespace

extern "C" int gl_update_connections(gl_ctx_t* ctx, const gl_map_view* map, int B, const int32_t* kf_row_dev, int Ccap, int32_t* conn_kf_dev,
                                     int32_t* conn_w_dev, int32_t* n_conn_dev, int32_t* kf_count_dev, int32_t* status_dev) {
  GL_REQUIRE(ctx, "null argument");
  GL_REQUIRE(B >= 0 && Ccap >= 1, "bad B / Ccap");
  if (B == 0) return GL_OK;
  BwArgs a = {};
  const int rc = map_from_view(__func__, map, nullptr, &a.m);
  if (rc != GL_OK) return rc;
  GL_REQUIRE(kf_row_dev && conn_kf_dev && conn_w_dev && n_conn_dev && status_dev, "null buffer");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  a.B = B;
  a.kf_row = kf_row_dev;
  a.Ccap = Ccap;
  a.conn_kf = conn_kf_dev;
  a.conn_w = conn_w_dev;
  a.n_conn = n_conn_dev;
  a.kf_count = kf_count_dev;
  a.conn_status = status_dev;
  if (kf_in_lds(c, map, 1)) {
    const size_t lds = (size_t)map->NKF * 4;
    GL_HIP(gl::ensure_dynamic_lds(c, (const void*)k_connections<true>, lds));
    k_connections<true><<<B, T_BW, lds, c->stream>>>(a);
  } else {
    a.kf_words = kf_count_dev;  // the counter itself
    if (!a.kf_words) {
      void* scratch = nullptr;
      const int rs = gl::ctx_scratch(c, (size_t)B * map->NKF * 4, &scratch, gl::SCRATCH_BAWINDOW);
      if (rs != GL_OK) return rs;
      a.kf_words = (int32_t*)scratch;
    }
    k_connections<false><<<B, T_BW, 0, c->stream>>>(a);
  }
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_ba_window_build(gl_ctx_t* ctx, const gl_map_view* map, const gl_map_ba_view* ba, int B, const int32_t* kf_row_dev,
                                  const gl_ba_window* win) {
  GL_REQUIRE(ctx && ba, "null argument");
  GL_REQUIRE(B >= 0, "bad B");
  if (B == 0) return GL_OK;
  BwArgs a = {};
  int rc = map_from_view(__func__, map, ba, &a.m);
  if (rc != GL_OK) return rc;
  rc = check_window(win);
  if (rc != GL_OK) return rc;
  GL_REQUIRE(kf_row_dev, "null buffer");
  GL_REQUIRE(map->NMP == 0 || (map->mp_pos && ba->mp_assoc), "null mp_pos / mp_assoc");
  GL_REQUIRE(map->NKF == 0 || ba->kf_pose, "null kf_pose");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  const bool lds = kf_in_lds(c, map, 2);
  const size_t NKF = (size_t)map->NKF, NMP = (size_t)map->NMP;
  const size_t maskw = (NKF * (size_t)map->NFK + 63) / 64 + 1;
  gl::Regions r = {0};
  const size_t o_words = lds ? 0 : r.take((size_t)B * 2 * NKF * 4);
  const size_t o_order = r.take((size_t)B * NKF * 4), o_word = r.take((size_t)B * NMP * 4), o_list = r.take((size_t)B * NMP * 4), o_lcnt = r.take((size_t)B * NMP * 4),
               o_mask = r.take((size_t)B * maskw * 8);
  void* scratch = nullptr;
  rc = gl::ctx_scratch(c, r.off, &scratch, gl::SCRATCH_BAWINDOW);
  if (rc != GL_OK) return rc;
  char* s = (char*)scratch;
  a.w = *win;
  a.B = B;
  a.kf_row = kf_row_dev;
  a.kf_words = lds ? nullptr : (int32_t*)(s + o_words);
  a.order = (int32_t*)(s + o_order);
  a.mp_word = (int32_t*)(s + o_word);
  a.list = (int32_t*)(s + o_list);
  a.lcnt = (int32_t*)(s + o_lcnt);
  a.posmask = (u64*)(s + o_mask);
  a.maskw = maskw;
  if (lds) {
    const size_t bytes = NKF * 8;
    GL_HIP(gl::ensure_dynamic_lds(c, (const void*)k_ba_window_build<true>, bytes));
    k_ba_window_build<true><<<B, T_BW, bytes, c->stream>>>(a);
  } else {
    k_ba_window_build<false><<<B, T_BW, 0, c->stream>>>(a);
  }
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_ba_window_apply(gl_ctx_t* ctx, const gl_map_view* map, double* mp_pos_dev, const gl_map_ba_view* ba, int B,
                                  const gl_ba_window* win, const uint8_t* assoc_dropped_dev, const uint8_t* obs_erase_dev,
                                  const int32_t* iters_dev, int32_t* erase_obs_dev, int32_t* n_erase_dev) {
  GL_REQUIRE(ctx && map && ba, "null argument");
  GL_REQUIRE(B >= 0, "bad B");
  if (B == 0) return GL_OK;
  GL_REQUIRE(map->NMP >= 0 && map->NKF >= 0, "bad NMP / NKF");
  const int rc = check_window(win);
  if (rc != GL_OK) return rc;
  GL_REQUIRE(assoc_dropped_dev && obs_erase_dev && iters_dev && erase_obs_dev && n_erase_dev, "null buffer");
  GL_REQUIRE(map->NMP == 0 || (mp_pos_dev && ba->mp_assoc), "null mp_pos / mp_assoc");
  GL_REQUIRE(map->NKF == 0 || ba->kf_pose, "null kf_pose");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  void* scratch = nullptr;
  const int rs = gl::ctx_scratch(c, (size_t)B * win->Ocap * 4, &scratch, gl::SCRATCH_BAWINDOW);
  if (rs != GL_OK) return rs;
  ApplyArgs a;
  a.m = *map;
  a.ba = *ba;
  a.w = *win;
  a.B = B;
  a.mp_pos = mp_pos_dev;
  a.assoc_dropped = assoc_dropped_dev;
  a.obs_erase = obs_erase_dev;
  a.iters = iters_dev;
  a.erase_obs = erase_obs_dev;
  a.n_erase = n_erase_dev;
  a.tmp = (int32_t*)scratch;
  k_ba_window_apply<<<B, T_BW, 0, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}
