// Tracking::updateLocalMap (tracking.cpp:119-207) on the device: the local key-frames, the reference key-frame and the local map
// points of B frames from the map points their features hold, over the whole map as caller-owned arrays (gl_map_view: the CSR of
// observations gl_update_map_points reads + the key-frames' mappoints_ table).  The rules, the quirks of the reference that are
// reproduced and the canonical order (ties -> the lowest key-frame row; lists in ascending row) are in gmmloc_hip.h.
// One workgroup per frame, four phases separated by barriers:
//   (a) a feature per thread: [with LocalMapDerive: feat_mp from the chain's associations, invalid held points cleared,] then one
//       integer atomic add per observation of the held point into the key-frame counters
//   (b) a contiguous run of key-frames per thread: how many of them are local (counted and valid) and the best (count, lowest row)
//       among them; a workgroup prefix sum gives each run its place in the ascending list, a wave + LDS reduction the reference
//       key-frame
//   (c) a local key-frame per wave: its kf_mp row read coalesced, validity tested, one atomic or per point into a bitmask over
//       map-point rows
//   (d) a contiguous run of mask words per thread: popcount, prefix sum, the ascending list written with no sort
// Counters (NKF <= LM_KF_LDS) and mask (NMP <= LM_MP_LDS) live in dynamic LDS sized to the map; beyond a bound that array lives in
// global memory instead (kf_count itself or the context's scratch), written with device-scope atomics and read back with atomic
// loads - same phases, same result.  Integer atomics only: nothing depends on the order the waves run in.
// k_local_map keeps gl_map_view as its argument and its own spelling of the map's rules (mapdev's mp_ok / obs_range / Words, gl_map_dev.hpp):
// with mapdev::Map and the helpers it measured 1.4 % slower on the 1 500-key-frame map at B = 1 (profiles/r15_map_shared_time.txt).
#include "gl_map_dev.hpp"

namespace {

using gl::mapdev::block_excl_scan;

constexpr int T_LM = 1024;
constexpr int LM_KF_LDS = 4096;     // 16 KB of counters
constexpr int LM_MP_LDS = 1 << 20;  // 128 KB of mask

struct LmArgs {
  gl_map_view m;
  int B, NF;
  gl::LocalMapLists L;
  gl::LocalMapDerive d;
  int derive;
  int words;           // mask words per frame
  int32_t* cnt_glob;   // B x NKF (global counters), or null
  uint32_t* mask_glob; // B x words (global mask), or null
};

template <bool CNT_LDS, bool MASK_LDS>
__global__ __launch_bounds__(T_LM) void k_local_map(LmArgs a) {
  extern __shared__ uint32_t lm_lds[];
  __shared__ int s_w[T_LM / 64];
  __shared__ unsigned long long s_best[T_LM / 64];
  __shared__ int s_any;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (b >= a.B) return;
  const int NMP = a.m.NMP, NKF = a.m.NKF, NFK = a.m.NFK, NOBS = a.m.NOBS, NF = a.NF, words = a.words;
  int* const l_cnt = (int*)lm_lds;
  uint32_t* const l_mask = lm_lds + (CNT_LDS ? NKF : 0);
  int* const g_cnt = CNT_LDS ? nullptr : a.cnt_glob + (size_t)b * NKF;
  uint32_t* const g_mask = MASK_LDS ? nullptr : a.mask_glob + (size_t)b * words;
  auto cnt_get = [&](int k) -> int {
    if constexpr (CNT_LDS) return l_cnt[k];
    else return __hip_atomic_load(g_cnt + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  auto mask_get = [&](int w) -> uint32_t {
    if constexpr (MASK_LDS) return l_mask[w];
    else return __hip_atomic_load(g_mask + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  auto sync = [&]() {
    if constexpr (!CNT_LDS || !MASK_LDS) __threadfence();
    __syncthreads();
  };

  for (int k = tid; k < NKF; k += T_LM) {
    if constexpr (CNT_LDS) l_cnt[k] = 0;
    else __hip_atomic_store(g_cnt + k, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  for (int w = tid; w < words; w += T_LM) {
    if constexpr (MASK_LDS) l_mask[w] = 0u;
    else __hip_atomic_store(g_mask + w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid == 0) s_any = 0;
  sync();

  // ---- (a) the counter (:129-145)
  const bool lost = a.derive && a.d.counts2 && a.d.counts2[(size_t)b * 4 + 3] == 2;
  bool any = false;
  for (int i = tid; i < NF; i += T_LM) {
    const size_t g = (size_t)b * NF + i;
    int m;
    if (a.derive) {
      const int j = a.d.match_last[g], q = a.d.match_kf ? a.d.match_kf[g] : -1;
      m = lost ? -1 : j >= 0 ? a.d.last_mp[(size_t)b * a.d.NL + j] : (q >= 0 && a.d.kf_feat_mp) ? a.d.kf_feat_mp[(size_t)b * a.d.NK + q] : -1;
      if (m >= 0 && m < NMP && a.m.mp_valid && !a.m.mp_valid[m]) {  // mappoints_[i] = nullptr: the feature holds nothing any more
        m = -1;
        if (j >= 0) a.d.match_last[g] = -1;
        else a.d.match_kf[g] = -1;
      }
      a.L.feat_mp[g] = m;
    } else {
      m = a.L.feat_mp[g];
    }
    if (m < 0 || m >= NMP) continue;
    if (a.m.mp_valid && !a.m.mp_valid[m]) {
      a.L.feat_mp[g] = -1;
      continue;
    }
    const int o0 = a.m.obs_ptr[m], o1 = a.m.obs_ptr[m + 1];
    if (o0 < 0 || o1 < o0 || o1 > NOBS) continue;
    for (int o = o0; o < o1; ++o) {
      const int k = a.m.obs_kf[o];
      if (k < 0 || k >= NKF) continue;
      if constexpr (CNT_LDS) atomicAdd(l_cnt + k, 1);
      else atomicAdd(g_cnt + k, 1);
      any = true;
    }
  }
  if (__any(any) && lane == 0) s_any = 1;  // (every writer stores the same value)
  sync();
  if (CNT_LDS && a.L.kf_count)
    for (int k = tid; k < NKF; k += T_LM) a.L.kf_count[(size_t)b * NKF + k] = l_cnt[k];
  if (!s_any) {  // (:147-148; workgroup-uniform) the lists and ref_kf keep the values passed in
    if (tid == 0) a.L.status[b] = GL_LOCAL_MAP_KEPT;
    return;
  }

  // ---- (b) local key-frames, ascending, and the reference key-frame (:150-166, :183-188)
  const int ck = (NKF + T_LM - 1) / T_LM;
  const int k0 = min(tid * ck, NKF), k1 = min(k0 + ck, NKF);
  int nloc = 0;
  unsigned long long best = 0ull;  // count << 32 | ~row: the largest count, then the lowest row
  for (int k = k0; k < k1; ++k) {
    const int c = cnt_get(k);
    if (c > 0 && (!a.m.kf_valid || a.m.kf_valid[k])) {
      ++nloc;
      const unsigned long long key = ((unsigned long long)(unsigned)c << 32) | (unsigned)(0x7fffffff - k);
      best = key > best ? key : best;
    }
  }
  int nkf_total;
  int pos = block_excl_scan<T_LM>(nloc, s_w, tid, &nkf_total);
  for (int k = k0; k < k1 && nloc > 0; ++k) {
    if (cnt_get(k) > 0 && (!a.m.kf_valid || a.m.kf_valid[k])) {
      if (pos < a.L.KFcap) a.L.local_kf[(size_t)b * a.L.KFcap + pos] = k;
      ++pos;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long t = __shfl_xor(best, o);
    best = t > best ? t : best;
  }
  if (lane == 0) s_best[wave] = best;

  // ---- (c) the mask of local map points (:191-201): a local key-frame per wave.  (Taking two features per thread through (a) together
  // and eight slots per lane through (c), loads first, was SLOWER: 56 -> 87 us on a map of 1 500 key-frames x 1 200 slots, B = 1 -
  // the plain loops below are what was kept.)
  for (int k = wave; k < NKF; k += T_LM / 64) {
    if (cnt_get(k) <= 0 || (a.m.kf_valid && !a.m.kf_valid[k])) continue;  // (the same k in every lane)
    const int32_t* row = a.m.kf_mp + (size_t)k * NFK;
    for (int j = lane; j < NFK; j += 64) {
      const int m = row[j];
      if (m < 0 || m >= NMP) continue;
      if (a.m.mp_valid && !a.m.mp_valid[m]) continue;
      if constexpr (MASK_LDS) atomicOr(l_mask + (m >> 5), 1u << (m & 31));
      else atomicOr(g_mask + (m >> 5), 1u << (m & 31));
    }
  }
  sync();
  if (tid == 0) {
    unsigned long long bb = 0ull;
    for (int i = 0; i < T_LM / 64; ++i) bb = s_best[i] > bb ? s_best[i] : bb;
    if (bb) a.L.ref_kf[b] = 0x7fffffff - (int)(unsigned)(bb & 0xffffffffull);
    a.L.n_local_kf[b] = nkf_total;
  }

  // ---- (d) the ascending list of local map points
  const int cw = (words + T_LM - 1) / T_LM;
  const int w0 = min(tid * cw, words), w1 = min(w0 + cw, words);
  int npt = 0;
  for (int w = w0; w < w1; ++w) npt += __popc(mask_get(w));
  int nmp_total;
  int at = block_excl_scan<T_LM>(npt, s_w, tid, &nmp_total);
  for (int w = w0; w < w1 && npt > 0; ++w) {
    uint32_t bits = mask_get(w);
    while (bits) {
      const int r = __ffs((int)bits) - 1;
      bits &= bits - 1;
      if (at < a.L.NPcap) a.L.local_mp[(size_t)b * a.L.NPcap + at] = w * 32 + r;
      ++at;
    }
  }
  if (tid == 0) {
    a.L.n_local_mp[b] = nmp_total;
    a.L.status[b] = (nmp_total > a.L.NPcap ? GL_LOCAL_MAP_MP_TRUNCATED : 0) | (nkf_total > a.L.KFcap ? GL_LOCAL_MAP_KF_TRUNCATED : 0);
  }
}

// The chain's local-map arrays from the whole map's through local_mp, a slot (or a last-frame / key-frame feature) per thread.
struct LmGatherArgs {
  gl_map_view m;
  int B, NL, NK, NPcap;
  const int32_t* local_mp;
  const int32_t* n_local_mp;
  const int32_t* last_mp;
  const int32_t* kf_feat_mp;
  gl::LocalMapGathered G;
};
__device__ __forceinline__ int lm_find(const int32_t* list, int n, int m) {  // index of m in the ascending list, or -1
  if (m < 0) return -1;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (list[mid] < m) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && list[lo] == m) ? lo : -1;
}
__global__ __launch_bounds__(256) void k_local_map_gather(LmGatherArgs a) {
  const int b = blockIdx.x, item = blockIdx.y * 256 + threadIdx.x;
  if (b >= a.B) return;
  const int NP = a.NPcap;
  const int32_t* list = a.local_mp + (size_t)b * NP;
  const int n = min(max(a.n_local_mp[b], 0), NP);
  if (item < NP) {
    const size_t g = (size_t)b * NP + item;
    const int m = item < n ? list[item] : -1;
    const bool on = m >= 0 && m < a.m.NMP;  // (a list kept from the caller may hold anything)
    uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
    double p[3] = {0, 0, 0}, nr[3] = {0, 0, 0};
    float dmax = 0.0f, dmin = 0.0f;
    if (on) {
      const uint4* s = (const uint4*)(a.m.mp_desc + (size_t)m * 32);
      d0 = s[0];
      d1 = s[1];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        p[k] = a.m.mp_pos[(size_t)m * 3 + k];
        nr[k] = a.m.mp_normal[(size_t)m * 3 + k];
      }
      dmax = a.m.mp_max_dist[m];
      dmin = a.m.mp_min_dist[m];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a.G.mp_pos[g * 3 + k] = p[k];
      a.G.mp_normal[g * 3 + k] = nr[k];
    }
    a.G.mp_max_dist[g] = dmax;
    a.G.mp_min_dist[g] = dmin;
    a.G.mp_cand[g] = on ? 1 : 0;
    uint4* dd = (uint4*)(a.G.mp_desc + g * 32);
    dd[0] = d0;
    dd[1] = d1;
  } else if (item < NP + a.NL) {
    const size_t g = (size_t)b * a.NL + (item - NP);
    a.G.last_to_local[g] = lm_find(list, n, a.last_mp[g]);
  } else if (item < NP + a.NL + a.NK) {
    const size_t g = (size_t)b * a.NK + (item - NP - a.NL);
    a.G.kf_to_local[g] = lm_find(list, n, a.kf_feat_mp[g]);
  }
}

bool cnt_in_lds(const gl::Ctx* c, const gl_map_view* m) { return m->NKF <= LM_KF_LDS && (size_t)m->NKF * 4 + 1024 <= (size_t)c->lds_max; }
int mask_words(const gl_map_view* m) { return (int)(((int64_t)m->NMP + 31) / 32); }
bool mask_in_lds(const gl::Ctx* c, const gl_map_view* m) {
  return m->NMP <= LM_MP_LDS && (cnt_in_lds(c, m) ? (size_t)m->NKF * 4 : 0) + (size_t)mask_words(m) * 4 + 1024 <= (size_t)c->lds_max;
}

template <bool CNT_LDS, bool MASK_LDS>
int lm_launch(gl::Ctx* c, const LmArgs& a) {
  const size_t lds = (CNT_LDS ? (size_t)a.m.NKF * 4 : 0) + (MASK_LDS ? (size_t)a.words * 4 : 0);
  GL_HIP(gl::ensure_dynamic_lds(c, (const void*)k_local_map<CNT_LDS, MASK_LDS>, lds));
  k_local_map<CNT_LDS, MASK_LDS><<<a.B, T_LM, lds, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

}  // namespace

namespace gl {

int local_map_check(const gl_map_view* map, int B, int NF, const LocalMapLists& L, bool need_point_arrays) {
  GL_REQUIRE(map, "null argument");
  GL_REQUIRE(B >= 0 && NF >= 1 && L.KFcap >= 1 && L.NPcap >= 1, "bad B / NF / KFcap / NPcap");
  if (B == 0) return GL_OK;
  mapdev::Map m;  // (for its checks: the kernels below take the view itself)
  const int rc = mapdev::map_from_view(__func__, map, nullptr, &m);
  if (rc != GL_OK) return rc;
  if (need_point_arrays)
    GL_REQUIRE(map->NMP == 0 || (map->mp_pos && map->mp_normal && map->mp_max_dist && map->mp_min_dist && map->mp_desc),
               "null mp_pos / mp_normal / mp_max_dist / mp_min_dist / mp_desc");
  GL_REQUIRE(L.feat_mp && L.local_kf && L.n_local_kf && L.local_mp && L.n_local_mp && L.ref_kf && L.status, "null buffer");
  return GL_OK;
}

size_t local_map_scratch_bytes(const Ctx* c, const gl_map_view* map, int B, bool have_kf_count) {
  Regions r = {0};
  if (!cnt_in_lds(c, map) && !have_kf_count) r.take((size_t)B * map->NKF * 4);
  if (!mask_in_lds(c, map)) r.take((size_t)B * mask_words(map) * 4);
  return r.off;
}

int local_map_launch(Ctx* c, const gl_map_view* map, int B, int NF, const LocalMapLists& L, const LocalMapDerive* derive, void* scratch) {
  LmArgs a;
  a.m = *map;
  a.B = B;
  a.NF = NF;
  a.L = L;
  a.derive = derive ? 1 : 0;
  a.d = derive ? *derive : LocalMapDerive{};
  a.words = mask_words(map);
  const bool cl = cnt_in_lds(c, map), ml = mask_in_lds(c, map);
  Regions r = {0};
  a.cnt_glob = cl ? nullptr : L.kf_count ? L.kf_count : (int32_t*)((char*)scratch + r.take((size_t)B * map->NKF * 4));
  a.mask_glob = ml ? nullptr : (uint32_t*)((char*)scratch + r.take((size_t)B * a.words * 4));
  if (cl) return ml ? lm_launch<true, true>(c, a) : lm_launch<true, false>(c, a);
  return ml ? lm_launch<false, true>(c, a) : lm_launch<false, false>(c, a);
}

size_t local_map_gathered_place(void* base, int B, int NPcap, int NL, int NK, LocalMapGathered* out) {
  Regions r = {0};
  const size_t np = (size_t)B * NPcap;
  const size_t o_pos = r.take(np * 24), o_nrm = r.take(np * 24), o_max = r.take(np * 4), o_min = r.take(np * 4), o_cand = r.take(np),
               o_desc = r.take(np * 32), o_l2l = r.take((size_t)B * NL * 4), o_k2l = r.take((size_t)B * (NK > 0 ? NK : 1) * 4);
  if (base && out) {
    char* s = (char*)base;
    out->mp_pos = (double*)(s + o_pos);
    out->mp_normal = (double*)(s + o_nrm);
    out->mp_max_dist = (float*)(s + o_max);
    out->mp_min_dist = (float*)(s + o_min);
    out->mp_cand = (uint8_t*)(s + o_cand);
    out->mp_desc = (uint8_t*)(s + o_desc);
    out->last_to_local = (int32_t*)(s + o_l2l);
    out->kf_to_local = (int32_t*)(s + o_k2l);
  }
  return r.off;
}

int local_map_gather_launch(Ctx* c, const gl_map_view* map, int B, int NL, int NK, const LocalMapLists& L, const int32_t* last_mp,
                            const int32_t* kf_feat_mp, const LocalMapGathered& G) {
  LmGatherArgs a;
  a.m = *map;
  a.B = B;
  a.NL = NL;
  a.NK = kf_feat_mp ? NK : 0;
  a.NPcap = L.NPcap;
  a.local_mp = L.local_mp;
  a.n_local_mp = L.n_local_mp;
  a.last_mp = last_mp;
  a.kf_feat_mp = kf_feat_mp;
  a.G = G;
  const int items = L.NPcap + NL + a.NK;
  k_local_map_gather<<<dim3((unsigned)B, (unsigned)((items + 255) / 256)), 256, 0, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

}  // namespace gl

extern "C" int gl_update_local_map(gl_ctx_t* ctx, const gl_map_view* map, int B, int NF, int KFcap, int NPcap, int32_t* feat_mp_dev,
                                   int32_t* local_kf_dev, int32_t* n_local_kf_dev, int32_t* local_mp_dev, int32_t* n_local_mp_dev,
                                   int32_t* ref_kf_dev, int32_t* kf_count_dev, int32_t* status_dev) {
  GL_REQUIRE(ctx, "null argument");
  const gl::LocalMapLists L = {KFcap, NPcap, feat_mp_dev, local_kf_dev, n_local_kf_dev, local_mp_dev, n_local_mp_dev, ref_kf_dev, kf_count_dev, status_dev};
  const int rc = gl::local_map_check(map, B, NF, L, false);
  if (rc != GL_OK || B == 0) return rc;
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  void* scratch = nullptr;
  const size_t bytes = gl::local_map_scratch_bytes(c, map, B, kf_count_dev != nullptr);
  if (bytes) {
    const int rs = gl::ctx_scratch(c, bytes, &scratch, gl::SCRATCH_LOCALMAP);
    if (rs != GL_OK) return rs;
  }
  return gl::local_map_launch(c, map, B, NF, L, nullptr, scratch);
}
