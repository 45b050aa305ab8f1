// Editing the resident map (gmmloc_hip.h): the key-frame culling of Localization::removeKeyFrames (localization.cpp:334-399) and the
// removals - Map::removeMapPoint (map.cpp:40-58), the local BA's erase loop (localization_opt.cpp:884-894), Map::removeKeyFrame
// (map.cpp:60-110) with the cascade of MapPoint::removeObservation (mappoint.cpp:94-118) - applied in place to the caller-owned arrays.
// The rules, the closed form of the sequential semantics and the declared deviation are in the header.
//   culling   one workgroup per candidate list.  The loop's state is the set C of the key-frames culled so far: a bit per key-frame
//             row in dynamic LDS, next to the bits of the rows already seen in the list.  The candidates are walked in order; per
//             candidate a slot per thread, each thread walks its point's CSR range against C; wave sums, two LDS integer atomics per
//             wave, thread 0 decides.  One pass over the candidate's points' observations per candidate, like conn_count.
//   removal   (a) k_me_mark: a flag per erased CSR position, a flag per removed point, the list RANK of every removed key-frame
//             (atomicMin: a duplicate is harmless); (b) k_me_points: a point per thread - what it loses, its weight, the step at
//             which it dies, the slots cleared, mp_ref_kf, its surviving count; (c) csr_rebuild_scan / k_me_scan_top: the exclusive scan
//             of (surviving count | died << 32) over the points, 4 096 points per workgroup and one workgroup over the partial sums;
//             (d) k_me_move: a point per thread copies its surviving entries to their new places.  The move is NOT in place: obs_kf /
//             obs_feat are first copied to the context's scratch and (d) reads the copy; the new obs_ptr is made in the scratch and
//             copied over the old one last, because (d) still reads the old ranges.  (c) and (d) are mapdev's rebuild of the CSR,
//             shared with gl_map_add and gl_map_fuse; its scan kernel is defined here.
// Everything is integer; the only atomics are atomicMin / atomicOr on words whose final value the inputs determine.
#include "gl_map_dev.hpp"

namespace {

using namespace gl::mapdev;  // Map, mp_ok, kf_ok, obs_range, obs_weight, list_len, tile_scan, CsrRebuild, csr_move_point

constexpr int T_CULL = 1024;
constexpr int T_ME = 256;
constexpr int RANK_NONE = 0x7f7f7f7f;  // (a byte pattern: the ranks are reset by one memset); also "never dies"

// ---------------------------------------------------------------------------------------------------------------- culling
struct CullArgs {
  Map m;
  const float* kf_depth;
  float th_depth;
  int B, Ccap;
  const int32_t *cand_kf, *n_cand;
  uint8_t* cull;
  int32_t *num_mps, *num_red, *status, *cull_rows, *n_cull;
};

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(T_CULL) void k_cull_keyframes(CullArgs a) {
  extern __shared__ unsigned cull_lds[];  // [0, nw): C; [nw, 2 nw): the rows seen
  __shared__ int s_cnt[2];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (b >= a.B) return;
  const Map& m = a.m;
  const int NKF = m.NKF, NFK = m.NFK, nw = (NKF + 31) >> 5;
  unsigned* const inC = cull_lds;
  unsigned* const seen = cull_lds + nw;
  for (int i = tid; i < 2 * nw; i += T_CULL) cull_lds[i] = 0u;
  if (tid < 2) s_cnt[tid] = 0;
  __syncthreads();
  const int n = min(max(a.n_cand[b], 0), a.Ccap);
  const size_t row0 = (size_t)b * a.Ccap;
  int nc = 0;  // (thread 0: the culled so far)
  for (int j = 0; j < n; ++j) {
    const int kf = a.cand_kf[row0 + j];
    int st = GL_CULL_JUDGED;
    if (kf < 0 || kf >= NKF) st = GL_CULL_BAD_ROW;
    else if (seen[kf >> 5] >> (kf & 31) & 1u) st = GL_CULL_DUPLICATE;
    else if (kf == m.kf_first) st = GL_CULL_FIRST;
    else if (!kf_ok(m, kf)) st = GL_CULL_INVALID;
    __syncthreads();  // (every thread has read `seen`)
    if (tid == 0 && st != GL_CULL_BAD_ROW && st != GL_CULL_DUPLICATE) seen[kf >> 5] |= 1u << (kf & 31);
    if (st != GL_CULL_JUDGED) {  // (workgroup-uniform)
      if (tid == 0) {
        a.cull[row0 + j] = 0;
        a.num_mps[row0 + j] = 0;
        a.num_red[row0 + j] = 0;
        a.status[row0 + j] = st;
      }
      __syncthreads();
      continue;
    }
    int mps = 0, red = 0;
    const size_t krow = (size_t)kf * NFK;
    for (int i = tid; i < NFK; i += T_CULL) {
      const int p = m.kf_mp[krow + i];
      if (!mp_ok(m, p)) continue;
      const float d = a.kf_depth[krow + i];
      if (d > a.th_depth || d < 0.f) continue;  // (:358-362; a slot that is not counted needs no walk)
      const int oct = m.kf_oct[krow + i];
      int o0, o1, w = 0, near = 0;
      bool byC = false;
      obs_range(m, p, &o0, &o1);
      // (obs_weight's rule written out: two entries at a time, the loads of their u_right and octave issued together - measured)
      for (int o = o0; o < o1; o += 2) {
        int k[2], f[2], oc[2];
        double ur[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const bool in = o + u < o1;
          k[u] = in ? m.obs_kf[o + u] : -1;
          f[u] = in ? m.obs_feat[o + u] : -1;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const bool kin = k[u] >= 0 && k[u] < NKF;
          const bool gone = kin && (inC[k[u] >> 5] >> (k[u] & 31) & 1u);  // removed with its key-frame
          byC = byC || gone;
          if (!(kin && !gone && f[u] >= 0 && f[u] < NFK)) k[u] = -1;  // (a feature outside the table: no octave, no weight)
          const size_t ft = k[u] >= 0 ? (size_t)k[u] * NFK + f[u] : 0;
          ur[u] = m.kf_uvr[ft * 3 + 2];
          oc[u] = m.kf_oct[ft];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if (k[u] < 0) continue;
          w += ur[u] >= 0.0 ? 2 : 1;
          near += k[u] != kf && oc[u] <= oct + 1;
        }
      }
      if (byC && w <= 2) continue;  // dead by the cascade
      ++mps;
      red += w > 3 && near >= 3;
    }
    mps = wave_sum(mps);
    red = wave_sum(red);
    if (lane == 0 && mps) {
      atomicAdd(&s_cnt[0], mps);
      atomicAdd(&s_cnt[1], red);
    }
    __syncthreads();
    if (tid == 0) {
      const int nm = s_cnt[0], nr = s_cnt[1];
      const int v = (double)nr > 0.9 * (double)nm ? 1 : 0;  // (:394)
      s_cnt[0] = s_cnt[1] = 0;
      a.cull[row0 + j] = (uint8_t)v;
      a.num_mps[row0 + j] = nm;
      a.num_red[row0 + j] = nr;
      a.status[row0 + j] = GL_CULL_JUDGED;
      if (v) {
        inC[kf >> 5] |= 1u << (kf & 31);
        a.cull_rows[row0 + nc++] = kf;
      }
    }
    __syncthreads();
  }
  if (tid == 0) a.n_cull[b] = nc;
}

// ---------------------------------------------------------------------------------------------------------------- removal
struct EditArgs {
  Map m;
  gl_map_remove_lists l;
  gl_map_remove_out out;
  // scratch
  int32_t* rank;    // NKF: the place of a removed key-frame in rm_kf, RANK_NONE
  uint8_t* pflag;   // NMP: 1 listed in rm_mp; 2 died in this call
  uint8_t* oflag;   // NOBS: 1 erased (a), then 1 lost (b)
  CsrRebuild rb;    // cnt: surviving entries | died << 32
};

__global__ __launch_bounds__(T_ME) void k_me_mark(EditArgs a) {
  const int g = blockIdx.x * T_ME + threadIdx.x, G = gridDim.x * T_ME;
  if (a.l.erase_obs) {
    const int n = list_len(a.l.n_erase, a.l.erase_cap);
    for (int i = g; i < n; i += G) {
      const int o = a.l.erase_obs[i];
      if (o >= 0 && o < a.m.NOBS) a.oflag[o] = 1;
    }
  }
  if (a.l.rm_mp) {
    const int n = list_len(a.l.n_rm_mp, a.l.rm_mp_cap);
    for (int i = g; i < n; i += G) {
      const int p = a.l.rm_mp[i];
      if (mp_row(a.m, p) && a.m.mp_valid[p]) a.pflag[p] = 1;
    }
  }
  if (a.l.rm_kf) {
    const int n = list_len(a.l.n_rm_kf, a.l.rm_kf_cap);
    for (int i = g; i < n; i += G) {
      const int k = a.l.rm_kf[i];
      if (!kf_row(a.m, k) || !a.m.kf_valid[k]) continue;
      if (k == a.m.kf_first) atomicOr(a.out.result + 2, GL_MAP_REMOVE_FIRST_REFUSED);  // (map.cpp:63)
      else atomicMin(a.rank + k, i);
    }
  }
}

__global__ __launch_bounds__(T_ME) void k_me_points(EditArgs a) {
  const int p = blockIdx.x * T_ME + threadIdx.x;
  const Map& m = a.m;
  if (p < m.NKF && a.rank[p] != RANK_NONE) m.kf_valid[p] = 0;  // (the grid covers max(NMP, NKF) threads)
  if (p >= m.NMP) return;
  int o0, o1;
  obs_range(m, p, &o0, &o1);
  if (!m.mp_valid[p]) {  // a dead point ignores removals (mappoint.cpp:99): its entries, if it has any, stay
    a.rb.cnt[p] = (u64)(o1 - o0);
    for (int o = o0; o < o1; ++o) a.oflag[o] = 0;
    return;
  }
  const int pf = a.pflag[p];
  auto rank_of = [&](int k) -> int { return kf_row(m, k) ? a.rank[k] : RANK_NONE; };
  int wtot = 0, w_er = 0, w_rk = 0, n_er = 0, n_rk = 0;
  for (int o = o0; o < o1; ++o) {
    const int k = m.obs_kf[o], w = obs_weight(m, k, m.obs_feat[o]);
    wtot += w;
    if (a.oflag[o]) {
      ++n_er;
      w_er += w;
    } else if (rank_of(k) != RANK_NONE) {
      ++n_rk;
      w_rk += w;
    }
  }
  if (!pf && n_er == 0 && n_rk == 0) {  // lost nothing: untouched
    a.rb.cnt[p] = (u64)(o1 - o0);
    return;
  }
  // the step at which it dies: -1 in the point / erase phase, else the rank of the first removed observer that leaves w <= 2
  const int w1 = wtot - w_er;
  int t = RANK_NONE;
  if (pf || (n_er > 0 && w1 <= 2)) t = -1;
  else if (n_rk > 0 && w1 - w_rk <= 2) {
    for (int o = o0; o < o1; ++o) {
      const int re = a.oflag[o] ? RANK_NONE : rank_of(m.obs_kf[o]);
      if (re == RANK_NONE || re >= t) continue;
      int w = w1;
      for (int o2 = o0; o2 < o1; ++o2) {
        const int k2 = m.obs_kf[o2];
        if (!a.oflag[o2] && rank_of(k2) <= re) w -= obs_weight(m, k2, m.obs_feat[o2]);
      }
      if (w <= 2) t = re;
    }
  }
  const bool dead = t != RANK_NONE;
  const int ref = m.mp_ref_kf ? m.mp_ref_kf[p] : -1;
  int keep = 0, first_k = -1;
  bool ref_lost = false;
  for (int o = o0; o < o1; ++o) {
    const int k = m.obs_kf[o], f = m.obs_feat[o];
    const bool er = a.oflag[o] != 0;
    const int rk = rank_of(k);
    const bool lost = dead || er || rk != RANK_NONE;
    // an erased observation clears its slot; a dying point clears its remaining observers', a removed key-frame's only if it died before
    const bool clear = er || (dead && (rk == RANK_NONE || t < rk));
    if (clear && slot_in(m, k, f)) {
      int32_t* slot = m.kf_mp + (size_t)k * m.NFK + f;
      if (*slot == p) *slot = -1;
    }
    a.oflag[o] = lost ? 1 : 0;
    if (!lost) {
      if (keep++ == 0) first_k = k;
    } else if (k == ref) {
      ref_lost = true;
    }
  }
  if (dead) {
    m.mp_valid[p] = 0;
    a.pflag[p] = 2;
    a.rb.cnt[p] = 1ull << 32;
  } else {
    a.rb.cnt[p] = (u64)keep;
    if (m.mp_ref_kf && ref_lost && keep > 0) m.mp_ref_kf[p] = first_k;
  }
}

// the exclusive scan of cnt inside every tile of SCAN_TILE words, the tile's sum to tile[] (csr_rebuild_scan)
__global__ __launch_bounds__(SCAN_T) void k_csr_scan(u64* cnt, u64* tile, const int32_t* n_dev, int n_host) {
  __shared__ u64 s_w[SCAN_T / 64];
  tile_scan(cnt, tile, n_dev ? (size_t)*n_dev : (size_t)n_host, s_w, threadIdx.x, blockIdx.x);
}

// one workgroup: the exclusive scan of the tile sums; the totals
__global__ __launch_bounds__(SCAN_T) void k_me_scan_top(EditArgs a, int ntile) {
  __shared__ u64 s_w[SCAN_T / 64];
  const int tid = threadIdx.x;
  const u64 carry = tile_scan_top(a.rb.tile, ntile, s_w, tid);
  if (tid == 0) {
    const int nobs = (int)(unsigned)(carry & 0xffffffffull), ndead = (int)(unsigned)(carry >> 32);
    a.rb.nptr[a.m.NMP] = nobs;
    a.out.result[0] = nobs;
    a.out.result[1] = ndead;
    if (ndead > a.out.dead_cap) atomicOr(a.out.result + 2, GL_MAP_REMOVE_DEAD_TRUNCATED);
  }
}

__global__ __launch_bounds__(T_ME) void k_me_move(EditArgs a) {
  const int p = blockIdx.x * T_ME + threadIdx.x;
  if (p >= a.m.NMP) return;
  const int di = (int)(unsigned)(csr_place(a.rb, p) >> 32);
  if (a.pflag[p] == 2 && di < a.out.dead_cap) a.out.dead_mp[di] = p;
  // (a removal only compacts: the limit is NOBS)
  csr_move_point(a.m, a.rb, p, a.m.NOBS, a.out.obs_new_pos, [&](int o) { return !a.oflag[o]; }, [](auto&) {});
}

}  // namespace

void gl::mapdev::csr_rebuild_scan(gl::Ctx* c, const CsrRebuild& rb, int ntile, const int32_t* n_dev, int n_host) {
  if (ntile > 0) k_csr_scan<<<ntile, SCAN_T, 0, c->stream>>>(rb.cnt, rb.tile, n_dev, n_host);
}

extern "C" int gl_cull_keyframes(gl_ctx_t* ctx, const gl_map_view* map, const gl_map_ba_view* ba, const float* kf_depth_dev, float th_depth, int B,
                                 int Ccap, const int32_t* cand_kf_dev, const int32_t* n_cand_dev, uint8_t* cull_dev, int32_t* num_mps_dev,
                                 int32_t* num_redundant_dev, int32_t* cand_status_dev, int32_t* cull_rows_dev, int32_t* n_cull_dev) {
  GL_REQUIRE(ctx && map && ba, "null argument");
  GL_REQUIRE(B >= 0 && Ccap >= 1, "bad B / Ccap");
  if (B == 0) return GL_OK;
  CullArgs a;
  const int rc = map_from_view(__func__, map, ba, &a.m);
  if (rc != GL_OK) return rc;
  GL_REQUIRE(map->NKF <= GL_CULL_MAX_KF, "more than GL_CULL_MAX_KF key-frames");
  GL_REQUIRE(map->NKF == 0 || map->NFK == 0 || kf_depth_dev, "null kf_depth");
  GL_REQUIRE(cand_kf_dev && n_cand_dev && cull_dev && num_mps_dev && num_redundant_dev && cand_status_dev && cull_rows_dev && n_cull_dev, "null buffer");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  const size_t lds = (size_t)((map->NKF + 31) / 32) * 2 * 4;
  GL_REQUIRE_LDS(c, lds + 256);
  a.kf_depth = kf_depth_dev;
  a.th_depth = th_depth;
  a.B = B;
  a.Ccap = Ccap;
  a.cand_kf = cand_kf_dev;
  a.n_cand = n_cand_dev;
  a.cull = cull_dev;
  a.num_mps = num_mps_dev;
  a.num_red = num_redundant_dev;
  a.status = cand_status_dev;
  a.cull_rows = cull_rows_dev;
  a.n_cull = n_cull_dev;
  GL_HIP(gl::ensure_dynamic_lds(c, (const void*)k_cull_keyframes, lds));
  k_cull_keyframes<<<B, T_CULL, lds, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_map_remove(gl_ctx_t* ctx, int NMP, int NKF, int NFK, int NOBS, const gl_map_edit* ed, const double* kf_uvr_dev, int kf_first,
                             const gl_map_remove_lists* lists, const gl_map_remove_out* out) {
  GL_REQUIRE(ctx && ed && lists && out, "null argument");
  EditArgs a = {};
  const int rc = map_from_edit(__func__, NMP, NKF, NFK, NOBS, ed, kf_uvr_dev, kf_first, &a.m);
  if (rc != GL_OK) return rc;
  GL_REQUIRE(NKF == 0 || ed->kf_valid, "null kf_valid");
  GL_REQUIRE(NKF == 0 || NFK == 0 || kf_uvr_dev, "null kf_uvr");
  GL_REQUIRE(lists->rm_mp_cap >= 0 && lists->erase_cap >= 0 && lists->rm_kf_cap >= 0, "bad list capacity");
  GL_REQUIRE(out->result, "null result");
  GL_REQUIRE(out->dead_cap >= 0 && (out->dead_cap == 0 || out->dead_mp), "bad dead_cap / null dead_mp");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  a.l = *lists;
  a.out = *out;
  if (!a.l.rm_mp || a.l.rm_mp_cap == 0) a.l.rm_mp = nullptr, a.l.rm_mp_cap = 0;
  if (!a.l.erase_obs || a.l.erase_cap == 0) a.l.erase_obs = nullptr, a.l.erase_cap = 0;
  if (!a.l.rm_kf || a.l.rm_kf_cap == 0) a.l.rm_kf = nullptr, a.l.rm_kf_cap = 0;
  GL_HIP(hipMemsetAsync(out->result, 0, 3 * sizeof(int32_t), c->stream));
  const int ntile = csr_tiles(NMP);
  gl::Regions r = {0};
  // rank first, the flags next to each other: two memsets reset them
  const size_t o_rank = r.take((size_t)NKF * 4), o_pflag = r.take((size_t)NMP), o_oflag = r.take((size_t)NOBS), flags_end = r.off;
  void* scratch = nullptr;
  const int rs = gl::ctx_scratch(c, flags_end + csr_rebuild_place(nullptr, NMP, NOBS, nullptr), &scratch, gl::SCRATCH_MAPEDIT);
  if (rs != GL_OK) return rs;
  char* s = (char*)scratch;
  a.rank = (int32_t*)(s + o_rank);
  a.pflag = (uint8_t*)(s + o_pflag);
  a.oflag = (uint8_t*)(s + o_oflag);
  csr_rebuild_place(s + flags_end, NMP, NOBS, &a.rb);
  if (NKF > 0) GL_HIP(hipMemsetAsync(a.rank, 0x7f, (size_t)NKF * 4, c->stream));
  if (flags_end > o_pflag) GL_HIP(hipMemsetAsync(a.pflag, 0, flags_end - o_pflag, c->stream));
  const int rb = csr_rebuild_begin(c, a.rb, a.m, out->obs_new_pos);
  if (rb != GL_OK) return rb;
  const int nlist = std::max(a.l.rm_mp_cap, std::max(a.l.erase_cap, a.l.rm_kf_cap));
  if (nlist > 0) k_me_mark<<<std::min((nlist + T_ME - 1) / T_ME, 1024), T_ME, 0, c->stream>>>(a);
  const int nrow = std::max(NMP, NKF);
  if (nrow > 0) k_me_points<<<(nrow + T_ME - 1) / T_ME, T_ME, 0, c->stream>>>(a);
  csr_rebuild_scan(c, a.rb, ntile, nullptr, NMP);
  k_me_scan_top<<<1, SCAN_T, 0, c->stream>>>(a, ntile);
  if (NMP > 0) k_me_move<<<(NMP + T_ME - 1) / T_ME, T_ME, 0, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  GL_HIP(hipMemcpyAsync(ed->obs_ptr, a.rb.nptr, ((size_t)NMP + 1) * 4, hipMemcpyDeviceToDevice, c->stream));
  return GL_OK;
}
