// Growing the resident map (gmmloc_hip.h): what ADDS to the caller-owned arrays of gl_map_edit - new map-point rows, new key-frames,
// MapPoint::addObservation / KeyFrame::addObservation (mappoint.cpp:72-82, keyframe.cpp:190-193), the loop of processNewKeyFrame
// (localization.cpp:424-437) - and the second half of Localization::fuseObservations (localization.cpp:299-321) with
// Map::replaceMapPoint (map.cpp:112-150).  The rules, the declared CSR order and what stays with the host are in the header.
//   gl_map_add   a parallel edit.  Every attach triple and every slot of a walked key-frame is a REQUEST with an index r (the triples
//                in list order, then the walks in list order, slots ascending).  (a) k_ma_mark: the new key-frames, the list rank of
//                every walked row; (b) k_ma_triples: the skips, the last triple of every slot (atomicMax of r on a word per slot), the
//                first request of every (point, key-frame) pair (atomicMin of r in an open-addressing table keyed by the pair);
//                (c) k_ma_walks: the same for the walk requests, on the slots as the triples leave them; (d) k_ma_resolve: a request
//                attaches iff its pair is not in the CSR and it is the pair's first; (e) k_ma_count + the scan: the new obs_ptr and
//                the sizes, checked against the capacities - NOTHING of the map has been written up to here; (f) k_ma_place /
//                k_ma_rows / k_ma_move / k_ma_ptr, each a no-op after a truncation: the rows, the slots, the entries moved through a
//                copy, a point's gained entries ordered by r.
//   gl_map_fuse  the sequential one.  k_mf_init: a word per point (weighted count, -1 invalid); k_mf_walk: ONE workgroup walks the
//                candidates in list order.  It never edits the CSR: an old entry that leaves its point gets a flag, a gained or moved
//                entry is a node of a per-point chain in a log (a node that moves on is relinked, so the log holds at most
//                NOBS + n_cand nodes).  Inside a step the workgroup works in parallel over the target's entries (a stamp per
//                key-frame: checkObservation) and over the source's (an exclusive scan gives the moved entries their places in
//                order).  Then one parallel rebuild: count, scan, stable move through a copy.
// Both rebuilds are mapdev's (CsrRebuild, csr_rebuild_scan, csr_move_point: gl_map_dev.hpp, shared with gl_map_remove).
// Everything is integer; the atomics are atomicMin / atomicMax / atomicCAS / atomicAdd on words whose final value the inputs determine.
#include "gl_map_dev.hpp"

namespace {

using namespace gl::mapdev;  // Map, mp_row, kf_row, slot_in, obs_range, obs_weight, list_len, block_excl_scan, CsrRebuild, csr_move_point

constexpr int T_MG = 256;
constexpr u64 H_EMPTY = ~0ull;
constexpr int R_NONE = 0x7f7f7f7f;  // (a byte pattern: one memset)

// ---------------------------------------------------------------------------------------------------------------- gl_map_add
struct AddArgs {
  Map m;  // the sizes on entry; mp_pos and mp_assoc are the caller's non-const arrays
  int NMPcap, OBScap;
  gl_map_add_lists l;
  gl_map_add_out out;
  unsigned hmask;
  // scratch
  int32_t* sizes;     // {NMP', n_tri, n_walk, n requests}
  uint8_t* kfnew;     // NKF: listed in new_kf
  int32_t* walkrank;  // NKF: the first place of the row in walk_kf, R_NONE
  int32_t* slotw;     // NKF x NFK: the last triple that names the slot, -1
  u64* hkey;          // the table: (point << 32 | key-frame), H_EMPTY
  int32_t* hval;      // the first request of the pair, R_NONE
  int32_t* req_mp;    // per request: its point, -1 for one that does nothing
  uint8_t* req_fl;    // per request: 1 attaches, 2 a walked slot whose point already observes
  int32_t* gcnt;      // per point: gained entries; then the cursor of k_ma_place
  int32_t* seg;       // the attaching requests, grouped by point
  CsrRebuild rb;      // over NMP' points; cnt: entries | gained << 32
};

__device__ __forceinline__ bool ma_truncated(const AddArgs& a) {
  return (a.out.result[5] & (GL_MAP_GROW_MP_TRUNCATED | GL_MAP_GROW_OBS_TRUNCATED)) != 0;
}
__device__ __forceinline__ bool ma_mp_ok(const AddArgs& a, int p, int NMP2) { return p >= 0 && p < NMP2 && (p >= a.m.NMP || a.m.mp_valid[p]); }
__device__ __forceinline__ bool ma_kf_ok(const AddArgs& a, int k) { return kf_row(a.m, k) && (a.m.kf_valid[k] || a.kfnew[k]); }

__device__ __forceinline__ unsigned h_slot(u64 key, unsigned mask) {
  key *= 0x9E3779B97F4A7C15ull;
  return (unsigned)(key >> 32) & mask;
}
__device__ __forceinline__ void h_insert(const AddArgs& a, int p, int k, int r) {
  const u64 key = (u64)(unsigned)p << 32 | (unsigned)k;
  unsigned h = h_slot(key, a.hmask);
  for (unsigned n = 0; n <= a.hmask; ++n, h = (h + 1) & a.hmask) {
    const u64 old = atomicCAS(a.hkey + h, H_EMPTY, key);
    if (old == H_EMPTY || old == key) {
      atomicMin(a.hval + h, r);
      return;
    }
  }
}
__device__ __forceinline__ int h_first(const AddArgs& a, int p, int k) {
  const u64 key = (u64)(unsigned)p << 32 | (unsigned)k;
  unsigned h = h_slot(key, a.hmask);
  for (unsigned n = 0; n <= a.hmask; ++n, h = (h + 1) & a.hmask) {
    const u64 at = a.hkey[h];
    if (at == key) return a.hval[h];
    if (at == H_EMPTY) break;
  }
  return R_NONE;
}

// the key-frame and feature of request r (a triple, or slot i of walk w)
__device__ __forceinline__ void ma_request(const AddArgs& a, int r, int n_tri, int* k, int* f) {
  if (r < n_tri) {
    *k = a.l.att_kf[r];
    *f = a.l.att_feat[r];
  } else {
    const int q = r - n_tri;
    *k = a.l.walk_kf[q / a.m.NFK];
    *f = q % a.m.NFK;
  }
}

__global__ __launch_bounds__(T_MG) void k_ma_mark(AddArgs a) {
  const int g = blockIdx.x * T_MG + threadIdx.x, G = gridDim.x * T_MG;
  const int n_new = a.l.new_pos ? list_len(a.l.n_new_mp, a.l.new_mp_cap) : 0;
  const int n_tri = a.l.att_mp ? list_len(a.l.n_attach, a.l.attach_cap) : 0;
  const int n_walk = a.l.walk_kf ? list_len(a.l.n_walk, a.l.walk_cap) : 0;
  if (g == 0) {
    a.sizes[0] = a.m.NMP + n_new;
    a.sizes[1] = n_tri;
    a.sizes[2] = n_walk;
    a.sizes[3] = n_tri + n_walk * a.m.NFK;
  }
  if (a.l.new_kf) {
    const int n = list_len(a.l.n_new_kf, a.l.new_kf_cap);
    for (int i = g; i < n; i += G) {
      const int k = a.l.new_kf[i];
      if (kf_row(a.m, k)) a.kfnew[k] = 1;
    }
  }
  for (int i = g; i < n_walk; i += G) {
    const int k = a.l.walk_kf[i];
    if (kf_row(a.m, k)) atomicMin(a.walkrank + k, i);
  }
}

__global__ __launch_bounds__(T_MG) void k_ma_triples(AddArgs a) {
  const int NMP2 = a.sizes[0], n_tri = a.sizes[1];
  for (int r = blockIdx.x * T_MG + threadIdx.x; r < n_tri; r += gridDim.x * T_MG) {
    const int p = a.l.att_mp[r], k = a.l.att_kf[r], f = a.l.att_feat[r];
    const bool ok = ma_mp_ok(a, p, NMP2) && f >= 0 && f < a.m.NFK && ma_kf_ok(a, k);
    a.req_mp[r] = ok ? p : -1;
    if (!ok) {
      atomicAdd(a.out.result + 3, 1);
      continue;
    }
    atomicMax(a.slotw + (size_t)k * a.m.NFK + f, r);
    h_insert(a, p, k, r);
  }
}

__global__ __launch_bounds__(T_MG) void k_ma_walks(AddArgs a) {
  const int NMP2 = a.sizes[0], n_tri = a.sizes[1], n_req = a.sizes[3];
  for (int r = n_tri + blockIdx.x * T_MG + threadIdx.x; r < n_req; r += gridDim.x * T_MG) {
    const int w = (r - n_tri) / a.m.NFK, i = (r - n_tri) % a.m.NFK;
    const int k = a.l.walk_kf[w];
    int p = -1;
    if (ma_kf_ok(a, k) && a.walkrank[k] == w) {
      const size_t s = (size_t)k * a.m.NFK + i;
      const int t = a.slotw[s];
      p = t >= 0 ? a.l.att_mp[t] : a.m.kf_mp[s];
      if (!ma_mp_ok(a, p, NMP2)) p = -1;
    }
    a.req_mp[r] = p;
    if (p >= 0) h_insert(a, p, k, r);
  }
}

__global__ __launch_bounds__(T_MG) void k_ma_resolve(AddArgs a) {
  const int n_tri = a.sizes[1], n_req = a.sizes[3];
  for (int r = blockIdx.x * T_MG + threadIdx.x; r < n_req; r += gridDim.x * T_MG) {
    const int p = a.req_mp[r];
    int fl = 0;
    if (p >= 0) {
      int k, f;
      ma_request(a, r, n_tri, &k, &f);
      bool has = false;
      if (p < a.m.NMP) {
        int o0, o1;
        obs_range(a.m, p, &o0, &o1);
        for (int o = o0; o < o1; ++o) has = has || a.m.obs_kf[o] == k;
      }
      if (!has && h_first(a, p, k) == r) {
        fl = 1;
        atomicAdd(a.gcnt + p, 1);
        atomicAdd(a.out.result + 2, 1);
      } else if (r >= n_tri) {
        fl = 2;
      }
    }
    a.req_fl[r] = (uint8_t)fl;
  }
}

__global__ __launch_bounds__(T_MG) void k_ma_count(AddArgs a) {
  const int p = blockIdx.x * T_MG + threadIdx.x;
  if (p >= a.sizes[0]) return;
  int old = 0;
  if (p < a.m.NMP) {
    int o0, o1;
    obs_range(a.m, p, &o0, &o1);
    old = o1 - o0;
  }
  const int g = a.gcnt[p];
  a.gcnt[p] = 0;
  a.rb.cnt[p] = (u64)(unsigned)(old + g) | (u64)(unsigned)g << 32;
}

// the top of the scan, the sizes against the capacities, and already_mp: the walked slots whose point already observes, in request order
__global__ __launch_bounds__(SCAN_T) void k_ma_top(AddArgs a, int ntile_cap) {
  __shared__ u64 s_w[SCAN_T / 64];
  __shared__ int s_i[SCAN_T / 64];
  const int tid = threadIdx.x;
  const int NMP2 = a.sizes[0], n_tri = a.sizes[1], n_req = a.sizes[3];
  const int ntile = min((NMP2 + SCAN_TILE - 1) / SCAN_TILE, ntile_cap);
  const u64 total = tile_scan_top(a.rb.tile, ntile, s_w, tid);
  const int nobs = (int)(unsigned)(total & 0xffffffffull);
  int carry = 0;
  for (int r0 = n_tri; r0 < n_req; r0 += SCAN_T) {
    const int r = r0 + tid;
    const bool is = r < n_req && a.req_fl[r] == 2;
    int tot;
    const int at = carry + block_excl_scan<SCAN_T, int>(is ? 1 : 0, s_i, tid, &tot);
    if (is && at < a.out.already_cap) a.out.already_mp[at] = a.req_mp[r];
    carry += tot;
  }
  if (tid == 0) {
    int st = 0;
    if (NMP2 > a.NMPcap) st |= GL_MAP_GROW_MP_TRUNCATED;
    if (nobs > a.OBScap) st |= GL_MAP_GROW_OBS_TRUNCATED;
    if (carry > a.out.already_cap) st |= GL_MAP_ADD_ALREADY_TRUNCATED;
    a.rb.nptr[NMP2] = nobs;
    a.out.result[0] = NMP2;
    a.out.result[1] = nobs;
    a.out.result[4] = carry;
    a.out.result[5] = st;
  }
}

__global__ __launch_bounds__(T_MG) void k_ma_place(AddArgs a) {
  if (ma_truncated(a)) return;
  const int n_req = a.sizes[3];
  for (int r = blockIdx.x * T_MG + threadIdx.x; r < n_req; r += gridDim.x * T_MG) {
    if (a.req_fl[r] != 1) continue;
    const int p = a.req_mp[r];
    const int base = (int)(unsigned)(csr_place(a.rb, p) >> 32);
    a.seg[base + atomicAdd(a.gcnt + p, 1)] = r;  // (any order: k_ma_move sorts the point's requests)
  }
}

// the new rows, the new key-frames, the slots of the triples
__global__ __launch_bounds__(T_MG) void k_ma_rows(AddArgs a) {
  if (ma_truncated(a)) return;
  const int g = blockIdx.x * T_MG + threadIdx.x, G = gridDim.x * T_MG;
  const int NMP2 = a.sizes[0], n_tri = a.sizes[1];
  for (int i = g; i < NMP2 - a.m.NMP; i += G) {
    const int p = a.m.NMP + i;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.m.mp_pos[(size_t)p * 3 + c] = a.l.new_pos[(size_t)i * 3 + c];
    a.m.mp_assoc[p] = a.l.new_assoc[i];
    if (a.m.mp_ref_kf) a.m.mp_ref_kf[p] = a.l.new_ref_kf[i];
    a.m.mp_valid[p] = 1;
  }
  for (int k = g; k < a.m.NKF; k += G)
    if (a.kfnew[k]) a.m.kf_valid[k] = 1;
  for (int r = g; r < n_tri; r += G) {
    const int p = a.req_mp[r];
    if (p < 0) continue;
    const size_t s = (size_t)a.l.att_kf[r] * a.m.NFK + a.l.att_feat[r];
    if (a.slotw[s] == r) a.m.kf_mp[s] = p;
  }
}

__global__ __launch_bounds__(T_MG) void k_ma_move(AddArgs a) {
  if (ma_truncated(a)) return;
  const int p = blockIdx.x * T_MG + threadIdx.x;
  if (p >= a.sizes[0]) return;
  const int n_tri = a.sizes[1];
  const int base = (int)(unsigned)(csr_place(a.rb, p) >> 32), g = a.gcnt[p];
  for (int i = 1; i < g; ++i) {  // the point's requests in list order (its own segment: no other thread touches it)
    const int r = a.seg[base + i];
    int j = i;
    for (; j > 0 && a.seg[base + j - 1] > r; --j) a.seg[base + j] = a.seg[base + j - 1];
    a.seg[base + j] = r;
  }
  csr_move_point(
      a.m, a.rb, p, a.OBScap, a.out.obs_new_pos, [](int) { return true; },
      [&](auto& put) {
        for (int i = 0; i < g; ++i) {
          int k, f;
          ma_request(a, a.seg[base + i], n_tri, &k, &f);
          if (put(k, f) < 0) return;
        }
      });
}

__global__ __launch_bounds__(T_MG) void k_ma_ptr(AddArgs a) {
  if (ma_truncated(a)) return;
  const int NMP2 = a.sizes[0];
  for (int p = blockIdx.x * T_MG + threadIdx.x; p <= NMP2; p += gridDim.x * T_MG) a.m.obs_ptr[p] = a.rb.nptr[p];
}

// ---------------------------------------------------------------------------------------------------------------- gl_map_fuse
struct FuseArgs {
  Map m;
  int OBScap, kf, n_cand, log_cap;
  const int32_t *cand_mp, *best_idx;
  gl_map_fuse_out out;
  // scratch
  int32_t* pw;      // NMP: the weighted count the point holds now, -1 invalid
  int32_t* head;    // NMP: the chain of the point's gained entries, -1
  int32_t* tail;
  int32_t* stamp;   // NKF: the step in which the key-frame was last marked as an observer of the target
  uint8_t* oflag;   // NOBS: 1 the entry has left its point (gone, or moved into a chain)
  int32_t* lkf;     // the log: key-frame, feature, the old position it came from (-1: attached), the next of its chain
  int32_t* lfeat;
  int32_t* lfrom;
  int32_t* lnext;
  CsrRebuild rb;    // cnt: the entries the point holds after the walk
};

__global__ __launch_bounds__(T_MG) void k_mf_init(FuseArgs a) {
  const int p = blockIdx.x * T_MG + threadIdx.x;
  if (p >= a.m.NMP) return;
  int w = -1;
  if (a.m.mp_valid[p]) {
    int o0, o1;
    obs_range(a.m, p, &o0, &o1);
    w = 0;
    for (int o = o0; o < o1; ++o) w += obs_weight(a.m, a.m.obs_kf[o], a.m.obs_feat[o]);
  }
  a.pw[p] = w;
}

// the result of a call that is refused for its capacity: the size that is needed, the bit
__global__ void k_mf_refuse(int32_t* result, int need) {
  result[0] = need;
  result[4] = GL_MAP_GROW_OBS_TRUNCATED;
}

__global__ __launch_bounds__(T_MG) void k_mf_walk(FuseArgs a) {
  __shared__ int s_scan[T_MG / 64];
  __shared__ int s_w;
  const int tid = threadIdx.x;
  const int NMP = a.m.NMP, NKF = a.m.NKF, NFK = a.m.NFK, kf = a.kf;
  int nlog = 0, n_fused = 0, n_att = 0, n_repl = 0;  // (workgroup-uniform)
  for (int j = 0; j < a.n_cand; ++j) {
    const int c = a.cand_mp[j], bi = a.best_idx[j];
    if (c < 0 || c >= NMP || bi < 0 || bi >= NFK) continue;
    __syncthreads();  // (the step before is complete)
    if (a.pw[c] < 0) continue;  // (:237: invalid - on entry, or replaced by an earlier step)
    int32_t* const slot = a.m.kf_mp + (size_t)kf * NFK + bi;
    const int q = *slot;  // (read HERE by every thread: the barrier below lies between this read and the step's writes to kf_mp)
    {                     // (:237: checkObservation(kf) on the entries it holds now)
      int o0, o1;
      obs_range(a.m, c, &o0, &o1);
      int hit = 0;
      for (int o = o0 + tid; o < o1; o += T_MG) hit |= !a.oflag[o] && a.m.obs_kf[o] == kf;
      if (tid == 0) {
        int e = a.head[c];
        for (int n = 0; e >= 0 && n < a.log_cap; ++n, e = a.lnext[e]) hit |= a.lkf[e] == kf;
      }
      if (__syncthreads_or(hit)) continue;
    }
    ++n_fused;  // (:320)
    if (q < 0) {  // (:315-316)
      if (tid == 0) {
        const int e = nlog, t = a.tail[c];
        a.lkf[e] = kf;
        a.lfeat[e] = bi;
        a.lfrom[e] = -1;
        a.lnext[e] = -1;
        if (t >= 0) a.lnext[t] = e;
        else a.head[c] = e;
        a.tail[c] = e;
        a.pw[c] += obs_weight(a.m, kf, bi);
        *slot = c;
      }
      ++nlog;
      ++n_att;
      continue;
    }
    if (q >= NMP || q == c) continue;  // (a row outside the table is no point; map.cpp:113)
    const int wq = a.pw[q], wc = a.pw[c];
    if (wq < 0) continue;  // (:303)
    const int src = wq > wc ? c : q, tgt = wq > wc ? q : c;  // (:305-313)
    const int step = j + 1;
    int o0, o1;
    obs_range(a.m, tgt, &o0, &o1);
    for (int o = o0 + tid; o < o1; o += T_MG) {
      const int k = a.m.obs_kf[o];
      if (!a.oflag[o] && k >= 0 && k < NKF) a.stamp[k] = step;
    }
    if (tid == 0) {
      s_w = 0;
      int e = a.head[tgt];
      for (int n = 0; e >= 0 && n < a.log_cap; ++n, e = a.lnext[e]) a.stamp[a.lkf[e]] = step;
    }
    __syncthreads();
    // src's entries in its CSR order (map.cpp:127-140): the old ones here, a place in the log for each that moves
    obs_range(a.m, src, &o0, &o1);
    const int first = nlog;
    int wsum = 0;
    for (int base = o0; base < o1; base += T_MG) {
      const int o = base + tid;
      const bool live = o < o1 && !a.oflag[o];
      const int k = live ? a.m.obs_kf[o] : -1, f = live ? a.m.obs_feat[o] : -1;
      const bool inr = live && k >= 0 && k < NKF && f >= 0 && f < NFK;
      const bool mv = inr && a.stamp[k] != step;
      int tot;
      const int at = block_excl_scan<T_MG, int>(mv ? 1 : 0, s_scan, tid, &tot);
      if (live) a.oflag[o] = 1;
      if (inr) a.m.kf_mp[(size_t)k * NFK + f] = mv ? tgt : -1;  // (replaceObservation :134 / removeObservation :138)
      if (mv) {
        const int e = nlog + at;
        a.lkf[e] = k;
        a.lfeat[e] = f;
        a.lfrom[e] = o;
        a.lnext[e] = e + 1;
        wsum += obs_weight(a.m, k, f);
      }
      nlog += tot;
    }
    if (wsum) atomicAdd(&s_w, wsum);
    __syncthreads();
    if (tid == 0) {
      int t = a.tail[tgt];
      if (nlog > first) {
        a.lnext[nlog - 1] = -1;
        if (t >= 0) a.lnext[t] = first;
        else a.head[tgt] = first;
        t = nlog - 1;
      }
      int w = s_w;
      int e = a.head[src];  // ... then the entries src gained itself
      for (int n = 0; e >= 0 && n < a.log_cap; ++n) {
        const int nx = a.lnext[e], k = a.lkf[e], f = a.lfeat[e];
        int32_t* const s = a.m.kf_mp + (size_t)k * NFK + f;
        if (a.stamp[k] != step) {
          *s = tgt;
          a.lnext[e] = -1;
          if (t >= 0) a.lnext[t] = e;
          else a.head[tgt] = e;
          t = e;
          w += obs_weight(a.m, k, f);
        } else {
          *s = -1;
        }
        e = nx;
      }
      a.tail[tgt] = t;
      a.head[src] = a.tail[src] = -1;
      a.pw[tgt] += w;
      a.pw[src] = -1;
      if (n_repl < a.out.repl_cap) {
        a.out.repl_src[n_repl] = src;
        a.out.repl_tgt[n_repl] = tgt;
      }
    }
    ++n_repl;
  }
  if (tid == 0) {
    a.out.result[1] = n_fused;
    a.out.result[2] = n_att;
    a.out.result[3] = n_repl;
    a.out.result[4] = n_repl > a.out.repl_cap ? GL_MAP_FUSE_REPL_TRUNCATED : 0;
  }
}

__global__ __launch_bounds__(T_MG) void k_mf_count(FuseArgs a) {
  const int p = blockIdx.x * T_MG + threadIdx.x;
  if (p >= a.m.NMP) return;
  if (a.pw[p] < 0 && a.m.mp_valid[p]) a.m.mp_valid[p] = 0;  // (map.cpp:121)
  int o0, o1, n = 0;
  obs_range(a.m, p, &o0, &o1);
  for (int o = o0; o < o1; ++o) n += !a.oflag[o];
  int e = a.head[p];
  for (int i = 0; e >= 0 && i < a.log_cap; ++i, e = a.lnext[e]) ++n;
  a.rb.cnt[p] = (u64)n;
}

__global__ __launch_bounds__(SCAN_T) void k_mf_top(FuseArgs a, int ntile) {
  __shared__ u64 s_w[SCAN_T / 64];
  const u64 total = tile_scan_top(a.rb.tile, ntile, s_w, threadIdx.x);
  if (threadIdx.x == 0) {
    a.rb.nptr[a.m.NMP] = (int)total;
    a.out.result[0] = (int)total;
  }
}

__global__ __launch_bounds__(T_MG) void k_mf_move(FuseArgs a) {
  const int p = blockIdx.x * T_MG + threadIdx.x;
  if (p >= a.m.NMP) return;
  csr_move_point(
      a.m, a.rb, p, a.OBScap, a.out.obs_new_pos, [&](int o) { return !a.oflag[o]; },
      [&](auto& put) {  // the chain of the entries it gained, in step order
        int e = a.head[p];
        for (int i = 0; e >= 0 && i < a.log_cap; ++i, e = a.lnext[e]) {
          const int at = put(a.lkf[e], a.lfeat[e]);
          if (at < 0) return;
          if (a.out.obs_new_pos && a.lfrom[e] >= 0) a.out.obs_new_pos[a.lfrom[e]] = at;
        }
      });
}

inline int grid_of(int n, int cap = 1024) { return std::max(1, std::min((n + T_MG - 1) / T_MG, cap)); }

}  // namespace

extern "C" int gl_map_add(gl_ctx_t* ctx, int NMP, int NKF, int NFK, int NOBS, int NMPcap, int OBScap, const gl_map_edit* ed, double* mp_pos_dev,
                          int32_t* mp_assoc_dev, const gl_map_add_lists* lists, const gl_map_add_out* out) {
  GL_REQUIRE(ctx && ed && lists && out, "null argument");
  AddArgs a = {};
  const int rc = map_from_edit(__func__, NMP, NKF, NFK, NOBS, ed, nullptr, -1, &a.m);
  if (rc != GL_OK) return rc;
  GL_REQUIRE(NMPcap >= NMP && OBScap >= NOBS, "a capacity below the size");
  GL_REQUIRE(NMPcap == 0 || ed->mp_valid, "null mp_valid");
  GL_REQUIRE(NKF == 0 || ed->kf_valid, "null kf_valid");
  GL_REQUIRE(OBScap == 0 || (ed->obs_kf && ed->obs_feat), "null obs_kf / obs_feat");
  GL_REQUIRE(lists->new_mp_cap >= 0 && lists->new_kf_cap >= 0 && lists->attach_cap >= 0 && lists->walk_cap >= 0, "bad list capacity");
  GL_REQUIRE(out->result, "null result");
  GL_REQUIRE(out->already_cap >= 0 && (out->already_cap == 0 || out->already_mp), "bad already_cap / null already_mp");
  a.l = *lists;
  if (!a.l.new_pos || a.l.new_mp_cap == 0) a.l.new_pos = nullptr, a.l.new_mp_cap = 0;
  if (!a.l.new_kf || a.l.new_kf_cap == 0) a.l.new_kf = nullptr, a.l.new_kf_cap = 0;
  if (!a.l.att_mp || a.l.attach_cap == 0) a.l.att_mp = nullptr, a.l.attach_cap = 0;
  if (!a.l.walk_kf || a.l.walk_cap == 0) a.l.walk_kf = nullptr, a.l.walk_cap = 0;
  GL_REQUIRE(!a.l.new_pos || (a.l.new_assoc && mp_pos_dev && mp_assoc_dev && (a.l.new_ref_kf || !ed->mp_ref_kf)), "new points without assoc / ref_kf / mp_pos / mp_assoc");
  GL_REQUIRE(!a.l.att_mp || (a.l.att_kf && a.l.att_feat), "null att_kf / att_feat");
  const int64_t n_req = (int64_t)a.l.attach_cap + (int64_t)a.l.walk_cap * NFK, NMPx64 = (int64_t)NMP + a.l.new_mp_cap;
  GL_REQUIRE(n_req < ((int64_t)1 << 29) && NMPx64 < ((int64_t)1 << 31) - 1, "lists too long");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  a.NMPcap = NMPcap, a.OBScap = OBScap;
  a.m.mp_pos = mp_pos_dev;
  a.m.mp_assoc = mp_assoc_dev;
  a.out = *out;
  const int R = (int)n_req, NMPx = (int)NMPx64;
  size_t H = 64;
  while (H < 2 * (size_t)R) H <<= 1;
  a.hmask = (unsigned)(H - 1);
  const int ntile = csr_tiles(NMPx);
  const size_t nslot = (size_t)NKF * NFK;
  gl::Regions r = {0};
  // the regions one memset resets lie next to each other: 0x00, then 0x7f, then 0xff
  const size_t o_kfnew = r.take((size_t)NKF), o_gcnt = r.take((size_t)NMPx * 4), zero_end = r.off;
  const size_t o_rank = r.take((size_t)NKF * 4), o_hval = r.take(H * 4), r7f_end = r.off;
  const size_t o_slotw = r.take(nslot * 4), o_hkey = r.take(H * 8), ff_end = r.off;
  const size_t o_sizes = r.take(16), o_rmp = r.take((size_t)R * 4), o_rfl = r.take((size_t)R), o_seg = r.take((size_t)R * 4), o_csr = r.off;
  void* scratch = nullptr;
  const int rs = gl::ctx_scratch(c, o_csr + csr_rebuild_place(nullptr, NMPx, NOBS, nullptr), &scratch, gl::SCRATCH_MAPEDIT);
  if (rs != GL_OK) return rs;
  char* s = (char*)scratch;
  a.kfnew = (uint8_t*)(s + o_kfnew);
  a.gcnt = (int32_t*)(s + o_gcnt);
  a.walkrank = (int32_t*)(s + o_rank);
  a.hval = (int32_t*)(s + o_hval);
  a.slotw = (int32_t*)(s + o_slotw);
  a.hkey = (u64*)(s + o_hkey);
  a.sizes = (int32_t*)(s + o_sizes);
  a.req_mp = (int32_t*)(s + o_rmp);
  a.req_fl = (uint8_t*)(s + o_rfl);
  a.seg = (int32_t*)(s + o_seg);
  csr_rebuild_place(s + o_csr, NMPx, NOBS, &a.rb);
  GL_HIP(hipMemsetAsync(out->result, 0, 6 * sizeof(int32_t), c->stream));
  GL_HIP(hipMemsetAsync(s + o_kfnew, 0, zero_end - o_kfnew, c->stream));
  GL_HIP(hipMemsetAsync(s + o_rank, 0x7f, r7f_end - o_rank, c->stream));
  GL_HIP(hipMemsetAsync(s + o_slotw, 0xff, ff_end - o_slotw, c->stream));
  const int rb = csr_rebuild_begin(c, a.rb, a.m, out->obs_new_pos);
  if (rb != GL_OK) return rb;
  const int nwalk_req = R - a.l.attach_cap;
  k_ma_mark<<<grid_of(std::max(a.l.new_kf_cap, a.l.walk_cap)), T_MG, 0, c->stream>>>(a);
  if (a.l.attach_cap > 0) k_ma_triples<<<grid_of(a.l.attach_cap), T_MG, 0, c->stream>>>(a);
  if (nwalk_req > 0) k_ma_walks<<<grid_of(nwalk_req), T_MG, 0, c->stream>>>(a);
  if (R > 0) k_ma_resolve<<<grid_of(R), T_MG, 0, c->stream>>>(a);
  if (NMPx > 0) k_ma_count<<<(NMPx + T_MG - 1) / T_MG, T_MG, 0, c->stream>>>(a);
  csr_rebuild_scan(c, a.rb, ntile, a.sizes, 0);
  k_ma_top<<<1, SCAN_T, 0, c->stream>>>(a, ntile);
  if (R > 0) k_ma_place<<<grid_of(R), T_MG, 0, c->stream>>>(a);
  k_ma_rows<<<grid_of(std::max(std::max(a.l.new_mp_cap, NKF), a.l.attach_cap)), T_MG, 0, c->stream>>>(a);
  if (NMPx > 0) k_ma_move<<<(NMPx + T_MG - 1) / T_MG, T_MG, 0, c->stream>>>(a);
  k_ma_ptr<<<grid_of(NMPx + 1), T_MG, 0, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_map_fuse(gl_ctx_t* ctx, int NMP, int NKF, int NFK, int NOBS, int OBScap, const gl_map_edit* ed, const double* kf_uvr_dev, int kf,
                           int n_cand, const int32_t* cand_mp_dev, const int32_t* best_idx_dev, const gl_map_fuse_out* out) {
  GL_REQUIRE(ctx && ed && out, "null argument");
  FuseArgs a = {};
  const int rc = map_from_edit(__func__, NMP, NKF, NFK, NOBS, ed, kf_uvr_dev, -1, &a.m);
  if (rc != GL_OK) return rc;
  GL_REQUIRE(n_cand >= 0, "bad n_cand");
  GL_REQUIRE(OBScap >= NOBS, "a capacity below the size");
  GL_REQUIRE((int64_t)NOBS + n_cand < ((int64_t)1 << 31) - 1, "NOBS + n_cand must be below 2^31");
  GL_REQUIRE(kf >= 0 && kf < NKF, "kf outside the table");
  GL_REQUIRE(NFK == 0 || kf_uvr_dev, "null kf_uvr");
  GL_REQUIRE(OBScap == 0 || (ed->obs_kf && ed->obs_feat), "null obs_kf / obs_feat");
  GL_REQUIRE(n_cand == 0 || (cand_mp_dev && best_idx_dev), "null cand_mp / best_idx");
  GL_REQUIRE(out->result, "null result");
  GL_REQUIRE(out->repl_cap >= 0 && (out->repl_cap == 0 || (out->repl_src && out->repl_tgt)), "bad repl_cap / null repl_src / repl_tgt");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  GL_HIP(hipMemsetAsync(out->result, 0, 5 * sizeof(int32_t), c->stream));
  if ((int64_t)NOBS + n_cand > OBScap) {  // every candidate may attach: known before anything is written
    k_mf_refuse<<<1, 1, 0, c->stream>>>(out->result, NOBS + n_cand);
    GL_HIP(hipGetLastError());
    return GL_OK;
  }
  a.OBScap = OBScap, a.kf = kf, a.n_cand = n_cand, a.log_cap = NOBS + n_cand;
  a.cand_mp = cand_mp_dev;
  a.best_idx = best_idx_dev;
  a.out = *out;
  const int ntile = csr_tiles(NMP);
  const size_t L = (size_t)a.log_cap;
  gl::Regions r = {0};
  const size_t o_stamp = r.take((size_t)NKF * 4), o_oflag = r.take((size_t)NOBS), zero_end = r.off;
  const size_t o_head = r.take((size_t)NMP * 4), o_tail = r.take((size_t)NMP * 4), ff_end = r.off;
  const size_t o_pw = r.take((size_t)NMP * 4), o_lkf = r.take(L * 4), o_lfeat = r.take(L * 4), o_lfrom = r.take(L * 4), o_lnext = r.take(L * 4),
               o_csr = r.off;
  void* scratch = nullptr;
  const int rs = gl::ctx_scratch(c, o_csr + csr_rebuild_place(nullptr, NMP, NOBS, nullptr), &scratch, gl::SCRATCH_MAPEDIT);
  if (rs != GL_OK) return rs;
  char* s = (char*)scratch;
  a.stamp = (int32_t*)(s + o_stamp);
  a.oflag = (uint8_t*)(s + o_oflag);
  a.head = (int32_t*)(s + o_head);
  a.tail = (int32_t*)(s + o_tail);
  a.pw = (int32_t*)(s + o_pw);
  a.lkf = (int32_t*)(s + o_lkf);
  a.lfeat = (int32_t*)(s + o_lfeat);
  a.lfrom = (int32_t*)(s + o_lfrom);
  a.lnext = (int32_t*)(s + o_lnext);
  csr_rebuild_place(s + o_csr, NMP, NOBS, &a.rb);
  if (zero_end > o_stamp) GL_HIP(hipMemsetAsync(s + o_stamp, 0, zero_end - o_stamp, c->stream));
  if (ff_end > o_head) GL_HIP(hipMemsetAsync(s + o_head, 0xff, ff_end - o_head, c->stream));
  const int rb = csr_rebuild_begin(c, a.rb, a.m, out->obs_new_pos);
  if (rb != GL_OK) return rb;
  const int gp = (NMP + T_MG - 1) / T_MG;
  if (NMP > 0) k_mf_init<<<gp, T_MG, 0, c->stream>>>(a);
  k_mf_walk<<<1, T_MG, 0, c->stream>>>(a);
  if (NMP > 0) k_mf_count<<<gp, T_MG, 0, c->stream>>>(a);
  csr_rebuild_scan(c, a.rb, ntile, nullptr, NMP);
  k_mf_top<<<1, SCAN_T, 0, c->stream>>>(a, ntile);
  if (NMP > 0) k_mf_move<<<gp, T_MG, 0, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  GL_HIP(hipMemcpyAsync(ed->obs_ptr, a.rb.nptr, ((size_t)NMP + 1) * 4, hipMemcpyDeviceToDevice, c->stream));
  return GL_OK;
}
