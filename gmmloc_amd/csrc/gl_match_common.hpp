// What the matchers share (gl_match.hip, gl_match_tri.hip, gl_match_bow.hip, gl_match_fuse.hip): each block below is one statement
// about the reference (orb_matcher.cpp, frame.cpp, init_config.hpp) - visiting order, float / double conversions, tie rules - that
// the kernels' parity with it rests on.  What differs between the callers comes in as a callable or a template parameter (T: the
// threads of the workgroup); nothing here asks which kernel it is in.
#pragma once

#include <climits>

#include "gl_internal.hpp"

namespace gl_match {

// ---- host: launch parameters ------------------------------------------------------------------------------------------------
// frame::scale_factors / level_sigma2 / inv_level_sigma2 (init_config.hpp:63-79), float as there; null: a table the caller lacks
inline void pyramid_scales(float scale_factor, float* sf, float* sigma2, float* sigma2_inv) {
  float s = 1.0f;
  for (int i = 0; i < 8; ++i) {
    if (i > 0) s *= scale_factor;
    const float s2 = s * s;
    if (sf) sf[i] = s;
    if (sigma2) sigma2[i] = s2;
    if (sigma2_inv) sigma2_inv[i] = 1.0f / s2;
  }
}

// ---- ORBmatcher::DescriptorDistance (orb_matcher.cpp:580-596): 256-bit Hamming distance ------------------------------------------
__device__ __forceinline__ int hamming256(const uint32_t* a, const uint32_t* __restrict__ b) {
  int d = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) d += __popc(a[w] ^ b[w]);
  return d;
}
__device__ __forceinline__ int hamming256(const uint32_t dm[8], const uint4& b0, const uint4& b1) {
  return __popc(dm[0] ^ b0.x) + __popc(dm[1] ^ b0.y) + __popc(dm[2] ^ b0.z) + __popc(dm[3] ^ b0.w) + __popc(dm[4] ^ b1.x) +
         __popc(dm[5] ^ b1.y) + __popc(dm[6] ^ b1.z) + __popc(dm[7] ^ b1.w);
}
__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  const uint32_t a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  return hamming256(a, b0, b1);
}

// "keep the three smallest keys" (k0 <= k1 <= k2) of a walk
template <class K>
__device__ __forceinline__ void keep3(K& k0, K& k1, K& k2, const K kx) {
  if (kx < k2) {
    k2 = kx;
    if (k2 < k1) {
      const K t = k1;
      k1 = k2;
      k2 = t;
    }
    if (k1 < k0) {
      const K t = k0;
      k0 = k1;
      k1 = t;
    }
  }
}

// ---- the 64 x 48 bucket grid of a frame's features (Frame::assignFeaturesToGrid, frame.cpp:54-79) as a CSR in LDS ------------------
struct FeatureGrid {
  static constexpr int GC = 64, GR = 48, NCELL = GC * GR;  // frame::grid_cols / grid_rows (config.h:57)
  // 32-bit words of LDS: cell_ptr, cursor, cell_idx
  static __host__ __device__ constexpr int words(int NF) { return 2 * NCELL + 1 + NF; }
  // mGridElementWidthInv / mGridElementHeightInv (init_config.hpp:50-54, frame.cpp:33-34)
  static void scale(const gl_camera* cam, float* col_inv, float* row_inv) {
    *col_inv = static_cast<float>(GC) / cam->width;
    *row_inv = static_cast<float>(GR) / cam->height;
  }
  template <int T>
  struct Shared {  // the caller's __shared__ scratch of build()
    int scan[T / 64], fast;
  };
  struct Window {  // getFeaturesInArea's cell rectangle; x0 > x1: nothing to visit
    int x0 = 1, x1 = 0, y0 = 0, y1 = 0;
  };

  int32_t* cell_ptr;  // NCELL + 1: cell (ix * GR + iy) holds the entries cell_ptr[c] .. cell_ptr[c + 1]
  int32_t* cursor;    // NCELL (grid build only)
  int32_t* cell_idx;  // NF: the entries' features, ascending inside a cell
  float col_inv, row_inv;

  __device__ __forceinline__ FeatureGrid(int32_t* lds, float col_inv_, float row_inv_)
      : cell_ptr(lds), cursor(lds + NCELL + 1), cell_idx(lds + 2 * NCELL + 1), col_inv(col_inv_), row_inv(row_inv_) {}

  __device__ __forceinline__ int cell_of(const double* __restrict__ feat_uv, const int32_t* __restrict__ feat_oct, int i) const {
    if (feat_oct[i] < 0) return -1;  // padding slot
    const double px = round((feat_uv[2 * i] - 0.0f) * col_inv), py = round((feat_uv[2 * i + 1] - 0.0f) * row_inv);
    if (!(px >= 0 && px < GC && py >= 0 && py < GR)) return -1;  // also rejects NaN
    return (int)px * GR + (int)py;
  }

  // CSR by cell, ascending feature index inside a cell.  s.fast afterwards: every gridded coordinate is a float value and no octave
  // is above max_oct (what a packed record / the level mask of the caller holds).  The 16-byte record walk is exact iff so: the
  // reference's (float)(double u - (double)x) is then the correctly rounded float difference, which is what u - x in float is (a
  // double has more than 2 x 24 + 2 bits), and (double)(float)u is u in its double expressions.
  template <int T>
  __device__ __forceinline__ void build(int tid, int NF, const double* __restrict__ feat_uv, const int32_t* __restrict__ feat_oct, int max_oct,
                                        Shared<T>& s) const {
    for (int c = tid; c <= NCELL; c += T) cell_ptr[c] = 0;
    if (tid == 0) s.fast = 1;
    __syncthreads();
    {
      bool fok = true;
      for (int i = tid; i < NF; i += T) {
        const int c = cell_of(feat_uv, feat_oct, i);
        if (c >= 0) {
          atomicAdd(&cell_ptr[c + 1], 1);
          const double u = feat_uv[2 * i], v = feat_uv[2 * i + 1];
          fok = fok && (double)(float)u == u && (double)(float)v == v && feat_oct[i] <= max_oct;
        }
      }
      if (!fok) s.fast = 0;
    }
    __syncthreads();
    {  // exclusive scan of NCELL counts: each thread scans a contiguous chunk, then the chunk sums
      constexpr int CH = (NCELL + T - 1) / T;
      const int c0 = tid * CH, c1 = min(NCELL, c0 + CH);
      int sum = 0;
      for (int c = c0; c < c1; ++c) sum += cell_ptr[c + 1];
      // exclusive scan of the T chunk sums: shuffle scan inside each wave, then the wave totals
      int inc = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if ((tid & 63) >= o) inc += up;
      }
      if ((tid & 63) == 63) s.scan[tid >> 6] = inc;
      __syncthreads();
      int run = inc - sum;
      for (int w = 0; w < (tid >> 6); ++w) run += s.scan[w];
      // No hazard asks for a barrier here (nothing below writes s.scan); the clock does, for the 16 waves of T = 1024 only: one frame's
      // searchByProjection takes 0.8 us (1.7 %) longer without it, one key-frame's fuse search (T = 512) 0.2 us longer with it
      // (profiles/r10_match_refactor_ab.txt).
      if (T > 512) __syncthreads();
      for (int c = c0; c < c1; ++c) {
        const int v = cell_ptr[c + 1];
        cell_ptr[c + 1] = run + v;  // inclusive end; cell_ptr[c] (= end of c-1) is its start
        run += v;
      }
      __syncthreads();
    }
    // fill through a per-cell cursor, then put every (short) cell list in ascending feature order: that
    // is the push_back order of the reference and decides ties between equal Hamming distances
    for (int c = tid; c < NCELL; c += T) cursor[c] = 0;
    __syncthreads();
    for (int i = tid; i < NF; i += T) {
      const int c = cell_of(feat_uv, feat_oct, i);
      if (c >= 0) cell_idx[cell_ptr[c] + atomicAdd(&cursor[c], 1)] = i;
    }
    __syncthreads();
    for (int c = tid; c < NCELL; c += T) {
      const int e0 = cell_ptr[c], e1 = cell_ptr[c + 1];
      for (int e = e0 + 1; e < e1; ++e) {  // insertion sort
        const int v = cell_idx[e];
        int k = e - 1;
        while (k >= e0 && cell_idx[k] > v) {
          cell_idx[k + 1] = cell_idx[k];
          --k;
        }
        cell_idx[k + 1] = v;
      }
    }
    __syncthreads();
  }
  __device__ __forceinline__ int entries() const { return cell_ptr[NCELL]; }

  // the 16-byte record of a CSR entry: {u, v, u_right, octave | feature << 8}
  static __device__ __forceinline__ int pack(int octave, int feature) { return (octave & 0xff) | (feature << 8); }
  static __device__ __forceinline__ int octave_of(int packed) { return packed & 0xff; }
  static __device__ __forceinline__ int feature_of(int packed) { return packed >> 8; }
  static __device__ __forceinline__ float4 record(const double* __restrict__ feat_uv, const float* __restrict__ feat_ur,
                                                  const int32_t* __restrict__ feat_oct, int i) {
    return make_float4((float)feat_uv[2 * i], (float)feat_uv[2 * i + 1], feat_ur[i], __int_as_float(pack(feat_oct[i], i)));
  }

  // Frame::getFeaturesInArea (frame.cpp:121-177): the cells a window of half size rr around (x, y) covers (float, as the reference
  // passes them); column ix's cells (ix, y0 .. y1) are contiguous in the CSR
  __device__ __forceinline__ Window window(float x, float y, float rr) const {
    Window w;
    w.x0 = max(0, (int)floorf((x - 0.0f - rr) * col_inv));
    w.x1 = min(GC - 1, (int)ceilf((x - 0.0f + rr) * col_inv));
    w.y0 = max(0, (int)floorf((y - 0.0f - rr) * row_inv));
    w.y1 = min(GR - 1, (int)ceilf((y - 0.0f + rr) * row_inv));
    if (!(w.x0 < GC && w.x1 >= 0 && w.y0 < GR && w.y1 >= 0) || w.y0 > w.y1) w.x1 = w.x0 - 1;  // nothing to visit
    return w;
  }
};

// The record walk of a window, all lanes of a wave together (the loop and the flushes are wave-uniform): entry(record, e) tests an
// entry and puts a survivor on the caller's list of candidates, whose length is cnt; flush() evaluates and empties a list of four.
// The caller flushes what is left at the end.  each_iteration(): a caller's profile may count the iterations (a counter kept here
// costs a register even when nobody reads it).
// The loop is a chain of LDS round trips, not of instructions (profiles/r6_match_walk_ab.txt: a walk costs its dependent iterations
// whatever the number of lanes that make it) - a column's range, then an entry, then what the entry leads to, one after the other.  So an iteration waits ONCE: the
// NEXT column's range is requested a column ahead, two entries are read per iteration, and whatever else a candidate needs (owner,
// descriptor) is requested in the flush, for the (<= 4) candidates together.
struct Nothing {
  __device__ __forceinline__ void operator()() const {}
};
template <class Entry, class Flush, class Each = Nothing>
__device__ __forceinline__ void walk_window_records(const FeatureGrid& g, const float4* rec16, const FeatureGrid::Window& w, bool active,
                                                    const int& cnt, Entry entry, Flush flush, Each each_iteration = Each()) {
  constexpr int GR = FeatureGrid::GR;
  bool more = active && w.x0 <= w.x1;
  int ix = w.x0 - 1, e = 0, e1 = 0;
  int ne = 0, ne1 = 0;  // the range of column ix + 1
  if (more) {
    ne = g.cell_ptr[w.x0 * GR + w.y0];
    ne1 = g.cell_ptr[w.x0 * GR + w.y1 + 1];
  }
  while (__any(more)) {
    if (more && e >= e1) {  // next column
      ++ix;
      if (ix > w.x1) {
        more = false;
      } else {
        e = ne;
        e1 = ne1;
        if (ix < w.x1) {
          ne = g.cell_ptr[(ix + 1) * GR + w.y0];
          ne1 = g.cell_ptr[(ix + 1) * GR + w.y1 + 1];
        }
      }
    }
    const bool h0 = more && e < e1, h1 = more && e + 1 < e1;
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
    if (h0) r0 = rec16[e];
    if (h1) r1 = rec16[e + 1];
    if (h0) entry(r0, e);
    if (__any(cnt == 4)) flush();
    if (h1) entry(r1, e + 1);
    if (__any(cnt == 4)) flush();
    e += h1 ? 2 : (h0 ? 1 : 0);
    each_iteration();
  }
}

// Queries by window class (the half size of a window is a factor x the scale of a pyramid level), so that the lanes of a wave walk
// windows of like size: counting sort over the NCLS classes in the given order - the LARGEST windows first (they set the pace of a
// wave), the invalid queries last -, stable within a class up to the order of the atomics (the order only decides which thread takes
// which query - never a result).  s_cls: NCLS ints.
template <int T, int NCLS, class ClsOf>
__device__ __forceinline__ void sort_queries_by_class(int tid, int NP, const int (&order)[NCLS], ClsOf cls_of, int* s_cls, uint16_t* qorder) {
  if (tid < NCLS) s_cls[tid] = 0;
  __syncthreads();
  for (int m = tid; m < NP; m += T) atomicAdd(&s_cls[cls_of(m)], 1);
  __syncthreads();
  if (tid == 0) {  // exclusive scan
    int run = 0;
    for (int k = 0; k < NCLS; ++k) {
      const int n = s_cls[order[k]];
      s_cls[order[k]] = run;
      run += n;
    }
  }
  __syncthreads();
  for (int m = tid; m < NP; m += T) qorder[atomicAdd(&s_cls[cls_of(m)], 1)] = (uint16_t)m;
  __syncthreads();
}

// ---- queries by vocabulary node (searchForTriangulation, searchByBoW) ------------------------------------------------------------
// The DBoW2 feature vectors of two key-frames as CSR (node ids ascending, node_ptr, node_idx in list order).  Query a = list entry a of
// key-frame 1 (the order the reference visits them in: std::map iterates node ids ascending, the lists are in push order); its
// partners are the list of the same node in key-frame 2.

// largest i with ptr[i] <= a  (the node of list entry a)
__device__ __forceinline__ int node_of(const int32_t* __restrict__ ptr, int nn, int a) {
  int lo = 0, hi = nn;  // ptr[lo] <= a < ptr[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= a) lo = mid;
    else hi = mid;
  }
  return lo;
}

// p + at x stride.  A member nobody reads is null: it stays so on the host; a kernel does not pay a select per pointer for a value it
// never uses (k_search_for_triangulation: two spilled scalar registers).
template <class V>
__host__ __device__ __forceinline__ const V* pair_row(const V* p, size_t at, size_t stride) {
#ifdef __HIP_DEVICE_COMPILE__
  return p + at * stride;
#else
  return p ? p + at * stride : p;
#endif
}

// One side's feature vector for B pairs, N features and NN node slots a pair
struct NodeList {
  const int32_t* nnode;     // B
  const int32_t* node_id;   // B x NN, ascending
  const int32_t* node_ptr;  // B x (NN + 1)
  const int32_t* node_idx;  // B x N, list order
  int N, NN;
};

// What a node matcher reads of one key-frame (or frame) of B pairs.  A matcher that does not read a member leaves it null.
struct KfSide {
  const double* uv;       // B x N x 2
  const float* ur;        // B x N
  const int32_t* oct;     // B x N
  const float* angle;     // B x N
  const uint8_t* desc;    // B x N x 32
  const uint8_t* has_mp;  // B x N
  NodeList nodes;         // (its N, NN are the side's)
  // the side of pair f alone: THE place a side's strides are applied
  __host__ __device__ __forceinline__ KfSide pair(int f) const {
    const size_t N = (size_t)nodes.N, NN = (size_t)nodes.NN;
    return KfSide{pair_row(uv, f, 2 * N),    pair_row(ur, f, N),   pair_row(oct, f, N), pair_row(angle, f, N),
                  pair_row(desc, f, 32 * N), pair_row(has_mp, f, N),
                  NodeList{pair_row(nodes.nnode, f, 1), pair_row(nodes.node_id, f, NN), pair_row(nodes.node_ptr, f, NN + 1),
                           pair_row(nodes.node_idx, f, N), nodes.N, nodes.NN}};
  }
};

struct NodeQueries {
  static __host__ __device__ constexpr size_t words(int N1, int NN1, int NN2) { return 3 * (size_t)N1 + (size_t)NN1 + 2 * (size_t)NN2 + 2; }
  // LDS of a whole node matcher in bytes: owner, owner_n (N2 each), choice (N1), then the tables below
  static constexpr size_t matcher_lds(int N1, int N2, int NN1, int NN2) { return (2 * (size_t)N2 + (size_t)N1 + words(N1, NN1, NN2)) * sizeof(int32_t); }

  int32_t* q_idx1;  // N1: the query's feature of key-frame 1, or -1 (not a query: not eligible, node not shared)
  int32_t* q_lo;    // N1: its partners = node_idx2[q_lo .. q_hi)
  int32_t* q_hi;
  // the three tables the queries are set up from (two binary searches per query: sixteen dependent GLOBAL loads each otherwise)
  int32_t* s_nptr1;  // NN1 + 1
  int32_t* s_nid2;   // NN2
  int32_t* s_nptr2;  // NN2 + 1

  __device__ __forceinline__ NodeQueries(int32_t* lds, int N1, int NN1, int NN2)
      : q_idx1(lds), q_lo(lds + N1), q_hi(lds + 2 * N1), s_nptr1(lds + 3 * N1), s_nid2(s_nptr1 + NN1 + 1), s_nptr2(s_nid2 + NN2) {}

  // l1, l2: the two lists of ONE pair.  eligible(i1): may feature i1 of key-frame 1 ask at all.  Returns the number of queries; they
  // are written by then, a barrier of the caller makes them visible.
  template <int T, class Eligible>
  __device__ __forceinline__ int setup(int tid, const NodeList& l1, const NodeList& l2, Eligible eligible) const {
    const int N1 = l1.N, N2 = l2.N, nn1 = min(*l1.nnode, l1.NN), nn2 = min(*l2.nnode, l2.NN);
    const int nq = nn1 > 0 ? min(l1.node_ptr[nn1], N1) : 0;  // list entries of key-frame 1
    for (int i = tid; i <= nn1; i += T) s_nptr1[i] = l1.node_ptr[i];
    for (int i = tid; i <= nn2; i += T) {
      s_nptr2[i] = l2.node_ptr[i];
      if (i < nn2) s_nid2[i] = l2.node_id[i];
    }
    __syncthreads();
    for (int a = tid; a < N1; a += T) {
      int idx1 = -1, lo = 0, hi = 0;
      if (a < nq) {
        const int n1 = node_of(s_nptr1, nn1, a);
        const int id = l1.node_id[n1];
        int l = 0, h = nn2;  // lower_bound of id in nid2
        while (l < h) {
          const int mid = (l + h) >> 1;
          if (s_nid2[mid] < id) l = mid + 1;
          else h = mid;
        }
        if (l < nn2 && s_nid2[l] == id) {
          const int i1 = l1.node_idx[a];
          if (i1 >= 0 && i1 < N1 && eligible(i1)) {
            idx1 = i1;
            lo = s_nptr2[l];
            hi = min(s_nptr2[l + 1], N2);
          }
        }
      }
      q_idx1[a] = idx1;
      q_lo[a] = lo;
      q_hi[a] = hi;
    }
    return nq;
  }
};

// ---- the owner fixed point ------------------------------------------------------------------------------------------------------
// The reference loops are ORDER DEPENDENT: what query m takes is skipped by every later query.  In every round each query picks among
// what no LOWER query owned in the previous round and claims it with atomicMin(&owner_n[pick], m); by induction the choices of the
// queries 0 .. r-1 are final after round r, and the iteration stops when the owner table repeats.  One round:
//     owner_round_begin  ... the queries ...  __syncthreads()  owner_round_end
// and, when that returns true and the round limit is not reached, a __syncthreads() before the next one.
// reset(i): owner_n[i] of a feature nobody has claimed yet (-1: not available at all, INT_MAX: free)
template <int T, class Reset>
__device__ __forceinline__ void owner_round_begin(int tid, int32_t* owner_n, int N, int* s_changed, Reset reset) {
  for (int i = tid; i < N; i += T) owner_n[i] = reset(i);
  if (tid == 0) *s_changed = 0;
  __syncthreads();
}
// owner <- owner_n; did any owner change
template <int T>
__device__ __forceinline__ bool owner_round_end(int tid, int32_t* owner, const int32_t* owner_n, int N, int* s_changed) {
  int ch = 0;
  for (int i = tid; i < N; i += T) {
    const int o = owner_n[i];
    if (o != owner[i]) ch = 1;
    owner[i] = o;
  }
  if (ch) *s_changed = 1;
  __syncthreads();
  return *s_changed != 0;
}

// ---- rotation consistency (computeThreeMaxima, orb_matcher.cpp:544-578) -------------------------------------------------------------
// Of the n matches i with valid(i), histogram rot_of(i) - the difference of the two key-points' angles - over 30 bins and drop(i) those
// outside the (up to) three fullest bins.  s_hist: 32 ints, s_keep: 3.  Ends with a barrier.
template <int T, class Valid, class RotOf, class Drop>
__device__ __forceinline__ void rotation_filter(int tid, int n, int* s_hist, int* s_keep, Valid valid, RotOf rot_of, Drop drop) {
  const float factor = 30 / 360.0f;
  auto bin_of = [&](int i) -> int {
    float rot = rot_of(i);
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == 30) bin = 0;
    return bin;
  };
  if (tid < 32) s_hist[tid] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += T)
    if (valid(i)) {
      const int b = bin_of(i);
      if (b >= 0 && b < 30) atomicAdd(&s_hist[b], 1);
    }
  __syncthreads();
  if (tid == 0) {
    int ind1 = -1, ind2 = -1, ind3 = -1, max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < 30; i++) {
      const int sz = s_hist[i];
      if (sz > max1) {
        max3 = max2;
        max2 = max1;
        max1 = sz;
        ind3 = ind2;
        ind2 = ind1;
        ind1 = i;
      } else if (sz > max2) {
        max3 = max2;
        max2 = sz;
        ind3 = ind2;
        ind2 = i;
      } else if (sz > max3) {
        max3 = sz;
        ind3 = i;
      }
    }
    if (max2 < 0.1f * (float)max1) {
      ind2 = -1;
      ind3 = -1;
    } else if (max3 < 0.1f * (float)max1) {
      ind3 = -1;
    }
    s_keep[0] = ind1;
    s_keep[1] = ind2;
    s_keep[2] = ind3;
  }
  __syncthreads();
  for (int i = tid; i < n; i += T)
    if (valid(i)) {
      const int b = bin_of(i);
      if (b >= 0 && b < 30 && b != s_keep[0] && b != s_keep[1] && b != s_keep[2]) drop(i);
    }
  __syncthreads();
}

// ---- the number of matches of the workgroup's unit (cnt: this thread's), and the counters ----------------------------------------
// s_cnt: T / 64 ints
template <int T>
__device__ __forceinline__ void count_matches(int tid, int cnt, int* s_cnt, int32_t* nmatches, int32_t* counters, int rounds) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int w = 0; w < T / 64; ++w) tot += s_cnt[w];
    *nmatches = tot;
    if (counters) {  // GL_COUNTER_MATCH_ROUNDS / _UNITS: rounds of the owner fixed point, units (frames, pairs)
      atomicAdd(&counters[1], rounds);
      atomicAdd(&counters[2], 1);
    }
  }
}

// ---- matches -> the per-match arrays of gl_create_map_points -----------------------------------------------------------------------
// What the triangulation reads of one key-frame of B pairs (N features, k candidate components a feature)
struct KfPointSide {
  const double* pose;    // B x 7
  const double* uv;      // B x N x 2
  const float* ur;       // B x N
  const float* depth;    // B x N
  const int32_t* oct;    // B x N
  const int32_t* cand;   // B x N x k
  const int32_t* ncand;  // B x N
  int N, k;
  __host__ __device__ __forceinline__ KfPointSide pair(int f) const {
    const size_t Nz = (size_t)N;
    return KfPointSide{pair_row(pose, f, 7),  pair_row(uv, f, 2 * Nz),   pair_row(ur, f, Nz),    pair_row(depth, f, Nz),
                       pair_row(oct, f, Nz), pair_row(cand, f, Nz * k), pair_row(ncand, f, Nz), N, k};
  }
};
// The per-match arrays of one side: a slot per match
struct MatchSide {
  double* pose;    // x 7
  double* uvr;     // x 3
  float* depth;
  int32_t* oct;
  int32_t* cand;   // x k
  int32_t* ncand;
};
// What gl_create_map_points leaves per match
struct MatchPoints {
  double* x3d;  // x 3
  int32_t* type;
  int32_t* comp;
};
// match (i, j) of pair f -> slot `at`: what Localization::createMapPoints reads per match (localization_opt.cpp:286-420)
__device__ __forceinline__ void gather_match(const KfPointSide& side1, const KfPointSide& side2, int f, int i, int j, const MatchSide& oa,
                                             const MatchSide& ob, int at) {
  const KfPointSide a = side1.pair(f), b = side2.pair(f);
  const int k = a.k;
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    oa.pose[(size_t)at * 7 + r] = a.pose[r];
    ob.pose[(size_t)at * 7 + r] = b.pose[r];
  }
  oa.uvr[(size_t)at * 3] = a.uv[(size_t)i * 2];
  oa.uvr[(size_t)at * 3 + 1] = a.uv[(size_t)i * 2 + 1];
  oa.uvr[(size_t)at * 3 + 2] = (double)a.ur[i];
  ob.uvr[(size_t)at * 3] = b.uv[(size_t)j * 2];
  ob.uvr[(size_t)at * 3 + 1] = b.uv[(size_t)j * 2 + 1];
  ob.uvr[(size_t)at * 3 + 2] = (double)b.ur[j];
  oa.depth[at] = a.depth[i];
  ob.depth[at] = b.depth[j];
  oa.oct[at] = a.oct[i];
  ob.oct[at] = b.oct[j];
  oa.ncand[at] = a.ncand[i];
  ob.ncand[at] = b.ncand[j];
  for (int c = 0; c < k; ++c) {
    oa.cand[(size_t)at * k + c] = a.cand[(size_t)i * k + c];
    ob.cand[(size_t)at * k + c] = b.cand[(size_t)j * k + c];
  }
}

}  // namespace gl_match
