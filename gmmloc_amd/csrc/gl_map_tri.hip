// Localization::createMapPoints (localization_opt.cpp:206-454) for ONE key-frame row of the resident map: the loop over its best
// covisible neighbours around the three per-pair pieces that exist already (gl_search_for_triangulation, the match gather, the per-match
// block of gl_create_map_points).  The loop is sequential because of one feedback: searchForTriangulation skips a feature of key-frame 1
// that holds a map point (orb_matcher.cpp:183-186) and createMapPoints gives it one (curr_kf_->addObservation(mappt, idx1), :433) before
// the next neighbour is searched.  That feedback is a byte per feature here (the mask), carried on the device from neighbour to
// neighbour; the host enqueues a fixed number of launches per neighbour whatever the device counts are and never reads anything back.
//   k_tri_pair_setup   a thread per neighbour: the skip bits (:254-262 and the list's own rules), computeFundamentalMatrix
//                      (math_utils.cpp:16-43) and the epipole (orb_matcher.cpp:156-161); expression order in gmmloc_hip.h
//   k_tri_rows         workgroup 0: key-frame 1's (u, v) / u_right tables, the mask from kf_mp[kf_row], feat_new, the counts;
//                      workgroup 1 + j: neighbour j's rows gathered into dense pair tables (a skipped neighbour: no vocabulary node)
//   per neighbour      k_search_for_triangulation (B = 1) -> k_tri_match_rows (the matches in ascending idx1 as the per-match arrays,
//                      the slots behind them as problems the create block leaves at once) -> k_tri_pre, k_optimize_triangulation,
//                      k_tri_post over NFK slots -> k_tri_accept (prefix scan over the matches: the lists of gl_map_add, the mask)
// 2 + 6 n_nb launches.  Integer stores and integer atomics only outside the three existing arithmetic kernels and the pair set-up, so
// the bytes do not depend on scheduling.  The file is compiled without contraction; the pair set-up uses + - x / (and one sqrt, the
// norm of the baseline) only.
#include "gl_device.hpp"
#include "gl_internal.hpp"
#include "gl_map_dev.hpp"  // block_excl_scan
#include "gl_match_common.hpp"

using namespace gld;
using namespace gl_match;  // KfSide, KfPointSide, MatchSide, MatchPoints, NodeList, gather_match

namespace {

typedef unsigned long long u64;
constexpr int ROW_T = 256;

struct PairK {
  double fx, fy, cx, cy;  // the camera's float scalars, widened (config.h)
};

// math_utils.cpp:16-43 in the order gmmloc_hip.h declares; F row-major
GL_DEV void fundamental(const PairK& k, const double* p1, const double* p2, double* F) {
  double R1[9], R2[9], R[9], r[3], E[9];
  qtoR(Quat{p1[0], p1[1], p1[2], p1[3]}, R1);
  qtoR(Quat{p2[0], p2[1], p2[2], p2[3]}, R2);
#pragma unroll
  for (int i = 0; i < 3; ++i) {  // rot_c1_w * rot_c2_w.conjugate() as R1 R2^T, then rot_c1_c2 * t_c2_w
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = (R1[i * 3] * R2[j * 3] + R1[i * 3 + 1] * R2[j * 3 + 1]) + R1[i * 3 + 2] * R2[j * 3 + 2];
    r[i] = (R[i * 3] * p2[4] + R[i * 3 + 1] * p2[5]) + R[i * 3 + 2] * p2[6];
  }
  const double tx = -r[0] + p1[4], ty = -r[1] + p1[5], tz = -r[2] + p1[6];  // -(rot_c1_c2 * t_c2_w) + t_c1_w
#pragma unroll
  for (int j = 0; j < 3; ++j) {  // skew(t12) * R, the zero products left out
    E[0 + j] = (-tz) * R[3 + j] + ty * R[6 + j];
    E[3 + j] = tz * R[0 + j] + (-tx) * R[6 + j];
    E[6 + j] = (-ty) * R[0 + j] + tx * R[3 + j];
  }
  // K^-1 = [1/fx 0 -cx/fx; 0 1/fy -cy/fy; 0 0 1] in closed form; G = E K^-1, F = K^-T G
  const double ifx = 1.0 / k.fx, ify = 1.0 / k.fy, mcx = -(k.cx / k.fx), mcy = -(k.cy / k.fy);
  double G[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    G[i * 3 + 0] = E[i * 3 + 0] * ifx;
    G[i * 3 + 1] = E[i * 3 + 1] * ify;
    G[i * 3 + 2] = (E[i * 3 + 0] * mcx + E[i * 3 + 1] * mcy) + E[i * 3 + 2];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    F[0 + j] = ifx * G[0 + j];
    F[3 + j] = ify * G[3 + j];
    F[6 + j] = (mcx * G[0 + j] + mcy * G[3 + j]) + G[6 + j];
  }
}

// orb_matcher.cpp:156-161: C2 = R2 t1 + t2 (Tcw1.translation(), not the camera centre: kept), invz in float
GL_DEV void epipole_of(const PairK& k, const double* p1, const double* p2, float* e) {
  const Quat q2 = Quat{p2[0], p2[1], p2[2], p2[3]};
  const double t1[3] = {p1[4], p1[5], p1[6]};
  double r[3];
  qrot(q2, t1, r);
  const double c0 = r[0] + p2[4], c1 = r[1] + p2[5], c2 = r[2] + p2[6];
  const float invz = 1.0f / (float)c2;
  e[0] = (float)((k.fx * c0) * (double)invz + k.cx);
  e[1] = (float)((k.fy * c1) * (double)invz + k.cy);
}

__global__ __launch_bounds__(64) void k_tri_pair_setup(PairK k, int NKF, const uint8_t* __restrict__ kf_valid, const double* __restrict__ kf_pose,
                                                       const double* __restrict__ kf_twc, int kf_row, const int32_t* __restrict__ conn_kf,
                                                       const int32_t* __restrict__ n_conn, int conn_cap, int first_nb, int n_nb, float mb,
                                                       int32_t* __restrict__ skip, int32_t* __restrict__ rows, double* __restrict__ fmat,
                                                       float* __restrict__ epipole, double* __restrict__ fmat_out, float* __restrict__ epipole_out) {
  const int j = threadIdx.x;
  if (j >= n_nb) return;
  const int len = min(max(*n_conn, 0), conn_cap);
  const int i = first_nb + j;
  int bits = 0, row = -1;
  if (i >= len) {
    bits = GL_TRI_SKIP_BEYOND;
  } else {
    row = conn_kf[i];
    if (row < 0 || row >= NKF) {
      bits = GL_TRI_SKIP_BAD_ROW;
    } else {
      if (row == kf_row) bits |= GL_TRI_SKIP_SELF;
      if (kf_valid && !kf_valid[row]) bits |= GL_TRI_SKIP_INVALID;
      for (int e = first_nb; e < i; ++e)
        if (conn_kf[e] == row) bits |= GL_TRI_SKIP_REPEATED;
      // :254-262: Vector3d difference, double norm, narrowed to float, float compare
      const double dx = kf_twc[(size_t)row * 3] - kf_twc[(size_t)kf_row * 3];
      const double dy = kf_twc[(size_t)row * 3 + 1] - kf_twc[(size_t)kf_row * 3 + 1];
      const double dz = kf_twc[(size_t)row * 3 + 2] - kf_twc[(size_t)kf_row * 3 + 2];
      const float baseline = (float)sqrt((dx * dx + dy * dy) + dz * dz);
      if (baseline < mb) bits |= GL_TRI_SKIP_BASELINE;
    }
  }
  double F[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  float e[2] = {0.0f, 0.0f};
  if (bits == 0) {
    const double* p1 = kf_pose + (size_t)kf_row * 7;
    const double* p2 = kf_pose + (size_t)row * 7;
    fundamental(k, p1, p2, F);
    epipole_of(k, p1, p2, e);
  }
  skip[j] = bits;
  if (rows) rows[j] = row;
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    fmat[(size_t)j * 9 + c] = F[c];
    if (fmat_out) fmat_out[(size_t)j * 9 + c] = F[c];
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    epipole[(size_t)j * 2 + c] = e[c];
    if (epipole_out) epipole_out[(size_t)j * 2 + c] = e[c];
  }
}

// The map's key-frame tables, a row per key-frame: a side of NKF "pairs", but for two tables the map keeps in a form of its own
struct KfTables {
  const double* kf_uvr;  // NKF x N x 3: (u, v, u_right) interleaved, all double
  const int32_t* kf_mp;  // NKF x N: a feature's map point (-1: none) where a side has a byte
  KfSide match;          // uv / ur / has_mp null
  KfPointSide point;     // uv / ur null
};
// (k_tri_rows is the one writer of key-frame 1's dense tables and of the pair tables, which everything after it reads as sides)
template <class V>
GL_DEV V* mut(const V* p) {
  return const_cast<V*>(p);
}

// side1 / point1: key-frame 1 (the map's row, dense uv / ur / mask); side2 / point2: the pair tables, neighbour j's at pair(j)
__global__ __launch_bounds__(ROW_T) void k_tri_rows(int kf_row, int n_nb, KfTables t, const int32_t* __restrict__ skip,
                                                    const int32_t* __restrict__ rows, KfSide side1, KfSide side2, KfPointSide point2,
                                                    int32_t* __restrict__ feat_new, int32_t* __restrict__ n_new, int32_t* __restrict__ n_attach,
                                                    int32_t* __restrict__ status) {
  const int tid = threadIdx.x, N = side2.nodes.N, NN = side2.nodes.NN, k = point2.k;
  if (blockIdx.x == 0) {
    const size_t f0 = (size_t)kf_row * N;
    for (int i = tid; i < N; i += ROW_T) {
      mut(side1.uv)[2 * i] = t.kf_uvr[(f0 + i) * 3];
      mut(side1.uv)[2 * i + 1] = t.kf_uvr[(f0 + i) * 3 + 1];
      mut(side1.ur)[i] = (float)t.kf_uvr[(f0 + i) * 3 + 2];
      mut(side1.has_mp)[i] = t.kf_mp[f0 + i] != -1 ? 1 : 0;  // getMapPoint(idx1) != nullptr: the pointer alone, whatever mp_valid says
      feat_new[i] = -1;
    }
    if (tid == 0) {
      *n_new = 0;
      *n_attach = 0;
      int searched = 0;
      for (int j = 0; j < n_nb; ++j) searched += skip[j] == 0 ? 1 : 0;
      *status = searched == 0 ? GL_TRI_NONE_SEARCHED : 0;
    }
    return;
  }
  const int j = blockIdx.x - 1;
  const KfSide d = side2.pair(j);
  if (skip[j] != 0) {  // no vocabulary node: the search finds no query, the stages behind it no match
    if (tid == 0) {
      mut(d.nodes.nnode)[0] = 0;
      mut(d.nodes.node_ptr)[0] = 0;
    }
    return;
  }
  const int row = rows[j];
  const size_t f0 = (size_t)row * N;
  const KfSide m = t.match.pair(row);
  const KfPointSide pm = t.point.pair(row), pd = point2.pair(j);
  for (int i = tid; i < N; i += ROW_T) {
    mut(d.uv)[i * 2] = t.kf_uvr[(f0 + i) * 3];
    mut(d.uv)[i * 2 + 1] = t.kf_uvr[(f0 + i) * 3 + 1];
    mut(d.ur)[i] = (float)t.kf_uvr[(f0 + i) * 3 + 2];
    mut(d.oct)[i] = m.oct[i];
    mut(d.angle)[i] = m.angle[i];
    mut(d.has_mp)[i] = t.kf_mp[f0 + i] != -1 ? 1 : 0;
    mut(pd.depth)[i] = pm.depth[i];
    mut(pd.ncand)[i] = pm.ncand[i];
    mut(d.nodes.node_idx)[i] = m.nodes.node_idx[i];
    for (int c = 0; c < k; ++c) mut(pd.cand)[(size_t)i * k + c] = pm.cand[(size_t)i * k + c];
  }
  const uint4* dsrc = (const uint4*)m.desc;
  uint4* ddst = (uint4*)mut(d.desc);
  for (int i = tid; i < 2 * N; i += ROW_T) ddst[i] = dsrc[i];
  for (int i = tid; i < NN; i += ROW_T) mut(d.nodes.node_id)[i] = m.nodes.node_id[i];
  for (int i = tid; i <= NN; i += ROW_T) mut(d.nodes.node_ptr)[i] = m.nodes.node_ptr[i];
  if (tid < 7) mut(pd.pose)[tid] = pm.pose[tid];
  if (tid == 0) mut(d.nodes.nnode)[0] = min(max(m.nodes.nnode[0], 0), NN);
}

// matches12 of ONE pair -> the per-match arrays in ascending feature index of key-frame 1 (= matched_pairs), as k_tri_gather makes
// them; a: key-frame 1, b: the pair's tables.  The slots behind the matches become problems the create block leaves at once: octave
// -1 (k_optimize_triangulation returns), identity poses and monocular key-points on the optical axis (k_tri_pre forms no point,
// k_tri_post writes type 0).
__global__ __launch_bounds__(ROW_T) void k_tri_match_rows(KfPointSide a, KfPointSide b, const int32_t* __restrict__ match, MatchSide oa,
                                                          MatchSide ob, int32_t* __restrict__ idx1, int32_t* __restrict__ idx2,
                                                          int32_t* __restrict__ count) {
  __shared__ int s_w[ROW_T / 64];
  const int tid = threadIdx.x, N = a.N, k = a.k;
  int run = 0;
  for (int i0 = 0; i0 < N; i0 += ROW_T) {
    const int i = i0 + tid;
    const int m2 = i < N ? match[i] : -1;
    const bool on = m2 >= 0 && m2 < N;
    int total;
    const int at = run + gl::mapdev::block_excl_scan<ROW_T, int>(on ? 1 : 0, s_w, tid, &total);
    run += total;
    if (on) {
      gather_match(a, b, 0, i, m2, oa, ob, at);
      idx1[at] = i;
      idx2[at] = m2;
    }
  }
  for (int at = run + tid; at < N; at += ROW_T) {
#pragma unroll
    for (int r = 0; r < 7; ++r) oa.pose[(size_t)at * 7 + r] = ob.pose[(size_t)at * 7 + r] = r == 3 ? 1.0 : 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) oa.uvr[(size_t)at * 3 + r] = ob.uvr[(size_t)at * 3 + r] = r == 2 ? -1.0 : 0.0;
    oa.depth[at] = ob.depth[at] = -1.0f;
    oa.oct[at] = ob.oct[at] = -1;
    oa.ncand[at] = ob.ncand[at] = 0;
    for (int c = 0; c < k; ++c) oa.cand[(size_t)at * k + c] = ob.cand[(size_t)at * k + c] = -1;
    idx1[at] = idx2[at] = -1;
  }
  if (tid == 0) *count = run;
}

struct AcceptOut {
  u64* new_pos;
  int32_t *new_assoc, *new_ref_kf, *new_type, *new_nb, *new_feat1, *new_feat2, *att_mp, *att_kf, *att_feat, *n_new, *n_attach, *feat_new,
      *nb_stats;
  int new_cap;
};

// What createMapPoints does with a match that passed (:406-446), over the matches in ascending idx1: the accepted ones are appended at
// the running count in that order; the feature of key-frame 1 now holds a point (:433), so it is no query at the next neighbour.  A
// rejected match (`continue`, :346-404) leaves the mask alone.
__global__ __launch_bounds__(ROW_T) void k_tri_accept(int N, int kf_row, int j, int nb_index, int mp_base, const int32_t* __restrict__ skip,
                                                      const int32_t* __restrict__ rows, const int32_t* __restrict__ nmatches,
                                                      const int32_t* __restrict__ count, const int32_t* __restrict__ idx1,
                                                      const int32_t* __restrict__ idx2, const u64* __restrict__ x3d,
                                                      const int32_t* __restrict__ type, const int32_t* __restrict__ comp,
                                                      uint8_t* __restrict__ mask, AcceptOut o) {
  __shared__ int s_w[ROW_T / 64];
  const int tid = threadIdx.x;
  const int cnt = min(max(*count, 0), N), base = *o.n_new, kf2 = rows[j];
  int run = 0;
  for (int m0 = 0; m0 < cnt; m0 += ROW_T) {
    const int m = m0 + tid;
    const int ty = m < cnt ? type[m] : 0;
    const bool on = ty > 0;
    int total;
    const int r = base + run + gl::mapdev::block_excl_scan<ROW_T, int>(on ? 1 : 0, s_w, tid, &total);
    run += total;
    if (on && r < o.new_cap) {
      const int i1 = idx1[m], i2 = idx2[m];
      for (int c = 0; c < 3; ++c) o.new_pos[(size_t)r * 3 + c] = x3d[(size_t)m * 3 + c];
      o.new_assoc[r] = comp[m];
      o.new_ref_kf[r] = kf_row;
      o.new_type[r] = ty;
      o.new_nb[r] = nb_index;
      o.new_feat1[r] = i1;
      o.new_feat2[r] = i2;
      o.att_mp[2 * r] = mp_base + r;
      o.att_kf[2 * r] = kf_row;
      o.att_feat[2 * r] = i1;
      o.att_mp[2 * r + 1] = mp_base + r;
      o.att_kf[2 * r + 1] = kf2;
      o.att_feat[2 * r + 1] = i2;
      mask[i1] = 1;
      o.feat_new[i1] = mp_base + r;
    }
  }
  if (tid == 0) {
    const int now = min(base + run, o.new_cap);
    *o.n_new = now;
    *o.n_attach = 2 * now;
    int32_t* st = o.nb_stats + (size_t)j * 8;
    st[0] = kf2;
    st[1] = skip[j];
    st[2] = nmatches[j];
    st[3] = run;
    st[4] = cnt - run;
    st[5] = 0;
    st[6] = 0;
    st[7] = 0;
  }
}

PairK make_pairk(const gl_camera* cam) {
  return PairK{(double)(float)cam->fx, (double)(float)cam->fy, (double)(float)cam->cx, (double)(float)cam->cy};
}

// per neighbour: what k_tri_pair_setup leaves, and the search's match count
struct PairWork {
  int32_t *skip, *rows;
  double* fmat;       // x 9
  float* epipole;     // x 2
  int32_t* nmatches;
  PairWork pair(int j) const { return PairWork{skip + j, rows + j, fmat + (size_t)j * 9, epipole + (size_t)j * 2, nmatches + j}; }
};

// The scratch of gl_create_map_points_from_map (SCRATCH_MAPTRI): the byte offset of each region, in the order of the stages
struct TriLayout {
  TriLayout(int n_nb, int N_, int NN_, int k_) : n((size_t)(n_nb > 0 ? n_nb : 1)), N((size_t)N_), NN((size_t)NN_), k((size_t)k_) {}
  const size_t n, N, NN, k;
  gl::Regions rg{0};
  const size_t skip = rg.take(n * 4), rows = rg.take(n * 4), fmat = rg.take(n * 72), epi = rg.take(n * 8), nm = rg.take(n * 4);  // PairWork
  const size_t uv1 = rg.take(N * 16), ur1 = rg.take(N * 4), mask = rg.take(N);  // key-frame 1, dense
  // the pair tables, n neighbours
  const size_t uv2 = rg.take(n * N * 16), ur2 = rg.take(n * N * 4), oct2 = rg.take(n * N * 4), ang2 = rg.take(n * N * 4),
               desc2 = rg.take(n * N * 32), mp2 = rg.take(n * N), dep2 = rg.take(n * N * 4), cand2 = rg.take(n * N * k * 4),
               nc2 = rg.take(n * N * 4), nn2 = rg.take(n * 4), nid2 = rg.take(n * NN * 4), nptr2 = rg.take(n * (NN + 1) * 4),
               nidx2 = rg.take(n * N * 4), pose2 = rg.take(n * 56);
  const size_t match = rg.take(N * 4);  // matches12 of the current pair
  // the per-match arrays, N slots
  const size_t m_pose1 = rg.take(N * 56), m_uvr1 = rg.take(N * 24), m_pose2 = rg.take(N * 56), m_uvr2 = rg.take(N * 24),
               m_dep1 = rg.take(N * 4), m_dep2 = rg.take(N * 4), m_oct1 = rg.take(N * 4), m_oct2 = rg.take(N * 4),
               m_cand1 = rg.take(N * k * 4), m_cand2 = rg.take(N * k * 4), m_n1 = rg.take(N * 4), m_n2 = rg.take(N * 4),
               m_idx1 = rg.take(N * 4), m_idx2 = rg.take(N * 4), count = rg.take(4);
  // gl_create_map_points' results and its own scratch
  const size_t x3d = rg.take(N * 24), type = rg.take(N * 4), comp = rg.take(N * 4), create = rg.take(gl::create_map_points_scratch_bytes((int)N));
  const size_t end = rg.off;
};

// base + layout -> what the stages take
struct TriScratch {
  PairWork nb;
  double* uv1;  // key-frame 1: dense (u, v), u_right, and the mask that grows from neighbour to neighbour
  float* ur1;
  uint8_t* mask;
  KfSide side2;        // the pair tables as the search reads them, neighbour j's at pair(j)
  KfPointSide point2;  // ... and as the match gather does
  int32_t* match;
  MatchSide m1, m2;
  int32_t *idx1, *idx2, *count;
  MatchPoints pts;
  void* create;
};
struct At {  // the start of a region as the pointer its member is
  char* p;
  template <class V>
  operator V*() const {
    return (V*)p;
  }
};
TriScratch tri_scratch(void* base, const TriLayout& L) {
  auto at = [base](size_t off) { return At{(char*)base + off}; };
  const int N = (int)L.N, NN = (int)L.NN, k = (int)L.k;
  const KfSide side2{at(L.uv2), at(L.ur2), at(L.oct2), at(L.ang2), at(L.desc2), at(L.mp2), NodeList{at(L.nn2), at(L.nid2), at(L.nptr2), at(L.nidx2), N, NN}};
  return TriScratch{PairWork{at(L.skip), at(L.rows), at(L.fmat), at(L.epi), at(L.nm)}, at(L.uv1), at(L.ur1), at(L.mask), side2,
                    KfPointSide{at(L.pose2), side2.uv, side2.ur, at(L.dep2), side2.oct, at(L.cand2), at(L.nc2), N, k}, at(L.match),
                    MatchSide{at(L.m_pose1), at(L.m_uvr1), at(L.m_dep1), at(L.m_oct1), at(L.m_cand1), at(L.m_n1)},
                    MatchSide{at(L.m_pose2), at(L.m_uvr2), at(L.m_dep2), at(L.m_oct2), at(L.m_cand2), at(L.m_n2)}, at(L.m_idx1), at(L.m_idx2),
                    at(L.count), MatchPoints{at(L.x3d), at(L.type), at(L.comp)}, at(L.create)};
}

}  // namespace

extern "C" {

int gl_tri_pair_setup(gl_ctx_t* ctx, const gl_camera* cam, int NKF, const uint8_t* kf_valid_dev, const double* kf_pose_dev,
                      const double* kf_twc_dev, int kf_row, const int32_t* conn_kf_dev, const int32_t* n_conn_dev, int conn_cap, int first_nb,
                      int n_nb, float mb, int32_t* skip_dev, double* fmat_dev, float* epipole_dev) {
  GL_REQUIRE(ctx && cam, "null argument");
  GL_REQUIRE(n_nb >= 0 && n_nb <= GL_TRI_NB_MAX, "n_nb outside [0, GL_TRI_NB_MAX]");
  if (n_nb == 0) return GL_OK;
  GL_REQUIRE(NKF >= 1 && kf_row >= 0 && kf_row < NKF, "kf_row outside [0, NKF)");
  GL_REQUIRE(first_nb >= 0 && conn_cap >= 0 && first_nb <= 0x7fffffff - n_nb, "bad first_nb / conn_cap");
  GL_REQUIRE(kf_pose_dev && kf_twc_dev && n_conn_dev && (conn_kf_dev || conn_cap == 0) && skip_dev && fmat_dev && epipole_dev, "null buffer");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  k_tri_pair_setup<<<1, 64, 0, c->stream>>>(make_pairk(cam), NKF, kf_valid_dev, kf_pose_dev, kf_twc_dev, kf_row, conn_kf_dev, n_conn_dev,
                                            conn_cap, first_nb, n_nb, mb, skip_dev, nullptr, fmat_dev, epipole_dev, nullptr, nullptr);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_create_map_points_from_map(gl_ctx_t* ctx, const gl_gmm_t* gmm, const gl_camera* cam, const gl_params* prm, float scale_factor,
                                  const gl_map_view* map, const gl_map_ba_view* ba, const gl_map_kf_tables* kt, int kf_row,
                                  const int32_t* conn_kf_dev, const int32_t* n_conn_dev, int conn_cap, int first_nb, int n_nb, float mb,
                                  int mp_base, const gl_tri_points_out* out) {
  GL_REQUIRE(ctx && gmm && cam && prm && map && ba && kt && out, "null argument");
  GL_REQUIRE(n_nb >= 0 && n_nb <= GL_TRI_NB_MAX, "n_nb outside [0, GL_TRI_NB_MAX]");
  const int N = map->NFK, NKF = map->NKF, NN = kt->NNcap, k = kt->k;
  GL_REQUIRE(NKF >= 1 && kf_row >= 0 && kf_row < NKF, "kf_row outside [0, NKF)");
  GL_REQUIRE(N >= 1 && N <= 4096, "NFK outside [1, 4096] (the on-chip capacity of gl_search_for_triangulation)");
  GL_REQUIRE(NN >= 1 && k >= 1 && k <= 8, "bad NNcap / k");
  GL_REQUIRE(cam->width > 0 && cam->height > 0, "camera width / height not set");
  GL_REQUIRE(first_nb >= 0 && conn_cap >= 0 && first_nb <= 0x7fffffff - n_nb && mp_base >= 0, "bad first_nb / conn_cap / mp_base");
  GL_REQUIRE(out->new_cap >= N, "new_cap < NFK (every feature of the key-frame may gain a point)");
  GL_REQUIRE(map->kf_mp && ba->kf_pose && ba->kf_twc && ba->kf_uvr && ba->kf_oct, "null kf_mp / kf_pose / kf_twc / kf_uvr / kf_oct");
  GL_REQUIRE(kt->kf_angle && kt->kf_desc && kt->kf_depth && kt->kf_nnode && kt->kf_node_id && kt->kf_node_ptr && kt->kf_node_idx && kt->kf_cand &&
                 kt->kf_ncand,
             "null key-frame table");
  GL_REQUIRE(n_conn_dev && (conn_kf_dev || conn_cap == 0), "null conn_kf / n_conn");
  GL_REQUIRE(out->new_pos && out->new_assoc && out->new_ref_kf && out->new_type && out->new_nb && out->new_feat1 && out->new_feat2 &&
                 out->att_mp && out->att_kf && out->att_feat && out->n_new && out->n_attach && out->feat_new && out->nb_stats && out->status,
             "null output buffer (only fmat / epipole are optional)");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  GL_REQUIRE_LDS(c, NodeQueries::matcher_lds(N, N, NN, NN));
  const TriLayout L(n_nb, N, NN, k);
  void* scratch = nullptr;
  const int rs = gl::ctx_scratch(c, L.end, &scratch, gl::SCRATCH_MAPTRI);
  if (rs != GL_OK) return rs;
  const TriScratch sc = tri_scratch(scratch, L);
  // the map's rows as sides of NKF "pairs"; key-frame 1: its row, with the dense (u, v) / u_right tables and the mask of k_tri_rows
  const KfTables t{ba->kf_uvr, map->kf_mp,
                   KfSide{nullptr, nullptr, ba->kf_oct, kt->kf_angle, kt->kf_desc, nullptr,
                          NodeList{kt->kf_nnode, kt->kf_node_id, kt->kf_node_ptr, kt->kf_node_idx, N, NN}},
                   KfPointSide{ba->kf_pose, nullptr, nullptr, kt->kf_depth, ba->kf_oct, kt->kf_cand, kt->kf_ncand, N, k}};
  KfSide side1 = t.match.pair(kf_row);
  KfPointSide point1 = t.point.pair(kf_row);
  side1.uv = point1.uv = sc.uv1;
  side1.ur = point1.ur = sc.ur1;
  side1.has_mp = sc.mask;
  const AcceptOut ao{(u64*)out->new_pos, out->new_assoc, out->new_ref_kf, out->new_type, out->new_nb,   out->new_feat1, out->new_feat2, out->att_mp,
                     out->att_kf,        out->att_feat,  out->n_new,      out->n_attach, out->feat_new, out->nb_stats,  out->new_cap};

  if (n_nb > 0) {
    k_tri_pair_setup<<<1, 64, 0, c->stream>>>(make_pairk(cam), NKF, map->kf_valid, ba->kf_pose, ba->kf_twc, kf_row, conn_kf_dev, n_conn_dev,
                                              conn_cap, first_nb, n_nb, mb, sc.nb.skip, sc.nb.rows, sc.nb.fmat, sc.nb.epipole, out->fmat,
                                              out->epipole);
    GL_HIP(hipGetLastError());
  }
  k_tri_rows<<<1 + n_nb, ROW_T, 0, c->stream>>>(kf_row, n_nb, t, sc.nb.skip, sc.nb.rows, side1, sc.side2, sc.point2, out->feat_new, out->n_new,
                                                out->n_attach, out->status);
  GL_HIP(hipGetLastError());
  for (int j = 0; j < n_nb; ++j) {
    const PairWork nb = sc.nb.pair(j);
    // ORBmatcher matcher(0.6, false): no orientation check; bOnlyStereo = false (:266)
    int rc = gl::launch_search_for_triangulation(c, scale_factor, 1, side1, sc.side2.pair(j), nb.fmat, nb.epipole, 0, 0, sc.match, nb.nmatches);
    if (rc != GL_OK) return rc;
    k_tri_match_rows<<<1, ROW_T, 0, c->stream>>>(point1, sc.point2.pair(j), sc.match, sc.m1, sc.m2, sc.idx1, sc.idx2, sc.count);
    GL_HIP(hipGetLastError());
    rc = gl::launch_create_map_points(c, gl::G(gmm), cam, prm, scale_factor, N, k, sc.m1, sc.m2, sc.pts, sc.create);
    if (rc != GL_OK) return rc;
    k_tri_accept<<<1, ROW_T, 0, c->stream>>>(N, kf_row, j, first_nb + j, mp_base, sc.nb.skip, sc.nb.rows, sc.nb.nmatches, sc.count, sc.idx1, sc.idx2,
                                             (const u64*)sc.pts.x3d, sc.pts.type, sc.pts.comp, sc.mask, ao);
    GL_HIP(hipGetLastError());
  }
  return GL_OK;
}

}  // extern "C"
