// ORBmatcher::searchForTriangulation (orb_matcher.cpp:141-293) with checkEpipolarDist (:119-139) and computeThreeMaxima
// (:544-578) for B key-frame pairs: the producer of the matches Localization::createMapPoints triangulates
// (localization_opt.cpp:266; gl_create_map_points takes them from here).  Integer / byte work: per vocabulary node the two
// key-frames share, 256-bit Hamming distances between its features of key-frame 1 and of key-frame 2, the epipole test of
// mono pairs, the epipolar chi2, then the rotation histogram.
//
// The reference loop is ORDER DEPENDENT like searchByProjection's (gl_match.hip): a feature of key-frame 2 taken by an
// earlier feature of key-frame 1 - earlier node, or earlier in the node's list - is skipped by every later one, which falls
// back to its next-best partner.  Same fixed point: queries are numbered by their position in key-frame 1's feature-vector
// list (= the order the reference visits them in: std::map iterates node ids ascending, the lists are in push order); in every
// round each query picks its best partner among those not owned by a LOWER query in the previous round, owner[partner] = min
// query that picked it; the choices of the queries 0 .. r-1 are final after round r, and the iteration stops when the owner
// table repeats.  "Best" is the reference's scan: minimum descriptor distance among the partners that pass the geometric
// tests, the LAST one of equal distance (`dist > bestDist` only skips worse candidates) - the geometric tests do not depend on
// the state of the scan, so this is what the sequential scan returns.
// The DBoW2 feature vectors arrive as CSR (node ids ascending, node_ptr, node_idx in list order); the fundamental matrix and
// the epipole are the host's (Eigen: K^-T E K^-1 and quaternion products, MathUtils::computeFundamentalMatrix).
// Every float / double conversion of the reference is kept (the file is compiled without contraction).
#include <climits>

#include "gl_internal.hpp"
#include "gl_map_dev.hpp"  // block_excl_scan
#include "gl_match_common.hpp"

namespace {

using namespace gl_match;
constexpr int T_T = 512;

struct TriP {
  int only_stereo, check_orientation;
  float sf[8], sigma2[8];
};

// (positional __restrict__ parameters, which the launcher unpacks: two KfSide by value spill scalar registers, r16_kf_side_kernel_meta.txt)
__global__ __launch_bounds__(T_T) void k_search_for_triangulation(
    TriP P, int B, int N1, int N2, int NN1, int NN2, const double* __restrict__ uv1_all, const float* __restrict__ ur1_all,
    const int32_t* __restrict__ oct1_all, const float* __restrict__ angle1_all, const uint8_t* __restrict__ desc1_all,
    const uint8_t* __restrict__ mp1_all, const int32_t* __restrict__ nn1_all, const int32_t* __restrict__ nid1_all,
    const int32_t* __restrict__ nptr1_all, const int32_t* __restrict__ nidx1_all, const double* __restrict__ uv2_all,
    const float* __restrict__ ur2_all, const int32_t* __restrict__ oct2_all, const float* __restrict__ angle2_all,
    const uint8_t* __restrict__ desc2_all, const uint8_t* __restrict__ mp2_all, const int32_t* __restrict__ nn2_all,
    const int32_t* __restrict__ nid2_all, const int32_t* __restrict__ nptr2_all, const int32_t* __restrict__ nidx2_all,
    const double* __restrict__ fmat_all, const float* __restrict__ epi_all, int32_t* __restrict__ match_all, int32_t* __restrict__ nmatches_all,
    int32_t* __restrict__ counters, uint4* __restrict__ cache_all) {
  extern __shared__ __attribute__((aligned(16))) int32_t lds[];
  int32_t* owner = lds;             // N2: lowest query that picked the feature in the previous round (-1: not available at all)
  int32_t* owner_n = owner + N2;    // N2: being rebuilt
  int32_t* choice = owner_n + N2;   // N1 (by query)
  const NodeQueries nodes(choice + N1, N1, NN1, NN2);
  const int32_t *q_idx1 = nodes.q_idx1, *q_lo = nodes.q_lo, *q_hi = nodes.q_hi;
  __shared__ int s_changed, s_hist[32], s_keep[4], s_cnt[T_T / 64];
  const int f = blockIdx.x, tid = threadIdx.x;
  if (f >= B) return;
  const KfSide s1 = KfSide{uv1_all, ur1_all, oct1_all, angle1_all, desc1_all, mp1_all, NodeList{nn1_all, nid1_all, nptr1_all, nidx1_all, N1, NN1}}.pair(f);
  const KfSide s2 = KfSide{uv2_all, ur2_all, oct2_all, angle2_all, desc2_all, mp2_all, NodeList{nn2_all, nid2_all, nptr2_all, nidx2_all, N2, NN2}}.pair(f);
  const double *uv1 = s1.uv, *uv2 = s2.uv;
  const float *ur1 = s1.ur, *ur2 = s2.ur;
  const int32_t *oct1 = s1.oct, *oct2 = s2.oct, *nidx2 = s2.nodes.node_idx;
  const uint32_t *desc1 = (const uint32_t*)s1.desc, *desc2 = (const uint32_t*)s2.desc;
  const uint8_t *mp1 = s1.has_mp, *mp2 = s2.has_mp;
  const double* F = fmat_all + (size_t)f * 9;
  const float ex = epi_all[2 * f], ey = epi_all[2 * f + 1];

  // ---- queries: list entry a of key-frame 1 -> its feature and the partner list of the same node in key-frame 2 ----
  // (who may ask: not the features with a map point, nor the mono ones under only-stereo)
  for (int a = tid; a < N1; a += T_T) choice[a] = -1;
  const int nq = nodes.setup<T_T>(tid, s1.nodes, s2.nodes,
                                  [&](int i1) { return oct1[i1] >= 0 && !mp1[i1] && !(P.only_stereo && !(ur1[i1] >= 0)); });
  for (int i = tid; i < N2; i += T_T) owner[i] = (oct2[i] >= 0 && !mp2[i] && !(P.only_stereo && !(ur2[i] >= 0))) ? INT_MAX : -1;
  __syncthreads();

  // ---- rounds of the fixed point ------------------------------------------------------------------------------------
  // Round 5: what a query can ever take is fixed by the tests that do not depend on the owners - the partners of its vocabulary node
  // with a distance <= TH_LOW that pass the epipole / epipolar tests; the owners only REMOVE partners.  The reference keeps, of
  // those, the smallest distance and among equal distances the LAST in list order: the smallest key
  //     dist << 26 | (1023 - position in the partner list) << 16 | feature of key-frame 2.
  // Round 1 evaluates every partner once (descriptors requested four at a time) and leaves the query's three smallest keys and
  // their number in a 16-byte record; a later round takes the first key whose feature no lower query owns, and walks again only if
  // all three are gone and there were more.
  constexpr uint32_t EMPTY = 0xffffffffu;
  uint4* cache = cache_all + (size_t)f * N1;
  auto walk = [&](int m, int idx1, uint32_t& k0, uint32_t& k1, uint32_t& k2, uint32_t& npass) {
    k0 = k1 = k2 = EMPTY;
    npass = 0;
    const bool bStereo1 = ur1[idx1] >= 0;
    const double u1 = uv1[2 * idx1], v1 = uv1[2 * idx1 + 1];
    // checkEpipolarDist: the line of kp1 in key-frame 2
    const double ea = u1 * F[0] + v1 * F[3] + F[6];
    const double eb = u1 * F[1] + v1 * F[4] + F[7];
    const double ec = u1 * F[2] + v1 * F[5] + F[8];
    const float den = (float)(ea * ea + eb * eb);
    uint32_t d1[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) d1[w] = desc1[(size_t)idx1 * 8 + w];
    const int lo = q_lo[m], hi = q_hi[m];
    for (int b0 = lo; b0 < hi; b0 += 4) {
      int id[4];
      uint4 da[4], db[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int idx2 = b0 + j < hi ? nidx2[b0 + j] : -1;
        if (idx2 >= N2) idx2 = -1;
        if (idx2 >= 0 && owner[idx2] < m) idx2 = -1;  // not available at all (-1), or taken by an earlier feature of key-frame 1
        id[j] = idx2;
        da[j] = db[j] = make_uint4(0, 0, 0, 0);
        if (idx2 >= 0) {
          const uint4* src = (const uint4*)(desc2 + (size_t)idx2 * 8);
          da[j] = src[0];
          db[j] = src[1];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int idx2 = id[j];
        if (idx2 < 0) continue;
        const int dist = hamming256(d1, da[j], db[j]);
        if (dist > 50) continue;  // TH_LOW
        const double u2 = uv2[2 * idx2], v2 = uv2[2 * idx2 + 1];
        const int oc2 = oct2[idx2] & 7;
        if (!bStereo1 && !(ur2[idx2] >= 0)) {
          const float distex = (float)((double)ex - u2);
          const float distey = (float)((double)ey - v2);
          if (distex * distex + distey * distey < 100.0f * P.sf[oc2]) continue;
        }
        const float num = (float)(ea * u2 + eb * v2 + ec);
        if (den == 0) continue;
        const float dsqr = num * num / den;
        if (!((double)dsqr < 3.84 * (double)P.sigma2[oc2])) continue;
        const int ord = b0 + j - lo;
        if (ord > 1023) {  // (a node with more than 1 024 partners: this query walks in every round)
          npass = EMPTY;
          continue;
        }
        uint32_t kx = ((uint32_t)dist << 26) | ((uint32_t)(1023 - ord) << 16) | (uint32_t)idx2;
        if (npass != EMPTY) ++npass;
        keep3(k0, k1, k2, kx);
      }
    }
  };
  // (a node of more than 1 024 partners cannot be keyed: such a query is evaluated the sequential way, in every round)
  auto walk_seq = [&](int m, int idx1) -> int {
    const bool bStereo1 = ur1[idx1] >= 0;
    const double u1 = uv1[2 * idx1], v1 = uv1[2 * idx1 + 1];
    const double ea = u1 * F[0] + v1 * F[3] + F[6];
    const double eb = u1 * F[1] + v1 * F[4] + F[7];
    const double ec = u1 * F[2] + v1 * F[5] + F[8];
    const float den = (float)(ea * ea + eb * eb);
    uint32_t d1[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) d1[w] = desc1[(size_t)idx1 * 8 + w];
    int bestDist = 50, bestIdx2 = -1;  // TH_LOW
    for (int b = q_lo[m]; b < q_hi[m]; ++b) {
      const int idx2 = nidx2[b];
      if (idx2 < 0 || idx2 >= N2) continue;
      if (owner[idx2] < m) continue;
      const int dist = hamming256(d1, desc2 + (size_t)idx2 * 8);
      if (dist > 50 || dist > bestDist) continue;
      const double u2 = uv2[2 * idx2], v2 = uv2[2 * idx2 + 1];
      const int oc2 = oct2[idx2] & 7;
      if (!bStereo1 && !(ur2[idx2] >= 0)) {
        const float distex = (float)((double)ex - u2);
        const float distey = (float)((double)ey - v2);
        if (distex * distex + distey * distey < 100.0f * P.sf[oc2]) continue;
      }
      const float num = (float)(ea * u2 + eb * v2 + ec);
      if (den == 0) continue;
      const float dsqr = num * num / den;
      if (!((double)dsqr < 3.84 * (double)P.sigma2[oc2])) continue;
      bestIdx2 = idx2;
      bestDist = dist;
    }
    return bestIdx2;
  };
  int rounds = 0;
  for (;;) {
    owner_round_begin<T_T>(tid, owner_n, N2, &s_changed, [&](int i) { return owner[i] < 0 ? -1 : INT_MAX; });
    for (int m = tid; m < nq; m += T_T) {
      const int idx1 = q_idx1[m];
      int bestIdx2 = -1;
      if (idx1 >= 0) {
        uint4 rec = make_uint4(EMPTY, EMPTY, EMPTY, 0);
        bool need_walk = rounds == 0;
        if (rounds > 0) {
          rec = cache[m];
          if (rec.w == EMPTY) {
            need_walk = true;
          } else {
            const uint32_t ks[3] = {rec.x, rec.y, rec.z};
            bool found = false;
#pragma unroll
            for (int j = 0; j < 3; ++j)
              if (!found && ks[j] != EMPTY && owner[ks[j] & 0xffffu] >= m) {
                bestIdx2 = (int)(ks[j] & 0xffffu);
                found = true;
              }
            if (!found && rec.w > 3u) need_walk = true;  // all three gone and there were more
          }
        }
        if (need_walk) {
          uint32_t k0, k1, k2, npass;
          walk(m, idx1, k0, k1, k2, npass);
          if (npass == EMPTY) {
            bestIdx2 = walk_seq(m, idx1);
            if (rounds == 0) cache[m] = make_uint4(EMPTY, EMPTY, EMPTY, EMPTY);
          } else {
            bestIdx2 = k0 == EMPTY ? -1 : (int)(k0 & 0xffffu);
            if (rounds == 0) cache[m] = make_uint4(k0, k1, k2, npass);
          }
        }
      }
      choice[m] = bestIdx2;
      if (bestIdx2 >= 0) atomicMin(&owner_n[bestIdx2], m);
    }
    __syncthreads();
    const bool changed = owner_round_end<T_T>(tid, owner, owner_n, N2, &s_changed);
    ++rounds;
    if (!changed || rounds > nq + 1) break;
    __syncthreads();
  }

  // ---- rotation consistency (:235-246, :264-281) ----------------------------------------------------------------------
  // (a query keeps its choice iff it owns it: in the fixed point every choice is owned by its query)
  if (P.check_orientation) {
    rotation_filter<T_T>(
        tid, nq, s_hist, s_keep, [&](int m) { return choice[m] >= 0; }, [&](int m) { return s1.angle[q_idx1[m]] - s2.angle[choice[m]]; },
        [&](int m) { choice[m] = -1; });
  }

  // ---- outputs: matches12 by feature of key-frame 1 ----------------------------------------------------------------
  int32_t* match = match_all + (size_t)f * N1;
  for (int i = tid; i < N1; i += T_T) match[i] = -1;
  __syncthreads();
  int cnt = 0;
  for (int m = tid; m < nq; m += T_T)
    if (q_idx1[m] >= 0 && choice[m] >= 0) {
      match[q_idx1[m]] = choice[m];
      ++cnt;
    }
  count_matches<T_T>(tid, cnt, s_cnt, &nmatches_all[f], counters, rounds);
}

// ---- matches -> the per-match arrays of gl_create_map_points, on the device ----------------------------------------------
// Localization::createMapPoints walks matched_pairs (ascending feature index of key-frame 1) and reads, per match, the two
// key-frames' poses, key-points (u, v, u_right), depths, octaves and candidate components (kf->comps_[idx], localization_opt.cpp:
// 286-420).  k_tri_offsets: exclusive scan of the pairs' match counts; k_tri_gather: one workgroup per pair compacts its matches
// in index order behind the pair's offset.
__global__ __launch_bounds__(256) void k_tri_offsets(int B, const int32_t* __restrict__ nmatches, int32_t* __restrict__ pair_off) {
  __shared__ int s_part[256];
  const int tid = threadIdx.x, per = (B + 255) / 256, b0 = tid * per, b1 = min(B, b0 + per);
  int s = 0;
  for (int b = b0; b < b1; ++b) s += max(nmatches[b], 0);
  s_part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < 256; ++t) {
      const int v = s_part[t];
      s_part[t] = run;
      run += v;
    }
    pair_off[B] = run;
  }
  __syncthreads();
  int run = s_part[tid];
  for (int b = b0; b < b1; ++b) {
    pair_off[b] = run;
    run += max(nmatches[b], 0);
  }
}

__global__ __launch_bounds__(256) void k_tri_gather(int B, int cap, const int32_t* __restrict__ match_all, const int32_t* __restrict__ pair_off,
                                                    KfPointSide a, KfPointSide b, MatchSide oa, MatchSide ob, int32_t* __restrict__ pair_of,
                                                    int32_t* __restrict__ idx1_of, int32_t* __restrict__ idx2_of) {
  __shared__ int s_w[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  if (f >= B) return;
  const int32_t* match = match_all + (size_t)f * a.N;
  int run = pair_off[f];
  for (int i0 = 0; i0 < a.N; i0 += 256) {
    const int i = i0 + tid;
    const int j = i < a.N ? match[i] : -1;
    const bool on = j >= 0 && j < b.N;
    int total;
    const int at = run + gl::mapdev::block_excl_scan<256, int>(on ? 1 : 0, s_w, tid, &total);
    run += total;
    if (on && at < cap) {
      gather_match(a, b, f, i, j, oa, ob, at);
      pair_of[at] = f;
      idx1_of[at] = i;
      idx2_of[at] = j;
    }
  }
}

}  // namespace

extern "C" int gl_gather_triangulation_matches(gl_ctx_t* ctx, int B, int N1, int N2, int k, int cap, const int32_t* match12_dev,
                                               const int32_t* nmatches_dev, const double* pose1_dev, const double* uv1_dev,
                                               const float* ur1_dev, const float* depth1_dev, const int32_t* oct1_dev, const int32_t* cand1_dev,
                                               const int32_t* ncand1_dev, const double* pose2_dev, const double* uv2_dev, const float* ur2_dev,
                                               const float* depth2_dev, const int32_t* oct2_dev, const int32_t* cand2_dev,
                                               const int32_t* ncand2_dev, int32_t* pair_off_dev, double* m_pose1_dev, double* m_uvr1_dev,
                                               float* m_depth1_dev, int32_t* m_oct1_dev, int32_t* m_cand1_dev, int32_t* m_n1_dev,
                                               double* m_pose2_dev, double* m_uvr2_dev, float* m_depth2_dev, int32_t* m_oct2_dev,
                                               int32_t* m_cand2_dev, int32_t* m_n2_dev, int32_t* m_pair_dev, int32_t* m_idx1_dev,
                                               int32_t* m_idx2_dev) {
  GL_REQUIRE(ctx, "null context");
  if (B == 0) return GL_OK;
  GL_REQUIRE(B > 0 && N1 >= 1 && N2 >= 1 && k >= 1 && cap >= 1, "bad B / N1 / N2 / k / cap");
  GL_REQUIRE(match12_dev && nmatches_dev && pose1_dev && uv1_dev && ur1_dev && depth1_dev && oct1_dev && cand1_dev && ncand1_dev && pose2_dev &&
                 uv2_dev && ur2_dev && depth2_dev && oct2_dev && cand2_dev && ncand2_dev && pair_off_dev && m_pose1_dev && m_uvr1_dev &&
                 m_depth1_dev && m_oct1_dev && m_cand1_dev && m_n1_dev && m_pose2_dev && m_uvr2_dev && m_depth2_dev && m_oct2_dev &&
                 m_cand2_dev && m_n2_dev && m_pair_dev && m_idx1_dev && m_idx2_dev,
             "null buffer");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  k_tri_offsets<<<1, 256, 0, c->stream>>>(B, nmatches_dev, pair_off_dev);
  k_tri_gather<<<B, 256, 0, c->stream>>>(B, cap, match12_dev, pair_off_dev,
                                         KfPointSide{pose1_dev, uv1_dev, ur1_dev, depth1_dev, oct1_dev, cand1_dev, ncand1_dev, N1, k},
                                         KfPointSide{pose2_dev, uv2_dev, ur2_dev, depth2_dev, oct2_dev, cand2_dev, ncand2_dev, N2, k},
                                         MatchSide{m_pose1_dev, m_uvr1_dev, m_depth1_dev, m_oct1_dev, m_cand1_dev, m_n1_dev},
                                         MatchSide{m_pose2_dev, m_uvr2_dev, m_depth2_dev, m_oct2_dev, m_cand2_dev, m_n2_dev}, m_pair_dev, m_idx1_dev,
                                         m_idx2_dev);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// k_search_for_triangulation for the callers inside the library (gl_map_tri.hip): the values as gl_search_for_triangulation's and
// already checked, the context's device current.  The round cache is the launcher's own (SCRATCH_CACHE).
int gl::launch_search_for_triangulation(Ctx* c, float scale_factor, int B, const KfSide& side1, const KfSide& side2, const double* fmat_dev,
                                        const float* epipole_dev, int only_stereo, int check_orientation, int32_t* match12_dev,
                                        int32_t* nmatches_dev) {
  TriP P;
  P.only_stereo = only_stereo;
  P.check_orientation = check_orientation;
  pyramid_scales(scale_factor, P.sf, P.sigma2, nullptr);
  const int N1 = side1.nodes.N;
  const size_t lds = NodeQueries::matcher_lds(N1, side2.nodes.N, side1.nodes.NN, side2.nodes.NN);
  GL_REQUIRE_LDS(c, lds);
  GL_HIP(gl::ensure_dynamic_lds(c, (const void*)k_search_for_triangulation, lds));
  void* cache = nullptr;  // 16 bytes per query: its three best partners of round 1 (the kernel's round loop)
  {
    const int rc = gl::ctx_scratch(c, (size_t)B * N1 * sizeof(uint4), &cache, gl::SCRATCH_CACHE);
    if (rc != GL_OK) return rc;
  }
  const NodeList &l1 = side1.nodes, &l2 = side2.nodes;
  k_search_for_triangulation<<<B, T_T, lds, c->stream>>>(P, B, N1, l2.N, l1.NN, l2.NN, side1.uv, side1.ur, side1.oct, side1.angle, side1.desc,
                                                        side1.has_mp, l1.nnode, l1.node_id, l1.node_ptr, l1.node_idx, side2.uv, side2.ur, side2.oct,
                                                        side2.angle, side2.desc, side2.has_mp, l2.nnode, l2.node_id, l2.node_ptr, l2.node_idx, fmat_dev,
                                                        epipole_dev, match12_dev, nmatches_dev, c->counters, (uint4*)cache);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

extern "C" int gl_search_for_triangulation(gl_ctx_t* ctx, float scale_factor, int B, int N1, int N2, int NN1, int NN2,
                                           const double* uv1_dev, const float* ur1_dev, const int32_t* oct1_dev, const float* angle1_dev,
                                           const uint8_t* desc1_dev, const uint8_t* has_mp1_dev, const int32_t* nnode1_dev,
                                           const int32_t* node_id1_dev, const int32_t* node_ptr1_dev, const int32_t* node_idx1_dev,
                                           const double* uv2_dev, const float* ur2_dev, const int32_t* oct2_dev, const float* angle2_dev,
                                           const uint8_t* desc2_dev, const uint8_t* has_mp2_dev, const int32_t* nnode2_dev,
                                           const int32_t* node_id2_dev, const int32_t* node_ptr2_dev, const int32_t* node_idx2_dev,
                                           const double* fmat_dev, const float* epipole_dev, int only_stereo, int check_orientation,
                                           int32_t* match12_dev, int32_t* nmatches_dev) {
  GL_REQUIRE(ctx, "null context");
  if (B == 0) return GL_OK;
  GL_REQUIRE(B > 0 && N1 >= 1 && N2 >= 1 && NN1 >= 1 && NN2 >= 1, "bad B / N1 / N2 / NN1 / NN2");
  GL_REQUIRE(N1 <= 4096 && N2 <= 4096, "N1 / N2 above the on-chip capacity (4096 features per key-frame)");
  GL_REQUIRE(uv1_dev && ur1_dev && oct1_dev && angle1_dev && desc1_dev && has_mp1_dev && nnode1_dev && node_id1_dev && node_ptr1_dev &&
                 node_idx1_dev && uv2_dev && ur2_dev && oct2_dev && angle2_dev && desc2_dev && has_mp2_dev && nnode2_dev && node_id2_dev &&
                 node_ptr2_dev && node_idx2_dev && fmat_dev && epipole_dev && match12_dev && nmatches_dev,
             "null buffer");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  return gl::launch_search_for_triangulation(
      c, scale_factor, B,
      KfSide{uv1_dev, ur1_dev, oct1_dev, angle1_dev, desc1_dev, has_mp1_dev, NodeList{nnode1_dev, node_id1_dev, node_ptr1_dev, node_idx1_dev, N1, NN1}},
      KfSide{uv2_dev, ur2_dev, oct2_dev, angle2_dev, desc2_dev, has_mp2_dev, NodeList{nnode2_dev, node_id2_dev, node_ptr2_dev, node_idx2_dev, N2, NN2}},
      fmat_dev, epipole_dev, only_stereo, check_orientation, match12_dev, nmatches_dev);
}
