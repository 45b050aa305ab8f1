// ORBmatcher::searchByBoW (orb_matcher.cpp:295-408) with computeThreeMaxima (:544-578) for B key-frame / frame pairs: the matcher
// of Tracking::trackReferenceKeyFrame (tracking.cpp:303) - the map points of the reference key-frame are handed to the features
// of the current frame that share their vocabulary node and pass the distance / ratio tests.  Integer / byte work: per shared
// node, 256-bit Hamming distances between the key-frame's features that hold a valid map point and the frame's features.
//
// The reference loop is ORDER DEPENDENT like the other matchers' (gl_match.hip, gl_match_tri.hip): a frame feature taken by an
// earlier key-frame feature - earlier in the node's list; nodes do not interact, a feature sits in one node - is skipped by
// every later one, which then sees other best / second-best distances.  Same fixed point: queries are numbered by their position
// in the key-frame's feature-vector list (the reference's visiting order); in every round each query scans its node's frame
// features that are not owned by a LOWER query in the previous round - best = FIRST of the minimum distance (`dist < bestDist1`),
// second best = the minimum of the rest (a later equal distance becomes second best, and the ratio test then fails) -, decides
// (bestDist1 <= TH_LOW and bestDist1 < nn_ratio * bestDist2, in float), and an accepting query claims its feature:
// owner[feature] = the lowest query that claimed it.  The decisions of the queries 0 .. r-1 of a node are final after round r;
// the iteration stops when the owner table repeats.  Then the rotation histogram.
#include <climits>

#include "gl_internal.hpp"
#include "gl_match_common.hpp"

namespace {

using namespace gl_match;
constexpr int T_B = 512;

__global__ __launch_bounds__(T_B) void k_search_by_bow(int B, float nn_ratio, int check_orientation, KfSide side1, KfSide side2,
                                                       int32_t* __restrict__ match_all, int32_t* __restrict__ nmatches_all,
                                                       int32_t* __restrict__ counters, uint4* __restrict__ cache_all,
                                                       const int32_t* __restrict__ run_flag) {
  extern __shared__ __attribute__((aligned(16))) int32_t lds[];
  const int N1 = side1.nodes.N, N2 = side2.nodes.N;
  int32_t* owner = lds;            // N2: lowest query that claimed the frame feature in the previous round (INT_MAX: nobody)
  int32_t* owner_n = owner + N2;   // N2: being rebuilt
  int32_t* choice = owner_n + N2;  // N1 (by query): the frame feature an ACCEPTING query takes, else -1
  const NodeQueries nodes(choice + N1, N1, side1.nodes.NN, side2.nodes.NN);
  const int32_t *q_idx1 = nodes.q_idx1, *q_lo = nodes.q_lo, *q_hi = nodes.q_hi;
  __shared__ int s_changed, s_hist[32], s_keep[4], s_cnt[T_B / 64];
  const int f = blockIdx.x, tid = threadIdx.x;
  if (f >= B) return;
  if (run_flag && run_flag[f] == 0) return;  // (gl_track_frame_chain's trackKeyFrame fallback: only the frames that need it)
  const KfSide s1 = side1.pair(f), s2 = side2.pair(f);  // (side 2 is a frame: no uv / ur / oct / has_mp)
  const uint32_t *desc1 = (const uint32_t*)s1.desc, *desc2 = (const uint32_t*)s2.desc;
  const uint8_t* mp1 = s1.has_mp;
  const int32_t* nidx2 = s2.nodes.node_idx;

  // ---- queries: the key-frame's features that hold a valid map point ----
  for (int a = tid; a < N1; a += T_B) choice[a] = -1;
  const int nq = nodes.setup<T_B>(tid, s1.nodes, s2.nodes, [&](int i1) { return mp1[i1] != 0; });
  for (int i = tid; i < N2; i += T_B) owner[i] = INT_MAX;
  __syncthreads();

  // Round 5: a query's partners and their distances do not depend on the owners, which only
  // REMOVE partners.  best = first of the smallest distance, second best = the smallest of the rest: the two smallest keys
  //     dist << 22 | position in the partner list << 12 | feature of the frame.
  // Round 1 evaluates every partner once (descriptors requested four at a time) and leaves the three smallest keys and their number
  // in a 16-byte record; a later round decides from the keys whose features no lower query owns whenever two are left or the
  // record held every partner, and walks again otherwise.
  constexpr uint32_t EMPTY = 0xffffffffu;
  uint4* cache = cache_all + (size_t)f * N1;
  auto decide = [&](uint32_t a, uint32_t b) -> int {
    if (a == EMPTY) return -1;
    const int bestDist1 = (int)(a >> 22), bestDist2 = b == EMPTY ? 256 : (int)(b >> 22);
    return (bestDist1 <= 50 && (float)bestDist1 < nn_ratio * (float)bestDist2) ? (int)(a & 0xfffu) : -1;  // TH_LOW, nn_ratio_
  };
  auto walk = [&](int m, int idx1, uint32_t& k0, uint32_t& k1, uint32_t& k2, uint32_t& npass) {
    k0 = k1 = k2 = EMPTY;
    npass = 0;
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
        if (idx2 >= 0 && owner[idx2] < m) idx2 = -1;  // matches[realIdxF] is set: taken by an earlier key-frame feature
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
        if (dist >= 256) continue;  // (never below the initial best / second best)
        const int ord = b0 + j - lo;
        if (ord > 1023) {  // (a node of more than 1 024 partners cannot be keyed: the sequential evaluation, in every round)
          npass = EMPTY;
          continue;
        }
        const uint32_t kx = ((uint32_t)dist << 22) | ((uint32_t)ord << 12) | (uint32_t)idx2;
        if (npass != EMPTY) ++npass;
        keep3(k0, k1, k2, kx);
      }
    }
  };
  auto walk_seq = [&](int m, int idx1) -> int {
    uint32_t d1[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) d1[w] = desc1[(size_t)idx1 * 8 + w];
    int bestDist1 = 256, bestIdxF = -1, bestDist2 = 256;
    for (int b = q_lo[m]; b < q_hi[m]; ++b) {
      const int idx2 = nidx2[b];
      if (idx2 < 0 || idx2 >= N2) continue;
      if (owner[idx2] < m) continue;
      const int dist = hamming256(d1, desc2 + (size_t)idx2 * 8);
      if (dist < bestDist1) {
        bestDist2 = bestDist1;
        bestDist1 = dist;
        bestIdxF = idx2;
      } else if (dist < bestDist2) {
        bestDist2 = dist;
      }
    }
    return (bestDist1 <= 50 && (float)bestDist1 < nn_ratio * (float)bestDist2) ? bestIdxF : -1;
  };
  int rounds = 0;
  for (;;) {
    owner_round_begin<T_B>(tid, owner_n, N2, &s_changed, [](int) { return INT_MAX; });
    for (int m = tid; m < nq; m += T_B) {
      const int idx1 = q_idx1[m];
      int take = -1;
      if (idx1 >= 0) {
        bool need_walk = rounds == 0;
        if (rounds > 0) {
          const uint4 rec = cache[m];
          if (rec.w == EMPTY) {
            need_walk = true;
          } else {
            uint32_t a = EMPTY, b2 = EMPTY;
            int nav = 0;
            const uint32_t ks[3] = {rec.x, rec.y, rec.z};
#pragma unroll
            for (int j = 0; j < 3; ++j)
              if (ks[j] != EMPTY && owner[ks[j] & 0xfffu] >= m) {
                if (nav == 0) a = ks[j];
                else if (nav == 1) b2 = ks[j];
                ++nav;
              }
            if (nav >= 2 || rec.w <= 3u) take = decide(a, b2);
            else need_walk = true;
          }
        }
        if (need_walk) {
          uint32_t k0, k1, k2, npass;
          walk(m, idx1, k0, k1, k2, npass);
          if (npass == EMPTY) {
            take = walk_seq(m, idx1);
            if (rounds == 0) cache[m] = make_uint4(EMPTY, EMPTY, EMPTY, EMPTY);
          } else {
            take = decide(k0, k1);
            if (rounds == 0) cache[m] = make_uint4(k0, k1, k2, npass);
          }
        }
      }
      choice[m] = take;
      if (take >= 0) atomicMin(&owner_n[take], m);
    }
    __syncthreads();
    const bool changed = owner_round_end<T_B>(tid, owner, owner_n, N2, &s_changed);
    ++rounds;
    if (!changed || rounds > nq + 1) break;
    __syncthreads();
  }

  // ---- rotation consistency (:362-374, :391-405) ------------------------------------------------------------------------
  // (in the fixed point every accepting query owns its choice)
  if (check_orientation) {
    rotation_filter<T_B>(
        tid, nq, s_hist, s_keep, [&](int m) { return choice[m] >= 0; }, [&](int m) { return s1.angle[q_idx1[m]] - s2.angle[choice[m]]; },
        [&](int m) { choice[m] = -1; });
  }

  // ---- outputs: matches by FRAME feature (the key-frame feature whose map point it gets) ------------------------------------
  int32_t* match = match_all + (size_t)f * N2;
  for (int i = tid; i < N2; i += T_B) match[i] = -1;
  __syncthreads();
  int cnt = 0;
  for (int m = tid; m < nq; m += T_B)
    if (q_idx1[m] >= 0 && choice[m] >= 0) {
      match[choice[m]] = q_idx1[m];
      ++cnt;
    }
  count_matches<T_B>(tid, cnt, s_cnt, &nmatches_all[f], counters, rounds);
}

}  // namespace

extern "C" int gl_search_by_bow(gl_ctx_t* ctx, float nn_ratio, int check_orientation, int B, int N1, int N2, int NN1, int NN2,
                                const float* angle1_dev, const uint8_t* desc1_dev, const uint8_t* has_mp1_dev, const int32_t* nnode1_dev,
                                const int32_t* node_id1_dev, const int32_t* node_ptr1_dev, const int32_t* node_idx1_dev,
                                const float* angle2_dev, const uint8_t* desc2_dev, const int32_t* nnode2_dev, const int32_t* node_id2_dev,
                                const int32_t* node_ptr2_dev, const int32_t* node_idx2_dev, int32_t* match21_dev, int32_t* nmatches_dev) {
  return gl::launch_bow_gated(
      ctx, nn_ratio, check_orientation, B,
      KfSide{nullptr, nullptr, nullptr, angle1_dev, desc1_dev, has_mp1_dev, NodeList{nnode1_dev, node_id1_dev, node_ptr1_dev, node_idx1_dev, N1, NN1}},
      KfSide{nullptr, nullptr, nullptr, angle2_dev, desc2_dev, nullptr, NodeList{nnode2_dev, node_id2_dev, node_ptr2_dev, node_idx2_dev, N2, NN2}},
      match21_dev, nmatches_dev, nullptr);
}

// the same with a per-frame switch (run_flag B int32, 0: the frame's workgroup returns at once and writes nothing; null: every frame).
// The sides' uv / ur / oct and side 2's has_mp are not read.
int gl::launch_bow_gated(gl_ctx_t* ctx, float nn_ratio, int check_orientation, int B, const KfSide& side1, const KfSide& side2, int32_t* match21_dev,
                         int32_t* nmatches_dev, const int32_t* run_flag) {
  const NodeList &l1 = side1.nodes, &l2 = side2.nodes;
  const int N1 = l1.N, N2 = l2.N, NN1 = l1.NN, NN2 = l2.NN;
  GL_REQUIRE(ctx, "null context");
  if (B == 0) return GL_OK;
  GL_REQUIRE(B > 0 && N1 >= 1 && N2 >= 1 && NN1 >= 1 && NN2 >= 1, "bad B / N1 / N2 / NN1 / NN2");
  GL_REQUIRE(N1 <= 4096 && N2 <= 4096, "N1 / N2 above the on-chip capacity (4096 features per frame)");
  GL_REQUIRE(side1.angle && side1.desc && side1.has_mp && l1.nnode && l1.node_id && l1.node_ptr && l1.node_idx && side2.angle && side2.desc &&
                 l2.nnode && l2.node_id && l2.node_ptr && l2.node_idx && match21_dev && nmatches_dev,
             "null buffer");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  const size_t lds = NodeQueries::matcher_lds(N1, N2, NN1, NN2);
  GL_REQUIRE_LDS(c, lds);
  GL_HIP(gl::ensure_dynamic_lds(c, (const void*)k_search_by_bow, lds));
  void* cache = nullptr;  // 16 bytes per query: its three best partners of round 1
  {
    const int rc = gl::ctx_scratch(c, (size_t)B * N1 * sizeof(uint4), &cache, gl::SCRATCH_CACHE);
    if (rc != GL_OK) return rc;
  }
  k_search_by_bow<<<B, T_B, lds, c->stream>>>(B, nn_ratio, check_orientation, side1, side2, match21_dev, nmatches_dev, c->counters, (uint4*)cache,
                                              run_flag);
  GL_HIP(hipGetLastError());
  return GL_OK;
}
