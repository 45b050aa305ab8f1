// The refresh of a map point's matcher inputs after its observations change - MapPoint::computeDistinctiveDescriptors
// (mappoint.cpp:126-190) and MapPoint::updateNormalAndDepth (mappoint.cpp:211-255) - for NP points in one launch.  Outputs are the
// mp_desc / mp_normal / mp_max_dist / mp_min_dist arrays that gl_project_map_points, gl_search_local_points, gl_fuse_search and the
// tracked-frame chain read.  One wave per 64 consecutive points, lane = point:
//   normal and depth  the lane walks its observations in list order: a serial left fold, as the reference sums
//   descriptor        N = the observations whose key-frame is valid.  N <= 2: the first of them (every median is element 0 of a sorted
//                     row, 0).  Points of at most MP_NMAX observations: PACKED - the descriptors of as many points as fit MP_ROWS
//                     rows are staged in LDS, a row per lane (the observations of invalid key-frames flagged), then one row per
//                     lane: its distances to the point's N descriptors, computed once into a 16-bit LDS column of that lane, then
//                     element (N-1)/2 of the sorted row by a 9-step binary search over the value, counting d <= v; the point's
//                     lane takes the first strictly smallest median.  More observations: GENERAL - the whole wave on one point, one row per lane and 64 rows at a time,
//                     the columns in LDS tiles of MP_ROWS; the median by a two-pass radix select over per-lane histograms (bits
//                     8..4 of the distance, then bits 3..0 inside the chosen bin), and the first minimum of (median, row) over the
//                     rows.  Exact for any N; only slower.
// Everything is integer arithmetic except the normal and the depth, which keep the reference's operations in its order (compiled
// without contraction; sqrt and / correctly rounded).
#include <climits>
#include <cmath>

#include "gl_internal.hpp"
#include "gl_match_common.hpp"

namespace {

using gl_match::hamming256;

constexpr int MP_ROWS = 128;  // descriptor rows per wave in LDS (a packed batch, a general tile)
constexpr int MP_NMAX = 32;   // the most observations of a point on the packed path (the lane's distance column)

struct MpP {
  int what, NP, NKF, NFK, NOBS;
  float sf[8];  // frame::scale_factors, init_config.hpp:67-76
};

struct MpLds {
  uint4 desc[MP_ROWS][2];  // 32-byte descriptor rows
  union {
    uint16_t dist[MP_NMAX][64];  // packed: dist[j][lane] = row(lane) . column j
    uint32_t hist[17][64];       // general: the lane's histogram of its row
  };
  uint16_t med[MP_ROWS];  // packed: the median of each row
  int32_t obs[MP_ROWS];   // packed: the row's observation
  int32_t info[MP_ROWS];  // packed: first row of the row's point | its observations << 8 | N << 16 | valid << 24; general: 1 if
                          // the tile's observation counts
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(v, m);
    v = o < v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(64) void k_update_map_points(MpP P, const double* __restrict__ kf_twc, const uint8_t* __restrict__ kf_valid,
                                                          const int32_t* __restrict__ kf_oct, const uint8_t* __restrict__ kf_desc,
                                                          const double* __restrict__ pos_all, const uint8_t* __restrict__ pt_valid,
                                                          const int32_t* __restrict__ ref_kf, const int32_t* __restrict__ obs_ptr,
                                                          const int32_t* __restrict__ obs_kf, const int32_t* __restrict__ obs_feat,
                                                          uint8_t* __restrict__ desc_out, double* __restrict__ normal_out,
                                                          float* __restrict__ max_out, float* __restrict__ min_out) {
  __shared__ MpLds S;
  const int lane = threadIdx.x;
  const int p = blockIdx.x * 64 + lane;
  // the point is touched at all only if it is valid, its row is a sub-range of [0, NOBS], non-empty, and every observation's
  // key-frame and feature index is in range
  int a0 = 0, a1 = 0;
  bool ok = false;
  if (p < P.NP) {
    a0 = obs_ptr[p];
    a1 = obs_ptr[p + 1];
    ok = a0 >= 0 && a0 < a1 && a1 <= P.NOBS && (!pt_valid || pt_valid[p]);
    for (int a = a0; ok && a < a1; ++a) {
      const int k = obs_kf[a], f = obs_feat[a];
      ok = k >= 0 && k < P.NKF && f >= 0 && f < P.NFK;
    }
    if (!ok) a0 = a1 = 0;
  }

  if ((P.what & 2) && ok) {  // updateNormalAndDepth
    const int r = ref_kf[p];
    if (r >= 0 && r < P.NKF) {
      const double px = pos_all[(size_t)p * 3], py = pos_all[(size_t)p * 3 + 1], pz = pos_all[(size_t)p * 3 + 2];
      double nx = 0.0, ny = 0.0, nz = 0.0;
      int feat_ref = 0;  // observations[pRefKF] on the local copy inserts feature 0 when the ref key-frame does not observe the point
      bool found = false;
      for (int a = a0; a < a1; ++a) {
        const int k = obs_kf[a];
        if (!found && k == r) {
          feat_ref = obs_feat[a];
          found = true;
        }
        const double* o = kf_twc + (size_t)k * 3;
        double vx = px - o[0], vy = py - o[1], vz = pz - o[2];
        const double sq = vx * vx + vy * vy + vz * vz;
        if (sq > 0.0) {  // Eigen::normalized: a zero vector stays zero
          const double s = sqrt(sq);
          vx = vx / s;
          vy = vy / s;
          vz = vz / s;
        }
        nx = nx + vx;
        ny = ny + vy;
        nz = nz + vz;
      }
      const int level = kf_oct[(size_t)r * P.NFK + feat_ref];
      if (level >= 0 && level < 8) {
        float sfl = P.sf[0];
#pragma unroll
        for (int L = 1; L < 8; ++L) sfl = level == L ? P.sf[L] : sfl;  // (no dynamic index into the argument block)
        const double* o = kf_twc + (size_t)r * 3;
        const double cx = px - o[0], cy = py - o[1], cz = pz - o[2];
        const float dist = (float)sqrt(cx * cx + cy * cy + cz * cz);
        const float mx = dist * sfl;
        const double n = (double)(a1 - a0);
        normal_out[(size_t)p * 3] = nx / n;
        normal_out[(size_t)p * 3 + 1] = ny / n;
        normal_out[(size_t)p * 3 + 2] = nz / n;
        max_out[p] = mx;
        min_out[p] = mx / P.sf[7];
      }
    }
  }

  if (!(P.what & 1)) return;  // uniform
  // computeDistinctiveDescriptors
  int N = 0, afirst = -1;
  for (int a = a0; a < a1; ++a) {
    if (!kf_valid || kf_valid[obs_kf[a]]) {
      if (N == 0) afirst = a;
      ++N;
    }
  }
  auto desc_at = [&](int a) { return (const uint4*)(kf_desc + ((size_t)obs_kf[a] * P.NFK + obs_feat[a]) * 32); };
  uint4* dst = (uint4*)(desc_out + (size_t)p * 32);
  if (N >= 1 && N <= 2) {
    const uint4* s = desc_at(afirst);
    dst[0] = s[0];
    dst[1] = s[1];
  }

  // PACKED: batches of whole points, in lane order, as many as fit MP_ROWS rows; a row per observation, the ones of invalid
  // key-frames flagged (no row, no column)
  const int n_all = a1 - a0;
  bool pend = N >= 3 && n_all <= MP_NMAX;
  while (__any(pend)) {
    const int n_take = pend ? n_all : 0;
    int inc = n_take;  // inclusive scan over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    const bool take = pend && inc <= MP_ROWS;  // a prefix of the pending lanes; the first one always fits (n_all <= MP_NMAX)
    const int start = inc - n_take;
    int R = take ? inc : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) R = max(R, __shfl_xor(R, m));
    if (take) {
      for (int i = 0; i < n_all; ++i) {
        S.info[start + i] = start | (n_all << 8) | (N << 16);
        S.obs[start + i] = a0 + i;
      }
    }
    wave_sync();
    for (int r = lane; r < R; r += 64) {  // staging: a row per lane
      const int a = S.obs[r];
      const uint4* s = desc_at(a);
      S.desc[r][0] = s[0];
      S.desc[r][1] = s[1];
      if (!kf_valid || kf_valid[obs_kf[a]]) S.info[r] |= 1 << 24;
    }
    wave_sync();
    for (int r = lane; r < R; r += 64) {
      const int inf = S.info[r], s = inf & 0xff, n = (inf >> 8) & 0xff;
      if (!(inf >> 24)) {
        S.med[r] = 0xffff;  // (never the smallest: the point has N >= 3 valid rows)
        continue;
      }
      const uint4 m0 = S.desc[r][0], m1 = S.desc[r][1];
      for (int j = 0; j < n; ++j)
        S.dist[j][lane] = (S.info[s + j] >> 24) ? (uint16_t)hamming256(m0, m1, S.desc[s + j][0], S.desc[s + j][1]) : (uint16_t)0x7fff;
      const int k = (((inf >> 16) & 0xff) - 1) / 2;  // vDists[0.5 * (N - 1)]: the smallest v with #(d <= v) > k
      int lo = 0, hi = 256;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int cnt = 0;
        for (int j = 0; j < n; ++j) cnt += S.dist[j][lane] <= mid ? 1 : 0;
        if (cnt > k) hi = mid;
        else lo = mid + 1;
      }
      S.med[r] = (uint16_t)lo;
    }
    wave_sync();
    if (take) {
      int best = INT_MAX, bi = 0;
      for (int i = 0; i < n_all; ++i) {
        const int m = S.med[start + i];
        if (m < best) {  // the first of equal medians wins
          best = m;
          bi = i;
        }
      }
      dst[0] = S.desc[start + bi][0];
      dst[1] = S.desc[start + bi][1];
    }
    pend = pend && !take;
    wave_sync();
  }

  // GENERAL: one point at a time by the whole wave
  unsigned long long gmask = __ballot(N >= 3 && n_all > MP_NMAX);
  while (gmask) {
    const int q = __ffsll((long long)gmask) - 1;
    gmask &= gmask - 1;
    const int b0 = __shfl(a0, q), b1 = __shfl(a1, q), nq = __shfl(N, q);
    const int k = (nq - 1) / 2;
    unsigned long long best = ~0ull;  // (median << 32 | observation), the first minimum over the rows
    for (int c0 = b0; c0 < b1; c0 += 64) {
      const int a = c0 + lane;
      bool row = false;
      uint4 m0 = make_uint4(0, 0, 0, 0), m1 = m0;
      if (a < b1) {
        row = !kf_valid || kf_valid[obs_kf[a]];
        const uint4* s = desc_at(a);
        m0 = s[0];
        m1 = s[1];
      }
      int bin = 0, rank = k, med = 0;
      for (int pass = 0; pass < 2; ++pass) {
        for (int h = 0; h < 17; ++h) S.hist[h][lane] = 0;
        for (int t0 = b0; t0 < b1; t0 += MP_ROWS) {
          const int nt = min(MP_ROWS, b1 - t0);
          wave_sync();
          for (int t = lane; t < nt; t += 64) {
            const int at = t0 + t;
            const bool v = !kf_valid || kf_valid[obs_kf[at]];
            S.info[t] = v ? 1 : 0;
            if (v) {
              const uint4* s = desc_at(at);
              S.desc[t][0] = s[0];
              S.desc[t][1] = s[1];
            }
          }
          wave_sync();
          for (int t = 0; t < nt; ++t) {
            if (!S.info[t]) continue;  // the same t in every lane
            const int d = hamming256(m0, m1, S.desc[t][0], S.desc[t][1]);
            if (pass == 0) S.hist[d >> 4][lane] += 1;
            else if ((d >> 4) == bin) S.hist[d & 15][lane] += 1;
          }
        }
        int cum = 0, sel = -1;
        const int nb = pass == 0 ? 17 : 16;
        for (int h = 0; h < nb; ++h) {
          const int c = (int)S.hist[h][lane];
          if (sel < 0) {
            if (cum + c > rank) sel = h;
            else cum += c;
          }
        }
        rank -= cum;
        if (pass == 0) bin = sel;
        else med = bin * 16 + sel;
      }
      const unsigned long long key = row ? ((unsigned long long)(unsigned)med << 32) | (unsigned)a : ~0ull;
      best = key < best ? key : best;
    }
    best = wave_min_u64(best);
    const int aw = (int)(unsigned)(best & 0xffffffffull);
    if (lane < 2) ((uint4*)(desc_out + (size_t)(blockIdx.x * 64 + q) * 32))[lane] = desc_at(aw)[lane];
    wave_sync();
  }
}

}  // namespace

extern "C" int gl_update_map_points(gl_ctx_t* ctx, float scale_factor, int what, int NP, int NKF, int NFK, int NOBS, const double* kf_twc_dev,
                                    const uint8_t* kf_valid_dev, const int32_t* kf_oct_dev, const uint8_t* kf_desc_dev, const double* pos_dev,
                                    const uint8_t* pt_valid_dev, const int32_t* ref_kf_dev, const int32_t* obs_ptr_dev, const int32_t* obs_kf_dev,
                                    const int32_t* obs_feat_dev, uint8_t* desc_dev, double* normal_dev, float* max_dist_dev, float* min_dist_dev) {
  GL_REQUIRE(ctx, "null argument");
  GL_REQUIRE(what >= 1 && what <= 3, "what must be 1 (descriptor), 2 (normal + depth) or 3 (both)");
  GL_REQUIRE(NP >= 0 && NKF >= 0 && NFK >= 0 && NOBS >= 0, "bad NP / NKF / NFK / NOBS");
  if (NP == 0) return GL_OK;
  GL_REQUIRE(obs_ptr_dev, "null obs_ptr");
  GL_REQUIRE(NOBS == 0 || (obs_kf_dev && obs_feat_dev), "null obs_kf / obs_feat");
  if (what & 1) GL_REQUIRE(kf_desc_dev && desc_dev, "what & 1: null kf_desc / desc");
  if (what & 2) {
    GL_REQUIRE(kf_twc_dev && kf_oct_dev && pos_dev && ref_kf_dev && normal_dev && max_dist_dev && min_dist_dev,
               "what & 2: null kf_twc / kf_oct / pos / ref_kf / normal / max_dist / min_dist");
    GL_REQUIRE(std::isfinite(scale_factor) && scale_factor > 0.0f, "bad scale factor");
  }
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  MpP P;
  P.what = what;
  P.NP = NP;
  P.NKF = NKF;
  P.NFK = NFK;
  P.NOBS = NOBS;
  gl_match::pyramid_scales(scale_factor, P.sf, nullptr, nullptr);
  k_update_map_points<<<(unsigned)((NP + 63) / 64), 64, 0, c->stream>>>(P, kf_twc_dev, kf_valid_dev, kf_oct_dev, kf_desc_dev, pos_dev, pt_valid_dev,
                                                                       ref_kf_dev, obs_ptr_dev, obs_kf_dev, obs_feat_dev, desc_dev, normal_dev,
                                                                       max_dist_dev, min_dist_dev);
  GL_HIP(hipGetLastError());
  return GL_OK;
}
