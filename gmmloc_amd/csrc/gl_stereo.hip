// Frame::computeStereoMatches (frame.cpp:179-349) for B frames: gl_stereo_matches.  The rules and the five declared deviations are in
// gmmloc_hip.h; tests/stereo_ref.py is the sequential model every output is compared with, bit for bit.
//
// One workgroup of 1 024 threads per frame, everything a frame needs between its stations in LDS, every output written once at the end:
//   (a) the right key-points as 16-byte records in a CSR by the FIRST row of their band (minr, clamped to the image).  A band is at
//       most `span` rows high, so the candidates of left row y lie in the buckets y - span .. y, which are contiguous in the CSR; each
//       entry's band is tested again on the record.  One entry per key-point (a row table as the reference builds it has ~ 5 - 17).
//       The reference visits a row's list in ascending right index and keeps the first strict minimum, which is the minimum of
//       (distance, index): the order inside the CSR decides nothing.
//   (b) a thread per left feature walks its buckets and keeps min((dist << 12) | iR) over the candidates with dist < 100.
//   (c) sixteen lanes per feature that passed :261 (four features a wave: the station is a chain of dependent loads, not of
//       instructions): a lane holds eight of the 121 window positions and forms its part of the eleven sums, the sixteen add them up,
//       every lane decides alike and the first keeps the result.
//   (d) the SAD at position n / 2 by two 256-bin histograms over the 16-bit SADs, then the reset pass and the stores.
// All float arithmetic below is single operations in source order (-ffp-contract=off); the two divisions go through double: the
// quotient of two floats rounded to double and then to float is the correctly rounded float quotient (53 >= 2 x 24 + 2).
#include "gl_device.hpp"
#include "gl_internal.hpp"
#include "gl_map_dev.hpp"  // block_excl_scan
#include "gl_match_common.hpp"

using gl_match::hamming256;

namespace {

constexpr int ST_T = 1024;  // threads of a frame's workgroup
constexpr int TH_HIGH = 100, TH_LOW = 50, TH_DESC = (TH_HIGH + TH_LOW) / 2;  // ORBmatcher::TH_HIGH / TH_LOW, th_desc_dist (:183)
constexpr int W = 5, L = 5;  // the window's half size (:270), the slide (:279)
constexpr int SAD_LANES = 16;  // lanes that share a feature's correlation
static_assert(GL_STEREO_MATCH_MAX <= 4096, "a right index is the low 12 bits of a key");

struct Levels {  // one pyramid's geometry
  int32_t width[8], height[8];
  int64_t stride[8], offset[8];
};
struct StereoArgs {
  float sf[8], sf_inv[8];  // frame::scale_factors / scale_factors_inv
  float mbf, maxD;         // (float)bf, mbf / mb (:210)
  int H, nlevels, span;    // camera::height; the levels; the most rows a band covers beyond its first
  int NF, NR;
  Levels lv[2];            // left, right
  int64_t frame_stride[2];
  const uint8_t* data[2];
};
struct Tables {  // what a kernel argument cannot be indexed for without a copy: the level tables, in LDS
  float sf[8], sf_inv[8];
  Levels lv[2];
};

__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }

// the record of right key-point iR: {uR bits, first row, last row, octave | iR << 8}; false: it takes no part (deviations 1 and 3)
__device__ __forceinline__ bool right_record(const Tables& t, int nlevels, int H, const float* __restrict__ r_uv,
                                             const int32_t* __restrict__ r_oct, int iR, int4* rec) {
  const int oct = r_oct[iR];
  if (oct < 0 || oct >= nlevels) return false;
  const float kpY = r_uv[2 * iR + 1];
  const float r = 2.0f * t.sf[oct];                           // :198
  const float maxr = ceilf(kpY + r), minr = floorf(kpY - r);  // :199-200
  if (!(maxr >= 0.0f && minr < (float)H)) return false;       // no row inside the image (or NaN)
  const int lo = minr < 0.0f ? 0 : (int)minr, hi = maxr > (float)(H - 1) ? H - 1 : (int)maxr;
  *rec = make_int4(__float_as_int(r_uv[2 * iR]), lo, hi, oct | (iR << 8));
  return true;
}

__global__ __launch_bounds__(ST_T) void k_stereo_matches(const StereoArgs A, const double* __restrict__ feat_uv_,
                                                         const int32_t* __restrict__ feat_oct_, const uint8_t* __restrict__ feat_desc_,
                                                         const float* __restrict__ r_uv_, const int32_t* __restrict__ r_oct_,
                                                         const uint8_t* __restrict__ r_desc_, const int32_t* __restrict__ n_left,
                                                         const int32_t* __restrict__ n_right, float* __restrict__ out_ur,
                                                         float* __restrict__ out_depth, int32_t* __restrict__ out_match,
                                                         int32_t* __restrict__ out_sad, int32_t* __restrict__ out_stat) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ Tables t;
  __shared__ int s_hist[256], s_w[ST_T / 64], s_cnt[4], s_sel[2];
  const int tid = threadIdx.x, b = blockIdx.x, lane = tid & (SAD_LANES - 1), group = tid / SAD_LANES;
  const int NF = A.NF, NR = A.NR, H = A.H, nlevels = A.nlevels;
  int4* s_rec = (int4*)lds;                 // NR
  int* s_match = (int*)(s_rec + NR);        // NF: the right index, -1
  int* s_sad = s_match + NF;                // NF
  float* s_ur = (float*)(s_sad + NF);       // NF
  float* s_depth = s_ur + NF;               // NF
  int* s_ptr = (int*)(s_depth + NF);        // H + 1
  int* s_cur = s_ptr + H + 1;               // H

  const double* feat_uv = feat_uv_ + (size_t)b * NF * 2;
  const int32_t* feat_oct = feat_oct_ + (size_t)b * NF;
  const uint4* feat_desc = (const uint4*)(feat_desc_ + (size_t)b * NF * 32);
  const float* r_uv = r_uv_ + (size_t)b * NR * 2;
  const int32_t* r_oct = r_oct_ + (size_t)b * NR;
  const uint4* r_desc = (const uint4*)(r_desc_ + (size_t)b * NR * 32);
  const int nL = n_left ? min(max(n_left[b], 0), NF) : NF, nR = n_right ? min(max(n_right[b], 0), NR) : NR;

  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      t.sf[k] = A.sf[k];
      t.sf_inv[k] = A.sf_inv[k];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        t.lv[s].width[k] = A.lv[s].width[k];
        t.lv[s].height[k] = A.lv[s].height[k];
        t.lv[s].stride[k] = A.lv[s].stride[k];
        t.lv[s].offset[k] = A.lv[s].offset[k];
      }
    }
  }
  if (tid < 4) s_cnt[tid] = 0;
  if (tid < 2) s_sel[tid] = 0;
  for (int c = tid; c <= H; c += ST_T) s_ptr[c] = 0;
  for (int c = tid; c < H; c += ST_T) s_cur[c] = 0;
  for (int i = tid; i < NF; i += ST_T) {
    s_match[i] = -1;
    s_sad[i] = -1;
    s_ur[i] = -1.0f;
    s_depth[i] = -1.0f;
  }
  __syncthreads();

  // ---- (a) the row table (:187-205) as a CSR by first row
  for (int iR = tid; iR < nR; iR += ST_T) {
    int4 rec;
    if (right_record(t, nlevels, H, r_uv, r_oct, iR, &rec)) atomicAdd(&s_ptr[rec.y + 1], 1);
  }
  __syncthreads();
  {
    const int ch = (H + ST_T - 1) / ST_T, c0 = min(tid * ch, H), c1 = min(c0 + ch, H);
    int sum = 0, total;
    for (int c = c0; c < c1; ++c) sum += s_ptr[c + 1];
    int run = gl::mapdev::block_excl_scan<ST_T, int>(sum, s_w, tid, &total);
    for (int c = c0; c < c1; ++c) {  // s_ptr[c + 1]: the end of bucket c; s_ptr[c] (the end of c - 1) is its start
      run += s_ptr[c + 1];
      s_ptr[c + 1] = run;
    }
  }
  __syncthreads();
  for (int iR = tid; iR < nR; iR += ST_T) {
    int4 rec;
    if (right_record(t, nlevels, H, r_uv, r_oct, iR, &rec)) s_rec[s_ptr[rec.y] + atomicAdd(&s_cur[rec.y], 1)] = rec;
  }
  __syncthreads();

  // ---- (b) the descriptor search (:217-261)
  for (int iL = tid; iL < nL; iL += ST_T) {
    const int levelL = feat_oct[iL];
    if (levelL < 0 || levelL >= nlevels) continue;                   // deviation 3
    const float vL = (float)feat_uv[2 * iL + 1], uL = (float)feat_uv[2 * iL];  // :220-221
    if (!(vL >= 0.0f && vL < (float)H)) continue;                    // deviation 2 (and NaN)
    const int row = (int)vL;                                         // :223, (size_t)vL
    const float minU = uL - A.maxD, maxU = uL;                       // :228-229, minD = 0
    if (maxU < 0.0f) continue;                                       // :231
    const uint4 d0 = feat_desc[2 * iL], d1 = feat_desc[2 * iL + 1];
    const uint32_t dl[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
    int best = INT_MAX;
    const int e1 = s_ptr[row + 1];
    for (int e = s_ptr[max(row - A.span, 0)]; e < e1; ++e) {
      const int4 rec = s_rec[e];
      if (row < rec.y || row > rec.z) continue;                      // :202, the band
      const int oct = rec.w & 0xff, iR = rec.w >> 8;
      if (oct < levelL - 1 || oct > levelL + 1) continue;            // :244
      const float uR = __int_as_float(rec.x);
      if (uR >= minU && uR <= maxU) {                                // :249
        const int dist = hamming256(dl, r_desc[2 * iR], r_desc[2 * iR + 1]);
        if (dist < TH_HIGH) best = min(best, (dist << 12) | iR);     // :253, first strict minimum in ascending iR
      }
    }
    if (best != INT_MAX && (best >> 12) < TH_DESC) {                 // :261
      s_match[iL] = best & 0xfff;
      atomicAdd(&s_cnt[0], 1);
    }
  }
  __syncthreads();

  // ---- (c) sub-pixel match by correlation (:262-333), SAD_LANES lanes per feature; every branch below is uniform over those lanes
  for (int iL = group; iL < nL; iL += ST_T / SAD_LANES) {
    const int iR0 = s_match[iL];
    if (iR0 < 0) continue;
    const int l = feat_oct[iL];
    const double ux = feat_uv[2 * iL], vy = feat_uv[2 * iL + 1];
    const float uL = (float)ux;
    const float uR0 = r_uv[2 * iR0];                                 // :263
    const float inv = t.sf_inv[l];                                   // :264
    const float scaleduL = (float)round(ux * (double)inv), scaledvL = (float)round(vy * (double)inv);  // :265-266, double products
    const float scaleduR0 = roundf(uR0 * inv);                       // :267, a float product
    const int wl = t.lv[0].width[l], hl = t.lv[0].height[l], wr = t.lv[1].width[l], hr = t.lv[1].height[l];
    // :284-287 (iniu = scaleduR0, endu = scaleduR0 + 11) and deviation 4: every window inside its level image
    const bool inside = !(scaleduR0 < 0.0f || scaleduR0 + (float)(L + W + 1) >= (float)wr) &&
                        scaledvL - (float)W >= 0.0f && scaledvL + (float)W < (float)min(hl, hr) &&
                        scaleduL - (float)W >= 0.0f && scaleduL + (float)W < (float)wl &&
                        scaleduR0 - (float)(L + W) >= 0.0f && scaleduR0 + (float)(L + W) < (float)wr;
    if (!inside) {
      if (lane == 0) s_match[iL] = -1;
      continue;
    }
    const int cu = (int)scaleduL, cv = (int)scaledvL, cr = (int)scaleduR0;
    const uint8_t* IL = A.data[0] + (size_t)b * A.frame_stride[0] + t.lv[0].offset[l];
    const uint8_t* IR = A.data[1] + (size_t)b * A.frame_stride[1] + t.lv[1].offset[l];
    const int64_t sl = t.lv[0].stride[l], sr = t.lv[1].stride[l];
    const int centreL = IL[cv * sl + cu];                            // :275
    int centreR[2 * L + 1], sum[2 * L + 1];
#pragma unroll
    for (int k = 0; k <= 2 * L; ++k) {
      centreR[k] = IR[cv * sr + cr + k - L];                         // :295
      sum[k] = 0;
    }
#pragma unroll
    for (int h = 0; h < ((2 * W + 1) * (2 * W + 1) + SAD_LANES - 1) / SAD_LANES; ++h) {
      const int p = lane + SAD_LANES * h;
      if (p < (2 * W + 1) * (2 * W + 1)) {
        const int py = p / (2 * W + 1), px = p - py * (2 * W + 1);
        const int a = (int)IL[(cv - W + py) * sl + (cu - W + px)] - centreL;
        const uint8_t* rrow = IR + (cv - W + py) * sr + (cr - L - W + px);
#pragma unroll
        for (int k = 0; k <= 2 * L; ++k) sum[k] += abs(a - ((int)rrow[k] - centreR[k]));  // :297, NORM_L1
      }
    }
    int bestDist = INT_MAX, bestinc = 0;
#pragma unroll
    for (int k = 0; k <= 2 * L; ++k) {
#pragma unroll
      for (int o = SAD_LANES / 2; o >= 1; o >>= 1) sum[k] += __shfl_xor(sum[k], o, 64);
      if (sum[k] < bestDist) {                                       // :298, first strict minimum
        bestDist = sum[k];
        bestinc = k - L;
      }
    }
    bool keep = !(bestinc == -L || bestinc == L);                    // :306
    int i1 = 0, i2 = 0, i3 = 0;
#pragma unroll
    for (int k = 0; k <= 2 * L; ++k) {
      i1 = k == bestinc + L - 1 ? sum[k] : i1;
      i2 = k == bestinc + L ? sum[k] : i2;
      i3 = k == bestinc + L + 1 ? sum[k] : i3;
    }
    float ur = -1.0f, depth = -1.0f;
    if (keep) {
      const float dist1 = (float)i1, dist2 = (float)i2, dist3 = (float)i3;  // :309-311
      const float deltaR = div_rn(dist1 - dist3, 2.0f * (dist1 + dist3 - 2.0f * dist2));  // :313-314
      keep = !(deltaR < -1.0f || deltaR > 1.0f);                     // :316 (NaN goes on, as there)
      float bestuR = t.sf[l] * ((scaleduR0 + (float)bestinc) + deltaR);  // :320-321
      float disparity = uL - bestuR;                                 // :323
      keep = keep && disparity >= 0.0f && disparity < A.maxD;        // :325
      if (disparity <= 0.0f) {                                       // :326-329
        disparity = 0.01f;
        bestuR = (float)((double)uL - 0.01);
      }
      depth = div_rn(A.mbf, disparity);                              // :330
      ur = bestuR;                                                   // :331
    }
    if (lane == 0) {
      if (keep) {
        s_sad[iL] = bestDist;                                        // :332
        s_ur[iL] = ur;
        s_depth[iL] = depth;
      } else {
        s_match[iL] = -1;
      }
    }
  }
  __syncthreads();

  // ---- (d) the median rule (:337-348): the SAD at position n / 2 of the ascending list, by its high and then its low byte
  int median = -1;
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = tid; i < 256; i += ST_T) s_hist[i] = 0;
    __syncthreads();
    const int hi = s_sel[0];  // (pass 1)
    for (int i = tid; i < nL; i += ST_T) {
      const int s = s_sad[i];
      if (s < 0) continue;
      if (pass == 0) atomicAdd(&s_hist[(s >> 8) & 0xff], 1);
      else if ((s >> 8) == hi) atomicAdd(&s_hist[s & 0xff], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int n = 0, k = s_sel[1];
      if (pass == 0) {
        for (int i = 0; i < 256; ++i) n += s_hist[i];
        s_cnt[1] = n;
        k = n / 2;                                                   // :338
      }
      int bin = -1;
      for (int i = 0; i < 256 && bin < 0; ++i) {
        if (k < s_hist[i]) bin = i;
        else k -= s_hist[i];
      }
      bin = max(bin, 0);  // (an empty list: nothing reads the value)
      s_sel[0] = pass == 0 ? bin : ((s_sel[0] << 8) | bin);
      s_sel[1] = k;
    }
    __syncthreads();
  }
  const int n_list = s_cnt[1];
  if (n_list > 0) median = s_sel[0];                                 // deviation 5: an empty list changes nothing
  const float thDist = (1.5f * 1.4f) * (float)median;                // :339
  for (int i = tid; i < NF; i += ST_T) {
    const int s = s_sad[i];
    float ur = s_ur[i], depth = s_depth[i];
    if (s >= 0 && n_list > 0 && !((float)s < thDist)) {              // :342-347
      ur = -1.0f;
      depth = -1.0f;
      atomicAdd(&s_cnt[2], 1);
    }
    out_ur[(size_t)b * NF + i] = ur;
    out_depth[(size_t)b * NF + i] = depth;
    if (out_match) out_match[(size_t)b * NF + i] = s_match[i];
    if (out_sad) out_sad[(size_t)b * NF + i] = s;
  }
  __syncthreads();
  if (out_stat && tid < 4) out_stat[(size_t)b * 4 + tid] = tid == 3 ? median : s_cnt[tid];
}

size_t stereo_lds(int NF, int NR, int H) { return (size_t)NR * 16 + (size_t)NF * 16 + ((size_t)2 * H + 1) * 4; }

int check_pyramid(const gl_image_pyramid* p, const char* which) {
  if (!p->data || p->nlevels < 1 || p->nlevels > 8 || p->frame_stride < 0) {
    gl::set_error("gl_stereo_matches: %s pyramid: null data, nlevels outside 1 .. 8 or a negative frame stride", which);
    return GL_ERR_ARG;
  }
  for (int l = 0; l < p->nlevels; ++l)
    if (p->width[l] < 1 || p->height[l] < 1 || p->stride[l] < p->width[l] || p->offset[l] < 0) {
      gl::set_error("gl_stereo_matches: %s pyramid, level %d: width / height < 1, stride < width or a negative offset", which, l);
      return GL_ERR_ARG;
    }
  return GL_OK;
}

}  // namespace

extern "C" {

int gl_stereo_matches(gl_ctx_t* ctx, const gl_camera* cam, double scale_factor, int B, int NF, int NR, const gl_stereo_in* in,
                      const gl_image_pyramid* left, const gl_image_pyramid* right, const gl_stereo_out* out) {
  GL_REQUIRE(ctx && cam && in && left && right && out, "null argument");
  GL_REQUIRE(B >= 1 && NF >= 1 && NR >= 1, "bad B / NF / NR");
  GL_REQUIRE(NF <= GL_STEREO_MATCH_MAX && NR <= GL_STEREO_MATCH_MAX, "more than GL_STEREO_MATCH_MAX left features or right key-points per frame");
  GL_REQUIRE(in->feat_uv && in->feat_oct && in->feat_desc && in->r_uv && in->r_oct && in->r_desc, "null input buffer");
  GL_REQUIRE(out->feat_ur && out->feat_depth, "null output buffer (match_r, sad and stat are optional)");
  GL_REQUIRE(cam->height >= 1, "camera height not set");
  if (int rc = check_pyramid(left, "left")) return rc;
  if (int rc = check_pyramid(right, "right")) return rc;
  GL_REQUIRE(left->nlevels == right->nlevels, "the two pyramids differ in their number of levels");
  gl::Ctx* c = gl::C(ctx);
  StereoArgs A = {};
  gl_match::pyramid_scales((float)scale_factor, A.sf, nullptr, nullptr);
  for (int l = 0; l < 8; ++l) A.sf_inv[l] = l == 0 ? 1.0f : 1.0f / A.sf[l];  // init_config.hpp:69,76
  A.mbf = (float)cam->bf;                            // frame.cpp:23
  const float mb = (float)(cam->bf / cam->fx);       // frame.cpp:24
  A.maxD = A.mbf / mb;                               // :208-210
  A.H = cam->height;
  A.nlevels = left->nlevels;
  {  // a band: floor(y - r) .. ceil(y + r), at most 2 r + 2 rows beyond its first
    const double r = 2.0 * (double)A.sf[A.nlevels - 1];
    A.span = r < (double)A.H ? (int)ceil(2.0 * r) + 2 : A.H;
  }
  A.NF = NF;
  A.NR = NR;
  const gl_image_pyramid* pyr[2] = {left, right};
  for (int s = 0; s < 2; ++s) {
    for (int l = 0; l < 8; ++l) {
      const bool have = l < A.nlevels;
      A.lv[s].width[l] = have ? pyr[s]->width[l] : 0;
      A.lv[s].height[l] = have ? pyr[s]->height[l] : 0;
      A.lv[s].stride[l] = have ? pyr[s]->stride[l] : 0;
      A.lv[s].offset[l] = have ? pyr[s]->offset[l] : 0;
    }
    A.frame_stride[s] = pyr[s]->frame_stride;
    A.data[s] = pyr[s]->data;
  }
  const size_t lds = stereo_lds(NF, NR, A.H);
  GL_REQUIRE_LDS(c, lds + sizeof(Tables) + 2048);
  GL_HIP(hipSetDevice(c->device));
  GL_HIP(gl::ensure_dynamic_lds(c, (const void*)k_stereo_matches, lds));
  k_stereo_matches<<<B, ST_T, lds, c->stream>>>(A, in->feat_uv, in->feat_oct, in->feat_desc, in->r_uv, in->r_oct, in->r_desc, in->n_left,
                                               in->n_right, out->feat_ur, out->feat_depth, out->match_r, out->sad, out->stat);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

}  // extern "C"
