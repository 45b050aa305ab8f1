// The regular half of ORBextractor (orb_extractor.cpp) for B images: gl_orb_describe.  The rules and the three declared deviations are
// in gmmloc_hip.h; tests/orb_ref.py is the sequential model every output is compared with, bit for bit.
//
//   k_orb_blur      the 7 x 7 blur of every level (:1029-1030) into the context's main scratch block, same geometry, tightly packed.
//                   One workgroup per 64 x 32 tile of a level: the tile with its 3-px halo (BORDER_REFLECT_101 by index, so the halo
//                   of a tile at the image's edge is the image's own pixels) as bytes in LDS, the row pass from there into LDS words
//                   (uint16 while 255 x the taps' sum fits, which it does for a sum of up to 257; uint32 above), the column pass out of
//                   LDS, eight rows a thread from fourteen values read once.  A level too small to hold a key-point (under 39 px) is
//                   left out; every byte k_orb_describe can read is written here first.
//   k_orb_describe  thirty-two lanes per key-point, eight key-points a workgroup.  The moments (:78-98): lane u + 15 walks column u of
//                   the patch on the UNBLURRED level, the thirty-two add up.  The 512 reads of the blurred level (:112-143): the
//                   pattern in LDS as one word per pair, laid out so that the lanes of a read hit different banks; lane i builds byte
//                   i, four lanes' bytes leave as one word.  Lane 0 stores the rest.  Every output is stored once.
// All float arithmetic below is single operations in source order (-ffp-contract=off); the division of fastAtan2 goes through double:
// the quotient of two floats rounded to double and then to float is the correctly rounded float quotient (53 >= 2 x 24 + 2).
#include <cfloat>

#include "gl_device.hpp"
#include "gl_internal.hpp"

namespace {

constexpr int HALF_PATCH = 15, EDGE = 19, REACH = 13;  // HALF_PATCH_SIZE, EDGE_THRESHOLD (:74-75); the pattern's largest coordinate
constexpr int SPAN = 18;                               // cvRound(13 sqrt 2): the farthest row / column a sample is read at
constexpr int BL_TW = 64, BL_TH = 32, BL_T = 256, HALO = 3;
constexpr int KP_LANES = 32, DS_T = 256, KP_PER_BLOCK = DS_T / KP_LANES;
// umax of :449-463 for HALF_PATCH_SIZE = 15 (749 pixels)
__device__ constexpr int UMAX[HALF_PATCH + 1] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};

struct OrbArgs {
  int32_t width[8], height[8];
  int64_t stride[8], offset[8];  // of the input pyramid
  int64_t boffset[8];            // of the blurred one (stride = width)
  int32_t tile0[8], tiles_x[8];  // k_orb_blur: a level's first tile and its tiles per row
  float sf[8];                   // mvScaleFactor (:413-416)
  int32_t w[4];                  // the blur's taps, centre first
  int nlevels, N;
  int64_t frame_stride, bframe_stride;
  const uint8_t* data;
  uint8_t* blurred;
};

// a[l] for a level that is not known at compile time, without indexing a kernel argument (which would make a copy of it)
template <typename T>
__device__ __forceinline__ T pick(const T (&a)[8], int l) {
  T v = a[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) v = k == l ? a[k] : v;
  return v;
}

// BORDER_REFLECT_101 by index (-1 -> 1, n -> n - 2) for n >= 4 and the indices a tile can need, -3 .. n + 2; an index beyond them
// (a tile that hangs over the level's edge) is first brought to the nearest of them: only outputs outside the level would read it
__device__ __forceinline__ int reflect101(int i, int n) {
  i = min(max(i, -HALO), n - 1 + HALO);
  i = i < 0 ? -i : i;
  return i >= n ? 2 * n - 2 - i : i;
}

template <typename RowT>
__global__ __launch_bounds__(BL_T) void k_orb_blur(const OrbArgs A) {
  constexpr int IN_H = BL_TH + 2 * HALO, PASSES = (IN_H + BL_T / BL_TW - 1) / (BL_T / BL_TW), ROWS = BL_TH * BL_TW / BL_T;
  __shared__ uint8_t s_in[IN_H][BL_TW + 2 * HALO + 2];
  __shared__ RowT s_row[IN_H][BL_TW];
  const int tid = threadIdx.x, b = blockIdx.y, tx = tid % BL_TW, ty = tid / BL_TW;
  int l = 0;
#pragma unroll
  for (int k = 1; k < 8; ++k) l += (k < A.nlevels && (int)blockIdx.x >= A.tile0[k]) ? 1 : 0;
  const int w = pick(A.width, l), h = pick(A.height, l), tiles_x = pick(A.tiles_x, l), t = (int)blockIdx.x - pick(A.tile0, l);
  const int ty0 = (t / tiles_x) * BL_TH, tx0 = (t % tiles_x) * BL_TW;
  const int64_t stride = pick(A.stride, l);
  const uint8_t* I = A.data + (int64_t)b * A.frame_stride + pick(A.offset, l);
  uint8_t* O = A.blurred + (int64_t)b * A.bframe_stride + pick(A.boffset, l);
  {  // the tile's own columns: a thread keeps its column, four rows a pass, the loads of all passes in flight together
    const int gx = reflect101(tx0 + tx, w);
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
      const int r = ty + k * (BL_T / BL_TW);
      if (r < IN_H) s_in[r][tx + HALO] = I[reflect101(ty0 + r - HALO, h) * stride + gx];
    }
    if (tid < IN_H * 2 * HALO) {  // the halo columns
      const int r = tid / (2 * HALO), j = tid % (2 * HALO), c = j < HALO ? j : BL_TW + j;
      s_in[r][c] = I[reflect101(ty0 + r - HALO, h) * stride + reflect101(tx0 + c - HALO, w)];
    }
  }
  __syncthreads();
  const int w0 = A.w[0], w1 = A.w[1], w2 = A.w[2], w3 = A.w[3];
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const int r = ty + k * (BL_T / BL_TW);
    if (r < IN_H) {
      const uint8_t* p = &s_in[r][tx + HALO];
      s_row[r][tx] = (RowT)(w0 * p[0] + w1 * (p[-1] + p[1]) + w2 * (p[-2] + p[2]) + w3 * (p[-3] + p[3]));
    }
  }
  __syncthreads();
  const int r0 = ty * ROWS, x = tx0 + tx;
  int v[ROWS + 2 * HALO];  // the column's row-pass values around the thread's rows, read once
#pragma unroll
  for (int j = 0; j < ROWS + 2 * HALO; ++j) v[j] = (int)s_row[r0 + j][tx];
  if (x >= w) return;
#pragma unroll
  for (int k = 0; k < ROWS; ++k) {
    const int y = ty0 + r0 + k;
    const int s = w0 * v[k + 3] + w1 * (v[k + 2] + v[k + 4]) + w2 * (v[k + 1] + v[k + 5]) + w3 * (v[k] + v[k + 6]);
    if (y < h) O[(int64_t)y * w + x] = (uint8_t)min((s + (1 << 15)) >> 16, 255);
  }
}

__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }

// cv::fastAtan2 as gmmloc_hip.h declares it
__device__ __forceinline__ float fast_atan2_deg(float y, float x) {
  constexpr float S = (float)(180.0 / 3.14159265358979323846);
  constexpr float P1 = 0.9997878412794807f * S, P3 = -0.3258083974640975f * S, P5 = 0.1555786518463281f * S, P7 = -0.04432655554792128f * S;
  const float ax = fabsf(x), ay = fabsf(y);
  const bool steep = ay > ax;
  const float c = div_rn(steep ? ax : ay, (steep ? ay : ax) + (float)DBL_EPSILON), c2 = c * c;
  float a = (((P7 * c2 + P5) * c2 + P3) * c2 + P1) * c;
  if (steep) a = 90.0f - a;
  if (x < 0.0f) a = 180.0f - a;
  if (y < 0.0f) a = 360.0f - a;
  return a;
}

// deviations 1 and 2: the key-point is described
__device__ __forceinline__ bool kp_live(const OrbArgs& A, int x, int y, int oct) {
  if (oct < 0 || oct >= A.nlevels) return false;
  const int w = pick(A.width, oct), h = pick(A.height, oct);
  return x >= EDGE && x <= w - 1 - EDGE && y >= EDGE && y <= h - 1 - EDGE;
}

// the blurred pixel of pattern entry (px, py) steered by (a, b) (:112-114), relative to the key-point at `centre`
__device__ __forceinline__ int steered(const uint8_t* centre, int w, int px, int py, float a, float b) {
  const float fx = (float)px, fy = (float)py;
  const int row = __float2int_rn(fx * b + fy * a), col = __float2int_rn(fx * a - fy * b);  // cvRound: half to even
  // (no effect for a finite angle: |row|, |col| <= 18 then; an angle that is not finite reads the centre instead of leaving the image)
  return centre[min(max(row, -SPAN), SPAN) * w + min(max(col, -SPAN), SPAN)];
}

__global__ __launch_bounds__(DS_T) void k_orb_describe(const OrbArgs A, const int32_t* __restrict__ kp_xy, const int32_t* __restrict__ kp_oct,
                                                       const int32_t* __restrict__ n_kp, const float* __restrict__ kp_angle,
                                                       const int8_t* __restrict__ pattern, uint32_t* __restrict__ out_desc,
                                                       float* __restrict__ out_angle, int32_t* __restrict__ out_moments,
                                                       float* __restrict__ out_uv32, double* __restrict__ out_uv64, int32_t* __restrict__ out_stat) {
  __shared__ char4 s_pat[256];  // pair q = 8 i + j (samples 2 q, 2 q + 1) at [j * 32 + i]: lane i reads [j * 32 + i]
  __shared__ int s_red[DS_T / 64][2];
  const int tid = threadIdx.x, b = blockIdx.y, lane = tid % KP_LANES, slot = blockIdx.x * KP_PER_BLOCK + tid / KP_LANES, N = A.N;
  {
    const int q = tid;  // DS_T == 256 pairs
    char4 p;
    p.x = (char)min(max((int)pattern[4 * q], -REACH), REACH);      // deviation 3: checked on the host when the pointer is new
    p.y = (char)min(max((int)pattern[4 * q + 1], -REACH), REACH);
    p.z = (char)min(max((int)pattern[4 * q + 2], -REACH), REACH);
    p.w = (char)min(max((int)pattern[4 * q + 3], -REACH), REACH);
    s_pat[(q % 8) * 32 + q / 8] = p;
  }
  __syncthreads();
  const int n = n_kp ? min(max(n_kp[b], 0), N) : N;
  if (slot < N) {  // (uniform over a key-point's lanes, as is every branch below)
    const size_t at = (size_t)b * N + slot;
    int x = 0, y = 0, oct = -1;
    if (slot < n) {
      x = kp_xy[2 * at];
      y = kp_xy[2 * at + 1];
      oct = kp_oct[at];
    }
    const bool live = slot < n && kp_live(A, x, y, oct);
    const int w = live ? pick(A.width, oct) : 0;
    int m10 = 0, m01 = 0;
    if (live && !kp_angle && lane <= 2 * HALF_PATCH) {  // :78-98
      const int64_t stride = pick(A.stride, oct);
      const uint8_t* centre = A.data + (int64_t)b * A.frame_stride + pick(A.offset, oct) + y * stride + x;
      const int u = lane - HALF_PATCH, au = abs(u);
#pragma unroll
      for (int v = -HALF_PATCH; v <= HALF_PATCH; ++v)
        if (au <= UMAX[v < 0 ? -v : v]) {
          const int val = centre[v * stride + u];
          m10 += u * val;
          m01 += v * val;
        }
    }
#pragma unroll
    for (int o = KP_LANES / 2; o >= 1; o >>= 1) {
      m10 += __shfl_xor(m10, o, KP_LANES);
      m01 += __shfl_xor(m01, o, KP_LANES);
    }
    float ang = -1.0f;
    uint32_t byte = 0;
    if (live) {
      ang = kp_angle ? kp_angle[at] : fast_atan2_deg((float)m01, (float)m10);  // :100
      const float rad = ang * (float)(3.1415926535897932384626433832795 / 180.f);  // :103, :106
      const float ca = (float)cos((double)rad), sb = (float)sin((double)rad);  // the correctly rounded float cos / sin (:107 calls libm's cosf / sinf: the header's `steering` row)
      const uint8_t* centre = A.blurred + (int64_t)b * A.bframe_stride + pick(A.boffset, oct) + (int64_t)y * w + x;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const char4 p = s_pat[j * 32 + lane];
        const int t0 = steered(centre, w, p.x, p.y, ca, sb), t1 = steered(centre, w, p.z, p.w, ca, sb);
        byte |= (uint32_t)(t0 < t1) << j;  // :116-143
      }
    }
    const uint32_t word = byte | (__shfl_down(byte, 1, KP_LANES) << 8) | (__shfl_down(byte, 2, KP_LANES) << 16) | (__shfl_down(byte, 3, KP_LANES) << 24);
    if (lane % 4 == 0) out_desc[at * 8 + lane / 4] = word;
    if (lane == 0) {
      const float s = live && oct != 0 ? pick(A.sf, oct) : 1.0f;  // :1039-1046
      const float u32 = live ? (float)x * s : -1.0f, v32 = live ? (float)y * s : -1.0f;
      if (out_angle) out_angle[at] = ang;
      if (out_moments) {
        out_moments[2 * at] = m10;
        out_moments[2 * at + 1] = m01;
      }
      if (out_uv32) {
        out_uv32[2 * at] = u32;
        out_uv32[2 * at + 1] = v32;
      }
      if (out_uv64) {
        out_uv64[2 * at] = (double)u32;
        out_uv64[2 * at + 1] = (double)v32;
      }
    }
  }
  if (out_stat && blockIdx.x == 0) {  // the frame's first workgroup counts; nothing is added up in global memory
    int described = 0, skipped = 0;
    for (int i = tid; i < n; i += DS_T) {
      const size_t at = (size_t)b * N + i;
      const bool live = kp_live(A, kp_xy[2 * at], kp_xy[2 * at + 1], kp_oct[at]);
      described += live;
      skipped += !live;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      described += __shfl_xor(described, o, 64);
      skipped += __shfl_xor(skipped, o, 64);
    }
    if (tid % 64 == 0) {
      s_red[tid / 64][0] = described;
      s_red[tid / 64][1] = skipped;
    }
    __syncthreads();
    if (tid < 2) {
      int sum = 0;
      for (int k = 0; k < DS_T / 64; ++k) sum += s_red[k][tid];
      out_stat[(size_t)b * 2 + tid] = sum;
    }
  }
}

}  // namespace

extern "C" {

int gl_orb_default_blur(double sigma, int32_t* w) {
  GL_REQUIRE(w, "null argument");
  GL_REQUIRE(std::isfinite(sigma) && sigma > 0.0, "sigma must be finite and positive");
  double g[4], sum = 0.0;
  for (int i = 0; i < 4; ++i) {
    g[i] = exp(-(double)(i * i) / (2.0 * sigma * sigma));
    sum += i == 0 ? g[i] : 2.0 * g[i];
  }
  int32_t t[4] = {256, 0, 0, 0};
  for (int i = 1; i < 4; ++i) {
    t[i] = (int32_t)nearbyint(256.0 * (g[i] / sum));
    t[0] -= 2 * t[i];
  }
  GL_REQUIRE(t[0] >= 0, "the rounded side taps leave a negative centre");
  for (int i = 0; i < 4; ++i) w[i] = t[i];
  return GL_OK;
}

int gl_orb_describe(gl_ctx_t* ctx, int B, int N, const gl_orb_in* in, const gl_image_pyramid* pyr, const gl_orb_out* out) {
  GL_REQUIRE(ctx && in && pyr && out, "null argument");
  GL_REQUIRE(B >= 1 && B <= 65535 && N >= 1, "bad B / N");
  GL_REQUIRE(N <= GL_ORB_MAX, "more than GL_ORB_MAX key-points per image");
  GL_REQUIRE(in->kp_xy && in->kp_oct && in->pattern && in->blur_w, "null input buffer (n_kp and kp_angle are optional)");
  GL_REQUIRE(out->desc, "null output buffer (all but desc are optional)");
  GL_REQUIRE(std::isfinite(in->scale_factor) && in->scale_factor > 0.0, "bad scale factor");
  GL_REQUIRE(pyr->data && pyr->nlevels >= 1 && pyr->nlevels <= 8 && pyr->frame_stride >= 0,
             "pyramid: null data, nlevels outside 1 .. 8 or a negative frame stride");
  for (int l = 0; l < pyr->nlevels; ++l)
    GL_REQUIRE(pyr->width[l] >= 1 && pyr->height[l] >= 1 && pyr->stride[l] >= pyr->width[l] && pyr->offset[l] >= 0,
               "pyramid: a level with width / height < 1, stride < width or a negative offset");
  int wsum = 0;
  for (int i = 0; i < 4; ++i) {
    GL_REQUIRE(in->blur_w[i] >= 0 && in->blur_w[i] <= 512, "blur_w: a tap outside 0 .. 512");
    wsum += (i == 0 ? 1 : 2) * in->blur_w[i];
  }
  GL_REQUIRE(wsum >= 1 && wsum <= 512, "blur_w: the seven taps must sum to 1 .. 512");
  gl::Ctx* c = gl::C(ctx);
  OrbArgs A = {};
  int64_t bytes = 0;
  int tiles = 0;
  float s = 1.0f;
  for (int l = 0; l < 8; ++l) {
    if (l > 0) s = (float)((double)s * in->scale_factor);  // :416: float times the extractor's DOUBLE scaleFactor
    A.sf[l] = s;
    const bool have = l < pyr->nlevels;
    A.width[l] = have ? pyr->width[l] : 0;
    A.height[l] = have ? pyr->height[l] : 0;
    A.stride[l] = have ? pyr->stride[l] : 0;
    A.offset[l] = have ? pyr->offset[l] : 0;
    A.boffset[l] = bytes;
    A.tile0[l] = tiles;
    A.tiles_x[l] = have ? (pyr->width[l] + BL_TW - 1) / BL_TW : 1;
    if (have) {
      bytes += (int64_t)pyr->width[l] * pyr->height[l];
      // a level under 2 x 19 + 1 px admits no key-point (deviation 2): nothing reads its blurred image, and it gets no tiles
      if (pyr->width[l] > 2 * EDGE && pyr->height[l] > 2 * EDGE) tiles += A.tiles_x[l] * ((pyr->height[l] + BL_TH - 1) / BL_TH);
    }
  }
  for (int i = 0; i < 4; ++i) A.w[i] = in->blur_w[i];
  A.nlevels = pyr->nlevels;
  A.N = N;
  A.frame_stride = pyr->frame_stride;
  A.bframe_stride = bytes;
  A.data = pyr->data;
  GL_HIP(hipSetDevice(c->device));
  if (c->orb_pattern != (const void*)in->pattern) {  // deviation 3
    int8_t host[1024];
    GL_HIP(hipMemcpyAsync(host, in->pattern, sizeof(host), hipMemcpyDeviceToHost, c->stream));
    GL_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 1024; ++i) GL_REQUIRE(host[i] >= -REACH && host[i] <= REACH, "a pattern entry outside [-13, 13]");
    c->orb_pattern = in->pattern;
  }
  void* scratch = nullptr;
  if (int rc = gl::ctx_scratch(c, (size_t)B * (size_t)bytes, &scratch)) return rc;
  A.blurred = (uint8_t*)scratch;
  if (tiles > 0 && 255 * wsum <= 65535) k_orb_blur<uint16_t><<<dim3(tiles, B), BL_T, 0, c->stream>>>(A);
  if (tiles > 0 && 255 * wsum > 65535) k_orb_blur<uint32_t><<<dim3(tiles, B), BL_T, 0, c->stream>>>(A);
  GL_HIP(hipGetLastError());
  k_orb_describe<<<dim3((N + KP_PER_BLOCK - 1) / KP_PER_BLOCK, B), DS_T, 0, c->stream>>>(A, in->kp_xy, in->kp_oct, in->n_kp, in->kp_angle, in->pattern,
                                                                                       (uint32_t*)out->desc, out->angle, out->moments, out->uv32,
                                                                                       out->uv64, out->stat);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

}  // extern "C"
