// GL_ASSOC_SCREENED: the exhaustive association (k_assoc_brute, gl_assoc.hip) as a packed-fp32 screen followed by an exact
// fp64 verify of the components the screen cannot rule out.  The output is GL_ASSOC_EXHAUSTIVE's, bit for bit, for every input.
//
//  k_assoc_screen        : grid = (point tiles, K splits) as the fp64 sweep.  A lane owns two or four points, in pairs packed into
//                          the two halves of v_pk_{fma,mul,add}_f32; the fp32 record of the current Gaussian is wave-uniform (scalar loads, SGPR
//                          operands).  Per pair it computes the quadratic form s_k and an error bound e_k (below), keeps
//                          U = min_k (s_k + e_k), and notes every chunk of 8 Gaussians whose min_k (s_k - e_k) is <= the running U
//                          in a short per-point list in LDS.  At the end of its split it writes U and the chunks still <= U.
//  k_assoc_screen_verify : up to 16 lanes per point, a split per lane and round.  U = min over the splits; every Gaussian of the listed chunks with s_k - e_k <= U is
//                          re-evaluated with the canonical fp64 chi2_rec in ascending k, keeping the first strict minimum (the
//                          rule of k_assoc_brute + k_assoc_merge).  The true minimiser always survives (s - e <= chi2 <= min U),
//                          and so does every Gaussian tied with it, so the first minimum among the survivors is the first overall.
//                          Points the screen cannot decide (a candidate dropped for lack of room that could still win, or
//                          coordinates whose fp32 values could overflow, NaN / inf included) are appended to a device list that
//                          the fp64 sweep (launch_assoc_sweep64) then resolves: correctness never depends on the list sizes.
//
// THE BOUND.  Notation: u = 2^-24 (fp32 unit roundoff), m = mean, p = point, o = the map's origin (fp64), d = p - m (real),
// A = cov_inv as stored in rec12 (9 entries, not exactly symmetric), S = (A + A^T) / 2, so that d^T A d = d^T S d.  The record
// holds M = fl32(m - o), a_ii = fl32(A_ii), b_ij = fl32(A_ij + A_ji) (i < j) and c = max over i of max(row i, column i) of |A|,
// rounded up; c >= ||S||_2 and c >= the row sums of |S|.  The lane holds P = fl32(p - o) and computes in fp32, fmaf explicit:
//     D = P - M,  s = D0 (a00 D0 + b01 D1 + b02 D2) + D1 (a11 D1 + b12 D2) + D2 a22 D2          (12 operations)
//     n = D0^2 + D1^2 + D2^2 + H,  E = c n,  hi = s + E G,  lo = s - E G                        (6 operations)
// with per-point G = 2^-20 + 2.5 beta, F = 2.5 beta + 8 beta^2, H = F / G (all rounded up), beta = 1.01 u (rho + R) + 1e-30,
// rho = |p - o|_inf, R = max_k |m_k - o|_inf.  So e = E G >= c (G ||D||^2 + F).  It dominates |s - chi2_rec| because:
//  (1) rounding of p and m: P - M = d + eps_p - eps_m, |eps| <= 1.01 u rho (resp. R) per coordinate (fp64 subtraction, then fp32
//      rounding; + 2^-126 where the value flushes to zero); the fp32 subtraction adds u |D_i|.  So D = d + eps with
//      ||eps|| <= 1.0001 u ||D|| + sqrt(3) beta, and |D^T S D - d^T S d| <= 2 c ||eps|| ||D|| + c ||eps||^2
//      <= c ((2.0002 u + sqrt(3) beta) ||D||^2 + sqrt(3) beta + 6 beta^2 + 2 u^2 ||D||^2), using 2 ||D|| <= ||D||^2 + 1;
//  (2) rounding of cov_inv to fp32, the asymmetry of the 9 entries included: |D^T (S~ - S) D| <= 1.01 u c ||D||^2;
//  (3) fp32 evaluation of s: at most 6 roundings along any product path, |s - D^T S~ D| <= 6.01 u |D|^T |S~| |D| <= 6.02 u c ||D||^2;
//  (4) the fp64 evaluation of chi2_rec itself (9 roundings with u64 = 2^-53, on d64 = fl64(p - m)): < 1e-14 u c ||D||^2;
//  (5) margin for the rounding of the bound itself and of hi / lo: the sum of (1)-(4) is < 9.1 u c ||D||^2 + 1.74 beta c (||D||^2 + 1)
//      + 6 beta^2 c, while e >= 16 u c ||D||^2 + 2.5 beta c (||D||^2 + 1) + 8 beta^2 c; the 6.9 u and 0.76 beta left over cover the
//      at most 5 roundings of n, E, hi / lo (|s| <= 1.01 c ||D||^2);
//  (6) underflow: c is floored at 1e-6 and beta carries 1e-30, so c F exceeds every absolute error of a flushed or subnormal
//      intermediate (< 1e-37 (1 + 6 (rho + R))).
// Overflow: a point whose fp32 values could exceed 1e37 - c_max (3.1 (rho + R)^2 + H)(1 + G) - is not screened at all but sent to
// the fp64 sweep, and a map with a non-finite fp32 record has no screen records (every point goes to the fp64 sweep).
// An MFMA "expanded form" (x^T A x - 2 mu^T A x + mu^T A mu) is not used: at 1e6-scale cov_inv its cancellation makes the fp32
// error of order 1 in chi2, and nearly every point would fall back.
//
// Compiled with -ffp-contract=off like the rest: every fused operation is an explicit fma.
#include <cmath>
#include <cstring>
#include <vector>

#include "gl_device.hpp"
#include "gl_internal.hpp"

using namespace gld;

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef const float __attribute__((address_space(4))) cfloat;

constexpr int kCap = 8;   // chunk candidates a lane keeps per point in LDS while it sweeps its split (kCap / NP: 32 KB per workgroup)
constexpr int kOut = 4;   // chunks per (split, point) handed to the verify kernel
constexpr float kLimit = 1e37f;

struct ScreenGeo {
  double o[3];
  double rmax, cmax;
  int K;
};

struct PtScreen {
  float P[3], G, H;
  bool ok;
};

// per-point quantities of the bound (THE BOUND above); `ok` false: the point is not screened (fp64 sweep)
__device__ __forceinline__ PtScreen screen_point(double x, double y, double z, const ScreenGeo& g) {
  PtScreen r;
  const double dx = x - g.o[0], dy = y - g.o[1], dz = z - g.o[2];
  const double rho = fmax(fabs(dx), fmax(fabs(dy), fabs(dz)));  // NaN-ignoring: NaN is caught below
  const double L = rho + g.rmax;
  const double beta = 1.01 * 0x1p-24 * L + 1e-30;
  const double G = 0x1p-20 + 2.5 * beta, F = 2.5 * beta + 8.0 * beta * beta, H = F / G;
  const double up = 1.0 + 0x1p-20;  // fp32 conversion rounds by < 2^-24: the stored values are >= the fp64 ones
  r.G = (float)(G * up);
  r.H = (float)(H * up);
  r.P[0] = (float)dx;
  r.P[1] = (float)dy;
  r.P[2] = (float)dz;
  const double big = g.cmax * (3.1 * L * L + H) * (1.0 + G);
  r.ok = (x == x) && (y == y) && (z == z) && big <= (double)kLimit;  // false for NaN / inf coordinates as well
  return r;
}

__device__ __forceinline__ f2 splat(float v) { return f2{v, v}; }
__device__ __forceinline__ f2 pfma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// hi / lo of one Gaussian (record r, wave-uniform) for the lane's two points: 18 packed operations
__device__ __forceinline__ void screen_pair(cfloat* r, f2 px, f2 py, f2 pz, f2 G, f2 H, f2& hi, f2& lo) {
  const f2 d0 = px - splat(r[0]), d1 = py - splat(r[1]), d2 = pz - splat(r[2]);
  const f2 t0 = pfma(d2, splat(r[7]), pfma(d1, splat(r[6]), d0 * splat(r[3])));
  const f2 t1 = pfma(d2, splat(r[8]), d1 * splat(r[4]));
  const f2 t2 = d2 * splat(r[5]);
  const f2 s = pfma(d2, t2, pfma(d1, t1, t0 * d0));
  const f2 n = pfma(d2, d2, pfma(d1, d1, pfma(d0, d0, H)));
  const f2 E = n * splat(r[9]);
  hi = pfma(E, G, s);
  lo = pfma(-E, G, s);
}

// the same arithmetic for one point (the verify kernel; its records are per-thread): a valid lo on its own
__device__ __forceinline__ float screen_lo(const float* __restrict__ r, const PtScreen& q) {
  const float d0 = q.P[0] - r[0], d1 = q.P[1] - r[1], d2 = q.P[2] - r[2];
  const float t0 = fmaf(d2, r[7], fmaf(d1, r[6], d0 * r[3]));
  const float t1 = fmaf(d2, r[8], d1 * r[4]);
  const float t2 = d2 * r[5];
  const float s = fmaf(d2, t2, fmaf(d1, t1, t0 * d0));
  const float n = fmaf(d2, d2, fmaf(d1, d1, fmaf(d0, d0, q.H)));
  return fmaf(-(n * r[9]), q.G, s);
}

// Per (split, point) outputs, SoA with stride Nstride: U, lost (the smallest chunk lo that had no room; +inf if none), the chunk
// count and kOut chunk starts / chunk lo.
struct ScreenOut {
  float* u;
  float* lost;
  int32_t* cnt;
  int32_t* k0;
  float* lo;
};

// NP packed pairs of points per lane (PPT = 2 NP points), 256 lanes per workgroup
template <int NP>
__global__ __launch_bounds__(256) void k_assoc_screen(const float* __restrict__ rec32, int K, int kchunk,
                                                      const double* __restrict__ pts, int Nstride, const int32_t* __restrict__ list,
                                                      const int32_t* __restrict__ count_dev, ScreenGeo geo, ScreenOut out) {
  constexpr int PPT = 2 * NP, CAP = kCap / NP, ST = PPT * 256;  // LDS: [CAP][PPT][256] chunk starts and chunk lo
  __shared__ int32_t lk[CAP * ST];
  __shared__ float ll[CAP * ST];
  const int N = count_dev ? *count_dev : Nstride;
  if (blockIdx.x * 256 * PPT >= N) return;
  const int tid = threadIdx.x;
  const int k_begin = blockIdx.y * kchunk;
  const int k_end = min(K, k_begin + kchunk);
  const int p0 = (blockIdx.x * 256 + tid) * PPT;
  cfloat* rc = (cfloat*)rec32;

  f2 px[NP], py[NP], pz[NP], G[NP], H[NP];
#pragma unroll
  for (int p = 0; p < PPT; ++p) {
    int n = min(p0 + p, N - 1);
    if (list) n = list[n];
    const PtScreen q = screen_point(pts[(size_t)n * 3 + 0], pts[(size_t)n * 3 + 1], pts[(size_t)n * 3 + 2], geo);
    px[p / 2][p % 2] = q.P[0];
    py[p / 2][p % 2] = q.P[1];
    pz[p / 2][p % 2] = q.P[2];
    G[p / 2][p % 2] = q.G;
    H[p / 2][p % 2] = q.H;
  }
  float U[PPT], lost[PPT];
  int cnt[PPT];
#pragma unroll
  for (int p = 0; p < PPT; ++p) {
    U[p] = __builtin_inff();
    lost[p] = __builtin_inff();
    cnt[p] = 0;
  }

  // note chunk k0 (its smallest lo) for point p; when the list is full, drop the entries the running U has ruled out first
  auto note = [&](int p, int k0, float lo) {
    int* kk = lk + p * 256 + tid;
    float* lv = ll + p * 256 + tid;
    if (cnt[p] == CAP) {
      int w = 0;
      for (int j = 0; j < CAP; ++j) {
        const float l = lv[j * ST];
        if (!(l > U[p])) {
          kk[w * ST] = kk[j * ST];
          lv[w * ST] = l;
          ++w;
        }
      }
      cnt[p] = w;
    }
    if (cnt[p] < CAP) {
      kk[cnt[p] * ST] = k0;
      lv[cnt[p] * ST] = lo;
      ++cnt[p];
    } else {
      lost[p] = fminf(lost[p], lo);
    }
  };

  for (int k0 = k_begin; k0 < k_end; k0 += 8) {
    cfloat* rec = rc + (size_t)k0 * 12;
    f2 hmin[NP], lmin[NP], hi, lo;
    const int ng = min(8, k_end - k0);
#pragma unroll
    for (int j = 0; j < NP; ++j) screen_pair(rec, px[j], py[j], pz[j], G[j], H[j], hmin[j], lmin[j]);
    if (ng == 8) {  // whole chunk: straight-line code, the scheduler hoists the scalar loads
#pragma unroll
      for (int g = 1; g < 8; ++g)
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          screen_pair(rec + g * 12, px[j], py[j], pz[j], G[j], H[j], hi, lo);
          hmin[j] = f2{fminf(hmin[j].x, hi.x), fminf(hmin[j].y, hi.y)};
          lmin[j] = f2{fminf(lmin[j].x, lo.x), fminf(lmin[j].y, lo.y)};
        }
    } else {
      for (int g = 1; g < ng; ++g)
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          screen_pair(rec + g * 12, px[j], py[j], pz[j], G[j], H[j], hi, lo);
          hmin[j] = f2{fminf(hmin[j].x, hi.x), fminf(hmin[j].y, hi.y)};
          lmin[j] = f2{fminf(lmin[j].x, lo.x), fminf(lmin[j].y, lo.y)};
        }
    }
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
      U[p] = fminf(U[p], hmin[p / 2][p % 2]);
      const float l = lmin[p / 2][p % 2];
      if (!(l > U[p])) note(p, k0, l);
    }
  }

#pragma unroll
  for (int p = 0; p < PPT; ++p) {
    const int n = p0 + p;
    if (n >= N) continue;
    const size_t o = (size_t)blockIdx.y * Nstride + n;
    const int* kk = lk + p * 256 + tid;
    const float* lv = ll + p * 256 + tid;
    int w = 0;
    float ls = lost[p];
    for (int j = 0; j < cnt[p]; ++j) {
      const float l = lv[j * ST];
      if (l > U[p]) continue;
      if (w < kOut) {
        out.k0[(size_t)w * gridDim.y * Nstride + o] = kk[j * ST];
        out.lo[(size_t)w * gridDim.y * Nstride + o] = l;
        ++w;
      } else {
        ls = fminf(ls, l);
      }
    }
    out.u[o] = U[p];
    out.lost[o] = ls;
    out.cnt[o] = w;
  }
}

// L lanes (a power of two <= 16) per point, each taking the splits s = lane, lane + L, ...: the per-split reads are latency-bound
// chains, and a point has up to ~100 splits.  The lanes' first minima are combined by (chi2, k) - lowest k on equal chi2 - which is
// the sequential first-strict-minimum rule because a screened point's chi2 values are all finite.
__global__ __launch_bounds__(256) void k_assoc_screen_verify(const double* __restrict__ rec12, const float* __restrict__ rec32,
                                                             int nsplit, int L, const double* __restrict__ pts, int Nstride,
                                                             const int32_t* __restrict__ list, const int32_t* __restrict__ count_dev,
                                                             ScreenGeo geo, ScreenOut in, int32_t* __restrict__ idx,
                                                             double* __restrict__ d2, int32_t* __restrict__ fb_list,
                                                             int32_t* __restrict__ fb_count, int32_t* __restrict__ counters) {
  __shared__ int red[2];
  const int N = count_dev ? *count_dev : Nstride;
  const int ppb = 256 / L;  // points per workgroup and round
  if (blockIdx.x * ppb >= N) return;  // whole workgroup: it has no point in any round
  if (threadIdx.x < 2) red[threadIdx.x] = 0;
  __syncthreads();
  const int sub = threadIdx.x & (L - 1);
  int verified = 0, fell = 0;
  for (int base = blockIdx.x * ppb; base < N; base += gridDim.x * ppb) {  // uniform: every lane takes part in the shuffles
    const int n = base + threadIdx.x / L;
    const bool act = n < N;
    const int nn = act ? n : N - 1;
    const int o = list ? list[nn] : nn;
    const double x = pts[(size_t)o * 3 + 0], y = pts[(size_t)o * 3 + 1], z = pts[(size_t)o * 3 + 2];
    const PtScreen q = screen_point(x, y, z, geo);
    float U = __builtin_inff(), lost = __builtin_inff();
    for (int s = sub; s < nsplit; s += L) {
      U = fminf(U, in.u[(size_t)s * Nstride + nn]);
      lost = fminf(lost, in.lost[(size_t)s * Nstride + nn]);
    }
    for (int off = 1; off < L; off <<= 1) {
      U = fminf(U, __shfl_xor(U, off, 64));
      lost = fminf(lost, __shfl_xor(lost, off, 64));
    }
    const bool fb = !q.ok || !(lost > U);  // not screened, or a chunk without room could still hold the minimum
    double best = __builtin_inf();
    int bi = 0x7fffffff;
    if (!fb) {
      for (int s = sub; s < nsplit; s += L) {
        const int c = in.cnt[(size_t)s * Nstride + nn];
        for (int j = 0; j < c; ++j) {
          const size_t e = ((size_t)j * nsplit + s) * Nstride + nn;
          if (in.lo[e] > U) continue;
          const int k0 = in.k0[e];
          const int k1 = min(geo.K, k0 + 8);
          for (int k = k0; k < k1; ++k) {
            if (screen_lo(rec32 + (size_t)k * 12, q) > U) continue;
            const double d = chi2_rec(rec12 + (size_t)k * 12, x, y, z);
            if (act) ++verified;
            if (d < best) {
              best = d;
              bi = k;
            }
          }
        }
      }
    }
    for (int off = 1; off < L; off <<= 1) {
      const double od = shfl_xor_f64(best, off);
      const int oi = __shfl_xor(bi, off, 64);
      const bool t = od < best || (od == best && oi < bi);
      best = t ? od : best;
      bi = t ? oi : bi;
    }
    if (act && sub == 0) {
      if (fb) {
        fb_list[atomicAdd(fb_count, 1)] = o;
        ++fell;
      } else {
        idx[o] = bi == 0x7fffffff ? -1 : bi;
        if (d2) d2[o] = best;
      }
    }
  }
  if (verified) atomicAdd(&red[0], verified);  // LDS first: one device atomic per workgroup and counter
  if (fell) atomicAdd(&red[1], fell);
  __syncthreads();
  if (threadIdx.x == 0 && red[0]) atomicAdd(counters + GL_COUNTER_ASSOC_SCREEN_VERIFIED, red[0]);
  if (threadIdx.x == 0 && red[1]) atomicAdd(counters + GL_COUNTER_ASSOC_SCREEN_FALLBACK, red[1]);
}

// a map without screen records: every (listed) point is a fallback
__global__ void k_screen_count_all(int N, const int32_t* __restrict__ count_dev, int32_t* __restrict__ counters) {
  atomicAdd(counters + GL_COUNTER_ASSOC_SCREEN_FALLBACK, count_dev ? *count_dev : N);
}

// Launch shape: two points per lane (four from 16 384 points), 256 lanes per workgroup; K splits as in the fp64 sweep.
void screen_shape(int K, int N, bool listed, int* ppt_o, int* ptiles_o, int* nsplit_o, int* kchunk_o) {
  const int ppt = gl::sweep_points(N, listed) >= 16384 ? 4 : 2;
  *ppt_o = ppt;
  gl::sweep_split(K, N, listed, ppt, ptiles_o, nsplit_o, kchunk_o);
}

}  // namespace

namespace gl {

// fp32 screen records (layout: gl_internal.hpp, Gmm::rec32), from the fp64 records, once per map
int build_screen_records(Ctx* c, Gmm* g) {
  const int K = g->K;
  std::vector<double> rec((size_t)K * 12);
  GL_HIP(hipStreamSynchronize(c->stream));  // rec12 is written by k_build_components on the context's stream
  GL_HIP(hipMemcpy(rec.data(), g->rec12, rec.size() * 8, hipMemcpyDeviceToHost));
  double lo[3], hi[3];
  for (int a = 0; a < 3; ++a) lo[a] = hi[a] = rec[a];
  bool ok = true;
  for (int k = 0; k < K; ++k)
    for (int a = 0; a < 3; ++a) {
      const double v = rec[(size_t)k * 12 + a];
      ok = ok && std::isfinite(v);
      lo[a] = std::min(lo[a], v);
      hi[a] = std::max(hi[a], v);
    }
  for (int a = 0; a < 3; ++a) g->scr_o[a] = 0.5 * lo[a] + 0.5 * hi[a];
  std::vector<float> r32((size_t)K * 12, 0.f);
  double rmax = 0, cmax = 0;
  for (int k = 0; k < K && ok; ++k) {
    const double* r = rec.data() + (size_t)k * 12;
    const double* A = r + 3;  // row-major 3 x 3
    float* w = r32.data() + (size_t)k * 12;
    double c = 0;
    for (int i = 0; i < 3; ++i) {
      const double row = std::fabs(A[i * 3]) + std::fabs(A[i * 3 + 1]) + std::fabs(A[i * 3 + 2]);
      const double col = std::fabs(A[i]) + std::fabs(A[3 + i]) + std::fabs(A[6 + i]);
      c = std::max(c, std::max(row, col));
    }
    c = std::max(c * (1.0 + 0x1p-20), 1e-6);  // covers the fp64 sums and the rounding to fp32 below
    for (int a = 0; a < 3; ++a) {
      const double d = r[a] - g->scr_o[a];
      rmax = std::max(rmax, std::fabs(d));
      w[a] = (float)d;
    }
    w[3] = (float)A[0];
    w[4] = (float)A[4];
    w[5] = (float)A[8];
    w[6] = (float)(A[1] + A[3]);
    w[7] = (float)(A[2] + A[6]);
    w[8] = (float)(A[5] + A[7]);
    w[9] = (float)c;
    cmax = std::max(cmax, (double)w[9]);
    for (int i = 0; i < 10; ++i) ok = ok && std::isfinite(w[i]);
  }
  g->scr_rmax = rmax * (1.0 + 1e-12);
  g->scr_cmax = cmax;
  ok = ok && std::isfinite(g->scr_rmax) && cmax * (g->scr_rmax * g->scr_rmax) < 1e30;
  if (!ok) return GL_OK;  // no screen: GL_ASSOC_SCREENED is the fp64 sweep for this map
  if (hipMalloc((void**)&g->rec32, r32.size() * 4) != hipSuccess) {
    set_error("gl_gmm_create: hipMalloc(%zu) failed", r32.size() * 4);
    return GL_ERR_NOMEM;
  }
  GL_HIP(hipMemcpy(g->rec32, r32.data(), r32.size() * 4, hipMemcpyHostToDevice));
  return GL_OK;
}

// GL_ASSOC_SCREENED: same arguments and results as launch_assoc_sweep (list / count_dev: the listed subset only)
int launch_assoc_screened(Ctx* c, const Gmm* g, const double* pts, int N, int32_t* idx, double* d2, const int32_t* list,
                          const int32_t* count_dev) {
  const int K = g->K;
  const size_t fb_bytes = assoc_scratch_bytes(K, N, true);
  if (!g->rec32) {  // map without screen records
    void* scratch = nullptr;
    int rc = ctx_scratch(c, assoc_scratch_bytes(K, N, list != nullptr), &scratch, SCRATCH_SCREEN);
    if (rc != GL_OK) return rc;
    k_screen_count_all<<<1, 1, 0, c->stream>>>(N, count_dev, c->counters);
    GL_HIP(hipGetLastError());
    return launch_assoc_sweep64(c, g, pts, N, idx, d2, list, count_dev, scratch);
  }
  int ppt, ptiles, nsplit, kchunk;
  screen_shape(K, N, list != nullptr, &ppt, &ptiles, &nsplit, &kchunk);
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t per = (size_t)nsplit * N;
  // | u | lost | cnt | k0 x kOut | lo x kOut | fallback count (256 B) | fallback list | fp64 sweep scratch |
  const size_t o_u = 0, o_lost = o_u + up(per * 4), o_cnt = o_lost + up(per * 4), o_k0 = o_cnt + up(per * 4),
               o_lo = o_k0 + up(per * 4 * kOut), o_fbc = o_lo + up(per * 4 * kOut), o_fbl = o_fbc + 256,
               o_sw = o_fbl + up((size_t)N * 4);
  void* scratch = nullptr;
  int rc = ctx_scratch(c, o_sw + fb_bytes, &scratch, SCRATCH_SCREEN);
  if (rc != GL_OK) return rc;
  char* s = (char*)scratch;
  ScreenOut so{(float*)(s + o_u), (float*)(s + o_lost), (int32_t*)(s + o_cnt), (int32_t*)(s + o_k0), (float*)(s + o_lo)};
  int32_t* fb_count = (int32_t*)(s + o_fbc);
  int32_t* fb_list = (int32_t*)(s + o_fbl);
  const ScreenGeo geo{{g->scr_o[0], g->scr_o[1], g->scr_o[2]}, g->scr_rmax, g->scr_cmax, K};
  {
    TimerScope ts(c, GL_TIMER_ASSOC);
    GL_HIP(hipMemsetAsync(fb_count, 0, 4, c->stream));
    if (ppt == 4)
      k_assoc_screen<2><<<dim3(ptiles, nsplit), 256, 0, c->stream>>>(g->rec32, K, kchunk, pts, N, list, count_dev, geo, so);
    else
      k_assoc_screen<1><<<dim3(ptiles, nsplit), 256, 0, c->stream>>>(g->rec32, K, kchunk, pts, N, list, count_dev, geo, so);
    GL_HIP(hipGetLastError());
    int L = 1;  // lanes per point: about one per four splits (one split more per lane costs less than idle lanes)
    while (4 * L < nsplit && L < 16) L <<= 1;
    k_assoc_screen_verify<<<std::min((N + 256 / L - 1) / (256 / L), 2048), 256, 0, c->stream>>>(g->rec12, g->rec32, nsplit, L, pts, N, list,
                                                                                               count_dev, geo, so, idx, d2, fb_list, fb_count, c->counters);
    GL_HIP(hipGetLastError());
  }
  return launch_assoc_sweep64(c, g, pts, N, idx, d2, fb_list, fb_count, s + o_sw);
}

}  // namespace gl
