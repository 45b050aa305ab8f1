// The irregular half of ORBextractor (orb_extractor.cpp) for B images: gl_orb_pyramid (ComputePyramid without its border, :1056-1080)
// and gl_orb_detect (ComputeKeyPointsOctTree without its last loop, :739-819).  The rules and the declared deviations are in
// gmmloc_hip.h; tests/orb_detect_ref.py is the sequential model every output is compared with, bit for bit.
//
//   k_orb_resize   one level from the level before it: a thread per output pixel, OpenCV's 8-bit fixed-point INTER_LINEAR as declared.
//   k_orb_fast     a workgroup per cell of :763-799: the cell image (at most 65 x 65) as bytes in LDS, a thread per pixel of the cell's
//                  region works out the corner score s (the largest t at which the segment test passes), the score tile in LDS feeds
//                  the 3 x 3 suppression.  A pixel is a corner at threshold t iff s >= t, and a corner survives suppression iff every
//                  neighbour's s is smaller - whatever t is, since a neighbour below t counts 0 < s.  So one pass serves both thresholds
//                  and the fallback is a workgroup-wide OR.  Writes the level's score map (0 where nothing is kept) and the cell's count.
//   k_orb_gather   count -> scan -> ordered write: a workgroup per cell adds up the counts of the cells before it in its level and
//                  writes its candidates, pixels row-major, behind them.  No atomics.
//   k_orb_octree   DistributeOctTree (:529-737), a workgroup per (image, level).  The level's candidates are a permutation array
//                  segmented by node; DivideNode is a stable 4-way split of the node's segment done by one wave with ballots (count,
//                  write, copy back), so a child's segment lies inside its parent's.  A phase-1 sweep divides all nodes at once, a
//                  wave per node, then rebuilds the node table IN LIST ORDER (children reversed, then the bNoMore nodes).  Phase 2 is
//                  wave 0 alone on a doubly linked list.  The working set lies in LDS when it fits, else in the main scratch block.
//   k_orb_collect  a workgroup per image: the levels' results one behind the other, the padding, the counts.
#include "gl_device.hpp"
#include "gl_internal.hpp"

namespace {

constexpr int EDGE = 19, BORDER = EDGE - 3;       // EDGE_THRESHOLD (:75); minBorderX / minBorderY (:747-748)
constexpr int CELL_MAX = 59, TILE = CELL_MAX + 6;  // ceil(width / (int)(width / 30)) <= 59; the cell image with its 3-px ring
constexpr int F_T = 256, O_T = 256, O_W = O_T / 64;
constexpr int LDS_DYN_MAX = 56 * 1024;             // the octree's working set stays in LDS up to here (static LDS comes on top)
constexpr int FB_BIT = 1 << 20;                    // in a cell's count word: the cell was redone at min_th

struct Node {
  int start, count;    // its keys: perm[start .. start + count)
  int x0, x1, y0, y1;  // UL.x, UR.x, UL.y, BL.y
};

struct DetArgs {
  int32_t width[8], height[8];
  int64_t stride[8], offset[8], moffset[8];  // of the pyramid; of the score map (stride = width)
  int32_t ncols[8], nrows[8], wcell[8], hcell[8], cell0[8];
  int32_t nfeat[8], nini[8], res0[8];  // mnFeaturesPerLevel; nIni (0: the level yields nothing); the level's first staging slot
  float hx[8];
  int nlevels, N, cand_cap, ini_th, min_th, ncells, res_cap, node_cap;
  int64_t frame_stride, mframe;
  const uint8_t* data;
  uint8_t* map;        // B x mframe: the kept scores
  int32_t* cellcnt;    // B x ncells
  uint32_t* cand_xy;   // B x 8 x cand_cap: x | y << 16, ROI coordinates
  uint8_t* cand_sc;    // B x 8 x cand_cap
  int32_t* tot;        // B x 8: the level's candidates, whether they fit or not
  int32_t* res_cnt;    // B x 8
  uint32_t* res_xy;    // B x res_cap
  uint8_t* res_sc;     // B x res_cap
};

template <typename T>
__device__ __forceinline__ T pick(const T (&a)[8], int l) {
  T v = a[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) v = k == l ? a[k] : v;
  return v;
}

__device__ __forceinline__ int block_sum(int v, int* s_red) {  // every thread gets the sum; s_red: one int per wave
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (threadIdx.x % 64 == 0) s_red[threadIdx.x / 64] = v;
  __syncthreads();
  int s = 0;
  for (int k = 0; k < (int)blockDim.x / 64; ++k) s += s_red[k];
  return s;
}

// ---- the pyramid
__device__ __forceinline__ void resize_coef(int d, double scale, int n, int& s, int& a0, int& a1) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) {
    s = 0;
    f = 0.0f;
  }
  if (s >= n - 1) {
    s = n - 1;
    f = 0.0f;
  }
  a1 = __float2int_rn(f * 2048.0f);  // cvRound: half to even
  a0 = __float2int_rn((1.0f - f) * 2048.0f);
}

__global__ __launch_bounds__(256) void k_orb_resize(uint8_t* data, int64_t frame_stride, int64_t soff, int64_t sstride, int sw, int sh, int64_t doff,
                                                    int64_t dstride, int dw, int dh, double scale_x, double scale_y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)dw * dh) return;
  const int dx = (int)(i % dw), dy = (int)(i / dw);
  int sx, sy, a0, a1, b0, b1;
  resize_coef(dx, scale_x, sw, sx, a0, a1);
  resize_coef(dy, scale_y, sh, sy, b0, b1);
  const uint8_t* S = data + (int64_t)blockIdx.y * frame_stride + soff;
  const int x1 = min(sx + 1, sw - 1);
  const uint8_t *p0 = S + (int64_t)sy * sstride, *p1 = S + (int64_t)min(sy + 1, sh - 1) * sstride;
  const int r0 = a0 * p0[sx] + a1 * p0[x1], r1 = a0 * p1[sx] + a1 * p1[x1];
  data[(int64_t)blockIdx.y * frame_stride + doff + (int64_t)dy * dstride + dx] = (uint8_t)((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2);
}

// ---- cell FAST
struct Cell {
  int l, x0, y0, rw, rh;  // the level; the cell image's first column / row in the ROI; its region's size (<= 0: nothing is computed)
  bool skipped;           // by one of the two `continue`s
};

__device__ __forceinline__ Cell cell_of(const DetArgs& A, int cell) {
  Cell c;
  c.l = 0;
#pragma unroll
  for (int k = 1; k < 8; ++k) c.l += (k < A.nlevels && cell >= A.cell0[k]) ? 1 : 0;
  const int ci = cell - pick(A.cell0, c.l), ncols = pick(A.ncols, c.l), wc = pick(A.wcell, c.l), hc = pick(A.hcell, c.l);
  const int maxbx = pick(A.width, c.l) - BORDER, maxby = pick(A.height, c.l) - BORDER;
  c.x0 = BORDER + (ci % ncols) * wc;
  c.y0 = BORDER + (ci / ncols) * hc;
  c.skipped = c.y0 >= maxby - 3 || c.x0 >= maxbx - 6;  // :767, :775
  c.rw = min(c.x0 + wc + 6, maxbx) - c.x0 - 6;         // :774-778, less the ring on both sides
  c.rh = min(c.y0 + hc + 6, maxby) - c.y0 - 6;
  if (c.skipped || c.rw <= 0 || c.rh <= 0) c.rw = c.rh = 0;
  return c;
}

__global__ __launch_bounds__(F_T) void k_orb_fast(const DetArgs A) {
  __shared__ uint8_t s_in[TILE][TILE + 3];
  __shared__ int16_t s_sc[CELL_MAX + 2][CELL_MAX + 3];
  __shared__ int s_red[F_T / 64];
  const int tid = threadIdx.x, b = blockIdx.y;
  const Cell c = cell_of(A, blockIdx.x);
  const int tw = c.rw + 6, npix = c.rw * c.rh;
  const int64_t stride = pick(A.stride, c.l);
  const uint8_t* I = A.data + (int64_t)b * A.frame_stride + pick(A.offset, c.l) + (int64_t)c.y0 * stride + c.x0;
  if (npix > 0)
    for (int i = tid; i < tw * (c.rh + 6); i += F_T) s_in[i / tw][i % tw] = I[(i / tw) * stride + i % tw];
  for (int i = tid; i < (CELL_MAX + 2) * (CELL_MAX + 3); i += F_T) (&s_sc[0][0])[i] = 0;
  __syncthreads();
  for (int p = tid; p < npix; p += F_T) {
    const int ry = p / c.rw, rx = p % c.rw;
    const uint8_t* q = &s_in[ry + 3][rx + 3];
    const int v = q[0];
    constexpr int W = TILE + 3;
    int mn[16], mx[16];
    {
      const int d[16] = {v - q[3 * W],      v - q[3 * W + 1],  v - q[2 * W + 2],  v - q[W + 3],  v - q[3],  v - q[-W + 3],  v - q[-2 * W + 2], v - q[-3 * W + 1],
                         v - q[-3 * W],     v - q[-3 * W - 1], v - q[-2 * W - 2], v - q[-W - 3], v - q[-3], v - q[W - 3],   v - q[2 * W - 2],  v - q[3 * W - 1]};
      int a2[16], b2[16], a4[16], b4[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        a2[k] = min(d[k], d[(k + 1) % 16]);
        b2[k] = max(d[k], d[(k + 1) % 16]);
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        a4[k] = min(a2[k], a2[(k + 2) % 16]);
        b4[k] = max(b2[k], b2[(k + 2) % 16]);
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) {  // the arc k .. k + 8
        mn[k] = min(min(a4[k], a4[(k + 4) % 16]), d[(k + 8) % 16]);
        mx[k] = max(max(b4[k], b4[(k + 4) % 16]), d[(k + 8) % 16]);
      }
    }
    int best = -255;
#pragma unroll
    for (int k = 0; k < 16; ++k) best = max(best, max(mn[k], -mx[k]));
    s_sc[ry + 1][rx + 1] = (int16_t)max(best - 1, 0);
  }
  __syncthreads();
  // (npix <= 59 x 59: at most 14 pixels a thread)
  uint32_t is_max = 0;
  int any_ini = 0;
  for (int p = tid, k = 0; p < npix; p += F_T, ++k) {
    const int ry = p / c.rw, rx = p % c.rw;
    const int16_t* q = &s_sc[ry + 1][rx + 1];
    constexpr int W = CELL_MAX + 3;
    const int s = q[0], m = max(max(max(q[-W - 1], q[-W]), max(q[-W + 1], q[-1])), max(max(q[1], q[W - 1]), max(q[W], q[W + 1])));
    if (s > m) {
      is_max |= 1u << k;
      any_ini |= s >= A.ini_th;
    }
  }
  const bool has_ini = __syncthreads_or(any_ini);
  const int th = has_ini ? A.ini_th : A.min_th;  // :785-788
  uint8_t* M = A.map + (int64_t)b * A.mframe + pick(A.moffset, c.l);
  const int w = pick(A.width, c.l);
  int count = 0;
  for (int p = tid, k = 0; p < npix; p += F_T, ++k) {
    const int ry = p / c.rw, rx = p % c.rw, s = s_sc[ry + 1][rx + 1];
    const bool keep = ((is_max >> k) & 1) && s >= th;
    M[(int64_t)(c.y0 + 3 + ry) * w + c.x0 + 3 + rx] = keep ? (uint8_t)s : 0;
    count += keep;
  }
  count = block_sum(count, s_red);
  if (tid == 0) A.cellcnt[(int64_t)b * A.ncells + blockIdx.x] = count | (!c.skipped && !has_ini ? FB_BIT : 0);
}

__global__ __launch_bounds__(F_T) void k_orb_gather(const DetArgs A) {
  __shared__ int s_red[F_T / 64], s_scan[F_T / 64];
  const int tid = threadIdx.x, b = blockIdx.y;
  const Cell c = cell_of(A, blockIdx.x);
  const int32_t* cnt = A.cellcnt + (int64_t)b * A.ncells;
  int before = 0;
  for (int i = pick(A.cell0, c.l) + tid; i < (int)blockIdx.x; i += F_T) before += cnt[i] & (FB_BIT - 1);
  before = block_sum(before, s_red);
  const int npix = c.rw * c.rh, per = (npix + F_T - 1) / F_T, p0 = min(tid * per, npix), p1 = min(p0 + per, npix), w = pick(A.width, c.l);
  const uint8_t* M = A.map + (int64_t)b * A.mframe + pick(A.moffset, c.l);
  int mine = 0;
  for (int p = p0; p < p1; ++p) mine += M[(int64_t)(c.y0 + 3 + p / c.rw) * w + c.x0 + 3 + p % c.rw] != 0;
  int incl = mine;  // the block's exclusive scan of `mine`
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (tid % 64 >= o) incl += t;
  }
  if (tid % 64 == 63) s_scan[tid / 64] = incl;
  __syncthreads();
  int at = before + incl - mine;
  for (int k = 0; k < tid / 64; ++k) at += s_scan[k];
  const int64_t base = ((int64_t)b * 8 + c.l) * A.cand_cap;
  for (int p = p0; p < p1; ++p) {
    const int x = c.x0 + 3 + p % c.rw, y = c.y0 + 3 + p / c.rw, s = M[(int64_t)y * w + x];
    if (s != 0) {
      if (at < A.cand_cap) {
        A.cand_xy[base + at] = (uint32_t)x | (uint32_t)y << 16;
        A.cand_sc[base + at] = (uint8_t)s;
      }
      ++at;
    }
  }
}

// ---- the octree
__device__ __forceinline__ void mem_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }  // what the wave wrote, every lane of it reads
__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ uint64_t lanes_below() { return (1ull << (threadIdx.x % 64)) - 1; }

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// DivideNode (:475-527) by one wave: the node's keys, in their order, into n1 n2 n3 n4; c[q]: the children's sizes
__device__ void divide(const Node nd, const uint32_t* __restrict__ xy, uint16_t* perm, uint16_t* tmp, int (&c)[4]) {
  const int lane = threadIdx.x % 64;
  const int mx = nd.x0 + (nd.x1 - nd.x0 + 1) / 2, my = nd.y0 + (nd.y1 - nd.y0 + 1) / 2;  // ceil of the halves (:477-478)
  c[0] = c[1] = c[2] = c[3] = 0;
  for (int p0 = 0; p0 < nd.count; p0 += 64) {
    const int p = p0 + lane;
    int q = -1;
    if (p < nd.count) {
      const uint32_t k = xy[perm[nd.start + p]];
      const int x = (int)(k & 0xFFFF) - BORDER, y = (int)(k >> 16) - BORDER;
      q = (x < mx ? 0 : 1) + (y < my ? 0 : 2);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] += __popcll(__ballot(q == j));
  }
  int r[4] = {0, c[0], c[0] + c[1], c[0] + c[1] + c[2]};
  for (int p0 = 0; p0 < nd.count; p0 += 64) {
    const int p = p0 + lane;
    int q = -1, key = 0;
    if (p < nd.count) {
      key = perm[nd.start + p];
      const uint32_t k = xy[key];
      const int x = (int)(k & 0xFFFF) - BORDER, y = (int)(k >> 16) - BORDER;
      q = (x < mx ? 0 : 1) + (y < my ? 0 : 2);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t m = __ballot(q == j);
      if (q == j) tmp[nd.start + r[j] + __popcll(m & lanes_below())] = (uint16_t)key;
      r[j] += __popcll(m);
    }
  }
  mem_sync();
  for (int p = lane; p < nd.count; p += 64) perm[nd.start + p] = tmp[nd.start + p];
  mem_sync();
}

__device__ __forceinline__ Node child_of(const Node& nd, int q, int start, int count) {
  const int mx = nd.x0 + (nd.x1 - nd.x0 + 1) / 2, my = nd.y0 + (nd.y1 - nd.y0 + 1) / 2;
  Node n;
  n.start = start;
  n.count = count;
  n.x0 = q & 1 ? mx : nd.x0;
  n.x1 = q & 1 ? nd.x1 : mx;
  n.y0 = q & 2 ? my : nd.y0;
  n.y1 = q & 2 ? nd.y1 : my;
  return n;
}

__global__ __launch_bounds__(O_T) void k_orb_octree(const DetArgs A, char* gws, int64_t ws_bytes, int in_lds) {
  extern __shared__ __align__(16) char s_dyn[];
  __shared__ int s_red[O_W], s_i[4];
  const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid % 64, wave = tid / 64;
  const int NC = A.node_cap, cap = (A.cand_cap + 7) & ~7, Nl = pick(A.nfeat, l), nini = pick(A.nini, l);
  char* ws = in_lds ? s_dyn : gws + ((int64_t)b * 8 + l) * ws_bytes;
  uint16_t *perm = (uint16_t*)ws, *tmp = perm + cap;
  Node *TA = (Node*)(tmp + cap), *TB = TA + NC;
  int *cc = (int*)(TB + NC), *cbase = cc + 4 * NC, *nbase = cbase + NC;
  const uint32_t* xy = A.cand_xy + ((int64_t)b * 8 + l) * A.cand_cap;
  const uint8_t* sc = A.cand_sc + ((int64_t)b * 8 + l) * A.cand_cap;
  uint32_t* res_xy = A.res_xy + (int64_t)b * A.res_cap + pick(A.res0, l);
  uint8_t* res_sc = A.res_sc + (int64_t)b * A.res_cap + pick(A.res0, l);

  int n = 0;
  {
    const int c0 = pick(A.cell0, l), c1 = c0 + pick(A.ncols, l) * pick(A.nrows, l);
    for (int i = c0 + tid; i < c1; i += O_T) n += A.cellcnt[(int64_t)b * A.ncells + i] & (FB_BIT - 1);
    n = block_sum(n, s_red);
  }
  if (tid == 0) A.tot[b * 8 + l] = n;
  if (n > A.cand_cap || nini < 1 || n == 0) {  // overflow (k_orb_collect empties the image); deviation: nIni < 1; nothing to distribute
    if (tid == 0) A.res_cnt[b * 8 + l] = 0;
    return;
  }
  // the initial nodes (:544-572)
  const float hx = pick(A.hx, l);
  const int hgt = pick(A.height, l) - 2 * BORDER;
  for (int bin = wave; bin < nini; bin += O_W) {
    int cnt = 0;
    for (int p0 = 0; p0 < n; p0 += 64) {
      const int p = p0 + lane;
      cnt += __popcll(__ballot(p < n && min((int)div_rn((float)((int)(xy[min(p, n - 1)] & 0xFFFF) - BORDER), hx), nini - 1) == bin));
    }
    if (lane == 0) cc[bin] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    int at = 0, nodes = 0;
    for (int bin = 0; bin < nini; ++bin) {
      const int cnt = cc[bin];
      cbase[bin] = at;
      if (cnt > 0) TA[nodes++] = Node{at, cnt, (int)(hx * (float)bin), (int)(hx * (float)(bin + 1)), 0, hgt};
      at += cnt;
    }
    s_i[0] = nodes;
  }
  __syncthreads();
  for (int bin = wave; bin < nini; bin += O_W) {
    int at = cbase[bin];
    for (int p0 = 0; p0 < n; p0 += 64) {
      const int p = p0 + lane;
      const bool in = p < n && min((int)div_rn((float)((int)(xy[min(p, n - 1)] & 0xFFFF) - BORDER), hx), nini - 1) == bin;
      const uint64_t m = __ballot(in);
      if (in) perm[at + __popcll(m & lanes_below())] = (uint16_t)p;
      at += __popcll(m);
    }
  }
  int nA = s_i[0], M = 0;
  __syncthreads();
  int* order = nullptr;  // phase 2 leaves the list's order here; phase 1 leaves the table in it
  for (;;) {
    // a phase-1 sweep (:594-645): every node that may be divided, a wave each
    for (int i = wave; i < nA; i += O_W) {
      const Node nd = TA[i];
      if (nd.count == 1) continue;
      int c[4];
      divide(nd, xy, perm, tmp, c);
      if (lane < 4) cc[4 * i + lane] = lane == 0 ? c[0] : lane == 1 ? c[1] : lane == 2 ? c[2] : c[3];
    }
    __syncthreads();
    if (wave == 0) {  // a child's rank in creation order, a bNoMore node's rank among its kind
      int cb = 0, nb = 0, nexp = 0;
      for (int i0 = 0; i0 < nA; i0 += 64) {
        const int i = i0 + lane;
        int nch = 0, nm = 0, ne = 0;
        if (i < nA) {
          if (TA[i].count == 1)
            nm = 1;
          else
            for (int q = 0; q < 4; ++q) {
              nch += cc[4 * i + q] > 0;
              ne += cc[4 * i + q] > 1;
            }
        }
        int sch = nch, snm = nm;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t0 = __shfl_up(sch, o, 64), t1 = __shfl_up(snm, o, 64);
          if (lane >= o) {
            sch += t0;
            snm += t1;
          }
          ne += __shfl_xor(ne, o, 64);
        }
        if (i < nA) {
          cbase[i] = cb + sch - nch;
          nbase[i] = nb + snm - nm;
        }
        cb += __shfl(sch, 63, 64);
        nb += __shfl(snm, 63, 64);
        nexp += ne;
      }
      if (lane == 0) {
        s_i[0] = cb;
        s_i[1] = nb;
        s_i[2] = nexp;
      }
    }
    __syncthreads();
    M = s_i[0];
    const int size = M + s_i[1], nexp = s_i[2];
    // push_front of every child, the parent erased (:605-643): the children reversed, then the bNoMore nodes as they stood
    for (int i = tid; i < nA; i += O_T) {
      const Node nd = TA[i];
      if (nd.count == 1) {
        TB[M + nbase[i]] = nd;
      } else {
        int c = cbase[i], st = nd.start;
        for (int q = 0; q < 4; ++q) {
          const int cnt = cc[4 * i + q];
          if (cnt > 0) TB[M - 1 - c++] = child_of(nd, q, st, cnt);
          st += cnt;
        }
      }
    }
    __syncthreads();
    {
      Node* t = TA;
      TA = TB;
      TB = t;
    }
    const int prev = nA;
    nA = size;
    if (nA >= Nl || nA == prev) break;  // :649
    if (nA + 3 * nexp > Nl) {           // :653: phase 2, one node at a time, wave 0 alone
      int *nxt = (int*)TB, *prv = nxt + NC, *cur = prv + NC, *old = cur + NC, *ord = old + NC;
      order = ord;
      if (wave == 0) {
        for (int i = lane; i < nA; i += 64) {
          nxt[i] = i + 1 < nA ? i + 1 : -1;
          prv[i] = i - 1;
        }
        int ncur = 0;  // vSizeAndPointerToNode in creation order: the table's first M entries from the back
        for (int c0 = 0; c0 < M; c0 += 64) {
          const int c = c0 + lane, idx = M - 1 - c;
          const bool e = c < M && TA[idx].count > 1;
          const uint64_t m = __ballot(e);
          if (e) cur[ncur + __popcll(m & lanes_below())] = (int)((uint32_t)TA[idx].count << 16 | (uint32_t)idx);  // size | node: the choice below reads no table
          ncur += __popcll(m);
        }
        mem_sync();
        int head = 0, size2 = nA, nid = nA;
        for (bool fin = false; !fin;) {
          const int prev2 = size2, nold = ncur;
          {
            int* t = cur;
            cur = old;
            old = t;
          }
          ncur = 0;
          for (int step = 0; step < nold; ++step) {
            // the largest first; among equal sizes the node created last (declared deviation 1 of the octree)
            int bc = -1, bj = -1;
            for (int j = lane; j < nold; j += 64) {
              const uint32_t e = (uint32_t)old[j];  // 0: divided already
              const int cnt = e ? (int)(e >> 16) : -1;
              if (cnt >= bc) {  // (j ascends)
                bc = cnt;
                bj = j;
              }
            }
            const int mc = wave_max(bc), j = wave_max(bc == mc ? bj : -1), id = old[j] & 0xFFFF;
            const Node nd = TA[id];
            int c[4];
            divide(nd, xy, perm, tmp, c);
            const int nch = (c[0] > 0) + (c[1] > 0) + (c[2] > 0) + (c[3] > 0);
            const int pn = nxt[id], pp = prv[id];
            if (lane == 0) {  // erase the parent
              old[j] = 0;
              if (pp >= 0) nxt[pp] = pn;
              if (pn >= 0) prv[pn] = pp;
            }
            if (head == id) head = pn;
            int st = nd.start, k = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              if (c[q] > 0) {
                const int cid = ++k == nch ? id : nid++;  // the last child takes the parent's slot
                if (lane == 0) {
                  TA[cid] = child_of(nd, q, st, c[q]);
                  nxt[cid] = head;
                  prv[cid] = -1;
                  if (head >= 0) prv[head] = cid;
                  if (c[q] > 1) cur[ncur] = (int)((uint32_t)c[q] << 16 | (uint32_t)cid);
                }
                head = cid;
                ncur += c[q] > 1;
              }
              st += c[q];
            }
            mem_sync();
            size2 += nch - 1;
            if (size2 >= Nl) break;  // :706
          }
          fin = size2 >= Nl || size2 == prev2;  // :710
        }
        if (lane == 0) {
          int k = 0;
          for (int id = head; id >= 0; id = nxt[id]) ord[k++] = id;
          s_i[3] = size2;
        }
      }
      __syncthreads();
      nA = s_i[3];
      break;
    }
  }
  // the key of maximum response per node, the first of equals (:720-734); a wave per node
  for (int k = wave; k < nA; k += O_W) {
    const Node nd = TA[order ? order[k] : k];
    int br = -1, bp = 0x7FFFFFFF;
    for (int p = lane; p < nd.count; p += 64) {
      const int r = sc[perm[nd.start + p]];
      if (r > br) {  // (p ascends)
        br = r;
        bp = p;
      }
    }
    const int mr = wave_max(br), p = -wave_max(br == mr ? -bp : -0x7FFFFFFF);
    if (lane == 0) {
      const int key = perm[nd.start + p];
      res_xy[k] = xy[key];
      res_sc[k] = sc[key];
    }
  }
  if (tid == 0) A.res_cnt[b * 8 + l] = nA;
}

__global__ __launch_bounds__(256) void k_orb_collect(const DetArgs A, int32_t* __restrict__ kp_xy, int32_t* __restrict__ kp_oct, int32_t* __restrict__ n_kp,
                                                      float* __restrict__ kp_resp, int32_t* __restrict__ level_count, int32_t* __restrict__ stat,
                                                      int32_t* __restrict__ cand_xy, float* __restrict__ cand_resp, int32_t* __restrict__ cand_count) {
  __shared__ int s_red[4], s_tot[8], s_first[9], s_mask;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    int mask = 0;
    for (int l = 0; l < 8; ++l) {
      s_tot[l] = l < A.nlevels ? A.tot[b * 8 + l] : 0;
      mask |= s_tot[l] > A.cand_cap ? 1 << l : 0;
    }
    s_first[0] = 0;
    for (int l = 0; l < 8; ++l) s_first[l + 1] = s_first[l] + (l < A.nlevels && !mask ? A.res_cnt[b * 8 + l] : 0);
    s_mask = mask;
  }
  __syncthreads();
  const int n = s_first[8];  // (<= N: the host has checked N against the levels' bounds)
  for (int i = tid; i < A.N; i += 256) {
    int l = -1, x = -1, y = -1;
    float r = 0.0f;
    if (i < n) {
      l = 0;
      for (int k = 1; k < 8; ++k) l += i >= s_first[k] ? 1 : 0;
      const int64_t at = (int64_t)b * A.res_cap + pick(A.res0, l) + i - s_first[l];
      x = (int)(A.res_xy[at] & 0xFFFF);
      y = (int)(A.res_xy[at] >> 16);
      r = (float)A.res_sc[at];
    }
    const int64_t o = (int64_t)b * A.N + i;
    kp_xy[2 * o] = x;
    kp_xy[2 * o + 1] = y;
    kp_oct[o] = l;
    if (kp_resp) kp_resp[o] = r;
  }
  int fb = 0;
  for (int i = tid; i < A.ncells; i += 256) fb += (A.cellcnt[(int64_t)b * A.ncells + i] & FB_BIT) != 0;
  fb = block_sum(fb, s_red);
  if (tid < 8) {
    if (level_count) level_count[b * 8 + tid] = s_first[tid + 1] - s_first[tid];
    if (cand_count) cand_count[b * 8 + tid] = s_tot[tid];
  }
  if (tid == 0) {
    n_kp[b] = n;
    if (stat) {
      int cands = 0;
      for (int l = 0; l < 8; ++l) cands += s_tot[l];
      stat[b * 4] = cands;
      stat[b * 4 + 1] = fb;
      stat[b * 4 + 2] = n;
      stat[b * 4 + 3] = s_mask;
    }
  }
  if (cand_xy || cand_resp)
    for (int64_t i = tid; i < (int64_t)8 * A.cand_cap; i += 256) {
      const int l = (int)(i / A.cand_cap), j = (int)(i % A.cand_cap);
      const bool have = j < min(s_tot[l], A.cand_cap);
      const int64_t at = (int64_t)b * 8 * A.cand_cap + i;
      const uint32_t k = have ? A.cand_xy[at] : 0;
      if (cand_xy) {
        cand_xy[2 * at] = have ? (int)(k & 0xFFFF) : -1;
        cand_xy[2 * at + 1] = have ? (int)(k >> 16) : -1;
      }
      if (cand_resp) cand_resp[at] = have ? (float)A.cand_sc[at] : 0.0f;
    }
}

// mvScaleFactor (:413-416)
void scale_table(double scale_factor, float* sf) {
  sf[0] = 1.0f;
  for (int l = 1; l < 8; ++l) sf[l] = (float)((double)sf[l - 1] * scale_factor);
}

int check_levels(const gl_image_pyramid* pyr, const char*& why) {
  if (!(pyr->nlevels >= 1 && pyr->nlevels <= 8 && pyr->frame_stride >= 0)) {
    why = "pyramid: nlevels outside 1 .. 8 or a negative frame stride";
    return 1;
  }
  for (int l = 0; l < pyr->nlevels; ++l)
    if (!(pyr->width[l] >= 1 && pyr->height[l] >= 1 && pyr->width[l] <= 32767 && pyr->height[l] <= 32767 && pyr->stride[l] >= pyr->width[l] &&
          pyr->offset[l] >= 0)) {
      why = "pyramid: a level with width / height outside 1 .. 32767, stride < width or a negative offset";
      return 1;
    }
  return 0;
}

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int gl_orb_pyramid_layout(int width, int height, int nlevels, double scale_factor, int row_pad, int64_t lead, gl_image_pyramid* pyr) {
  GL_REQUIRE(pyr, "null argument");
  GL_REQUIRE(width >= 1 && height >= 1 && width <= 32767 && height <= 32767 && nlevels >= 1 && nlevels <= 8 && row_pad >= 0 && lead >= 0,
             "width / height outside 1 .. 32767, nlevels outside 1 .. 8, or a negative row_pad / lead");
  GL_REQUIRE(std::isfinite(scale_factor) && scale_factor >= 1.0, "scale factor must be finite and >= 1");
  float sf[8];
  scale_table(scale_factor, sf);
  gl_image_pyramid p = {};
  p.nlevels = nlevels;
  int64_t at = lead;
  for (int l = 0; l < nlevels; ++l) {
    const float inv = 1.0f / sf[l];  // :423
    p.width[l] = (int)nearbyintf((float)width * inv);  // :1059-1060, cvRound: half to even
    p.height[l] = (int)nearbyintf((float)height * inv);
    GL_REQUIRE(p.width[l] >= 1 && p.height[l] >= 1, "a level comes out empty");
    p.stride[l] = p.width[l] + row_pad;
    p.offset[l] = at;
    at += p.stride[l] * p.height[l];
  }
  p.frame_stride = at;
  p.data = pyr->data;
  *pyr = p;
  return GL_OK;
}

int gl_orb_features_per_level(int nfeatures, int nlevels, double scale_factor, int32_t* out) {
  GL_REQUIRE(out, "null argument");
  GL_REQUIRE(nfeatures >= 0 && nlevels >= 1 && nlevels <= 8, "nfeatures < 0 or nlevels outside 1 .. 8");
  GL_REQUIRE(std::isfinite(scale_factor) && scale_factor > 1.0, "scale factor must be finite and above 1");
  const float factor = (float)(1.0 / scale_factor);  // :430: 1.0f / (double)scaleFactor
  float desired = (float)nfeatures * (1.0f - factor);
  desired = desired / (1.0f - (float)pow((double)factor, (double)nlevels));  // :431-433
  int sum = 0;
  for (int l = 0; l < nlevels - 1; ++l) {
    out[l] = (int32_t)nearbyintf(desired);
    sum += out[l];
    desired = desired * factor;
  }
  out[nlevels - 1] = std::max(nfeatures - sum, 0);
  return GL_OK;
}

int gl_orb_pyramid(gl_ctx_t* ctx, int B, const gl_image_pyramid* pyr, double scale_factor) {
  GL_REQUIRE(ctx && pyr && pyr->data, "null argument");
  GL_REQUIRE(B >= 1 && B <= 65535, "bad B");
  const char* why = nullptr;
  if (check_levels(pyr, why)) GL_REQUIRE(false, why);
  gl_image_pyramid want = {};
  if (int rc = gl_orb_pyramid_layout(pyr->width[0], pyr->height[0], pyr->nlevels, scale_factor, 0, 0, &want)) return rc;
  int64_t lo[8], hi[8], end = 0;
  for (int l = 0; l < pyr->nlevels; ++l) {
    GL_REQUIRE(pyr->width[l] == want.width[l] && pyr->height[l] == want.height[l], "pyramid: a level's size is not the layout rule's");
    lo[l] = pyr->offset[l];
    hi[l] = pyr->offset[l] + (int64_t)(pyr->height[l] - 1) * pyr->stride[l] + pyr->width[l];
    end = std::max(end, hi[l]);
    for (int k = 0; k < l; ++k) GL_REQUIRE(hi[k] <= lo[l] || hi[l] <= lo[k], "pyramid: two levels overlap");
  }
  GL_REQUIRE(B == 1 || pyr->frame_stride >= end, "pyramid: the frames overlap");
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  for (int l = 1; l < pyr->nlevels; ++l) {  // :1069: each level from the one before it
    const int sw = pyr->width[l - 1], sh = pyr->height[l - 1], dw = pyr->width[l], dh = pyr->height[l];
    const double scale_x = 1.0 / ((double)dw / (double)sw), scale_y = 1.0 / ((double)dh / (double)sh);
    k_orb_resize<<<dim3((unsigned)(((int64_t)dw * dh + 255) / 256), B), 256, 0, c->stream>>>((uint8_t*)pyr->data, pyr->frame_stride, pyr->offset[l - 1],
                                                                                           pyr->stride[l - 1], sw, sh, pyr->offset[l], pyr->stride[l], dw,
                                                                                           dh, scale_x, scale_y);
    GL_HIP(hipGetLastError());
  }
  return GL_OK;
}

int gl_orb_detect_bound(const gl_image_pyramid* pyr, int nfeatures, double scale_factor, int32_t* per_level) {
  GL_REQUIRE(pyr && per_level, "null argument");
  const char* why = nullptr;
  if (check_levels(pyr, why)) GL_REQUIRE(false, why);
  int32_t nfeat[8];
  if (int rc = gl_orb_features_per_level(nfeatures, pyr->nlevels, scale_factor, nfeat)) return rc;
  for (int l = 0; l < pyr->nlevels; ++l) {
    const int w = pyr->width[l] - 2 * BORDER, h = pyr->height[l] - 2 * BORDER;
    const bool cells = w >= 30 && h >= 30;  // nCols >= 1 and nRows >= 1
    const int nini = cells ? (int)roundf((float)w / (float)h) : 0;  // :535
    per_level[l] = nini >= 1 ? std::max(nfeat[l] + 2, 4 * nini) : 0;
  }
  return GL_OK;
}

int gl_orb_detect(gl_ctx_t* ctx, int B, int N, const gl_image_pyramid* pyr, int nfeatures, double scale_factor, int ini_th, int min_th, int cand_cap,
                  const gl_orb_detect_out* out) {
  GL_REQUIRE(ctx && pyr && out && pyr->data, "null argument");
  GL_REQUIRE(B >= 1 && B <= 65535 && N >= 1, "bad B / N");
  GL_REQUIRE(N <= GL_ORB_MAX, "more than GL_ORB_MAX key-points per image");
  GL_REQUIRE(out->kp_xy && out->kp_oct && out->n_kp, "null output buffer (kp_xy, kp_oct and n_kp are required)");
  GL_REQUIRE(min_th >= 1 && min_th <= ini_th && ini_th <= 254, "thresholds: 1 <= min_th <= ini_th <= 254");
  GL_REQUIRE(cand_cap >= 1 && cand_cap <= 65535, "cand_cap outside 1 .. 65535");
  int32_t bound[8];
  if (int rc = gl_orb_detect_bound(pyr, nfeatures, scale_factor, bound)) return rc;
  DetArgs A = {};
  if (int rc = gl_orb_features_per_level(nfeatures, pyr->nlevels, scale_factor, A.nfeat)) return rc;
  int64_t mbytes = 0;
  int cells = 0, res = 0, node_cap = 4;
  for (int l = 0; l < pyr->nlevels; ++l) {
    A.width[l] = pyr->width[l];
    A.height[l] = pyr->height[l];
    A.stride[l] = pyr->stride[l];
    A.offset[l] = pyr->offset[l];
    A.moffset[l] = mbytes;
    mbytes += (int64_t)pyr->width[l] * pyr->height[l];
    const float width = (float)(pyr->width[l] - 2 * BORDER), height = (float)(pyr->height[l] - 2 * BORDER);  // :755-756
    const int ncols = (int)(width / 30.0f), nrows = (int)(height / 30.0f);                                    // :758-759
    A.cell0[l] = cells;
    A.res0[l] = res;
    if (ncols >= 1 && nrows >= 1) {  // (deviation: the reference divides by zero)
      A.ncols[l] = ncols;
      A.nrows[l] = nrows;
      A.wcell[l] = (int)ceilf(width / (float)ncols);  // :760-761
      A.hcell[l] = (int)ceilf(height / (float)nrows);
      GL_REQUIRE(A.wcell[l] <= CELL_MAX && A.hcell[l] <= CELL_MAX, "a cell above 59 px");
      cells += ncols * nrows;
      A.nini[l] = (int)roundf(width / height);  // :535
      if (A.nini[l] >= 1) A.hx[l] = width / (float)A.nini[l];  // :537
      GL_REQUIRE(A.nini[l] <= 1024, "a level more than 1 024 times as wide as tall");
    }
    res += bound[l];
    node_cap = std::max(node_cap, bound[l] + 2);
  }
  for (int l = pyr->nlevels; l < 8; ++l) {
    A.cell0[l] = cells;
    A.res0[l] = res;
  }
  GL_REQUIRE(N >= res, "N is below the sum of the levels' bounds max(N_l + 2, 4 nIni_l) (gl_orb_detect_bound)");
  A.nlevels = pyr->nlevels;
  A.N = N;
  A.cand_cap = cand_cap;
  A.ini_th = ini_th;
  A.min_th = min_th;
  A.ncells = cells;
  A.res_cap = std::max(res, 1);
  A.node_cap = node_cap;
  A.frame_stride = pyr->frame_stride;
  A.mframe = mbytes;
  A.data = pyr->data;
  // the octree's working set: perm, tmp; two node tables; the children's sizes; two rank arrays
  const size_t capa = ((size_t)cand_cap + 7) & ~(size_t)7;
  const size_t ws = align16(2 * capa * sizeof(uint16_t) + (size_t)node_cap * (2 * sizeof(Node) + 6 * sizeof(int)));
  const bool in_lds = ws <= (size_t)LDS_DYN_MAX;
  // the main scratch block
  size_t at = 0;
  auto take = [&at](size_t bytes) {
    const size_t o = at;
    at = align16(at + bytes);
    return o;
  };
  const size_t o_map = take((size_t)B * mbytes), o_cnt = take((size_t)B * std::max(cells, 1) * 4), o_cxy = take((size_t)B * 8 * cand_cap * 4),
               o_csc = take((size_t)B * 8 * cand_cap), o_tot = take((size_t)B * 8 * 4), o_rcnt = take((size_t)B * 8 * 4),
               o_rxy = take((size_t)B * A.res_cap * 4), o_rsc = take((size_t)B * A.res_cap), o_ws = take(in_lds ? 0 : (size_t)B * 8 * ws);
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  void* scratch = nullptr;
  if (int rc = gl::ctx_scratch(c, at, &scratch)) return rc;
  char* s = (char*)scratch;
  A.map = (uint8_t*)(s + o_map);
  A.cellcnt = (int32_t*)(s + o_cnt);
  A.cand_xy = (uint32_t*)(s + o_cxy);
  A.cand_sc = (uint8_t*)(s + o_csc);
  A.tot = (int32_t*)(s + o_tot);
  A.res_cnt = (int32_t*)(s + o_rcnt);
  A.res_xy = (uint32_t*)(s + o_rxy);
  A.res_sc = (uint8_t*)(s + o_rsc);
  if (cells > 0) {
    k_orb_fast<<<dim3(cells, B), F_T, 0, c->stream>>>(A);
    GL_HIP(hipGetLastError());
    k_orb_gather<<<dim3(cells, B), F_T, 0, c->stream>>>(A);
    GL_HIP(hipGetLastError());
  }
  k_orb_octree<<<dim3(pyr->nlevels, B), O_T, in_lds ? ws : 0, c->stream>>>(A, s + o_ws, (int64_t)ws, in_lds ? 1 : 0);
  GL_HIP(hipGetLastError());
  k_orb_collect<<<B, 256, 0, c->stream>>>(A, out->kp_xy, out->kp_oct, out->n_kp, out->kp_response, out->level_count, out->stat, out->cand_xy,
                                          out->cand_resp, out->cand_count);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

}  // extern "C"
