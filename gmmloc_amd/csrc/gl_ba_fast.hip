// Single-pose structure-constrained refinement, on-chip fast path: the instances of gl_ba_fast_impl.hpp
// (DENSE by LDS class, SPREAD; exact fp64 point step, and the fp32-cached step as an option) + the launcher.
#include <algorithm>
#include <cstdlib>

#include "gl_ba_common.hpp"

using namespace gld;
using namespace glba;

// ---- launch scratch and its producer ------------------------------------------------------------------------------
// Per point of the launch, in the PERMUTED order of its frame: the observation in normalised image coordinates (24 B),
// the original index (perm), the flag word, the gated association: 36 B.  (The plane record {n, n.mu} of a point's
// component is NOT copied per point: the passes fetch it from the map's K x 4 table by the association - 128 KB shared
// by every frame of an XCD instead of 64 KB per frame, which is what lets the per-pass streams of the 32 frames of an
// XCD stay in its 4 MB L2: fabric-side reads 12.0 -> 0.6 GB per launch.)
namespace {
struct PrepView {
  double* gobn;
  int32_t* perm;
  int32_t* pfl;
  int32_t* assoc_p;
};
// Fixed observer key-frames of an anchored launch (kFixed instances of the refine), written by k_ba1_prep into the launch's
// scratch: the key-frames' poses as {R, t}; per point and key-frame - SoA by key-frame, the frame's permuted point order -
// the normalised observation, octave | stereo << 4 (-1: not observed) and the edge's stale chi2; ferase: the caller's output.
struct FixedV {
  int F;
  double* fRt;         // B x F x 12
  double* fobn;        // B x F x L x 3
  int32_t* foct;       // B x F x L
  double* chif;        // B x F x L
  uint8_t* ferase;     // B x L x F (caller's order) or null
};
// the ONE argument of k_ba1_fast (the kernel re-reads its fields from the kernel-argument segment for every frame it draws)
struct BafKArgs {
  glba::BaK k;
  glba::GmmDev gm;
  int B, L, G, S;
  double* pose_io;
  double* pts_io;
  int32_t* assoc_all;
  uint8_t* dropped_all;
  uint8_t* erase_all;
  int32_t* iters_out;
  double* pn_all;
  int32_t* trials_out;
  int NB;
  unsigned long long* parts;
  int* ctl;
  long long limit;
  int xcc_trusted;
  const int32_t* oct_all;
  const uint8_t* prior_all;
  double* prior_mi;
  double* stage;
  int nb_prev;
  int32_t* counters;
  int32_t* outer_out;
  FixedV fxv;
  int32_t* edges_out;
  int* frame_ctr;
  // the fused front (kFront instances, ba1_front): != 0 - the refine makes each frame's records in its own set-up, k_ba1_prep does not
  // run; pn_all then holds one set of records per WORKGROUP of the launch.  obs_all, d2_all: the inputs k_ba1_prep would have read.
  int front, nwg;  // (nwg: the workgroups of the launch)
  const double* obs_all;
  const double* d2_all;
};
__host__ __device__ inline PrepView prep_view(double* scratch, int B, int L) {
  PrepView v;
  const size_t n = (size_t)B * L;
  v.gobn = scratch;
  v.perm = (int32_t*)(scratch + n * 3);
  v.pfl = v.perm + n;
  v.assoc_p = v.pfl + n;
  return v;
}

// Set-up of a refine launch, one workgroup per frame: the association gate chi2 <= 9 (checkMapAssociation,
// gmmloc_opt.cpp:230-232), the flag word of every point, its normalised observation - and the ORDER the
// refine walks the frame in: a stable partition that puts the points associated with a NON-degenerate component (the
// volumetric ~5 % of a map, whose EdgePt2Gaussian needs the full 3x3 block R L L^T R^T instead of a rank-1 plane term)
// behind all the others.  A wave of 64 consecutive points then takes the expensive branch only in the last chunk or two of
// a frame instead of in 96 % of its slots (one such lane was enough to make the wave issue ~100 extra instructions per
// point and pass).  The order is a function of the frame's data alone, so the canonical summation order built on it stays
// independent of the launch shape and of the batch.
// A: the refine's arguments (k_ba1_prep writes the records, exchange words, inverse measurements and fixed-observer records they
// point to); beside them the caller's observations, Mahalanobis distances and fixed-observer inputs, and the frame queue.
constexpr int PREP_T = 256, PREP_C = 8;  // rounds of 256 consecutive points: frames up to 2 048 points
__global__ __launch_bounds__(PREP_T) void k_ba1_prep(BafKArgs A, const double* __restrict__ obs_all, const double* __restrict__ d2_all,
                                                    gl::TrackFixed fin, int* __restrict__ frame_ctr) {
  __shared__ int cnt[PREP_C][PREP_T / 64];   // non-degenerate-component points per (round, wave)
  __shared__ int cnt0[PREP_C][PREP_T / 64];  // slots WITHOUT a map point per (round, wave) (round 6: they go last, see below)
  const BaK& k = A.k;
  const int B = A.B, L = A.L, F = A.fxv.F;
  const int32_t* const oct_all = A.oct_all;
  int32_t* const assoc_all = A.assoc_all;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (f >= B) return;
  if (f == 0 && tid == 0) *frame_ctr = 0;  // the queue the refine's persistent workgroups draw their frames from
  if (A.parts) {  // latency shape next: this frame's exchange words and {abort, done} start at zero (no separate memset)
    const int nxw = 2 * A.G * 64;
    for (int i = tid; i < nxw; i += PREP_T) A.parts[(size_t)f * nxw + i] = 0ull;
    if (tid < 2) A.ctl[2 * f + tid] = 0;
  }
  if (A.prior_all && A.prior_all[f] && tid == 0) {  // EdgeSE3QuatPrior::_inverseMeasurement of the frame's INPUT pose, as {R, t}
    const SE3 Ti = se3_inverse(se3_load(A.pose_io + (size_t)f * 7));
    double Ri[9];
    qtoR(Ti.r, Ri);
#pragma unroll
    for (int i = 0; i < 9; ++i) A.prior_mi[(size_t)f * 12 + i] = Ri[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) A.prior_mi[(size_t)f * 12 + 9 + i] = Ti.t[i];
  }
  if (F > 0 && tid < F) {  // the fixed key-frames' poses T_cw as {R, t}
    const SE3 T = se3_load(fin.pose + ((size_t)f * F + tid) * 7);
    double Rm[9];
    qtoR(T.r, Rm);
    double* o = A.fxv.fRt + ((size_t)f * F + tid) * 12;
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = Rm[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) o[9 + i] = T.t[i];
  }
  const size_t gbase = (size_t)f * L;
  const PrepView pv = prep_view(A.pn_all, B, L);
  const int rounds = (L + PREP_T - 1) / PREP_T;
  // round j, thread t: point j 256 + t (coalesced); index order = (round, wave, lane)
  int a_[PREP_C], fl_[PREP_C];
#pragma unroll
  for (int j = 0; j < PREP_C; ++j) {
    const int l = j * PREP_T + tid;
    a_[j] = -1;
    fl_[j] = 0;
    if (j < rounds && l < L) {
      const size_t g = gbase + l;
      const int oc = oct_all[g];
      int a = assoc_all[g];
      if (d2_all && k.gate_chi2 >= 0 && !(d2_all[g] <= k.gate_chi2)) a = -1;
      if (oc < 0) a = -1;
      assoc_all[g] = a;  // the gated association, in the caller's order (the refine writes the final one)
      int fl = 0;
      if (oc >= 0) {
        fl = 1 | ((oc & 7) << 8);                              // F_EXISTS, octave
        if (!(obs_all[g * 3 + 2] < 0)) fl |= 2;                // F_STEREO
        if (a >= 0) fl |= 4 | ((A.gm.flags[a] & 1) ? 8 : 0);   // F_ASSOC, F_DEG
      }
      a_[j] = a;
      fl_[j] = fl;
    }
    const unsigned long long bal = __ballot((fl_[j] & 12) == 4);  // associated and not degenerate
    const unsigned long long bal0 = __ballot(fl_[j] == 0 && j < rounds && j * PREP_T + tid < L);  // no map point in the slot
    if (lane == 0) {
      cnt[j][wave] = __popcll(bal);
      cnt0[j][wave] = __popcll(bal0);
    }
  }
  __syncthreads();
  int total = 0, total0 = 0;
#pragma unroll
  for (int j = 0; j < PREP_C; ++j)
#pragma unroll
    for (int w = 0; w < PREP_T / 64; ++w) {
      total += cnt[j][w];
      total0 += cnt0[j][w];
    }
  // Round 6: a stable partition in THREE classes - the points of planar components (and the unassociated ones), the points of
  // non-degenerate components, the slots without a map point.  The reference's frame has one slot per FEATURE (1 200) and a few hundred
  // map points: with the empty slots LAST the chunks behind the frame's points hold nothing, every wave skips them with one test
  // (load_pt: no active edge in any lane), and since a group's chunks are interleaved (g, g + G, ...) the points still spread evenly
  // over the waves - the refine costs what its POINTS cost, not what its slots cost (profiles/r6_track_sparse.txt).
  const int n_others = L - total - total0, n_exist = L - total0;
  const double ifx = 1.0 / k.fx, ify = 1.0 / k.fy;
  int base = 0, base0 = 0;  // non-degenerate-component points / empty slots before this (round, wave)
#pragma unroll
  for (int j = 0; j < PREP_C; ++j) {
#pragma unroll
    for (int w = 0; w < PREP_T / 64; ++w)
      if (w < wave) {
        base += cnt[j][w];
        base0 += cnt0[j][w];
      }
    const int l = j * PREP_T + tid;
    const bool isnd = (fl_[j] & 12) == 4;
    const bool isempty = fl_[j] == 0 && j < rounds && l < L;
    const unsigned long long bal = __ballot(isnd), bal0 = __ballot(isempty);
    const int before = base + __popcll(bal & ((1ull << lane) - 1ull));
    const int before0 = base0 + __popcll(bal0 & ((1ull << lane) - 1ull));
    if (j < rounds && l < L) {
      const int lp = isempty ? n_exist + before0 : isnd ? n_others + before : l - before - before0;  // stable in all three classes
      const size_t g = gbase + l, gp = gbase + lp;
      pv.perm[gp] = l;
      pv.pfl[gp] = fl_[j];
      pv.assoc_p[gp] = a_[j];
      pv.gobn[gp * 3] = (obs_all[g * 3] - k.cx) * ifx;
      pv.gobn[gp * 3 + 1] = (obs_all[g * 3 + 1] - k.cy) * ify;
      pv.gobn[gp * 3 + 2] = (obs_all[g * 3 + 2] - k.cx) * ifx;
      for (int kf = 0; kf < F; ++kf) {  // the point's observations by the fixed key-frames, by key-frame, in the permuted order
        const size_t src = g * F + kf, dst = ((size_t)f * F + kf) * L + lp;
        const int fo = fl_[j] ? fin.oct[src] : -1;
        const double u = fin.obs[src * 3], v = fin.obs[src * 3 + 1], ur = fin.obs[src * 3 + 2];
        A.fxv.fobn[dst * 3] = (u - k.cx) * ifx;
        A.fxv.fobn[dst * 3 + 1] = (v - k.cy) * ify;
        A.fxv.fobn[dst * 3 + 2] = (ur - k.cx) * ifx;
        A.fxv.foct[dst] = fo < 0 ? -1 : ((fo & 7) | (!(ur < 0) ? 16 : 0));
        A.fxv.chif[dst] = 0.0;
      }
    }
#pragma unroll
    for (int w = 0; w < PREP_T / 64; ++w)
      if (w >= wave) {  // the rest of this round: the bases now count everything before round j + 1
        base += cnt[j][w];
        base0 += cnt0[j][w];
      }
  }
}
}  // namespace

// The instances of gl_ba_fast_impl.hpp: per namespace, its LDS capacity in points, waves at most, SPREAD (latency shape) or DENSE,
// fp32-cached point step (option ba_step32), gauge anchor of the pose (prior edge / fixed pose), fixed observer key-frames, and
// `wide`: the plain DENSE instance for maps of more than 65 536 components (the others keep a thread's associations in registers,
// 16 bits each).
// -DGL_BAF_QUICK builds the first two alone (tools/baf_quick.sh: register / ISA checks).
namespace {
struct BafCfg {
  int mcap, nw;
  bool spread, step32, prior, fixed, wide;
};
// the instances that carry the fused front (kFront): plain DENSE and its wide twins
constexpr bool baf_front(const BafCfg& c) { return !c.spread && !c.step32 && !c.prior && !c.fixed; }
namespace bafd2000 { constexpr BafCfg kCfg{2000, 8, false, false, false, false, false}; }     // DENSE, exact step: 1 frame per CU
namespace bafs { constexpr BafCfg kCfg{256, 8, true, false, false, false, false}; }           // SPREAD, exact step
#ifndef GL_BAF_QUICK
namespace bafd496 { constexpr BafCfg kCfg{496, 2, false, false, false, false, false}; }       // 4 frames per CU
namespace bafd1000 { constexpr BafCfg kCfg{1000, 4, false, false, false, false, false}; }     // 2 frames per CU
namespace bafs32 { constexpr BafCfg kCfg{256, 8, true, true, false, false, false}; }          // fp32-cached step: the SPREAD kernel
namespace bafd2000s32 { constexpr BafCfg kCfg{2000, 8, false, true, false, false, false}; }   // ... and the largest DENSE class
namespace bafd496p { constexpr BafCfg kCfg{496, 2, false, false, true, false, false}; }       // anchored (gl_track_frames_anchored), exact step
namespace bafd1000p { constexpr BafCfg kCfg{992, 4, false, false, true, false, false}; }      // (992: two frames per CU with the prior edge's records)
namespace bafd2000p { constexpr BafCfg kCfg{2000, 8, false, false, true, false, false}; }
namespace bafsp { constexpr BafCfg kCfg{256, 8, true, false, true, false, false}; }
namespace bafd496f { constexpr BafCfg kCfg{496, 2, false, false, true, true, false}; }        // anchored with fixed observer key-frames (F = 1 .. 4),
namespace bafd1000f { constexpr BafCfg kCfg{984, 4, false, false, true, true, false}; }       // batch shape (984: with the key-frames' poses too)
namespace bafd2000f { constexpr BafCfg kCfg{2000, 8, false, false, true, true, false}; }
namespace bafd496w { constexpr BafCfg kCfg{496, 2, false, false, false, false, true}; }       // plain DENSE for maps of more than 65 536 components
namespace bafd1000w { constexpr BafCfg kCfg{1000, 4, false, false, false, false, true}; }
namespace bafd2000w { constexpr BafCfg kCfg{2000, 8, false, false, false, false, true}; }
#endif
}  // namespace
#define GL_BAF_NS bafd2000
#include "gl_ba_fast_impl.hpp"
#define GL_BAF_NS bafs
#include "gl_ba_fast_impl.hpp"
#ifndef GL_BAF_QUICK
#define GL_BAF_NS bafd496
#include "gl_ba_fast_impl.hpp"
#define GL_BAF_NS bafd1000
#include "gl_ba_fast_impl.hpp"
#define GL_BAF_NS bafs32
#include "gl_ba_fast_impl.hpp"
#define GL_BAF_NS bafd2000s32
#include "gl_ba_fast_impl.hpp"
#define GL_BAF_NS bafd496p
#include "gl_ba_fast_impl.hpp"
#define GL_BAF_NS bafd1000p
#include "gl_ba_fast_impl.hpp"
#define GL_BAF_NS bafd2000p
#include "gl_ba_fast_impl.hpp"
#define GL_BAF_NS bafsp
#include "gl_ba_fast_impl.hpp"
#define GL_BAF_NS bafd496f
#include "gl_ba_fast_impl.hpp"
#define GL_BAF_NS bafd1000f
#include "gl_ba_fast_impl.hpp"
#define GL_BAF_NS bafd2000f
#include "gl_ba_fast_impl.hpp"
#define GL_BAF_NS bafd496w
#include "gl_ba_fast_impl.hpp"
#define GL_BAF_NS bafd1000w
#include "gl_ba_fast_impl.hpp"
#define GL_BAF_NS bafd2000w
#include "gl_ba_fast_impl.hpp"
namespace {
// HW_REG_XCC_ID (hwreg 20, 4 bits): the XCD the wave runs on
__device__ __forceinline__ int xcc_id() { return __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 15; }
__global__ void k_xcc_probe(int* out) {
  if (threadIdx.x == 0) out[blockIdx.x] = xcc_id();
}
}  // namespace

namespace gl {

// The same-XCD form of the latency shape's exchange (plain stores that stay in the XCD's L2, read by L1-bypassing loads)
// is only valid if the workgroups of a frame really share an XCD.  The kernel checks that at run time with the XCC ids
// its workgroups report; this probe decides whether those reports can be trusted at all: 64 blocks must report ids in
// 0..7, block b the same as block b % 8, and the eight residues eight different ones (the known placement of this
// hardware).  Anything else - another partition mode, another device - leaves the device-scope form in place.
bool probe_xcc_ids(Ctx* c) {
  int* d = nullptr;
  if (hipMalloc((void**)&d, 64 * sizeof(int)) != hipSuccess) return false;
  int h[64];
  bool ok = hipMemsetAsync(d, 0xff, 64 * sizeof(int), c->stream) == hipSuccess;
  if (ok) {
    k_xcc_probe<<<64, 64, 0, c->stream>>>(d);
    ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
         hipStreamSynchronize(c->stream) == hipSuccess;
  }
  (void)hipFree(d);
  if (!ok) return false;
  unsigned seen = 0;
  for (int b = 0; b < 64; ++b) {
    if (h[b] < 0 || h[b] > 7 || h[b] != h[b & 7]) return false;
    seen |= 1u << h[b];
  }
  return seen == 0xffu;
}

bool ba1_fast_supported(int L) { return L <= 2000; }

// the canonical summation order of a frame of stride L (gl_ba_fast_impl.hpp): G groups of S chunks of 64 points
static void canon_order(int L, int* G, int* S) {
  const int nch = (L + 63) / 64;
  *G = (nch + 3) / 4;
  *S = (nch + *G - 1) / *G;
}

struct BafInst {
  BafCfg cfg;
  void (*kern)(BafKArgs);
  size_t lds;  // dynamic LDS of a workgroup (the carve of ba1_fast_frame)
};
static const BafInst kBafInst[] = {
    {bafd2000::kCfg, bafd2000::k_ba1_fast, bafd2000::kLdsBytes},
    {bafs::kCfg, bafs::k_ba1_fast, bafs::kLdsBytes},
    {bafd496::kCfg, bafd496::k_ba1_fast, bafd496::kLdsBytes},
    {bafd1000::kCfg, bafd1000::k_ba1_fast, bafd1000::kLdsBytes},
    {bafs32::kCfg, bafs32::k_ba1_fast, bafs32::kLdsBytes},
    {bafd2000s32::kCfg, bafd2000s32::k_ba1_fast, bafd2000s32::kLdsBytes},
    {bafd496p::kCfg, bafd496p::k_ba1_fast, bafd496p::kLdsBytes},
    {bafd1000p::kCfg, bafd1000p::k_ba1_fast, bafd1000p::kLdsBytes},
    {bafd2000p::kCfg, bafd2000p::k_ba1_fast, bafd2000p::kLdsBytes},
    {bafsp::kCfg, bafsp::k_ba1_fast, bafsp::kLdsBytes},
    {bafd496f::kCfg, bafd496f::k_ba1_fast, bafd496f::kLdsBytes},
    {bafd1000f::kCfg, bafd1000f::k_ba1_fast, bafd1000f::kLdsBytes},
    {bafd2000f::kCfg, bafd2000f::k_ba1_fast, bafd2000f::kLdsBytes},
    {bafd496w::kCfg, bafd496w::k_ba1_fast, bafd496w::kLdsBytes},
    {bafd1000w::kCfg, bafd1000w::k_ba1_fast, bafd1000w::kLdsBytes},
    {bafd2000w::kCfg, bafd2000w::k_ba1_fast, bafd2000w::kLdsBytes},
};
// The instance a launch takes: the flags of the launch, the smallest LDS class that holds the points of a workgroup (DENSE: the
// frame, SPREAD: one group).  The fixed-observer instances carry the anchored code (the prior is a per-frame flag); the anchored
// instances exist with the exact step only.  K: the components of the launch's map (only the plain DENSE instances depend on it).
static const BafInst* baf_instance(const Ctx* c, bool spread, bool prior, int F, int points, int K) {
  const bool anch = prior || F > 0;
  const bool s32 = c->opt.ba_step32 != 0 && !anch;
  const bool wide = !spread && !anch && !s32 && K > 65536;  // (the instances that keep the associations in registers)
  const BafInst* best = nullptr;
  for (const BafInst& in : kBafInst)
    if (in.cfg.spread == spread && in.cfg.step32 == s32 && in.cfg.prior == anch && in.cfg.fixed == (F > 0) && in.cfg.wide == wide &&
        in.cfg.mcap >= points && (!best || in.cfg.mcap < best->cfg.mcap))
      best = &in;
  return best;
}

// Shape: SPREAD when every workgroup of the batch gets a CU of its own (B G <= 2 CUs: the frame-at-a-time caller, small
// batches) and the device holds all of them at once, DENSE otherwise.  Both add in the same order: the choice never shows in
// the results (option ba_shape forces one: 0 DENSE, 1 SPREAD where it fits).  Then the scratch of that shape: only SPREAD has
// exchange words and a staging area.  !fast: the general kernel's regions alone.
// The workgroups of a batch-shaped launch: persistent ones (option ba_persist, default on), as many as the device holds at once,
// drawing their frames from frame_ctr, where the batch is larger than that; else one per frame.
static int dense_grid(Ctx* c, const BafInst* in, int B, int G, int* grid, bool* persistent) {
  GL_HIP(ensure_dynamic_lds(c, (const void*)in->kern, in->lds));
  *grid = B;
  *persistent = false;
  if (c->opt.ba_persist != 0) {
    int occ = 0;
    (void)ctx_occupancy(c, (const void*)in->kern, 64 * G, in->lds, &occ);
    if (occ > 0 && (long)occ * c->ncu < (long)B) {
      *grid = occ * c->ncu;
      *persistent = true;
    }
  }
  return GL_OK;
}

// front_ok: the call is one the fused front serves (track_frames_impl); K: the components of the map.
int ba1_layout(Ctx* c, int B, int L, int F, bool prior, bool fast, Ba1Layout* out, bool front_ok, int K) {
  int G, S;
  canon_order(L, &G, &S);
  bool spread = (long)B * G <= 2 * c->ncu;  // two workgroups of 256 threads fit a CU (LDS 2 x 80 KB, 2 waves per SIMD; checked below)
  if (c->opt.ba_shape == 0) spread = false;
  if (c->opt.ba_shape == 1) spread = true;  // forced (tests); a shape that does not fit the device still goes DENSE
  if (F > 0 || !fast) spread = false;       // (fixed observers: batch-shaped instances only)
  if (spread) {
    const BafInst* in = baf_instance(c, true, prior, 0, 64 * S, 0);
    GL_REQUIRE(in, "no refine instance for this launch");
    GL_HIP(ensure_dynamic_lds(c, (const void*)in->kern, in->lds));
    int occ = 0;
    (void)ctx_occupancy(c, (const void*)in->kern, 256, in->lds, &occ);
    // ... per XCD: the kernel keeps the workgroups of a frame on ONE XCD (frame f -> XCD f % 8), so what has to fit is the
    // ceil(B / 8) frames of an XCD into that XCD's share of the slots (a frame whose siblings queue behind the resident
    // ones would sit in the rendezvous until its time limit and be redone by the follow-up kernel: correct, but slow)
    spread = (long)((B + 7) / 8) * G <= (long)occ * (c->ncu / 8);
  }
  const size_t n = (size_t)B * L;
  Ba1Layout& o = *out;
  o = Ba1Layout{};
  o.spread = spread;
  // The fused front: a batch-shaped launch of an instance that has it (kFront) makes the records of a frame in the refine's own
  // set-up, one set per WORKGROUP of the launch instead of one per frame (option ba_front, default 1; 0: k_ba1_prep, A/B and tests)
  size_t nrec = n;
  if (fast && !spread && front_ok && c->opt.ba_front != 0) {
    const BafInst* in = baf_instance(c, false, prior, F, L, K);
    GL_REQUIRE(in, "no refine instance for this launch");
    if (baf_front(in->cfg)) {
      int grid = 0;
      bool persistent = false;
      const int rc = dense_grid(c, in, B, G, &grid, &persistent);
      if (rc != GL_OK) return rc;
      o.front = true;
      nrec = (size_t)grid * L;
    }
  }
  Regions r{0};
  if (!fast) {
    o.trial = r.take(n * 3 * sizeof(double));
    o.chi = r.take(n * sizeof(double));
    o.lev = r.take(n);
  } else {
    o.rec = r.take(nrec * (3 * sizeof(double) + 3 * sizeof(int32_t)));
    o.frame_ctr = r.take(sizeof(int));
    o.prior_mi = r.take((size_t)B * 12 * sizeof(double));
    if (spread) {
      o.parts = r.take((size_t)B * 2 * G * 64 * sizeof(unsigned long long));
      o.ctl = r.take((size_t)B * 2 * sizeof(int));
      o.stage = r.take(n * (3 * sizeof(double) + sizeof(int32_t)) + (size_t)B * 8 * sizeof(double));
    }
    if (F > 0) {
      o.frt = r.take((size_t)B * F * 12 * sizeof(double));
      o.fobn = r.take(n * F * 3 * sizeof(double));
      o.foct = r.take(n * F * sizeof(int32_t));
      o.chif = r.take(n * F * sizeof(double));
    }
  }
  o.end = r.off;
  return GL_OK;
}

// one workgroup of G waves per frame; LDS class by stride (4 / 2 / 1 frames per CU)
static int launch_dense(Ctx* c, BafKArgs a, int* frame_ctr, int K) {
  const BafInst* in = baf_instance(c, false, a.prior_all != nullptr, a.fxv.F, a.L, K);
  GL_REQUIRE(in, "no refine instance for this launch");
  const int threads = 64 * a.G;
  a.NB = 1;
  a.parts = nullptr;
  int grid = 0;
  bool persistent = false;
  const int rc = dense_grid(c, in, a.B, a.G, &grid, &persistent);
  if (rc != GL_OK) return rc;
  if (persistent) a.frame_ctr = frame_ctr;
  a.nwg = grid;
  GL_REQUIRE(!a.front || baf_front(in->cfg), "refine instance without the fused front");  // (ba1_layout chose the same instance)
  in->kern<<<grid, threads, in->lds, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// Few frames (the frame-at-a-time caller): one point per thread, a workgroup of 256 threads = the <= 4 slot waves of ONE
// group, G workgroups per frame on as many CUs (one wave per SIMD: nothing to share the issue slots with); with G > 1 the
// reductions of a Levenberg trial cross the workgroups through tagged words in global memory.  That needs the workgroups
// of a frame co-resident.  A cooperative launch guarantees it and costs 31 us per call here (0.463 vs 0.432 ms for one
// frame); the kernel is launched plainly instead, with the rendezvous protocol of gld::Coop: a frame whose workgroups do not
// all show up within the time limit (another launch holds the CUs and waits for its own) gives up without writing
// anything, and the one-workgroup kernel that follows redoes exactly those frames - same bits, so the caller never sees
// which kernel answered.  (ba1_layout has checked that the launch fits the device.)
static int launch_spread(Ctx* c, BafKArgs a) {
  const BafInst* in = baf_instance(c, true, a.prior_all != nullptr, 0, 64 * a.S, 0);
  GL_REQUIRE(in, "no refine instance for this launch");
  GL_HIP(ensure_dynamic_lds(c, (const void*)in->kern, in->lds));
  a.NB = a.G;
  a.limit = (long long)(c->opt.ba_rendezvous_us * 100.0);  // wall_clock64() ticks at 100 MHz
  if (c->opt.ba_test_abort_seq > 0) a.limit = -(long long)c->opt.ba_test_abort_seq;  // tests: a give-up in the middle of the schedule
  a.xcc_trusted = (c->xcc_ids_trusted && c->opt.ba_same_xcd != 0) ? 1 : 0;
  // (NB > 1: 64 block indices per 8 frames, the kernel's map from block to (frame, group) keeps a frame on one XCD)
  const int grid = a.NB > 1 ? 64 * ((a.B + 7) / 8) : a.B;
  in->kern<<<grid, 256, in->lds, c->stream>>>(a);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// scratch: laid out by ba1_layout(..., fast = true)
int launch_ba1_fast(Ctx* c, const Gmm* g, const gl_camera* cam, const gl_params* prm, int B, int L, double* pose,
                    double* pts, const double* obs, const int32_t* oct, int32_t* assoc, const double* d2, double gate,
                    uint8_t* dropped, uint8_t* erase, int32_t* iters, char* scratch, const Ba1Layout& lay, const uint8_t* prior,
                    const TrackFixed* fixed) {
  BafKArgs a{};
  a.k = make_bak(cam, prm, gate);
  a.gm = GmmDev{g->rec12, g->axis, g->sqrt_info, g->hgw, g->flags, g->plane4};
  a.B = B;
  a.L = L;
  canon_order(L, &a.G, &a.S);
  a.pose_io = pose;
  a.pts_io = pts;
  a.assoc_all = assoc;
  a.dropped_all = dropped;
  a.erase_all = erase;
  a.iters_out = iters;
  a.pn_all = (double*)(scratch + lay.rec);
  a.trials_out = (c->stats && c->stats_n >= B) ? c->stats : nullptr;
  a.NB = 1;
  a.oct_all = oct;
  a.prior_all = prior;
  a.prior_mi = (double*)(scratch + lay.prior_mi);
  a.counters = c->counters;
  a.outer_out = a.trials_out ? c->stats_iters : nullptr;
  if (fixed)
    a.fxv = FixedV{fixed->F, (double*)(scratch + lay.frt), (double*)(scratch + lay.fobn), (int32_t*)(scratch + lay.foct),
                   (double*)(scratch + lay.chif), fixed->erase};
  a.edges_out = (c->stats_edges && c->stats_edges_n >= B) ? c->stats_edges : nullptr;
  if (lay.spread) {
    a.parts = (unsigned long long*)(scratch + lay.parts);
    a.ctl = (int*)(scratch + lay.ctl);
    a.stage = (double*)(scratch + lay.stage);
  }
  int* const frame_ctr = (int*)(scratch + lay.frame_ctr);
  if (lay.front) {  // the refine's own set-up makes the records (ba1_front): no k_ba1_prep, the frame queue starts at zero
    a.front = 1;
    a.obs_all = obs;
    a.d2_all = d2;
    GL_HIP(hipMemsetAsync(frame_ctr, 0, sizeof(int), c->stream));
    TimerScope ts(c, GL_TIMER_BA);
    return launch_dense(c, a, frame_ctr, g->K);
  }
  {  // set-up: gate, flags, normalised observations, the order the refine walks each frame in - and, before a latency-shape
     // launch, the zeros its exchange words start from
    TimerScope ts(c, GL_TIMER_BA_PREP);
    k_ba1_prep<<<B, PREP_T, 0, c->stream>>>(a, obs, d2, fixed ? *fixed : TrackFixed{}, frame_ctr);
  }
  GL_HIP(hipGetLastError());
  TimerScope ts(c, GL_TIMER_BA);  // the refine kernel proper
  if (!lay.spread) return launch_dense(c, a, frame_ctr, g->K);
  const int rc = launch_spread(c, a);
  if (rc != GL_OK || a.G == 1) return rc;  // (one workgroup per frame: nothing to follow up)
  a.nb_prev = a.G;  // follow-up: staged results of the complete frames -> the caller's buffers, the others redone
  return launch_dense(c, a, frame_ctr, g->K);
}

}  // namespace gl
#endif  // GL_BAF_QUICK
