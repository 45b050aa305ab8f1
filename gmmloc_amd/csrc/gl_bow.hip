// The DBoW2 vocabulary on the device and ORBVocabulary::transform (orb_vocabulary.cpp:20-40 ->
// TemplatedVocabulary::transform(features, v, fv, levelsup), orb_dbow2/include/orb_dbow2/dbow2/TemplatedVocabulary.h:1150-1218, and the
// per-feature descent :1241-1283): the producer of the feature vectors the node matchers read (gl_match_common.hpp: NodeList).
// Integer work throughout; the rules and the declared behaviours are in gmmloc_hip.h.
//
//   k_voc_build    gl_voc_create: the records into layout order - the children of a node contiguous and in child order, so that one
//                  step of the descent is one contiguous gather
//   k_bow_descend  16 lanes (one DPP row) per feature: lane c takes child c, the row's minimum of (distance, child position) is the
//                  reference's `d < best_d` walk; a node of more than 16 children in chunks of 16, ascending.  Six dependent gathers for
//                  the ORB vocabulary: latency bound, so the features of a frame are spread over NF / 16 workgroups
//   k_bow_csr      one workgroup per frame: the kept (node, feature) pairs sorted in LDS, node boundaries, the CSR or the truncation bit
#include <climits>

#include "gl_internal.hpp"
#include "gl_match_common.hpp"

namespace {

using gl_match::hamming256;

constexpr int T_V = 256;
// record i (node i + 1) to layout position pos[i]; link[i]: the layout position of its first child, or the word id of a leaf
__global__ __launch_bounds__(T_V) void k_voc_build(int n_rec, const uint4* __restrict__ desc_in, const float* __restrict__ weight_in,
                                                   const int32_t* __restrict__ pos, const int32_t* __restrict__ nchild,
                                                   const int32_t* __restrict__ link, uint4* __restrict__ desc_out, int4* __restrict__ meta_out) {
  const int i = blockIdx.x * T_V + threadIdx.x;
  if (i >= n_rec) return;
  const size_t at = (size_t)pos[i];
  desc_out[2 * at] = desc_in[2 * (size_t)i];
  desc_out[2 * at + 1] = desc_in[2 * (size_t)i + 1];
  meta_out[at] = make_int4(i + 1, nchild[i], link[i], __float_as_int(weight_in[i]));
}

// minimum over the 16 lanes of a DPP row, in every lane of the row (row_ror:8, 4, 2, 1).  The rows of a wave may have diverged: a row
// reads its own lanes only, and the lanes of a row run together.
__device__ __forceinline__ int row_min16(int v) {
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x128, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x124, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x122, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x121, 0xf, 0xf, false));
  return v;
}

constexpr int T_D = 256, ROW = 16;
// grid (ceil(NF / 16), B).  key_out B x NF: the node of a kept feature (weight > 0), -1 for a stopped word or a padding slot.
__global__ __launch_bounds__(T_D) void k_bow_descend(int NF, int nid_level, int root_children, const uint4* __restrict__ vdesc,
                                                     const int4* __restrict__ vmeta, const uint4* __restrict__ feat_desc,
                                                     const int32_t* __restrict__ feat_oct, int32_t* __restrict__ word_out,
                                                     int32_t* __restrict__ node_out, float* __restrict__ weight_out,
                                                     int32_t* __restrict__ key_out) {
  const int lane = threadIdx.x & (ROW - 1);
  const int i = blockIdx.x * (T_D / ROW) + threadIdx.x / ROW;
  if (i >= NF) return;  // (a whole row)
  const size_t fi = (size_t)blockIdx.y * NF + i;
  if (feat_oct && feat_oct[fi] < 0) {  // padding slot
    if (lane == 0) {
      if (word_out) word_out[fi] = -1;
      if (node_out) node_out[fi] = -1;
      if (weight_out) weight_out[fi] = 0.0f;
      key_out[fi] = -1;
    }
    return;
  }
  const uint4 fa = feat_desc[2 * fi], fb = feat_desc[2 * fi + 1];
  const uint32_t d[8] = {fa.x, fa.y, fa.z, fa.w, fb.x, fb.y, fb.z, fb.w};
  int first = 0, n = root_children, level = 0, nid = 0;  // (`if (nid_level <= 0) *nid = 0`, :1251)
  int4 m;
  for (;;) {
    ++level;
    int best_d = INT_MAX, best_c = 0;
    for (int c0 = 0; c0 < n; c0 += ROW) {  // ascending chunks and a strict compare: the first of equal children wins (:1264-1273)
      const int c = c0 + lane;
      int key = INT_MAX;
      if (c < n) {
        const uint4* p = vdesc + 2 * ((size_t)first + c);
        key = (hamming256(d, p[0], p[1]) << 4) | lane;
      }
      key = row_min16(key);
      if ((key >> 4) < best_d) {
        best_d = key >> 4;
        best_c = c0 + (key & (ROW - 1));
      }
    }
    m = vmeta[(size_t)first + best_c];
    if (level == nid_level) nid = m.x;  // :1275-1276
    if (m.y == 0) break;                // isLeaf(): no children (:1278)
    first = m.z;
    n = m.y;
  }
  if (level < nid_level) nid = m.x;  // DECLARED: a leaf above the level asked for is its own node
  if (lane == 0) {
    const float w = __int_as_float(m.w);
    if (word_out) word_out[fi] = m.z;
    if (node_out) node_out[fi] = nid;
    if (weight_out) weight_out[fi] = w;
    key_out[fi] = w > 0 ? nid : -1;  // `if (w > 0) // not stopped` (:1181, :1209): false for 0.0f, -0.0f and NaN
  }
}

constexpr int T_C = 1024, NF_MAX = GL_BOW_MAX_FEATURES;
// P: the power of two at or above NF.  The pairs are unique, so the sorted order is the std::map's: nodes ascending, the features
// of a node ascending.
__global__ __launch_bounds__(T_C) void k_bow_csr(int NF, int P, int NNcap, const int32_t* __restrict__ key_all, gl_bow_out out) {
  __shared__ uint64_t keys[NF_MAX];
  __shared__ int s_wave[T_C / 64];
  constexpr uint64_t NONE = ~0ull;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int32_t* key_in = key_all + (size_t)f * NF;
  for (int i = tid; i < P; i += T_C) {
    const int node = i < NF ? key_in[i] : -1;
    keys[i] = node >= 0 ? ((uint64_t)node << 12) | (uint64_t)i : NONE;
  }
  __syncthreads();
  // bitonic sort, ascending.  The steps whose partner lies within the wave's 64 keys (distance j <= 32) run in registers, through
  // the wave's lanes, without a barrier between them: 15 of the 66 steps of 2 048 keys are left to LDS.
  for (int k = 2; k <= P; k <<= 1) {
    int j = k >> 1;
    for (; j >= 64; j >>= 1) {
      for (int i = tid; i < P; i += T_C) {
        const int x = i ^ j;
        if (x > i) {
          const uint64_t a = keys[i], b = keys[x];
          if ((a > b) == ((i & k) == 0)) {
            keys[i] = b;
            keys[x] = a;
          }
        }
      }
      __syncthreads();
    }
    for (int i = tid; i < P; i += T_C) {  // (i ^ j < P: the partner's lane is active whenever this one is)
      uint64_t a = keys[i];
      for (int jj = j; jj > 0; jj >>= 1) {
        const uint64_t b = __shfl_xor((unsigned long long)a, jj);
        const bool keep_min = ((i & jj) == 0) == ((i & k) == 0);  // the lower position of an ascending pair, the upper of a descending one
        a = keep_min ? (a < b ? a : b) : (a < b ? b : a);
      }
      keys[i] = a;
    }
    __syncthreads();
  }
  // a thread takes CH consecutive entries: its kept entries and the node heads among them, then the running sums over the threads
  const int CH = P > T_C ? P / T_C : 1;
  const int i0 = min(tid * CH, P), i1 = min(i0 + CH, P);
  int heads = 0, kept = 0;
  for (int i = i0; i < i1; ++i) {
    const uint64_t a = keys[i];
    if (a == NONE) break;
    ++kept;
    if (i == 0 || (keys[i - 1] >> 12) != (a >> 12)) ++heads;
  }
  const int mine = heads | (kept << 16);  // (both at most 4 096)
  int incl = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if ((tid & 63) >= d) incl += up;
  }
  if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
  __syncthreads();
  int before = 0, total = 0;
  for (int w = 0; w < T_C / 64; ++w) {
    if (w < (tid >> 6)) before += s_wave[w];
    total += s_wave[w];
  }
  const int nnode = total & 0xffff, nkept = total >> 16;
  const bool fits = nnode <= NNcap;
  if (tid == 0) {
    out.nnode[f] = nnode;
    out.status[f] = fits ? 0 : GL_BOW_NODES_TRUNCATED;
  }
  if (!fits) return;
  int32_t* node_id = out.node_id + (size_t)f * NNcap;
  int32_t* node_ptr = out.node_ptr + (size_t)f * (NNcap + 1);
  int32_t* node_idx = out.node_idx + (size_t)f * NF;
  if (tid == 0) node_ptr[nnode] = nkept;
  int r = ((before + incl) & 0xffff) - heads;
  for (int i = i0; i < i1; ++i) {
    const uint64_t a = keys[i];
    if (a == NONE) break;
    node_idx[i] = (int32_t)(a & 0xfff);
    if (i == 0 || (keys[i - 1] >> 12) != (a >> 12)) {
      node_id[r] = (int32_t)(a >> 12);
      node_ptr[r] = i;
      ++r;
    }
  }
}

inline gl::Voc* V(const gl_voc_t* v) { return (gl::Voc*)v; }

}  // namespace

extern "C" {

int gl_voc_create(gl_ctx_t* ctx, int n_nodes, const int32_t* parent, const uint8_t* desc, const float* weight, const uint8_t* is_leaf, int k,
                  int L, gl_voc_t** out) {
  GL_REQUIRE(ctx && parent && desc && weight && is_leaf && out, "null argument");
  gl::VocLayout lay;
  {
    const int rc = gl::voc_check(n_nodes, parent, is_leaf, GL_ERR_ARG, &lay);
    if (rc != GL_OK) return rc;
  }
  gl::Ctx* c = gl::C(ctx);
  GL_HIP(hipSetDevice(c->device));
  const size_t n_rec = (size_t)n_nodes - 1;
  std::vector<int32_t> nchild(n_rec), link(n_rec);
  for (size_t i = 0; i < n_rec; ++i) {
    nchild[i] = lay.nchild[i + 1];
    link[i] = nchild[i] ? lay.first[i + 1] : lay.word[i];
  }
  gl::Voc* v = new gl::Voc();
  v->device = c->device;
  v->n_nodes = n_nodes;
  v->n_words = lay.n_words;
  v->k = k;
  v->L = L;
  v->max_children = lay.max_children;
  v->min_leaf_level = lay.min_leaf_level;
  v->root_children = lay.nchild[0];
  v->bytes = n_rec * (32 + sizeof(int4));
  // staging: the caller's arrays as they are, and the three derived words per record
  void* stage[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const void* src[5] = {desc, weight, lay.pos.data(), nchild.data(), link.data()};
  const size_t bytes[5] = {n_rec * 32, n_rec * 4, n_rec * 4, n_rec * 4, n_rec * 4};
  int rc = GL_OK;
  auto alloc = [&](void** p, size_t b) {
    if (rc == GL_OK && hipMalloc(p, b) != hipSuccess) {
      gl::set_error("gl_voc_create: hipMalloc(%zu) failed", b);
      rc = GL_ERR_NOMEM;
    }
  };
  alloc(&v->desc, n_rec * 32);
  alloc(&v->meta, n_rec * sizeof(int4));
  for (int j = 0; j < 5; ++j) alloc(&stage[j], bytes[j]);
  for (int j = 0; j < 5 && rc == GL_OK; ++j)
    if (hipMemcpy(stage[j], src[j], bytes[j], hipMemcpyHostToDevice) != hipSuccess) {
      gl::set_error("gl_voc_create: upload failed");
      rc = GL_ERR_DEVICE;
    }
  if (rc == GL_OK) {
    k_voc_build<<<(unsigned)((n_rec + T_V - 1) / T_V), T_V, 0, c->stream>>>((int)n_rec, (const uint4*)stage[0], (const float*)stage[1],
                                                                           (const int32_t*)stage[2], (const int32_t*)stage[3],
                                                                           (const int32_t*)stage[4], (uint4*)v->desc, (int4*)v->meta);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
      gl::set_error("gl_voc_create: the layout kernel failed");
      rc = GL_ERR_DEVICE;
    }
  }
  for (void* p : stage)
    if (p) (void)hipFree(p);
  if (rc != GL_OK) {
    gl_voc_destroy((gl_voc_t*)v);
    return rc;
  }
  *out = (gl_voc_t*)v;
  return GL_OK;
}

int gl_voc_load_file(gl_ctx_t* ctx, const char* path, gl_voc_t** out) {
  GL_REQUIRE(ctx && path && out, "null argument");
  gl::VocFile f;
  const int rc = gl::read_voc_file(path, &f);
  if (rc != GL_OK) return rc;
  return gl_voc_create(ctx, f.n_nodes, f.parent.data(), f.desc.data(), f.weight.data(), f.is_leaf.data(), f.k, f.L, out);
}

int gl_voc_destroy(gl_voc_t* voc) {
  if (!voc) return GL_OK;
  gl::Voc* v = V(voc);
  (void)hipSetDevice(v->device);
  if (v->desc) (void)hipFree(v->desc);
  if (v->meta) (void)hipFree(v->meta);
  delete v;
  return GL_OK;
}

int gl_voc_info(const gl_voc_t* voc, double info[7]) {
  GL_REQUIRE(voc && info, "null argument");
  const gl::Voc* v = V(voc);
  info[0] = v->n_nodes;
  info[1] = v->n_words;
  info[2] = v->k;
  info[3] = v->L;
  info[4] = v->max_children;
  info[5] = v->min_leaf_level;
  info[6] = (double)v->bytes;
  return GL_OK;
}

int gl_bow_transform(gl_ctx_t* ctx, const gl_voc_t* voc, int levelsup, int B, int NF, int NNcap, const uint8_t* feat_desc_dev,
                     const int32_t* feat_oct_dev, const gl_bow_out* out) {
  GL_REQUIRE(ctx && voc && out, "null argument");
  GL_REQUIRE(levelsup >= 0, "negative levelsup");
  if (B == 0) return GL_OK;
  GL_REQUIRE(B > 0 && B <= 65535 && NF >= 1 && NF <= NF_MAX && NNcap >= 1 && NNcap <= NF_MAX, "bad B / NF / NNcap (NF, NNcap in 1 .. 4096)");
  GL_REQUIRE(feat_desc_dev && out->nnode && out->node_id && out->node_ptr && out->node_idx && out->status, "null buffer");
  GL_REQUIRE(((uintptr_t)feat_desc_dev & 15) == 0, "feat_desc not aligned to 16 bytes");
  gl::Ctx* c = gl::C(ctx);
  const gl::Voc* v = V(voc);
  GL_REQUIRE(v->device == c->device, "the vocabulary lives on another device than the context");
  GL_HIP(hipSetDevice(c->device));
  void* key = nullptr;  // B x NF: the node of every kept feature
  {
    const int rc = gl::ctx_scratch(c, (size_t)B * NF * sizeof(int32_t), &key);
    if (rc != GL_OK) return rc;
  }
  const long nid_level = (long)v->L - levelsup;
  k_bow_descend<<<dim3((NF + T_D / ROW - 1) / (T_D / ROW), B), T_D, 0, c->stream>>>(
      NF, (int)(nid_level < 0 ? 0 : nid_level), v->root_children, (const uint4*)v->desc, (const int4*)v->meta, (const uint4*)feat_desc_dev,
      feat_oct_dev, out->word_id, out->node, out->weight, (int32_t*)key);
  GL_HIP(hipGetLastError());
  int P = 1;
  while (P < NF) P <<= 1;
  k_bow_csr<<<B, T_C, 0, c->stream>>>(NF, P, NNcap, (const int32_t*)key, *out);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

}  // extern "C"
