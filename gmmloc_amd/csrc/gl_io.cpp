// .gmm map stream reader / writer (host C++, no protobuf dependency).
// Framing (gmmloc/src/utils/protobuf_utils.cpp:12-29,42-80; writer :31-40,82-100):
//   varint32 count, then count x { varint32 size, ComponentProto bytes }.
// ComponentProto (gmmloc/proto/gmmloc/GMM.proto:5-14, proto2):
//   1 bool is_degenerated, 2 bool is_salient,
//   3 repeated double mean [packed], 4 repeated double covariance [packed].
// The reference loader ignores fields 1-2 and recomputes them
// (gmm_utils.cpp:50-61); covariance is read row-major (:54-59).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gl_internal.hpp"

namespace gl {

namespace {
bool get_varint(const std::vector<uint8_t>& b, size_t& pos, uint64_t& out) {
  out = 0;
  for (int shift = 0; shift < 64; shift += 7) {
    if (pos >= b.size()) return false;
    const uint8_t c = b[pos++];
    out |= (uint64_t)(c & 0x7F) << shift;
    if (!(c & 0x80)) return true;
  }
  return false;
}
void put_varint(std::vector<uint8_t>& b, uint64_t v) {
  while (v >= 0x80) {
    b.push_back((uint8_t)(v | 0x80));
    v >>= 7;
  }
  b.push_back((uint8_t)v);
}
int fail(const char* msg) {
  set_error("%s", msg);
  return GL_ERR_FORMAT;
}
}  // namespace

int read_gmm_file(const char* path, std::vector<double>& mean, std::vector<double>& cov) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    set_error("Could not open protobuf file to load layer: %s", path);  // gmm_utils.cpp:19-22
    return GL_ERR_IO;
  }
  std::vector<uint8_t> buf;
  uint8_t tmp[65536];
  size_t n;
  while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
  fclose(f);
  size_t pos = 0;
  uint64_t count = 0;
  if (!get_varint(buf, pos, count)) return fail("failed read number of messages.");  // gmm_utils.cpp:27-30
  if (count == 0) return fail("protobuf file empty!");                               // gmm_utils.cpp:32-35
  mean.clear();
  cov.clear();
  for (uint64_t i = 0; i < count; ++i) {
    uint64_t size = 0;
    if (!get_varint(buf, pos, size) || size == 0 || size > buf.size() - pos)  // never pos + size: it wraps
      return fail("failed to read component message.");  // gmm_utils.cpp:44-47
    const size_t end = pos + size;
    size_t nm = 0, nc = 0;
    double m[3] = {0, 0, 0}, c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    auto take = [&](int field, double v) {
      if (field == 3) {
        if (nm < 3) m[nm] = v;
        ++nm;
      } else if (field == 4) {
        if (nc < 9) c[nc] = v;
        ++nc;
      }
    };
    while (pos < end) {
      uint64_t tag = 0;
      if (!get_varint(buf, pos, tag)) return fail("truncated tag");
      const int field = (int)(tag >> 3), wt = (int)(tag & 7);
      if (wt == 0) {
        uint64_t v;
        if (!get_varint(buf, pos, v)) return fail("truncated varint");
      } else if (wt == 2) {
        uint64_t len = 0;
        if (!get_varint(buf, pos, len) || pos > end || len > end - pos) return fail("bad length-delimited field");
        if (field == 3 || field == 4) {
          if (len % 8) return fail("bad packed double field");
          for (uint64_t o = 0; o < len; o += 8) {
            double v;
            memcpy(&v, &buf[pos + o], 8);
            take(field, v);
          }
        }
        pos += len;
      } else if (wt == 1) {  // unpacked double
        if (pos > end || end - pos < 8) return fail("truncated double");
        double v;
        memcpy(&v, &buf[pos], 8);
        pos += 8;
        take(field, v);
      } else if (wt == 5) {
        if (pos > end || end - pos < 4) return fail("truncated fixed32");
        pos += 4;
      } else {
        return fail("unsupported wire type");
      }
    }
    if (pos != end) return fail("Could not consume protobuf message.");
    if (nm != 3 || nc != 9)  // CHECK_EQ(mean_size, 3) / CHECK_EQ(covariance_size, 9), gmm_utils.cpp:50-51
      return fail("component with mean_size != 3 or covariance_size != 9");
    mean.insert(mean.end(), m, m + 3);
    cov.insert(cov.end(), c, c + 9);
  }
  return GL_OK;
}

// saveGMMModel (gmm_utils.cpp:69-119): is_degenerated, is_salient, mean[3],
// covariance[9] ("cov(i)" walks Eigen's column-major storage, :102-104).
int write_gmm_file(const char* path, const double* mean, const double* cov, const uint8_t* flags, int K) {
  std::vector<uint8_t> out;
  put_varint(out, (uint64_t)K);
  for (int k = 0; k < K; ++k) {
    std::vector<uint8_t> msg;
    msg.push_back(0x08);
    msg.push_back((flags[k] & 1) ? 1 : 0);
    msg.push_back(0x10);
    msg.push_back((flags[k] & 2) ? 1 : 0);
    msg.push_back(0x1A);
    put_varint(msg, 24);
    const uint8_t* p = (const uint8_t*)(mean + 3 * k);
    msg.insert(msg.end(), p, p + 24);
    msg.push_back(0x22);
    put_varint(msg, 72);
    for (int i = 0; i < 9; ++i) {  // column-major walk of the row-major array
      const double v = cov[9 * k + (i % 3) * 3 + (i / 3)];
      const uint8_t* q = (const uint8_t*)&v;
      msg.insert(msg.end(), q, q + 8);
    }
    put_varint(out, msg.size());
    out.insert(out.end(), msg.begin(), msg.end());
  }
  FILE* f = fopen(path, "wb");
  if (!f) {
    set_error("fail to save model, path: %s", path);
    return GL_ERR_IO;
  }
  const size_t w = fwrite(out.data(), 1, out.size(), f);
  fclose(f);
  if (w != out.size()) {
    set_error("short write");
    return GL_ERR_IO;
  }
  return GL_OK;
}


// ---- the DBoW2 vocabulary (gmmloc_hip.h: "the DBoW2 vocabulary and ORBVocabulary::transform") ------------------------------------------
// The consistency rules of a tree given as records, and what the device layout needs of it: child counts, the layout position of
// every record (the records in the order (parent, id): a node's children are contiguous and in child order, the children of node p
// start at first[p]), word ids, levels.  `err` is what a violation returns: GL_ERR_FORMAT from a file, GL_ERR_ARG from arrays.
int voc_check(int n_nodes, const int32_t* parent, const uint8_t* is_leaf, int err, VocLayout* out) {
  auto bad = [&](const char* what, long node) {
    set_error("vocabulary: %s (node %ld)", what, node);
    return err;
  };
  if (n_nodes < 2) return bad("fewer than two nodes", 0L);
  const size_t n_rec = (size_t)n_nodes - 1;
  VocLayout& v = *out;
  v.nchild.assign(n_nodes, 0);
  v.first.assign(n_nodes, 0);
  v.pos.assign(n_rec, 0);
  v.word.assign(n_rec, -1);
  std::vector<int32_t> level(n_nodes, 0);
  for (size_t i = 0; i < n_rec; ++i) {
    const long id = (long)i + 1;
    if (parent[i] < 0 || parent[i] >= id) return bad("parent outside [0, own id)", id);
    if (parent[i] > 0 && is_leaf[parent[i] - 1]) return bad("a record flagged leaf has a child", (long)parent[i]);
    ++v.nchild[parent[i]];
    level[id] = level[parent[i]] + 1;
  }
  v.n_words = v.max_children = 0;
  v.min_leaf_level = INT32_MAX;
  int32_t at = 0;
  for (int p = 0; p < n_nodes; ++p) {
    v.first[p] = at;
    at += v.nchild[p];
    if (v.nchild[p] > v.max_children) v.max_children = v.nchild[p];
    if (p > 0) {
      if (is_leaf[p - 1]) {
        v.word[p - 1] = v.n_words++;
        if (level[p] < v.min_leaf_level) v.min_leaf_level = level[p];
      } else if (v.nchild[p] == 0) {
        return bad("a record not flagged leaf has no child", (long)p);
      }
    }
  }
  std::vector<int32_t> cursor(v.first);
  for (size_t i = 0; i < n_rec; ++i) v.pos[i] = cursor[parent[i]]++;
  return GL_OK;
}

// loadFromBinaryFile (TemplatedVocabulary.h:1477-1522) without its phantom record: exactly nb_nodes - 1 records
int read_voc_file(const char* path, VocFile* out) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    set_error("cannot open vocabulary file: %s", path);
    return GL_ERR_IO;
  }
  std::vector<uint8_t> buf;
  {
    std::vector<uint8_t> tmp(1 << 20);
    size_t n;
    while ((n = fread(tmp.data(), 1, tmp.size(), f)) > 0) buf.insert(buf.end(), tmp.begin(), tmp.begin() + n);
  }
  fclose(f);
  if (buf.size() < 24) return fail("vocabulary file shorter than its header");
  uint32_t nb_nodes, size_node;
  int32_t kL[2];
  memcpy(&nb_nodes, &buf[0], 4);
  memcpy(&size_node, &buf[4], 4);
  memcpy(kL, &buf[8], 8);
  if (size_node != 41) return fail("vocabulary file: size_node != 41");
  if (nb_nodes < 2 || nb_nodes > (uint32_t)INT32_MAX) return fail("vocabulary file: nb_nodes outside [2, 2^31)");
  const size_t n_rec = (size_t)nb_nodes - 1;
  if (buf.size() != 24 + n_rec * 41) return fail("vocabulary file shorter or longer than its header says");
  out->n_nodes = (int)nb_nodes;
  out->k = kL[0];
  out->L = kL[1];
  out->parent.resize(n_rec);
  out->desc.resize(n_rec * 32);
  out->weight.resize(n_rec);
  out->is_leaf.resize(n_rec);
  for (size_t i = 0; i < n_rec; ++i) {
    const uint8_t* r = &buf[24 + i * 41];
    memcpy(&out->parent[i], r, 4);
    memcpy(&out->desc[i * 32], r + 4, 32);
    memcpy(&out->weight[i], r + 36, 4);
    out->is_leaf[i] = r[40] ? 1 : 0;  // `if (buf[8+F::L])`, :1508
  }
  VocLayout lay;
  return voc_check(out->n_nodes, out->parent.data(), out->is_leaf.data(), GL_ERR_FORMAT, &lay);
}

}  // namespace gl

extern "C" {

int gl_voc_file_read(const char* path, int32_t* parent, uint8_t* desc, float* weight, uint8_t* is_leaf, int cap, int* n_nodes_out,
                     int* k_L_out) {
  GL_REQUIRE(path && n_nodes_out, "null argument");
  gl::VocFile v;
  const int rc = gl::read_voc_file(path, &v);
  if (rc != GL_OK) return rc;
  const size_t n_rec = (size_t)v.n_nodes - 1;
  if (parent || desc || weight || is_leaf) {
    GL_REQUIRE(cap >= 0 && (size_t)cap >= n_rec, "output capacity too small");
    if (parent) memcpy(parent, v.parent.data(), 4 * n_rec);
    if (desc) memcpy(desc, v.desc.data(), 32 * n_rec);
    if (weight) memcpy(weight, v.weight.data(), 4 * n_rec);
    if (is_leaf) memcpy(is_leaf, v.is_leaf.data(), n_rec);
  }
  *n_nodes_out = v.n_nodes;
  if (k_L_out) {
    k_L_out[0] = v.k;
    k_L_out[1] = v.L;
  }
  return GL_OK;
}

int gl_gmm_file_read(const char* path, double* mean, double* cov, int cap, int* K_out) {
  GL_REQUIRE(path && K_out, "null argument");
  std::vector<double> m, c;
  const int rc = gl::read_gmm_file(path, m, c);
  if (rc != GL_OK) return rc;
  const int K = (int)(m.size() / 3);
  *K_out = K;
  if (mean || cov) {
    GL_REQUIRE(cap >= K, "output capacity too small");
    if (mean) memcpy(mean, m.data(), sizeof(double) * 3 * K);
    if (cov) memcpy(cov, c.data(), sizeof(double) * 9 * K);
  }
  return GL_OK;
}

int gl_gmm_file_write(const char* path, const double* mean, const double* cov, const uint8_t* flags, int K) {
  GL_REQUIRE(path && mean && cov && flags && K > 0, "bad argument");
  return gl::write_gmm_file(path, mean, cov, flags, K);
}

// Map::summarize (map.cpp:162-188): one line per frame, `timestamp tx ty tz qx qy qz qw` of T_wc in TUM
// format -- std::fixed, 6 digits for the stamp, 9 for the pose, single spaces, '\n'.
int gl_write_tum_trajectory(const char* path, const double* stamps, const double* pose_wc, int N) {
  GL_REQUIRE(path && (N == 0 || (stamps && pose_wc)) && N >= 0, "bad argument");
  FILE* f = fopen(path, "w");
  if (!f) {
    gl::set_error("gl_write_tum_trajectory: cannot open %s", path);
    return GL_ERR_IO;
  }
  for (int i = 0; i < N; ++i) {
    const double* p = pose_wc + (size_t)i * 7;  // qx qy qz qw tx ty tz
    fprintf(f, "%.6f %.9f %.9f %.9f %.9f %.9f %.9f %.9f\n", stamps[i], p[4], p[5], p[6], p[0], p[1], p[2], p[3]);
  }
  fclose(f);
  return GL_OK;
}

}  // extern "C"
