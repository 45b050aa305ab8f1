// ============================================================================
// TEST INFRASTRUCTURE ONLY.  Real-code oracle for ORBVocabulary's reader and
// transform (row 8f-6): this wrapper instantiates the reference's OWN DBoW2,
// TemplatedVocabulary<FORB::TDescriptor, FORB> (orb_dbow2/include/orb_dbow2/
// dbow2/TemplatedVocabulary.h) with its FORB / BowVector / FeatureVector /
// ScoringObject sources, included and compiled from where they lie in the
// reference tree -- nothing is copied into this repository.  The one OpenCV
// header they ask for is this project's stand-in (oracle/cv_standin).
// Built by oracle/Makefile into oracle/_ref/libdbow2_ref.so (git-ignored).
//
// What the wrapper adds is access only: the per-feature transform and m_nodes
// are protected members, reached through a subclass.  `nid` is pre-set to
// DBREF_NID_UNSET before every per-feature call, so that a call which leaves
// it unwritten (a leaf above level L - levelsup) is observable without
// reading an indeterminate value.
// ============================================================================
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "orb_dbow2/dbow2/FORB.h"
#include "orb_dbow2/dbow2/TemplatedVocabulary.h"

namespace {
const uint32_t DBREF_NID_UNSET = 0xFFFFFFFFu;

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> VocBase;

cv::Mat descriptor(const uint8_t* bytes) {
  cv::Mat m(1, DBoW2::FORB::L, CV_8U);
  std::memcpy(m.data, bytes, DBoW2::FORB::L);
  return m;
}

uint32_t float_bits(double w) {  // the weight came from a float of the file: the way back is exact
  const float f = (float)w;
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

struct Voc : public VocBase {
  using VocBase::transform;

  int n_nodes() const { return (int)m_nodes.size(); }
  bool is_word(const Node& nd) const { return nd.word_id < m_words.size() && m_words[nd.word_id] == &nd; }

  int dump(int32_t* parent, uint8_t* desc, uint32_t* weight, int32_t* word_id, int32_t* child_ptr, int32_t* child_ids, int child_cap) const {
    int at = 0;
    for (size_t i = 0; i < m_nodes.size(); ++i) {
      const Node& nd = m_nodes[i];
      parent[i] = (int32_t)nd.parent;
      if (nd.descriptor.empty())
        std::memset(desc + 32 * i, 0, 32);  // the root has none
      else
        std::memcpy(desc + 32 * i, nd.descriptor.data, 32);
      weight[i] = float_bits(nd.weight);
      word_id[i] = (i > 0 && is_word(nd)) ? (int32_t)nd.word_id : -1;
      child_ptr[i] = at;
      for (size_t c = 0; c < nd.children.size(); ++c, ++at)
        if (at < child_cap) child_ids[at] = (int32_t)nd.children[c];
    }
    child_ptr[m_nodes.size()] = at;
    return at;
  }

  void feature(const uint8_t* bytes, int levelsup, int32_t* word, uint32_t* wbits, uint32_t* nid_out, int32_t* final_node, double* w_out) const {
    DBoW2::WordId id = 0;
    DBoW2::WordValue w = 0;
    DBoW2::NodeId nid = DBREF_NID_UNSET;
    transform(descriptor(bytes), id, w, &nid, levelsup);
    *word = (int32_t)id;
    *wbits = float_bits(w);
    *nid_out = (uint32_t)nid;
    *final_node = (int32_t)m_words[id]->id;
    *w_out = w;
  }
};

// a feature vector in map order -> (nnode, node_id [n], node_ptr [n + 1], node_idx [n])
void flatten(const DBoW2::FeatureVector& fv, int32_t* nnode, int32_t* node_id, int32_t* node_ptr, int32_t* node_idx) {
  int r = 0, at = 0;
  for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it, ++r) {
    node_id[r] = (int32_t)it->first;
    node_ptr[r] = at;
    for (size_t j = 0; j < it->second.size(); ++j) node_idx[at++] = (int32_t)it->second[j];
  }
  node_ptr[r] = at;
  *nnode = r;
}

// The reference's loader tests nothing: a file that does not open, or whose length or parents disagree with its header, makes it
// index out of range.  The wrapper is only ever given well-formed files and says no to anything else before the loader sees it.
bool well_formed(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  uint32_t hdr[6];
  bool ok = std::fread(hdr, 4, 6, f) == 6 && hdr[1] == 41 && hdr[0] >= 2 && hdr[0] < (1u << 28);
  if (ok) {
    const uint32_t n = hdr[0] - 1;
    std::vector<uint8_t> rec((size_t)41 * n);
    ok = std::fread(rec.data(), 41, n, f) == n && std::fgetc(f) == EOF;
    for (uint32_t i = 0; ok && i < n; ++i) {
      int32_t p;
      std::memcpy(&p, &rec[(size_t)41 * i], 4);
      ok = p >= 0 && (uint32_t)p <= i && (p == 0 || rec[(size_t)41 * (p - 1) + 40] == 0);  // an earlier node that is no leaf
    }
    std::vector<uint8_t> has_child(n + 1, 0);
    for (uint32_t i = 0; ok && i < n; ++i) {
      int32_t p;
      std::memcpy(&p, &rec[(size_t)41 * i], 4);
      has_child[p] = 1;
    }
    for (uint32_t i = 0; ok && i < n; ++i) ok = rec[(size_t)41 * i + 40] != 0 || has_child[i + 1];
  }
  std::fclose(f);
  return ok;
}
}  // namespace

extern "C" {
void* dbref_load(const char* path) {
  if (!well_formed(path)) return nullptr;
  Voc* v = new Voc();
  if (!v->loadFromBinaryFile(path)) {
    delete v;
    return nullptr;
  }
  return v;
}
void dbref_destroy(void* h) { delete (Voc*)h; }

// out: m_nodes.size(), size() (words), k, L
void dbref_info(void* h, int32_t* out) {
  const Voc* v = (const Voc*)h;
  out[0] = v->n_nodes();
  out[1] = (int32_t)v->size();
  out[2] = v->getBranchingFactor();
  out[3] = v->getDepthLevels();
}

// per node id 0 .. m_nodes.size() - 1 (the root and the phantom included): parent, 32 descriptor bytes, weight as float bits,
// word_id or -1, children in stored order as child_ids[child_ptr[id] .. child_ptr[id + 1]) -> the number of children in all
int dbref_nodes(void* h, int32_t* parent, uint8_t* desc, uint32_t* weight, int32_t* word_id, int32_t* child_ptr, int32_t* child_ids, int child_cap) {
  return ((const Voc*)h)->dump(parent, desc, weight, word_id, child_ptr, child_ids, child_cap);
}

// transform(feature, id, weight, &nid, levelsup) for n descriptors: word id, weight bits, nid (DBREF_NID_UNSET where the call
// left it unwritten) and the final node m_words[word]->id
void dbref_transform(void* h, const uint8_t* desc, int n, int levelsup, int32_t* word, uint32_t* wbits, uint32_t* nid, int32_t* final_node) {
  const Voc* v = (const Voc*)h;
  double w;
  for (int i = 0; i < n; ++i) v->feature(desc + (size_t)32 * i, levelsup, word + i, wbits + i, nid + i, final_node + i, &w);
}

// One frame's feature vector, twice.  (a): FeatureVector::addFeature on the per-feature results for the features with weight > 0,
// with the final node where nid was left unwritten.  (b): the vector overload transform(features, bv, fv, levelsup) itself, run only
// when no nid was left unwritten (it would read an indeterminate value otherwise); *b_nnode = -1 when it was not run.
// Arrays: node_id [n], node_ptr [n + 1], node_idx [n].  -> the number of features whose nid was left unwritten
int dbref_frame(void* h, const uint8_t* desc, int n, int levelsup, int32_t* a_nnode, int32_t* a_node_id, int32_t* a_node_ptr, int32_t* a_node_idx,
                int32_t* b_nnode, int32_t* b_node_id, int32_t* b_node_ptr, int32_t* b_node_idx) {
  const Voc* v = (const Voc*)h;
  DBoW2::FeatureVector fa;
  int unwritten = 0;
  for (int i = 0; i < n; ++i) {
    int32_t word, final_node;
    uint32_t wbits, nid;
    double w;
    v->feature(desc + (size_t)32 * i, levelsup, &word, &wbits, &nid, &final_node, &w);
    if (nid == DBREF_NID_UNSET) {
      ++unwritten;
      nid = (uint32_t)final_node;
    }
    if (w > 0) fa.addFeature(nid, (unsigned int)i);
  }
  flatten(fa, a_nnode, a_node_id, a_node_ptr, a_node_idx);
  *b_nnode = -1;
  if (unwritten == 0) {
    std::vector<cv::Mat> features;
    features.reserve(n);
    for (int i = 0; i < n; ++i) features.push_back(descriptor(desc + (size_t)32 * i));
    DBoW2::BowVector bv;
    DBoW2::FeatureVector fb;
    v->transform(features, bv, fb, levelsup);
    flatten(fb, b_nnode, b_node_id, b_node_ptr, b_node_idx);
  }
  return unwritten;
}

int dbref_distance(const uint8_t* a, const uint8_t* b) { return DBoW2::FORB::distance(descriptor(a), descriptor(b)); }
}
