// Drives the vocabulary calls of include/gmmloc_hip/gmm_adapter.hpp (loadVocabulary, bowTransform, bowTransformIntoTables) on one
// frame dumped by tests/test_gpu_bow.py and writes the results back for comparison with the Python host.
//   bow_check <map.gmm> <voc.bin> <frame.bin> <out.bin>
// frame.bin: int32 N, levelsup, NNcap; uint8 desc[N*32]; int32 oct[N]
// out.bin:   bowTransform: int32 nnode, nidx; node_id[nnode], node_ptr[nnode+1], node_idx[nidx];
//            bowTransformIntoTables on row 1 of two-row tables whose four CSR arrays were filled with 0xF9 bytes: int32 status,
//            nnode[2], node_id[2*NNcap], node_ptr[2*(NNcap+1)], node_idx[2*N]
#include <algorithm>
#include <cstdio>
#include <vector>

#include "driver_io.hpp"

template <class T>
static void rd(FILE* f, T* p, size_t n) {
  if (n && fread(p, sizeof(T), n, f) != n) throw std::runtime_error("short read");
}
template <class T>
static void wr(FILE* f, const T* p, size_t n) {
  if (n && fwrite(p, sizeof(T), n, f) != n) throw std::runtime_error("short write");
}

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  try {
    gmmloc_hip::GMM gmm;
    if (!load_model(argv[1], gmm)) return 1;
    if (!gmm.loadVocabulary(argv[2])) {
      fprintf(stderr, "loadVocabulary: %s\n", gmmloc_hip::GMM::last_error());
      return 1;
    }
    FILE* f = fopen(argv[3], "rb");
    if (!f) return 1;
    int32_t hdr[3];
    rd(f, hdr, 3);
    const size_t N = (size_t)hdr[0], NN = (size_t)hdr[2];
    const int levelsup = hdr[1];
    std::vector<uint8_t> desc(N * 32);
    std::vector<int32_t> oct(N);
    rd(f, desc.data(), desc.size());
    rd(f, oct.data(), N);
    fclose(f);
    FILE* o = fopen(argv[4], "wb");
    if (!o) return 1;

    const gmmloc_hip::GMM::FeatureVector fv = gmm.bowTransform(desc, levelsup);
    const int32_t counts[2] = {(int32_t)fv.node_id.size(), (int32_t)fv.node_idx.size()};
    wr(o, counts, 2);
    wr(o, fv.node_id.data(), fv.node_id.size());
    wr(o, fv.node_ptr.data(), fv.node_ptr.size());
    wr(o, fv.node_idx.data(), fv.node_idx.size());

    // two key-frame rows; row 1 holds the frame
    gmmloc_hip::DevBuf d_desc(gmm.ctx(), 2 * N * 32), d_oct(gmm.ctx(), 2 * N * 4), d_nnode(gmm.ctx(), 2 * 4), d_id(gmm.ctx(), 2 * NN * 4),
        d_ptr(gmm.ctx(), 2 * (NN + 1) * 4), d_idx(gmm.ctx(), 2 * N * 4);
    std::vector<uint8_t> desc2(2 * N * 32, 0);
    std::vector<int32_t> oct2(2 * N, 0);
    std::copy(desc.begin(), desc.end(), desc2.begin() + N * 32);
    std::copy(oct.begin(), oct.end(), oct2.begin() + N);
    d_desc.upload(desc2.data());
    d_oct.upload(oct2.data());
    for (gmmloc_hip::DevBuf* b : {&d_nnode, &d_id, &d_ptr, &d_idx}) {
      const std::vector<uint8_t> fill(b->bytes(), 0xF9);
      b->upload(fill.data());
    }
    gl_map_view view{};
    view.NKF = 2, view.NFK = (int32_t)N;
    gl_map_ba_view ba{};
    ba.kf_oct = d_oct.as<int32_t>();
    gmm.setResidentMap(view, ba);
    gl_map_kf_tables kt{};
    kt.kf_desc = d_desc.as<uint8_t>(), kt.kf_nnode = d_nnode.as<int32_t>(), kt.kf_node_id = d_id.as<int32_t>(), kt.kf_node_ptr = d_ptr.as<int32_t>();
    kt.kf_node_idx = d_idx.as<int32_t>(), kt.NNcap = (int32_t)NN, kt.k = 1;
    gmm.setResidentKeyFrameTables(kt);
    const int32_t status = gmm.bowTransformIntoTables(1, levelsup);
    wr(o, &status, 1);
    for (gmmloc_hip::DevBuf* b : {&d_nnode, &d_id, &d_ptr, &d_idx}) {
      std::vector<uint8_t> h(b->bytes());
      b->download(h.data());
      wr(o, h.data(), h.size());
    }
    fclose(o);
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "bow_check: %s\n", e.what());
    return 1;
  }
}
