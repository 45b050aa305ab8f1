// Driver of tests/test_gpu_orb_adapter.py: ORBextractor's orientation and descriptors through the C++ host mirror
// (include/gmmloc_hip/gmm_adapter.hpp: orbDescribe), plain C++17 over the C-ABI.
//   orb_check model.gmm scene.bin out.bin
// scene.bin: int32 {N, nlevels, row_pad, has_angle}, int32 blur_w[4], double scale_factor, kp_xy (N x 2 i32), kp_oct (N i32), kp_angle
// (N f32, when has_angle), the pattern (512 x 2 i8), then per level int32 {width, height} and the image with row_pad bytes behind every
// row (stride = width + row_pad) - a bordered buffer as the extractor keeps it.
// out.bin: desc (N x 32 u8), angle (N f32), moments (N x 2 i32), uv32 (N x 2 f32), uv64 (N x 2 f64), stat (2 i32).
#include "driver_io.hpp"

using namespace gmmloc_hip;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  GMM model;
  if (!load_model(argv[1], model)) return 1;
  std::ifstream in(argv[2], std::ios::binary);
  const auto hd = rd<int32_t>(in, 4);
  const auto blur_w = rd<int32_t>(in, 4);
  const auto sf = rd<double>(in, 1);
  const size_t N = (size_t)hd[0];
  const int nlevels = hd[1], row_pad = hd[2];
  const auto xy = rd<int32_t>(in, N * 2);
  const auto oct = rd<int32_t>(in, N);
  const auto angle = rd<float>(in, hd[3] ? N : 0);
  const auto pattern = rd<int8_t>(in, 1024);
  std::vector<std::vector<uint8_t>> store;
  std::vector<GMM::ImageLevel> pyr;
  for (int l = 0; l < nlevels; ++l) {
    const auto wh = rd<int32_t>(in, 2);
    const int64_t stride = wh[0] + row_pad;
    store.push_back(rd<uint8_t>(in, (size_t)stride * (size_t)wh[1]));
    pyr.push_back(GMM::ImageLevel{nullptr, wh[0], wh[1], stride});
  }
  if (!in) return 3;
  for (int l = 0; l < nlevels; ++l) pyr[(size_t)l].ptr = store[(size_t)l].data();
  const GMM::OrbFeatures r = model.orbDescribe(xy, oct, pattern, pyr, blur_w, sf[0], angle);
  std::ofstream out(argv[3], std::ios::binary);
  wr(out, r.desc), wr(out, r.angle), wr(out, r.moments), wr(out, r.uv32), wr(out, r.uv64);
  wr(out, std::vector<int32_t>(r.stat, r.stat + 2));
  return out ? 0 : 4;
}
