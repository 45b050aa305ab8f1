// Driver of tests/test_gpu_stereo_adapter.py: Frame::computeStereoMatches through the C++ host mirror
// (include/gmmloc_hip/gmm_adapter.hpp: computeStereoMatches), plain C++17 over the C-ABI.
//   stereo_check model.gmm scene.bin out.bin
// scene.bin: int32 {NF, NR, nlevels, height, row_pad}, double {fx, bf, scale_factor}, then feat_uv (NF x 2 f64), feat_oct (NF i32),
// feat_desc (NF x 32 u8), r_uv (NR x 2 f32), r_oct (NR i32), r_desc (NR x 32 u8), then per side (left, right) and level int32 {width,
// height} and the image with row_pad bytes behind every row (stride = width + row_pad) - a bordered buffer as the extractor keeps it.
// out.bin: feat_ur, feat_depth (NF f32), match_r, sad (NF i32), stat (4 i32).
#include "driver_io.hpp"

using namespace gmmloc_hip;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  GMM model;
  if (!load_model(argv[1], model)) return 1;
  std::ifstream in(argv[2], std::ios::binary);
  const auto hd = rd<int32_t>(in, 5);
  const auto cm = rd<double>(in, 3);
  const size_t NF = (size_t)hd[0], NR = (size_t)hd[1];
  const int nlevels = hd[2], row_pad = hd[4];
  const auto uv = rd<double>(in, NF * 2);
  const auto oct = rd<int32_t>(in, NF);
  const auto desc = rd<uint8_t>(in, NF * 32);
  GMM::RightKeyPoints right;
  right.uv = rd<float>(in, NR * 2);
  right.oct = rd<int32_t>(in, NR);
  right.desc = rd<uint8_t>(in, NR * 32);
  std::vector<std::vector<uint8_t>> store;
  std::vector<GMM::ImageLevel> pyr[2];
  for (int s = 0; s < 2; ++s)
    for (int l = 0; l < nlevels; ++l) {
      const auto wh = rd<int32_t>(in, 2);
      const int64_t stride = wh[0] + row_pad;
      store.push_back(rd<uint8_t>(in, (size_t)stride * (size_t)wh[1]));
      pyr[s].push_back(GMM::ImageLevel{nullptr, wh[0], wh[1], stride});
    }
  if (!in) return 3;
  for (int s = 0; s < 2; ++s)
    for (int l = 0; l < nlevels; ++l) pyr[s][(size_t)l].ptr = store[(size_t)(s * nlevels + l)].data();
  gl_camera cam{};
  cam.fx = cam.fy = cm[0], cam.bf = cm[1], cam.width = 752, cam.height = hd[3];
  model.setCamera(cam);
  const GMM::StereoMatches r = model.computeStereoMatches(uv, oct, desc, right, pyr[0], pyr[1], cm[2]);
  std::ofstream out(argv[3], std::ios::binary);
  wr(out, r.ur), wr(out, r.depth), wr(out, r.match_r), wr(out, r.sad);
  wr(out, std::vector<int32_t>(r.stat, r.stat + 4));
  return out ? 0 : 4;
}
