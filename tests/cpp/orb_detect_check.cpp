// Driver of tests/test_gpu_orb_detect_adapter.py: ORBextractor's pyramid, detection and the composite through the C++ host mirror
// (include/gmmloc_hip/gmm_adapter.hpp: orbPyramid, orbDetect, orbExtract), plain C++17 over the C-ABI.
//   orb_detect_check model.gmm scene.bin out.bin
// scene.bin: int32 {width, height, row_pad, nlevels, nfeatures, ini_th, min_th, cand_cap}, the pattern (512 x 2 i8), the image with
// row_pad bytes behind every row.
// out.bin: per level int32 {width, height} and its pixels; then for orbDetect and for orbExtract: int32 n, level_count (8), stat (4),
// kp_xy (n x 2 i32), kp_oct (n i32), kp_response (n f32); then orbExtract's desc (n x 32 u8), angle (n f32), moments (n x 2 i32), uv32
// (n x 2 f32), uv64 (n x 2 f64), stat (2 i32).
#include "driver_io.hpp"

using namespace gmmloc_hip;

static void key_points(std::ofstream& out, const GMM::OrbKeyPoints& r) {
  wr(out, std::vector<int32_t>{(int32_t)r.kp_oct.size()});
  wr(out, std::vector<int32_t>(r.level_count, r.level_count + 8));
  wr(out, std::vector<int32_t>(r.stat, r.stat + 4));
  wr(out, r.kp_xy), wr(out, r.kp_oct), wr(out, r.kp_response);
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  GMM model;
  if (!load_model(argv[1], model)) return 1;
  std::ifstream in(argv[2], std::ios::binary);
  const auto hd = rd<int32_t>(in, 8);
  const auto pattern = rd<int8_t>(in, 1024);
  const int64_t stride = hd[0] + hd[2];
  const auto pixels = rd<uint8_t>(in, (size_t)stride * (size_t)hd[1]);
  if (!in) return 3;
  const GMM::ImageLevel image{pixels.data(), hd[0], hd[1], stride};
  GMM::OrbDetectConfig cfg;
  cfg.nlevels = hd[3], cfg.nfeatures = hd[4], cfg.ini_th = hd[5], cfg.min_th = hd[6], cfg.cand_cap = hd[7];
  std::ofstream out(argv[3], std::ios::binary);
  const GMM::OrbPyramidHost pyr = model.orbPyramid(image, cfg.nlevels, cfg.scale_factor);
  for (size_t l = 0; l < pyr.levels.size(); ++l) {
    wr(out, std::vector<int32_t>{pyr.width[l], pyr.height[l]});
    wr(out, pyr.levels[l]);
  }
  key_points(out, model.orbDetect(image, cfg));
  const GMM::OrbKeyPoints r = model.orbExtract(image, pattern, cfg);
  key_points(out, r);
  wr(out, r.features.desc), wr(out, r.features.angle), wr(out, r.features.moments), wr(out, r.features.uv32), wr(out, r.features.uv64);
  wr(out, std::vector<int32_t>(r.features.stat, r.features.stat + 2));
  return out ? 0 : 4;
}
