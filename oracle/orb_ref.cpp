// ============================================================================
// TEST INFRASTRUCTURE ONLY.  Real-code oracle for the half of ORBextractor that
// gl_orb_describe replaces: this wrapper #includes the reference's OWN
// gmmloc/src/cv/orb_extractor.cpp from where it lies in the reference tree
// (which reaches its file-static functions) and compiles it against this
// project's stand-in for OpenCV (oracle/cv_standin) -- nothing of the
// reference is copied into this repository.  Built by oracle/Makefile into
// oracle/_ref/liborb_ref.so (-ffp-contract=off) and, for one measurement,
// oracle/_ref/liborb_ref_contract.so (-O3 -mfma -ffp-contract=fast).
//
// What runs here is the reference's: the constructor's tables (umax, pattern,
// mvScaleFactor), IC_Angle / computeOrientation, computeOrbDescriptor /
// computeDescriptors, and the overload of cos / sin that its line
// `float a = (float)cos(angle)` resolves to.  What is the stand-in's: the
// matrix, cvRound and the polynomial of fastAtan2.  The blur is the caller's.
// The wrapper adds access only.
// ============================================================================
#include <cstdint>
#include <type_traits>
#include <vector>

#include "../src/cv/orb_extractor.cpp"  // from -I$(REF)/gmmloc/include: the reference's file, where it lies

namespace gmmloc {
// The reference's `cos(angle)` / `sin(angle)` on a float, under its own using-directives (this scope sees what its functions see):
// the float overloads of <cmath>, which are libm's cosf / sinf, and not the double ones.
static_assert(std::is_same<decltype(cos(std::declval<float>())), float>::value, "the reference's cos(float) is no longer the float overload");
static_assert(std::is_same<decltype(sin(std::declval<float>())), float>::value, "the reference's sin(float) is no longer the float overload");

namespace {
struct Tables : public ORBextractor {
  Tables() : ORBextractor(1000) {}
  const std::vector<int>& u_max() const { return umax; }
  const std::vector<cv::Point>& own_pattern() const { return pattern; }
  const std::vector<float>& scale_factors() const { return mvScaleFactor; }
};

const Tables& tables() {
  static const Tables t;
  return t;
}

cv::Mat level(const uint8_t* img, int width, int height, int64_t stride) { return cv::Mat(height, width, CV_8UC1, const_cast<uint8_t*>(img), (size_t)stride); }

// the expressions of computeOrbDescriptor's first two lines, in this translation unit and under its flags
void steering(float kp_angle, float* a_out, float* b_out) {
  float angle = (float)kp_angle * factorPI;
  float a = (float)cos(angle), b = (float)sin(angle);
  *a_out = a;
  *b_out = b;
}
}  // namespace
}  // namespace gmmloc

extern "C" {
// umax [16], pattern [512 x 2] (x, y), mvScaleFactor [8] of a constructed extractor -> the number of pattern entries
int orbref_tables(int32_t* umax, int32_t* pattern, float* scale_factor) {
  const gmmloc::Tables& t = gmmloc::tables();
  if (t.u_max().size() != 16 || t.scale_factors().size() != 8) return -1;
  for (int i = 0; i < 16; ++i) umax[i] = t.u_max()[i];
  for (int i = 0; i < 8; ++i) scale_factor[i] = t.scale_factors()[i];
  const int n = (int)t.own_pattern().size();
  for (int i = 0; i < n && i < 512; ++i) pattern[2 * i] = t.own_pattern()[i].x, pattern[2 * i + 1] = t.own_pattern()[i].y;
  return n;
}

// computeOrientation on the level img (width x height, `stride` bytes per row) for n key-points (x, y) that keep 15 px from every edge:
// angle [n], and the moments m_10 / m_01 [n] as the reference handed them to fastAtan2 (floats of integers below 2^24: exact).
// One key-point per call of computeOrientation, so that the stand-in's record of the last call is that key-point's.
void orbref_orientation(const uint8_t* img, int width, int height, int64_t stride, const int32_t* kp_xy, int n, float* angle, int32_t* m_10,
                        int32_t* m_01) {
  const cv::Mat image = gmmloc::level(img, width, height, stride);
  for (int i = 0; i < n; ++i) {
    std::vector<cv::KeyPoint> kp(1);
    kp[0].pt = cv::Point2f((float)kp_xy[2 * i], (float)kp_xy[2 * i + 1]);
    gmmloc::computeOrientation(image, kp, gmmloc::tables().u_max());
    float y, x;
    cv::standin_last_atan2_args(&y, &x);
    angle[i] = kp[0].angle;
    m_01[i] = (int32_t)y;
    m_10[i] = (int32_t)x;
  }
}

// computeDescriptors on the ALREADY BLURRED level for n key-points (x, y) with their angles (degrees) that keep 19 px from every edge;
// pattern: 512 x 2 int8 (x, y), entries within [-13, 13], or NULL for the extractor's own -> desc [n x 32]
void orbref_describe(const uint8_t* blurred, int width, int height, int64_t stride, const int32_t* kp_xy, const float* kp_angle, int n,
                     const int8_t* pattern, uint8_t* desc) {
  const cv::Mat image = gmmloc::level(blurred, width, height, stride);
  std::vector<cv::Point> pat;
  if (pattern)
    for (int i = 0; i < 512; ++i) pat.push_back(cv::Point(pattern[2 * i], pattern[2 * i + 1]));
  else
    pat = gmmloc::tables().own_pattern();
  std::vector<cv::KeyPoint> kp(n);
  for (int i = 0; i < n; ++i) {
    kp[i].pt = cv::Point2f((float)kp_xy[2 * i], (float)kp_xy[2 * i + 1]);
    kp[i].angle = kp_angle[i];
  }
  cv::Mat out;
  gmmloc::computeDescriptors(image, kp, out, pat);
  for (int i = 0; i < n; ++i) std::memcpy(desc + (size_t)32 * i, out.ptr(i), 32);
}

// (a, b) of computeOrbDescriptor for n angles in degrees: this host's cos / sin of a float after the factorPI multiply
void orbref_steering(const float* kp_angle, int n, float* a, float* b) {
  for (int i = 0; i < n; ++i) gmmloc::steering(kp_angle[i], a + i, b + i);
}
}
