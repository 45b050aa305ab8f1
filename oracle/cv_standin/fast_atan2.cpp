// ============================================================================
// TEST INFRASTRUCTURE ONLY.  cv::fastAtan2 of this project's OpenCV stand-in:
// the rule that include/gmmloc_hip.h DECLARES in its `angle` row, one IEEE
// binary32 operation per step in source order.  ALWAYS compiled with
// -ffp-contract=off (oracle/Makefile), whatever the flags of the code that
// calls it.  It is this project's statement and not OpenCV's binary: a test
// that compares an angle with it shows which arguments the reference passes,
// in which order, and nothing about the polynomial.
// ============================================================================
#include <cfloat>
#include <cmath>

#include "opencv2/core/core.hpp"

namespace cv {
namespace {
thread_local float last_y = 0.f, last_x = 0.f;
}

float fastAtan2(float y, float x) {
  last_y = y, last_x = x;
  const float scale = (float)(180.0 / 3.14159265358979323846);
  const float p1 = 0.9997878412794807f * scale, p3 = -0.3258083974640975f * scale, p5 = 0.1555786518463281f * scale, p7 = -0.04432655554792128f * scale;
  const float ax = std::fabs(x), ay = std::fabs(y);
  const bool steep = ay > ax;
  volatile float den = (steep ? ay : ax) + (float)DBL_EPSILON;  // (volatile: each step below is a float of its own, never kept wider)
  volatile float c = (steep ? ax : ay) / den;
  volatile float c2 = c * c;
  volatile float a = p7 * c2;
  a = a + p5;
  a = a * c2;
  a = a + p3;
  a = a * c2;
  a = a + p1;
  a = a * c;
  if (steep) a = 90.0f - a;
  if (x < 0.0f) a = 180.0f - a;
  if (y < 0.0f) a = 360.0f - a;
  return a;
}

void standin_last_atan2_args(float* y, float* x) {
  *y = last_y;
  *x = last_x;
}
}  // namespace cv
